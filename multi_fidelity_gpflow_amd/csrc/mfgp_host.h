// What the host translation units of the C ABI (mfgp_capi.hip, mfgp_posterior_capi.hip) share.  Host-only: no
// device translation unit includes it.  gpr_layout, gpr_factor and copy_block are defined in mfgp_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mfgp.h"
#include "mfgp_internal.h"

struct mfgp_handle_s {
    int device;
    hipStream_t stream;
    int nb;
    int grad_chunk;
    int flow_wgs;   // k_chol_flow grid (one workgroup per CU); 0: launch-per-step Cholesky
    int flow_min_t; // fewest 32-tiles a factorization needs to take the flow (below: the step launches)
    int ncu;        // compute units of the device
    int gram_wgs;   // k_gram tile workgroups, LML layout (0: one per CU; < 0: one per tile; MFGP_GRAM_WGS)
    int flow_trace; // k_chol_flow writes its diagnostic timeline into the workspace
    long long flow_timeout;   // k_chol_flow hand-off wait bound (100 MHz ticks)
    int f32_panel;  // fp32 path: 128-wide tile columns per outer panel (trailing-update K = 128 * f32_panel)
    int f32_lookahead;          // fp32 sweep: factor the next panel beside the trailing update
    int f32_reserve;            // CUs the capped trailing update leaves to the side stream
    int f32_refine;             // fp32 value-only LML (one step) / predict mean (this many steps): fp64 refinement (mfgp_set_f32_refine)
    int tiny;                   // small problems (n, p <= 64, D <= 16, AR1 kernel): one-launch LML step (default on; MFGP_TINY=0 / mfgp_set_tiny(h, 0) disables)
    hipStream_t side;           // its high-priority side stream + fork / join events (created with the handle)
    hipEvent_t ev_fork, ev_join;
    int svgp_qs_packed;         // mfgp_set_svgp_qs_packed: mfgp_svgp_elbo_grad's q_sqrt / gq_sqrt as packed triangles
    int step_fusion;            // mfgp_set_step_fusion: mfgp_gpr_adam_steps defers each step's reduction into the next flow launch
    int resident;               // mfgp_set_resident: fp64 value+grad flow calls may skip the set-up launch
    struct {                    // the last fp64 LML call on this handle, when it left its workspace set
        const void* ws;         // up for the next one (k_grad's grad_next_setup); ws == nullptr: none
        int n, p, d, flow_wgs;
    } res;
};

#define CHECK_H(h) \
    if ((h) == nullptr) return MFGP_ERR_ARG
#define CHECK_D(d) \
    if ((d) < 1 || (d) > MFGP_MAX_D) return MFGP_ERR_DIM

namespace mfgp {

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

constexpr double GRAPH_JITTER = 1e-6;   // graph.py:96: K_full += 1e-6 I

static inline hipError_t last() { return hipGetLastError(); }

struct GprLayout {
    int nb, npad, T, ppad, Tp, G, gstride, ng;
    double *A, *R, *Xo, *Dd, *ldiag, *alpha, *zpart, *gpart, *items;
    int* gorder;   // k_grad workgroup -> task table (+ key), built or verified by k_gram each call
    int* cnt;   // reduce-arrival counter, zeroed by k_gram each call
    int ncnt;
    // k_chol_flow (flow_wgs > 0): flags (zeroed) + owner table (built or verified) by k_gram each call
    int flow_wgs, nflags;
    int *flags, *own;
    double* pub;        // publication area (sentinel-filled by k_gram)
    long npub;
    long long* trace;   // k_chol_flow timeline (diagnostic; written only when enabled)
    int ntrace;
    int gchunk;         // k_grad's task chunk (m-tiles per task)
    size_t bytes;
};
GprLayout gpr_layout(int nb, int n, int p, int d, void* ws, int grad_chunk, int nlf = 0, int flow_wgs = 0,
                     int flow_min_t = 0);

// The LML-layout Gram and the launch-per-step factorization on L (gram_lml_and_factor at tile size nb):
// L.Xo then holds [L^{-1} | Z].
void gpr_factor(int nb, hipStream_t s, const GprLayout& L, int n, int p, int d, const double* X, int ldx,
                const double* Y, int ldy, const double* theta, int* info, int nlf);

// dst[r][c] = src[r][c] over rows x cols (k_copy_block)
void copy_block(hipStream_t s, const double* src, long lds, double* dst, long ldd, int rows, int cols);

// base_conditional(full_cov=True) from A = L^{-1} K(X, X*) (Kt row tiles, padded rows 0, ld nspad):
// K(X*, X*) into Kss, Cov = Kss - A^T A, its nstar x nstar block into cov.
template <int NB>
static void cov_from_a(hipStream_t s, const double* Xs, int ldxs, int nstar, const double* theta, int d, int nlf,
                       const double* Am, int nspad, int Kt, double* Kss, double* Cov, double* cov, int ldc) {
    const int Ts = nspad / NB;
    if (nlf) (void)hipMemsetAsync(Kss, 0, sizeof(double) * (size_t)nspad * nspad, s);
    GramArgs gs{};
    gs.X1 = Xs; gs.ldx1 = ldxs; gs.n1 = nstar;
    gs.X2 = Xs; gs.ldx2 = ldxs; gs.n2 = nstar;
    gs.theta = theta; gs.D = d; gs.rbf_only = 0;
    gs.out = Kss; gs.ldo = nspad; gs.padded = 0; gs.tiles_c = Ts; gs.nlf = nlf;
    gs.diag_add = nlf ? GRAPH_JITTER : 0.0;   // graph.py:96 adds the jitter inside K(X*, X*) too
    if (nlf) launch_gram<NB>(gs, Ts * Ts, 1, s);
    else launch_gram_dense(gs, 1, nspad, nspad, s);
    BgemmArgs b{};
    b.A = Am; b.lda = nspad;
    b.B = Am; b.ldb = nspad;
    b.Cin = Kss; b.ldc = nspad; b.beta = 1.0;
    b.D = Cov; b.ldd = nspad;
    b.alpha = -1.0;
    b.Mt = Ts; b.Nt = Ts; b.Kt = Kt;
    launch_bgemm(NB, s, 1, 0, b, 1);
    copy_block(s, Cov, nspad, cov, ldc, nstar, nstar);
}

}  // namespace mfgp
