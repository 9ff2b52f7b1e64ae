// What the host translation units of the C ABI share.  Host-only: no device translation unit includes it.
//   mfgp_capi.hip            the handle and its settings, Gram / kdiag, potrf_inv, copy_block, mvn_sample,
//                            adam_packed, the SVGP entries
//   mfgp_fence.hip           the device-wide flow fence (mfgp_fence.h) and mfgp_flow_fence
//   mfgp_gpr_capi.hip        fp64 GPR / graph-kernel training and predict: gpr_layout, gpr_factor
//   mfgp_f32_capi.hip        the fp32 path, the fp32 settings and the dtype-generic *_ex entries
//   mfgp_posterior_capi.hip  the cached posterior: its caches, the workspace chain, the forward drivers
//   mfgp_density.hip         mfgp_mvn_logpdf and mfgp_mvn_fisher, beside their kernels
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mfgp.h"
#include "mfgp_internal.h"
#include "mfgp_device.h"   // theta_size, MFGP_MAX_LF

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

// One GPR call, filled once by its C-ABI entry and taken by const reference by every driver and builder:
// a driver's signature names everything it reads, and nothing else does.  T: the scalar of X and Y
// (fp64, or float on the fp32 path); theta is fp64 and read-only here -- the Adam entries' writable
// theta travels in FinArgs::theta (adam_fin) alone.  A size query fills n, p, d, nlf only.
template <class T>
struct GprProblemT {
    int n, p, d, nlf;         // nlf: 0 the linear multi-fidelity kernel, m >= 1 the graph kernel
    const T* X; int ldx;
    const T* Y; int ldy;
    const double* theta;
    void* ws; size_t ws_bytes;
    int* info;
};
using GprProblem = GprProblemT<double>;
template <class T>
struct GprPredictIOT {
    int nstar;
    const T* Xs; int ldxs;
    T* mean; int ldm;
    T* var;
    T* cov; int ldc;          // cov == nullptr: no covariance block
};
using GprPredictIO = GprPredictIOT<double>;

// The argument checks of the GPR entries, before any device work, in the order the return codes of a
// call that is wrong in several ways depend on: handle, d (MFGP_ERR_DIM), nlf in lf_min..MFGP_MAX_LF,
// sizes, then rest_ok (the entry's own pointers and leading dimensions).
static inline int gpr_check_dims(mfgp_handle_t h, int n, int p, int d, int nlf, int lf_min, bool rest_ok) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf < lf_min || nlf > MFGP_MAX_LF) return MFGP_ERR_ARG;
    return n < 1 || p < 1 || !rest_ok ? MFGP_ERR_ARG : MFGP_OK;
}
template <class T>
static int gpr_check(mfgp_handle_t h, const GprProblemT<T>& P, int lf_min, bool rest_ok) {
    return gpr_check_dims(h, P.n, P.p, P.d, P.nlf, lf_min, P.X && P.Y && P.theta && P.ws && P.info && rest_ok);
}
// a predict entry's second check, behind its nstar == 0 return
template <class T>
static bool gpr_predict_io_ok(const GprPredictIOT<T>& io, bool want_cov) {
    return io.Xs && io.mean && io.var && (!want_cov || (io.cov && io.ldc >= io.nstar));
}

// One cached-posterior call (mfgp_posterior_capi.hip), filled once by its C-ABI entry as a GPR call is:
// which cache (a size query leaves cache and cache_bytes zero), and the query both families share.  What
// a query carries beyond the forward selects the call: cov (GPR predict), grad (the VJP call), dens (the
// log-density call; with dens->gX the VJP fed the density's own gradients) or jac (the Jacobian call).
struct GprCacheRef { int nlf, n, p, d; const void* cache; size_t cache_bytes; };
struct SvgpCacheRef { int m, l, p, d, mixed; const void* cache; size_t cache_bytes; };
struct PostGradIO {
    const double* gmean; long ldgm;
    const double* gvar;
    double* gX; long ldgx;
};
struct LogdensIO {
    const double* Y; long y_rs;
    const double* obs_var; long ov_rs;
    const double* obs_cov; int ldc;
    double* logp;
    double* gX; int ldgx;     // nullptr: the value only, the call ends behind the density launch
    int* info;
};
struct JacIO {
    const void* weights; size_t weights_bytes;   // alpha = L^{-T} Z / Lm^{-T} q_mu (mfgp_*_jacobian_weights)
    double* J; long ldj;                         // [nstar][d][ldj], outputs fastest
};
struct PostQuery {
    int nstar;
    const double* Xs; int ldxs;
    void* ws; size_t ws_bytes;
    double* mean; int ldm;    // SVGP: f_mu [nstar x p], ldm = p
    double* var;              // GPR [nstar]; SVGP: f_var [nstar x p]
    double* cov; int ldc;
    const PostGradIO* grad;
    const LogdensIO* dens;
    const JacIO* jac;         // the Jacobian call: the forward, then k_jac_gpr / k_jac_svgp on the weights
};
// The posterior entries' argument checks, in gpr_check_dims' order: handle, d (MFGP_ERR_DIM), the family's
// sizes, then rest_ok; an SVGP cache without a mixing matrix has a latent per output.
static inline int gpr_post_check(mfgp_handle_t h, const GprCacheRef& c, bool rest_ok) {
    return gpr_check_dims(h, c.n, c.p, c.d, c.nlf, 0, rest_ok);
}
static inline int svgp_post_check(mfgp_handle_t h, const SvgpCacheRef& c, bool rest_ok) {
    CHECK_H(h);
    CHECK_D(c.d);
    if (c.m < 1 || c.l < 1 || c.p < 1 || !rest_ok) return MFGP_ERR_ARG;
    return !c.mixed && c.l != c.p ? MFGP_ERR_ARG : MFGP_OK;
}
// the pointers and leading dimensions every compute entry with a query needs (p outputs, d inputs)
static inline bool post_query_ok(const PostQuery& q, const void* cache, int p, int d) {
    return cache && q.Xs && q.ws && q.mean && q.var && q.ldxs >= d + 1 && q.ldm >= p;
}

// Below this many 32-tiles the launch-per-step Cholesky is faster than the persistent flow (one
// 256-workgroup launch costs more than a few short step launches): fp64 value+grad evaluation,
// flow vs steps (tools/flow_threshold.py): T = 2: 67.5 vs 56.8 us, T = 5: 83.2 vs 79.7, T = 7:
// 95.3 vs 96.2, T = 9: 106.2 vs 110.6, T = 24: 195.9 vs 247.1.
constexpr int FLOW_MIN_TILES = 8;

// What of the handle's schedule a layout depends on; no_flow: the launch-per-step factorization whatever
// the handle says (predict, the posterior build).
struct GprSched { int grad_chunk, flow_wgs, flow_min_t; };
static inline GprSched gpr_sched(mfgp_handle_t h) { return {h->grad_chunk, h->flow_wgs, h->flow_min_t}; }
static inline GprSched gpr_sched_no_flow(mfgp_handle_t h) { return {h->grad_chunk, 0, 0}; }
// reads n, p, d, nlf and ws of P (ws == nullptr only counts)
GprLayout gpr_layout(int nb, const GprProblem& P, const GprSched& sc);

// The LML-layout Gram and the launch-per-step factorization on L (gram_lml_and_factor at tile size nb):
// L.Xo then holds [L^{-1} | Z].
void gpr_factor(int nb, hipStream_t s, const GprLayout& L, const GprProblem& P);

// The evaluation part of k_reduce_items' / k_gpr_tiny's argument block: the problem, what to write, and
// the Adam part (adam_fin) when the call is an Adam step.  The caller adds where its partial sums lie.
template <class T>
static FinArgs fin_eval(const GprProblemT<T>& P, int G, int want_grad, double* out, const FinArgs* adam) {
    FinArgs f{};
    if (adam) f = *adam;
    f.info = P.info; f.P = P.p; f.D = P.d; f.want_grad = want_grad; f.out = out; f.n = P.n;
    f.adam = adam != nullptr;
    f.G = G;
    return f;
}
// The Adam part from the C arguments of an Adam entry.  The one place FinArgs::theta is set: the step
// refreshes the constrained theta the evaluation reads through the descriptor's const pointer.
static inline FinArgs adam_fin(int d, double* theta, double* u, double* m, double* v, const unsigned char* trainable,
                               const int* tie, int* step, double lr, double b1, double b2, double eps,
                               double* loss_hist) {
    FinArgs f{};
    f.theta = theta; f.u = u; f.m = m; f.v = v; f.trainable = trainable; f.tie = tie; f.step = step;
    f.lr = lr; f.b1 = b1; f.b2 = b2; f.eps = eps; f.loss_hist = loss_hist;
    f.noise_index = theta_size(d) - 1;
    return f;
}

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
