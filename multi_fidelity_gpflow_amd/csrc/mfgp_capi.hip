// C-ABI entry points of libmfgp.so (declared in include/mfgp.h): the handle and its settings, Gram / kdiag,
// potrf_inv, mvn_sample, adam_packed and the SVGP entries.  The GPR, fp32, posterior and fence families
// have their own translation units (mfgp_host.h lists them).
//
// Host-side orchestration only: workspace carving, argument blocks, kernel
// launch sequences on the handle's stream.  No allocation, no synchronisation
// (every sequence is hipGraph-capturable).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>

#include "mfgp_device.h"
#include "mfgp_host.h"

namespace mfgp {

// Diagnostic: with MFGP_SEGV_TRACE=1 in the environment when the library loads, a host SIGSEGV prints
// the native call stack (symbol names from the dynamic tables) to stderr before the default action.
static void segv_trace(int sig) {
    void* fr[64];
    const int n = backtrace(fr, 64);
    static const char msg[] = "\nlibmfgp: SIGSEGV, native stack:\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    backtrace_symbols_fd(fr, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
__attribute__((constructor)) static void segv_trace_install() {
    const char* e = getenv("MFGP_SEGV_TRACE");
    if (e && atoi(e) != 0) signal(SIGSEGV, segv_trace);
}

// ---------------------------------------------------------------- potrf_inv
template <int NB>
__global__ void k_pad_copy(const double* A, long lda, long sA, double* Ap, int n, int npad) {
    const int b = blockIdx.z;
    const long total = (long)npad * npad;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int r = (int)(e / npad), c = (int)(e % npad);
        double v = (r == c) ? 1.0 : 0.0;
        if (r < n && c < n) v = A[b * sA + (long)r * lda + c];
        Ap[b * total + e] = v;
    }
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_factor_first(double* Ap, int npad, double* Dd, long sD, double* ldiag,
                                                           int* info) {
    constexpr int E = TileCfg<NB>::ELEMS;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* T0 = smem;
    double* R0 = T0 + E;
    double* dg = R0 + E;
    int& bad = *reinterpret_cast<int*>(dg + NB);
    const int b = blockIdx.z;
    tile_load<NB>(T0, Ap + (long)b * npad * npad, npad);
    __syncthreads();
    tile_potrf_inv<NB>(T0, R0, dg, &bad);
    tile_store<NB>(Dd + b * sD, NB, R0);
    for (int r = threadIdx.x; r < NB; r += NTHREADS) ldiag[(long)b * npad + r] = dg[r];
    if (threadIdx.x == 0 && bad && info[b] == 0) info[b] = bad;
}

__global__ void k_copy_lower_out(const double* Xo, long ldx, long sX, double* Linv, long ldl, long sL, int n) {
    const int b = blockIdx.z;
    const long total = (long)n * n;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int r = (int)(e / n), c = (int)(e % n);
        Linv[b * sL + (long)r * ldl + c] = (c <= r) ? Xo[b * sX + (long)r * ldx + c] : 0.0;
    }
}

__global__ void k_copy_vec(const double* src, long ss, double* dst, long sd, int n) {
    const int b = blockIdx.z;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        dst[b * sd + i] = src[b * ss + i];
}

struct PotrfLayout {
    int npad, T;
    double *A, *R, *Xo, *Dd, *ldiag;
    size_t bytes;
};

static PotrfLayout potrf_layout(int nb, int n, int batch, void* ws) {
    PotrfLayout L;
    L.T = ceil_div(n, nb);
    L.npad = L.T * nb;
    const size_t mat = (size_t)L.npad * L.npad;
    Carve c(ws);
    L.A = c.take<double>(mat * batch);
    L.R = c.take<double>(mat * batch);
    L.Xo = c.take<double>(mat * batch);
    L.Dd = c.take<double>((size_t)L.T * nb * nb * batch);
    L.ldiag = c.take<double>((size_t)L.npad * batch);
    L.bytes = c.off + 256;
    return L;
}

template <int NB>
static int potrf_inv_impl(mfgp_handle_t h, int n, int batch, const double* A, int lda, long sA, void* ws,
                          size_t ws_bytes, double* Linv, int ldl, long sLo, double* ldiag, int* info) {
    const PotrfLayout L = potrf_layout(NB, n, batch, ws);
    if (ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    const long mat = (long)L.npad * L.npad;
    const int blocks = (int)std::min<long>((mat + 255) / 256, 2048);
    (void)hipMemsetAsync(info, 0, sizeof(int) * batch, s);
    hipLaunchKernelGGL(k_pad_copy<NB>, dim3(blocks, 1, batch), dim3(256), 0, s, A, (long)lda, sA, L.A, n, L.npad);
    hipLaunchKernelGGL(k_rhs_init, dim3(blocks, 1, batch), dim3(256), 0, s, L.R, (long)L.npad, mat, L.npad, 0,
                       (const double*)nullptr, 0L, 0L, n, 0);
    hipLaunchKernelGGL(k_factor_first<NB>, dim3(1, 1, batch), dim3(NTHREADS),
                       sizeof(double) * (2 * NB * (NB + 2) + NB + 2), s, L.A, L.npad, L.Dd, (long)L.T * NB * NB,
                       L.ldiag, info);
    CholArgs c{};
    c.A = L.A; c.lda = L.npad; c.sA = mat;
    c.R = L.R; c.ldr = L.npad; c.sR = mat;
    c.Xo = L.Xo; c.ldx = L.npad; c.sX = mat;
    c.Dd = L.Dd; c.sD = (long)L.T * NB * NB; c.ldiag = L.ldiag; c.sL = L.npad; c.info = info;
    c.T = L.T; c.Tp = 0; c.k = 0;
    launch_chol_steps<NB>(c, batch, s);
    const long tot = (long)n * n;
    const int b2 = (int)std::min<long>((tot + 255) / 256, 2048);
    hipLaunchKernelGGL(k_copy_lower_out, dim3(b2, 1, batch), dim3(256), 0, s, L.Xo, (long)L.npad, mat, Linv,
                       (long)ldl, sLo, n);
    if (ldiag)
        hipLaunchKernelGGL(k_copy_vec, dim3(ceil_div(n, 256), 1, batch), dim3(256), 0, s, L.ldiag, (long)L.npad,
                           ldiag, (long)n, n);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

__global__ void k_copy_block(const double* src, long lds, double* dst, long ldd, int rows, int cols) {
    const long total = (long)rows * cols;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int r = (int)(e / cols), c = (int)(e % cols);
        dst[(long)r * ldd + c] = src[(long)r * lds + c];
    }
}
void copy_block(hipStream_t s, const double* src, long lds, double* dst, long ldd, int rows, int cols) {
    const long tot = (long)rows * cols;
    hipLaunchKernelGGL(k_copy_block, dim3((int)std::min<long>((tot + 255) / 256, 2048)), dim3(256), 0, s, src, lds, dst,
                       ldd, rows, cols);
}

int adam_packed_impl(hipStream_t st, int n, double* u, double* c, const double* g, double* m, double* v,
                     const unsigned char* trainable, const unsigned char* transform, const unsigned char* span,
                     int* step, const double* lr_sched, double b1, double b2, double eps, const double* out,
                     double klm, double* loss_hist, double* kl_hist, const int* info, int ninfo);

}  // namespace mfgp

using namespace mfgp;

extern "C" {

int mfgp_version(void) { return 100; }

// Build provenance: build.py passes the hash of the sources the library is compiled from (every
// file of csrc/ and include/mfgp.h, build.source_hash()); the marker string also lets the builder
// read the id from the file without loading it.
#ifndef MFGP_BUILD_ID
#define MFGP_BUILD_ID "unknown"
#endif
__attribute__((used)) static const char k_build_marker[] = "mfgp-build-id:" MFGP_BUILD_ID;
const char* mfgp_build_id(void) { return k_build_marker + 14; }

const char* mfgp_error_string(int code) {
    switch (code) {
        case MFGP_OK: return "ok";
        case MFGP_ERR_ARG: return "invalid argument";
        case MFGP_ERR_WORKSPACE: return "workspace too small";
        case MFGP_ERR_LAUNCH: return "kernel launch failed";
        case MFGP_ERR_DIM: return "unsupported input dimension (1 <= d <= 32)";
        case MFGP_ERR_FENCE: return "flow fence held by another host thread past the bound (WAIT without RECORD?)";
        default: return "unknown error";
    }
}

int mfgp_create(int device, mfgp_handle_t* out) {
    if (!out) return MFGP_ERR_ARG;
    mfgp_handle_s* h = (mfgp_handle_s*)calloc(1, sizeof(mfgp_handle_s));
    if (!h) return MFGP_ERR_ARG;
    h->device = device;
    h->stream = nullptr;
    h->nb = 32;
    h->grad_chunk = 24;   // k_grad m-tiles per task (sweep at Goku T = 37: 16 -> 33.8 us, 24 -> 31.9, 40 -> 36.7)
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ncu = 0;
    h->ncu = ncu;
    h->flow_wgs = ncu;
    h->flow_min_t = FLOW_MIN_TILES;
    h->flow_timeout = FLOW_TIMEOUT_TICKS;
    h->f32_panel = 6;
    h->f32_lookahead = 1;
    h->f32_reserve = 32;
    h->gram_wgs = 0;
    if (const char* gv = getenv("MFGP_GRAM_WGS")) h->gram_wgs = atoi(gv);
    h->tiny = 1;   // small problems (n, p <= 64, D <= 16) in one launch: 37.0 us against 43.5 us of kernel
                   // time for the step sequence at HBS, 3.93 vs 4.31 ms for 100 captured Adam steps
                   // (MFGP_TINY=0 / mfgp_set_tiny(h, 0): the step sequence)
    if (const char* tv = getenv("MFGP_TINY")) h->tiny = atoi(tv) != 0;
    if (const char* rv = getenv("MFGP_F32_RESERVE")) h->f32_reserve = std::max(0, atoi(rv));
    if (const char* la = getenv("MFGP_F32_LOOKAHEAD")) h->f32_lookahead = atoi(la) != 0;
    h->f32_refine = 2;
    if (const char* rf = getenv("MFGP_F32_REFINE")) h->f32_refine = std::min(2, std::max(0, atoi(rf)));
    {
        int lo = 0, hi = 0;
        int cur = -1;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) hi = 0;
        if (hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, hi) != hipSuccess) h->side = nullptr;
        if (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) h->ev_fork = nullptr;
        if (hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) h->ev_join = nullptr;
        if (cur >= 0) (void)hipSetDevice(cur);
    }
    if (const char* fp = getenv("MFGP_F32_PANEL")) h->f32_panel = std::max(1, atoi(fp));
    if (const char* fl = getenv("MFGP_FLOW")) if (atoi(fl) == 0) h->flow_wgs = 0;
    h->step_fusion = 1;
    if (const char* sf = getenv("MFGP_STEP_FUSION")) h->step_fusion = atoi(sf) != 0;
    if (const char* gc = getenv("MFGP_GRAD_CHUNK")) h->grad_chunk = std::max(1, atoi(gc));
    const char* env = getenv("MFGP_TILE");
    if (env && atoi(env) == 64) h->nb = 64;
    *out = h;
    return MFGP_OK;
}

int mfgp_destroy(mfgp_handle_t h) {
    if (h) {
        if (h->side) (void)hipStreamDestroy(h->side);
        if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
        if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    }
    free(h);
    return MFGP_OK;
}

int mfgp_set_stream(mfgp_handle_t h, void* stream) {
    CHECK_H(h);
    h->stream = (hipStream_t)stream;
    return MFGP_OK;
}

int mfgp_set_tile(mfgp_handle_t h, int nb) {
    CHECK_H(h);
    if (nb != 32 && nb != 64) return MFGP_ERR_ARG;
    h->nb = nb;
    return MFGP_OK;
}

int mfgp_get_tile(mfgp_handle_t h) { return h ? h->nb : MFGP_ERR_ARG; }

int mfgp_set_flow(mfgp_handle_t h, int enable) {
    CHECK_H(h);
    if (enable < 0 || enable > 3) return MFGP_ERR_ARG;
    h->flow_wgs = enable ? h->ncu : 0;
    h->flow_trace = enable == 2;
    h->flow_min_t = enable == 3 ? 0 : FLOW_MIN_TILES;
    return MFGP_OK;
}

int mfgp_set_flow_timeout_us(mfgp_handle_t h, long long us) {
    CHECK_H(h);
    if (us < 0) return MFGP_ERR_ARG;
    h->flow_timeout = us * 100;   // s_memrealtime: 100 MHz
    return MFGP_OK;
}

int mfgp_set_tiny(mfgp_handle_t h, int enable) {
    if (!h) return MFGP_ERR_ARG;
    h->tiny = enable != 0;
    return MFGP_OK;
}

int mfgp_get_tiny(mfgp_handle_t h) { return h ? h->tiny : MFGP_ERR_ARG; }

int mfgp_set_step_fusion(mfgp_handle_t h, int enable) {
    CHECK_H(h);
    h->step_fusion = enable != 0;
    return MFGP_OK;
}

int mfgp_get_step_fusion(mfgp_handle_t h) { return h ? h->step_fusion : 0; }

int mfgp_set_resident(mfgp_handle_t h, int enable) {
    if (!h) return MFGP_ERR_ARG;
    h->resident = enable != 0;
    return MFGP_OK;
}

int mfgp_get_grad_chunk(mfgp_handle_t h) { return h ? h->grad_chunk : MFGP_ERR_ARG; }

int mfgp_get_flow(mfgp_handle_t h) { return h ? (h->flow_wgs > 0 ? (h->flow_min_t ? 1 : 3) : 0) : MFGP_ERR_ARG; }

static int gram_common(mfgp_handle_t h, int n1, int n2, int d, const double* X1, int ldx1, const double* X2,
                       int ldx2, const double* params, double diag_add, double* K, int ldk, int rbf, int nlf = 0) {
    CHECK_H(h);
    CHECK_D(d);
    if (n1 < 0 || n2 < 0 || !X1 || !X2 || !params || !K) return MFGP_ERR_ARG;
    if (n1 == 0 || n2 == 0) return MFGP_OK;
    GramArgs g{};
    g.X1 = X1; g.ldx1 = ldx1; g.n1 = n1;
    g.X2 = X2; g.ldx2 = ldx2; g.n2 = n2;
    g.theta = params; g.D = d; g.rbf_only = rbf;
    g.out = K; g.ldo = ldk; g.padded = 0; g.diag_add = diag_add; g.nlf = nlf;
    const int nb = h->nb;
    g.tiles_c = ceil_div(n2, nb);
    const int blocks = ceil_div(n1, nb) * g.tiles_c;
    TILE_CALL(nb, launch_gram, g, blocks, 1, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

int mfgp_rbf_gram(mfgp_handle_t h, int n1, int n2, int d, const double* X1, int ldx1, const double* X2, int ldx2,
                  const double* params, double* K, int ldk) {
    return gram_common(h, n1, n2, d, X1, ldx1, X2, ldx2, params, 0.0, K, ldk, 1);
}

int mfgp_mf_gram(mfgp_handle_t h, int n1, int n2, int d, const double* X1, int ldx1, const double* X2, int ldx2,
                 const double* theta, double diag_add, double* K, int ldk) {
    return gram_common(h, n1, n2, d, X1, ldx1, X2, ldx2, theta, diag_add, K, ldk, 0);
}

int mfgp_mf_kdiag(mfgp_handle_t h, int n, int d, const double* X, int ldx, const double* theta, double* out) {
    CHECK_H(h);
    CHECK_D(d);
    if (n < 0 || !X || !theta || !out) return MFGP_ERR_ARG;
    if (n == 0) return MFGP_OK;
    hipLaunchKernelGGL(k_kdiag, dim3(ceil_div(n, 256)), dim3(256), 0, h->stream, X, (long)ldx, n, d, theta, out, 0);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

// ---------------------------------------------------------------- graph kernel (graph.py)
#define CHECK_LF(m) \
    if ((m) < 1 || (m) > MFGP_MAX_LF) return MFGP_ERR_ARG

int mfgp_gmf_gram(mfgp_handle_t h, int nlf, int n1, int n2, int d, const double* X1, int ldx1, const double* X2,
                  int ldx2, const double* theta, double diag_add, double* K, int ldk) {
    CHECK_LF(nlf);
    return gram_common(h, n1, n2, d, X1, ldx1, X2, ldx2, theta, diag_add, K, ldk, 0, nlf);
}

int mfgp_gmf_kdiag(mfgp_handle_t h, int nlf, int n, int d, const double* X, int ldx, const double* theta,
                   double* out) {
    CHECK_H(h);
    CHECK_D(d);
    CHECK_LF(nlf);
    if (n < 0 || !X || !theta || !out) return MFGP_ERR_ARG;
    if (n == 0) return MFGP_OK;
    hipLaunchKernelGGL(k_kdiag, dim3(ceil_div(n, 256)), dim3(256), 0, h->stream, X, (long)ldx, n, d, theta, out,
                       nlf);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

int mfgp_theta_from_u(mfgp_handle_t h, const double* u, double* theta, int g, int noise_index) {
    CHECK_H(h);
    if (!u || !theta || g < 1 || g > 256) return MFGP_ERR_ARG;
    hipLaunchKernelGGL(k_theta_from_u, dim3(1), dim3(256), 0, h->stream, u, theta, g, noise_index);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

int mfgp_potrf_inv_workspace_size(mfgp_handle_t h, int n, int batch, size_t* bytes) {
    CHECK_H(h);
    if (n < 1 || batch < 1 || !bytes) return MFGP_ERR_ARG;
    *bytes = potrf_layout(h->nb, n, batch, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_potrf_inv(mfgp_handle_t h, int n, int batch, const double* A, int lda, long sA, void* ws, size_t ws_bytes,
                   double* Linv, int ldl, long sL, double* ldiag, int* info) {
    CHECK_H(h);
    if (n < 1 || batch < 1 || !A || !ws || !Linv || !info) return MFGP_ERR_ARG;
    return TILE_CALL(h->nb, potrf_inv_impl, h, n, batch, A, lda, sA, ws, ws_bytes, Linv, ldl, sL, ldiag, info);
}

int mfgp_mvn_sample_workspace_size(mfgp_handle_t h, int n, int batch, size_t* bytes) {
    CHECK_H(h);
    if (n < 0 || batch < 1 || batch > 65535 || !bytes) return MFGP_ERR_ARG;
    *bytes = mvn_sample_ws_bytes(n, batch);
    return MFGP_OK;
}

int mfgp_mvn_sample(mfgp_handle_t h, int n, int batch, int nsamp, int ncol, const double* cov, int ldc, long sC,
                    double jitter, const double* mean, long mean_rs, long mean_bs, const double* eps, double* out,
                    long rs, long ss, long bs, void* ws, size_t ws_bytes, int* info) {
    CHECK_H(h);
    if (n < 0 || nsamp < 0 || batch < 1 || batch > 65535 || ncol < 1 || ldc < n) return MFGP_ERR_ARG;
    if ((long)nsamp * ncol > 0x7fffffffL) return MFGP_ERR_ARG;
    if (n == 0 || nsamp == 0) return MFGP_OK;
    if (!cov || !mean || !eps || !out || !ws || !info || eps == out) return MFGP_ERR_ARG;
    if (ws_bytes < mvn_sample_ws_bytes(n, batch)) return MFGP_ERR_WORKSPACE;
    SampleArgs a{};
    a.cov = cov; a.ldc = ldc; a.sC = sC; a.jitter = jitter;
    a.mean = mean; a.mean_rs = mean_rs; a.mean_bs = mean_bs;
    a.eps = eps; a.out = out; a.rs = rs; a.ss = ss; a.bs = bs;
    a.info = info;
    a.n = n; a.batch = batch; a.nsamp = nsamp; a.ncol = ncol;
    launch_mvn_sample(a, ws, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

int mfgp_svgp_workspace_size(mfgp_handle_t h, int n, int m, int l, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (n < 1 || m < 1 || l < 1 || p < 1 || !bytes) return MFGP_ERR_ARG;
    *bytes = (size_t)svgp_workspace_bytes(h->nb, n, m, l, p, d);
    return MFGP_OK;
}

static SvgpStreams svgp_streams(mfgp_handle_t h) { return SvgpStreams{h->stream, h->side, h->ev_fork, h->ev_join}; }

// The argument checks of the six ELBO entries, before any device work.  go: the gradient outputs of a
// gradient entry (nullptr: a value entry, whose g_mu / g_var may be NULL and whose noise is a host value).
static int svgp_check(mfgp_handle_t h, const SvgpProblem& P, const SvgpLik& lik, const SvgpFwdOut& o,
                      const SvgpGradOut* go) {
    CHECK_H(h);
    CHECK_D(P.d);
    if (P.n < 1 || P.m < 1 || P.l < 1 || P.p < 1 || !P.X || !P.Y || !P.Z || !P.thetas || !P.q_mu || !P.q_sqrt ||
        !P.ws || !o.out || !P.info)
        return MFGP_ERR_ARG;
    if ((go || lik.kind == SvgpLik::MASKED) && !lik.noise_dev) return MFGP_ERR_ARG;
    if (go && (!o.g_mu || !o.g_var || !go->gZ || !go->gtheta || !go->gq_mu || !go->gq_sqrt || !go->gnoise))
        return MFGP_ERR_ARG;
    if (P.qs_packed != 0 && P.qs_packed != 1) return MFGP_ERR_ARG;
    if (lik.kind == SvgpLik::MASKED && lik.pn != 1 && lik.pn != P.p) return MFGP_ERR_ARG;
    if (!P.W && P.l != P.p) return MFGP_ERR_ARG;
    if (go && P.W && !go->gW) return MFGP_ERR_ARG;
    if (P.ldx < P.d + 1 || P.ldz < P.d + 1 || P.ldy < P.p) return MFGP_ERR_ARG;
    if (lik.kind == SvgpLik::HET && lik.ldu < P.p) return MFGP_ERR_ARG;
    // the VE reverse kernels keep a row's state in LDS
    if (go && lik.kind == SvgpLik::HET && svgp_ve_het_rows(P.p, P.l) == 0) return MFGP_ERR_DIM;
    if (go && lik.kind == SvgpLik::MASKED && svgp_ve_masked_rows(P.p, P.l) == 0) return MFGP_ERR_DIM;
    return MFGP_OK;
}

// noise: the host variance of a value entry; noise_dev: the device variance of a gradient entry
static SvgpLik svgp_lik_gaussian(double noise, const double* noise_dev, const double* Yunc = nullptr, int ldu = 0) {
    SvgpLik lik;
    lik.kind = Yunc ? SvgpLik::HET : SvgpLik::GAUSSIAN;   // Yunc == NULL: the homoscedastic kernels and launches
    lik.noise = noise; lik.noise_dev = noise_dev;
    lik.Yunc = Yunc; lik.ldu = ldu;
    return lik;
}
static SvgpLik svgp_lik_masked(const double* noise_dev, int pn) {
    SvgpLik lik;
    lik.kind = SvgpLik::MASKED;
    lik.noise_dev = noise_dev; lik.pn = pn;
    return lik;
}

int mfgp_svgp_elbo(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx, const double* Y,
                   int ldy, const double* Z, int ldz, const double* thetas, const double* q_mu,
                   const double* q_sqrt, const double* W, double noise, double scale, double jitter, void* ws,
                   size_t ws_bytes, double* out, double* g_mu, double* g_var, int* info) {
    const SvgpProblem P{n, m, l, p, d, X, ldx, Y, ldy, Z, ldz, thetas, q_mu, q_sqrt, 0, W, scale, 1.0, jitter,
                        ws, ws_bytes, info};
    const SvgpLik lik = svgp_lik_gaussian(noise, nullptr);
    const SvgpFwdOut o{out, g_mu, g_var};
    if (const int rc = svgp_check(h, P, lik, o, nullptr)) return rc;
    return svgp_elbo_impl(h->nb, svgp_streams(h), P, lik, o);
}

int mfgp_svgp_grad_workspace_size(mfgp_handle_t h, int n, int m, int l, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (bytes == nullptr || n < 1 || m < 1 || l < 1 || p < 1) return MFGP_ERR_ARG;
    *bytes = svgp_grad_workspace_bytes(h->nb, n, m, l, p, d);
    return MFGP_OK;
}

int mfgp_svgp_elbo_grad(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx,
                        const double* Y, int ldy, const double* Z, int ldz, const double* thetas,
                        const double* q_mu, const double* q_sqrt, const double* W, const double* noise,
                        double scale, double kl_mult, double jitter, void* ws, size_t ws_bytes, double* out, double* g_mu,
                        double* g_var, double* gZ, double* gtheta, double* gq_mu, double* gq_sqrt, double* gW,
                        double* gnoise, int* info) {
    const SvgpProblem P{n, m, l, p, d, X, ldx, Y, ldy, Z, ldz, thetas, q_mu, q_sqrt, h ? h->svgp_qs_packed : 0, W, scale, kl_mult, jitter,
                        ws, ws_bytes, info};
    const SvgpLik lik = svgp_lik_gaussian(0.0, noise);
    const SvgpFwdOut o{out, g_mu, g_var};
    const SvgpGradOut go{gZ, gtheta, gq_mu, gq_sqrt, gW, gnoise};
    if (const int rc = svgp_check(h, P, lik, o, &go)) return rc;
    return svgp_grad_impl(h->nb, svgp_streams(h), P, lik, o, go);
}

int mfgp_svgp_elbo_het(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx, const double* Y,
                       int ldy, const double* Yunc, int ldu, const double* Z, int ldz, const double* thetas,
                       const double* q_mu, const double* q_sqrt, const double* W, double noise, double scale,
                       double jitter, void* ws, size_t ws_bytes, double* out, double* g_mu, double* g_var, int* info) {
    const SvgpProblem P{n, m, l, p, d, X, ldx, Y, ldy, Z, ldz, thetas, q_mu, q_sqrt, 0, W, scale, 1.0, jitter,
                        ws, ws_bytes, info};
    const SvgpLik lik = svgp_lik_gaussian(noise, nullptr, Yunc, ldu);
    const SvgpFwdOut o{out, g_mu, g_var};
    if (const int rc = svgp_check(h, P, lik, o, nullptr)) return rc;
    return svgp_elbo_impl(h->nb, svgp_streams(h), P, lik, o);
}

int mfgp_svgp_elbo_grad_het(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx,
                            const double* Y, int ldy, const double* Yunc, int ldu, const double* Z, int ldz,
                            const double* thetas, const double* q_mu, const double* q_sqrt, int qs_packed,
                            const double* W, const double* noise, double scale, double kl_mult, double jitter,
                            void* ws, size_t ws_bytes, double* out, double* g_mu, double* g_var, double* gZ,
                            double* gtheta, double* gq_mu, double* gq_sqrt, double* gW, double* gnoise, int* info) {
    const SvgpProblem P{n, m, l, p, d, X, ldx, Y, ldy, Z, ldz, thetas, q_mu, q_sqrt, qs_packed, W, scale, kl_mult, jitter,
                        ws, ws_bytes, info};
    const SvgpLik lik = svgp_lik_gaussian(0.0, noise, Yunc, ldu);
    const SvgpFwdOut o{out, g_mu, g_var};
    const SvgpGradOut go{gZ, gtheta, gq_mu, gq_sqrt, gW, gnoise};
    if (const int rc = svgp_check(h, P, lik, o, &go)) return rc;
    return svgp_grad_impl(h->nb, svgp_streams(h), P, lik, o, go);
}

int mfgp_svgp_elbo_masked(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx,
                          const double* Y, int ldy, const double* Z, int ldz, const double* thetas, const double* q_mu,
                          const double* q_sqrt, const double* W, const double* noise, int pn, double scale,
                          double jitter, void* ws, size_t ws_bytes, double* out, double* g_mu, double* g_var,
                          int* info) {
    const SvgpProblem P{n, m, l, p, d, X, ldx, Y, ldy, Z, ldz, thetas, q_mu, q_sqrt, 0, W, scale, 1.0, jitter,
                        ws, ws_bytes, info};
    const SvgpLik lik = svgp_lik_masked(noise, pn);
    const SvgpFwdOut o{out, g_mu, g_var};
    if (const int rc = svgp_check(h, P, lik, o, nullptr)) return rc;
    return svgp_elbo_impl(h->nb, svgp_streams(h), P, lik, o);
}

int mfgp_svgp_elbo_grad_masked(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx,
                               const double* Y, int ldy, const double* Z, int ldz, const double* thetas,
                               const double* q_mu, const double* q_sqrt, int qs_packed, const double* W,
                               const double* noise, int pn, double scale, double kl_mult, double jitter, void* ws,
                               size_t ws_bytes, double* out, double* g_mu, double* g_var, double* gZ, double* gtheta,
                               double* gq_mu, double* gq_sqrt, double* gW, double* gnoise, int* info) {
    const SvgpProblem P{n, m, l, p, d, X, ldx, Y, ldy, Z, ldz, thetas, q_mu, q_sqrt, qs_packed, W, scale, kl_mult, jitter,
                        ws, ws_bytes, info};
    const SvgpLik lik = svgp_lik_masked(noise, pn);
    const SvgpFwdOut o{out, g_mu, g_var};
    const SvgpGradOut go{gZ, gtheta, gq_mu, gq_sqrt, gW, gnoise};
    if (const int rc = svgp_check(h, P, lik, o, &go)) return rc;
    return svgp_grad_impl(h->nb, svgp_streams(h), P, lik, o, go);
}

int mfgp_set_svgp_qs_packed(mfgp_handle_t h, int packed) {
    CHECK_H(h);
    if (packed != 0 && packed != 1) return MFGP_ERR_ARG;
    h->svgp_qs_packed = packed;
    return MFGP_OK;
}

int mfgp_adam_packed(mfgp_handle_t h, int n, double* u, double* c, const double* g, double* m, double* v,
                     const unsigned char* trainable, const unsigned char* transform, const unsigned char* span,
                     int* step, const double* lr_sched, double beta1, double beta2, double eps, const double* out,
                     double kl_mult, double* loss_hist, double* kl_hist) {
    CHECK_H(h);
    if (n < 1 || !u || !c || !g || !m || !v || !trainable || !transform || !step || !lr_sched || !out)
        return MFGP_ERR_ARG;
    return adam_packed_impl(h->stream, n, u, c, g, m, v, trainable, transform, span, step, lr_sched, beta1, beta2, eps,
                            out, kl_mult, loss_hist, kl_hist, nullptr, 0);
}

int mfgp_adam_packed_ex(mfgp_handle_t h, int n, double* u, double* c, const double* g, double* m, double* v,
                        const unsigned char* trainable, const unsigned char* transform, const unsigned char* span,
                        int* step, const double* lr_sched, double beta1, double beta2, double eps,
                        const double* out, double kl_mult, double* loss_hist, double* kl_hist, const int* info,
                        int ninfo) {
    CHECK_H(h);
    if (n < 1 || !u || !c || !g || !m || !v || !trainable || !transform || !step || !lr_sched || !out || ninfo < 0 ||
        (ninfo > 0 && !info))
        return MFGP_ERR_ARG;
    return adam_packed_impl(h->stream, n, u, c, g, m, v, trainable, transform, span, step, lr_sched, beta1, beta2, eps,
                            out, kl_mult, loss_hist, kl_hist, info, ninfo);
}

int mfgp_svgp_predict(mfgp_handle_t h, int nstar, int m, int l, int p, int d, const double* Xs, int ldxs,
                      const double* Z, int ldz, const double* thetas, const double* q_mu, const double* q_sqrt,
                      const double* W, double jitter, void* ws, size_t ws_bytes, double* g_mu, double* g_var,
                      double* f_mu, double* f_var, int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar < 1 || m < 1 || l < 1 || p < 1 || !Xs || !Z || !thetas || !q_mu || !q_sqrt || !ws || !g_mu ||
        !g_var || !f_mu || !f_var || !info)
        return MFGP_ERR_ARG;
    if (!W && l != p) return MFGP_ERR_ARG;
    const SvgpProblem P{nstar, m, l, p, d, Xs, ldxs, nullptr, 0, Z, ldz, thetas, q_mu, q_sqrt, 0, W, 1.0, 1.0, jitter,
                        ws, ws_bytes, info};
    return svgp_predict_impl(h->nb, svgp_streams(h), P, SvgpFwdOut{nullptr, g_mu, g_var, f_mu, f_var});
}

int mfgp_svgp_predict_cov_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar < 1 || m < 1 || l < 1 || p < 1 || !bytes) return MFGP_ERR_ARG;
    *bytes = svgp_predict_cov_workspace_bytes(h->nb, nstar, m, l, p, d);
    return MFGP_OK;
}

int mfgp_svgp_predict_cov(mfgp_handle_t h, int mode, int nstar, int m, int l, int p, int d, const double* Xs,
                          int ldxs, const double* Z, int ldz, const double* thetas, const double* q_mu,
                          const double* q_sqrt, const double* W, double jitter, void* ws, size_t ws_bytes,
                          double* g_mu, double* g_var, double* f_mu, double* f_var, double* f_cov, int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (mode < 1 || mode > 3 || nstar < 1 || m < 1 || l < 1 || p < 1 || !Xs || !Z || !thetas || !q_mu || !q_sqrt ||
        !ws || !g_mu || !g_var || !f_mu || !f_var || !f_cov || !info)
        return MFGP_ERR_ARG;
    if (!W && l != p) return MFGP_ERR_ARG;
    const SvgpProblem P{nstar, m, l, p, d, Xs, ldxs, nullptr, 0, Z, ldz, thetas, q_mu, q_sqrt, 0, W, 1.0, 1.0, jitter,
                        ws, ws_bytes, info};
    const int rc = svgp_predict_cov_impl(h->nb, svgp_streams(h), P, SvgpFwdOut{nullptr, g_mu, g_var, f_mu, f_var},
                                         SvgpCovOut{mode, f_cov});
    return rc == -2 ? MFGP_ERR_WORKSPACE : (rc ? MFGP_ERR_LAUNCH : MFGP_OK);
}

int mfgp_selftest_mfma(mfgp_handle_t h, double* out) {
    CHECK_H(h);
    if (!out) return MFGP_ERR_ARG;
    hipLaunchKernelGGL(k_selftest_mfma, dim3(1), dim3(64), 0, h->stream, out);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

}  // extern "C"
