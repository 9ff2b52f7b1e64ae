// C-ABI entry points of the fp64 GPR / graph-kernel training and predict calls (include/mfgp.h:
// mfgp_gpr_*, mfgp_gmf_gpr_*): the workspace layout, the argument blocks and the launch sequences.
// Host-side orchestration only: no allocation, no synchronisation (every sequence is hipGraph-capturable).
#include <algorithm>

#include "mfgp_device.h"
#include "mfgp_host.h"
#include "mfgp_fence.h"
#include "mfgp_flow.h"

namespace mfgp {

// The persistent Cholesky needs every workgroup resident (one per CU) and the owner table
// to hold every tile; otherwise the launch-per-step sequence runs.
static int flow_grid(int nb, int T, int Tp, int flow_wgs, int min_t) {
    if (nb != 32 || flow_wgs < 2 || T > 255 || T < min_t) return 0;
    if (flow_ntiles(T, Tp) > FLOW_WAVES * (flow_wgs - 1) * FLOW_MAXOWN) return 0;
    return flow_wgs;
}

GprLayout gpr_layout(int nb, const GprProblem& P, const GprSched& sc) {
    GprLayout L;
    L.nb = nb;
    L.T = ceil_div(P.n, nb);
    L.npad = L.T * nb;
    L.Tp = ceil_div(P.p > 0 ? P.p : 1, nb);
    L.ppad = L.Tp * nb;
    L.G = kernel_theta_size(P.nlf, P.d);
    L.gstride = (L.G + 3) & ~3;
    L.flow_wgs = flow_grid(nb, L.T, L.Tp, sc.flow_wgs, sc.flow_min_t);
    L.gchunk = sc.grad_chunk;
    L.ng = grad_tasks(L.T, L.gchunk);
    Carve c(P.ws);
    const size_t ldr = (size_t)L.npad + L.ppad;
    L.A = c.take<double>((size_t)L.npad * L.npad);
    L.R = c.take<double>((size_t)L.npad * ldr);
    L.Xo = c.take<double>((size_t)(L.npad + 2 * L.ppad) * ldr);   // + alpha^T rows (k_grad)
    L.Dd = c.take<double>((size_t)L.T * nb * nb);
    L.ldiag = c.take<double>(L.npad);
    L.alpha = c.take<double>((size_t)L.npad * L.ppad);
    L.zpart = c.take<double>((size_t)L.T * L.Tp);
    L.gpart = c.take<double>((size_t)L.ng * L.gstride);
    L.items = c.take<double>((size_t)L.G + 8);
    L.ncnt = 1;
    L.cnt = c.take<int>((size_t)L.ncnt);
    L.gorder = c.take<int>((size_t)L.ng + SCHED_KEY);
    L.nflags = L.flow_wgs ? flow_nflags(L.T, L.Tp) : 0;
    L.flags = c.take<int>((size_t)L.nflags * FLOW_FSTRIDE);
    L.npub = L.flow_wgs ? flow_npub(L.T, L.Tp) : 0;
    L.pub = c.take<double>((size_t)L.npub);
    L.own = c.take<int>(L.flow_wgs ? (size_t)FLOW_WAVES * (L.flow_wgs - 1) * FLOW_MAXOWN + SCHED_KEY : 0);
    L.ntrace = L.flow_wgs ? flow_trace_count(L.T, L.flow_wgs) : 0;
    L.trace = c.take<long long>((size_t)L.ntrace);
    L.bytes = c.off + 256;
    return L;
}

// k_gram (LML layout) with more lower tiles than CUs: one workgroup per CU, tile (0,0) and its
// fused factor alone on workgroup 0 (beside two other tile workgroups it took ~2x as long, and
// it is the launch's tail), the rest looping over the other tiles.  0: one tile per workgroup.
static int gram_tile_wgs(mfgp_handle_t h, int T, int extra) {
    const int nt = T * (T + 1) / 2;
    if (h->gram_wgs < 0) return 0;
    const int wgs = (h->gram_wgs > 0 ? h->gram_wgs : h->ncu) - extra;
    return (wgs > 1 && nt > wgs) ? wgs : 0;
}

// ---------------------------------------------------------------- argument blocks of one call on the layout L
// The LML-layout Gram: K + s2 I lower tiles into L.A, [I | Y] into L.R, tile (0,0) factored.  cnt, isent,
// gorder and the flow tables stay unset (the launch then skips that work): prep_args adds them.
static GramArgs gram_lml_args(const GprLayout& L, const GprProblem& P) {
    GramArgs g{};
    g.R = L.R; g.ldr = (long)L.npad + L.ppad; g.sR = 0; g.Y = P.Y; g.ldy = P.ldy; g.sY = 0; g.p = P.p; g.ppad = L.ppad;
    g.X1 = P.X; g.ldx1 = P.ldx; g.sx1 = 0; g.n1 = P.n;
    g.X2 = P.X; g.ldx2 = P.ldx; g.sx2 = 0; g.n2 = P.n;
    g.theta = P.theta; g.stheta = 0; g.D = P.d; g.rbf_only = 0;
    g.out = L.A; g.ldo = L.npad; g.so = 0;
    g.padded = 1; g.npad = L.npad; g.tiles_c = L.T; g.add_noise = 1; g.diag_add = P.nlf ? GRAPH_JITTER : 0.0;
    g.Dd = L.Dd; g.sD = 0; g.ldiag = L.ldiag; g.sL = 0; g.info = P.info; g.nlf = P.nlf;
    return g;
}
// the set-up launch in front of an AR1 flow evaluation (sentinel fill, schedule tables, item slots)
static GramArgs prep_args(const GprLayout& L, const GprProblem& P, bool order) {
    GramArgs g = gram_lml_args(L, P);
    g.cnt = L.cnt; g.ncnt = L.ncnt;
    if (MFGP_REDUCE_FLAG) { g.isent = L.items; g.nisent = L.G + 2; }
    if (order) { g.gorder = L.gorder; g.gT = L.T; g.gchunk = L.gchunk; g.gTp = L.Tp; }
    if (L.flow_wgs) { g.fown = L.own; g.fW = FLOW_WAVES * (L.flow_wgs - 1); g.fflags = L.flags; g.nfflags = L.nflags; g.fpub = L.pub; g.npub = L.npub; }
    return g;
}
// the launch-per-step factorization; with_alpha: also alpha = L^{-T} Z and the sum Z^2 partials
static CholArgs chol_args(const GprLayout& L, const GprProblem& P, bool with_alpha) {
    const long ldr = L.npad + L.ppad;
    CholArgs c{};
    c.A = L.A; c.lda = L.npad; c.sA = 0;
    c.R = L.R; c.ldr = ldr; c.sR = 0;
    c.Xo = L.Xo; c.ldx = ldr; c.sX = 0;
    c.Dd = L.Dd; c.sD = 0; c.ldiag = L.ldiag; c.sL = 0; c.info = P.info;
    c.T = L.T; c.Tp = L.Tp; c.k = 0;
    if (with_alpha) { c.alpha = L.alpha; c.ldal = L.ppad; c.zpart = L.zpart; c.n = P.n; c.p = P.p; }
    return c;
}
static FlowArgs flow_args(mfgp_handle_t h, const GprLayout& L, const GprProblem& P, bool flow_gram) {
    const long ldr = L.npad + L.ppad;
    FlowArgs fa{};
    fa.A = L.A; fa.lda = L.npad;
    fa.R = L.R; fa.ldr = ldr;
    fa.Xo = L.Xo; fa.ldx = ldr;
    fa.Dd = L.Dd; fa.ldiag = L.ldiag; fa.info = P.info;
    fa.alpha = L.alpha; fa.ldal = L.ppad; fa.zpart = L.zpart;
    fa.flags = L.flags; fa.own = L.own; fa.pub = L.pub;
    fa.T = L.T; fa.Tp = L.Tp; fa.n = P.n; fa.p = P.p;
    fa.trace = h->flow_trace ? L.trace : nullptr;
    fa.nwaves = FLOW_WAVES * (L.flow_wgs - 1);
    fa.timeout = h->flow_timeout;
    fa.X = P.X; fa.ldxi = P.ldx; fa.Y = P.Y; fa.ldy = P.ldy; fa.theta = P.theta; fa.D = P.d;
    fa.gram = flow_gram ? 1 : 0;
    return fa;
}
static GradArgs grad_args(const GprLayout& L, const GprProblem& P, bool leaves_setup) {
    GradArgs ga{L.Xo, (long)L.npad + L.ppad, P.X, (long)P.ldx, P.theta, L.gpart, L.gstride, L.T, L.Tp, P.n, P.p, P.d,
                L.gchunk, P.nlf, L.gchunk + L.T + L.Tp < 2048 ? L.gorder : nullptr};
    if (leaves_setup) {   // the next evaluation's set-up, after the flow
        ga.fpub = L.pub; ga.npub = L.npub;
        ga.isent = L.items; ga.nisent = L.G + 2;
    }
    return ga;
}
static FinArgs fin_args(const GprLayout& L, const GprProblem& P, int want_grad, double* out, const FinArgs* adam) {
    FinArgs f = fin_eval(P, L.G, want_grad, out, adam);
    f.zpart = L.zpart; f.nz = L.T * L.Tp;
    f.ldiag = L.ldiag;
    f.gpart = L.gpart; f.ng = L.ng; f.gstride = L.gstride;
    f.items = L.items;
    f.cnt = L.cnt;
    f.flag = MFGP_REDUCE_FLAG;   // the Gram / set-up launch (or the previous k_grad) filled items[] with the sentinel
    f.abortw = L.flow_wgs ? L.flags : nullptr;
    return f;
}

template <int NB>
static void gram_lml_and_factor(hipStream_t s, const GprLayout& L, const GprProblem& P) {
    launch_gram<NB>(gram_lml_args(L, P), L.T * (L.T + 1) / 2, 1, s);
    launch_chol_steps<NB>(chol_args(L, P, false), 1, s);
}
void gpr_factor(int nb, hipStream_t s, const GprLayout& L, const GprProblem& P) {
    TILE_CALL(nb, gram_lml_and_factor, s, L, P);
}

// Resident mode: whether the previous fp64 LML call on this handle left the workspace of P set up for
// the same problem (k_grad's tail), and the record a call that does so leaves.
static bool res_matches(mfgp_handle_t h, const GprLayout& L, const GprProblem& P) {
    return h->resident && h->res.ws == P.ws && h->res.n == P.n && h->res.p == P.p && h->res.d == P.d &&
           h->res.flow_wgs == L.flow_wgs;
}
static void res_record(mfgp_handle_t h, const GprLayout& L, const GprProblem& P) {
    h->res.ws = P.ws; h->res.n = P.n; h->res.p = P.p; h->res.d = P.d; h->res.flow_wgs = L.flow_wgs;
}

// Optional per-phase event marks (diagnostic timing; never used on the hot path).
struct PhaseMarks {
    hipEvent_t ev[8];
    int count = 0;
    void mark(hipStream_t s) { (void)hipEventRecord(ev[count++], s); }
};

template <int NB>
static int gpr_value_grad(mfgp_handle_t h, const GprProblem& P, int want_grad, double* out, const FinArgs* adam,
                          PhaseMarks* pm) {
    const GprLayout L = gpr_layout(NB, P, gpr_sched(h));
    if (P.ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    if (L.G > FIN_MAXG) return MFGP_ERR_ARG;   // finalize_body stages theta in LDS
    hipStream_t s = h->stream;
    if (pm) pm->mark(s);
    if (NB == 32 && h->tiny && gpr_tiny_fits(P.n, P.p, P.d, P.nlf)) {   // the whole step in one workgroup
        const FinArgs f = fin_eval(P, L.G, want_grad, out, adam);    // no partial sums: no items / cnt / flag
        if (pm) pm->mark(s);
        launch_gpr_tiny(P.X, P.ldx, P.Y, P.ldy, P.theta, P.n, P.p, P.d, want_grad, P.info, f, s);
        if (pm) { pm->mark(s); pm->mark(s); pm->mark(s); }
        return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
    }
    if (pm) pm->mark(s);
    // the flow fence before any launch of the sequence: a fence held past its bound by another
    // host thread fails the call with nothing enqueued; once past it, the flow is always recorded
    FenceTurn fence(L.flow_wgs ? h->device : -1, s);
    if (fence.rc != MFGP_OK) return fence.rc;
    // The AR1 flow path (NB = 32, nlf = 0): the Gram is formed inside k_chol_flow, so the launch
    // in front of it only sets up the workspace (sentinel fill, schedule tables, item slots) --
    // and a value+grad call leaves exactly that set-up behind (k_grad's tail).  In resident mode
    // a value+grad call whose workspace the previous fp64 LML call on this handle left set up for
    // the same problem starts with the flow itself.
    const bool flow_gram = NB == 32 && L.flow_wgs && !P.nlf;
    const bool leaves_setup = flow_gram && want_grad;
    const bool skip_prep = leaves_setup && res_matches(h, L, P);
    h->res.ws = nullptr;
    if (!skip_prep) {
        const bool order = want_grad && L.gchunk + L.T + L.Tp < 2048;   // gram LDS holds the histogram
        GramArgs g = prep_args(L, P, order);
        const int extra = (order ? 1 : 0) + (L.flow_wgs ? 1 : 0);
        if (flow_gram) {
            launch_flow_prep(g, std::max(h->ncu, 2) + extra, s);
        } else {
            if (L.flow_wgs) g.Dd = nullptr;   // the flow factors D_0 itself
            g.tile_wgs = gram_tile_wgs(h, L.T, extra);
            launch_gram<NB>(g, (g.tile_wgs ? g.tile_wgs : L.T * (L.T + 1) / 2) + extra, 1, s);
        }
    }
    if (pm) pm->mark(s);
    if (L.flow_wgs) {
        launch_chol_flow(flow_args(h, L, P, flow_gram), L.flow_wgs, s);
        fence.commit(s);
    } else {
        launch_chol_steps<NB>(chol_args(L, P, true), 1, s);
    }
    if (pm) pm->mark(s);
    if (want_grad) launch_grad<NB>(grad_args(L, P, leaves_setup), s);
    if (pm) pm->mark(s);
    const FinArgs f = fin_args(L, P, want_grad, out, adam);
    hipLaunchKernelGGL(k_reduce_items, dim3(2 + (want_grad ? L.G : 0)), dim3(NTHREADS), 0, s, f);
    if (pm) pm->mark(s);
    if (last() != hipSuccess) return MFGP_ERR_LAUNCH;
    if (leaves_setup) res_record(h, L, P);
    return MFGP_OK;
}

// Whether mfgp_gpr_adam_steps may defer the step reduction into the next flow launch: only where
// the flow forms its own Gram (the AR1 kernel, 32-tiles, the flow on and taken at this size, not
// the one-launch tiny path) and one wave holds every item (flow_head_diag).
static bool adam_steps_fusable(mfgp_handle_t h, const GprProblem& P) {
    if (!h->step_fusion || h->nb != 32 || !MFGP_REDUCE_FLAG) return false;
    if (h->tiny && gpr_tiny_fits(P.n, P.p, P.d, 0)) return false;
    const GprLayout L = gpr_layout(32, P, gpr_sched(h));
    return L.flow_wgs != 0 && L.G <= FLOW_HEAD_MAXG;
}

// nsteps Adam steps as [set-up if not resident] flow, grad, flow*, grad, ..., flow*, grad,
// k_reduce_items: flow* (FlowArgs::head) finishes the previous step in its head phase, so only the
// last step pays for the reduction launch.  The fence is taken once; h->res is left as after a
// single step.  Bitwise the results of nsteps mfgp_gpr_adam_step calls.
static int gpr_adam_steps_fused(mfgp_handle_t h, const GprProblem& P, double* out, const FinArgs* adam, int nsteps) {
    const GprLayout L = gpr_layout(32, P, gpr_sched(h));
    if (P.ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    FenceTurn fence(h->device, s);
    if (fence.rc != MFGP_OK) return fence.rc;
    const bool skip_prep = res_matches(h, L, P);
    h->res.ws = nullptr;
    if (!skip_prep) {
        const bool order = L.gchunk + L.T + L.Tp < 2048;
        launch_flow_prep(prep_args(L, P, order), std::max(h->ncu, 2) + (order ? 1 : 0) + 1, s);
    }
    const FinArgs f = fin_args(L, P, 1, out, adam);
    FlowArgs fa = flow_args(h, L, P, true);
    const GradArgs ga = grad_args(L, P, true);
    for (int t = 0; t < nsteps; ++t) {
        fa.head = t > 0;
        if (fa.head) fa.fin = f;
        launch_chol_flow(fa, L.flow_wgs, s);
        if (t == nsteps - 1) fence.commit(s);
        launch_grad<32>(ga, s);
    }
    hipLaunchKernelGGL(k_reduce_items, dim3(2 + L.G), dim3(NTHREADS), 0, s, f);
    if (last() != hipSuccess) return MFGP_ERR_LAUNCH;
    res_record(h, L, P);
    return MFGP_OK;
}

// ---------------------------------------------------------------- predict
struct PredLayout {
    GprLayout g;
    int nspad, Ts;
    double *Kmn, *Am, *kdiag;
    double *Kss, *Cov;   // full_cov only: K(X*, X*) and Kss - A^T A (nspad x nspad)
    size_t bytes;
};

static PredLayout pred_layout(mfgp_handle_t h, const GprProblem& P, int nstar, bool full_cov) {
    const int nb = h->nb;
    PredLayout PL;
    PL.g = gpr_layout(nb, P, gpr_sched_no_flow(h));
    PL.Ts = ceil_div(nstar > 0 ? nstar : 1, nb);
    PL.nspad = PL.Ts * nb;
    Carve c(P.ws);
    c.off = PL.g.bytes;
    PL.Kmn = c.take<double>((size_t)PL.g.npad * PL.nspad);
    PL.Am = c.take<double>((size_t)PL.g.npad * PL.nspad);
    PL.kdiag = c.take<double>(PL.nspad);
    const size_t sq = full_cov ? (size_t)PL.nspad * PL.nspad : 0;
    PL.Kss = c.take<double>(sq);
    PL.Cov = c.take<double>(sq);
    PL.bytes = c.off + 256;
    return PL;
}

template <int NB>
static int predict_impl(mfgp_handle_t h, const GprProblem& P, const GprPredictIO& io) {
    const PredLayout PL = pred_layout(h, P, io.nstar, io.cov != nullptr);
    if (P.ws_bytes < PL.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    if (NB == 32 && h->tiny && !P.nlf && !io.cov && gpr_tiny_pred_fits(P.n, P.p, P.d, io.nstar)) {   // small problems: one launch
        launch_gpr_tiny_pred(P.X, P.ldx, P.Y, P.ldy, io.Xs, io.ldxs, io.nstar, P.theta, P.n, P.p, P.d, io.mean, io.ldm,
                             io.var, P.info, s);
        return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
    }
    const GprLayout& L = PL.g;
    gram_lml_and_factor<NB>(s, L, P);
    if (P.nlf) (void)hipMemsetAsync(PL.Kmn, 0, sizeof(double) * (size_t)L.npad * PL.nspad, s);
    GramArgs g{};
    g.X1 = P.X; g.ldx1 = P.ldx; g.n1 = P.n;
    g.X2 = io.Xs; g.ldx2 = io.ldxs; g.n2 = io.nstar;
    g.theta = P.theta; g.D = P.d; g.rbf_only = 0;
    g.out = PL.Kmn; g.ldo = PL.nspad; g.padded = 0; g.tiles_c = PL.Ts; g.diag_add = 0.0; g.nlf = P.nlf;
    if (P.nlf) launch_gram<NB>(g, L.T * PL.Ts, 1, s);
    else launch_gram_dense(g, 1, L.npad, PL.nspad, s);   // zero padding written by the kernel
    hipLaunchKernelGGL(k_kdiag, dim3(ceil_div(io.nstar, 256)), dim3(256), 0, s, io.Xs, (long)io.ldxs, io.nstar, P.d,
                       P.theta, PL.kdiag, P.nlf);
    const long ldr = L.npad + L.ppad;
    PredAArgs pa{L.Xo, ldr, PL.Kmn, (long)PL.nspad, PL.Am, (long)PL.nspad, PL.Ts};
    PredOutArgs po{PL.Am, (long)PL.nspad, L.Xo, ldr, PL.kdiag, io.mean, (long)io.ldm, io.var, L.T, L.Tp, io.nstar, P.p};
    launch_pred<NB>(pa, po, L.T, s);
    if (io.cov)
        cov_from_a<NB>(s, io.Xs, io.ldxs, io.nstar, P.theta, P.d, P.nlf, PL.Am, PL.nspad, L.T, PL.Kss, PL.Cov, io.cov,
                       io.ldc);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

// The entries below differ in whether they take nlf (the graph kernel: 1..MFGP_MAX_LF; predict_cov:
// 0..MFGP_MAX_LF) and a covariance block; each fills the descriptors and calls one of these.
static int workspace_size(mfgp_handle_t h, int nlf, int lf_min, int n, int p, int d, size_t* bytes) {
    if (const int rc = gpr_check_dims(h, n, p, d, nlf, lf_min, bytes != nullptr)) return rc;
    *bytes = gpr_layout(h->nb, GprProblem{n, p, d, nlf}, gpr_sched(h)).bytes;
    return MFGP_OK;
}
static int predict_workspace_size(mfgp_handle_t h, int nlf, int lf_min, int n, int p, int d, int nstar, bool full_cov,
                                  size_t* bytes) {
    if (const int rc = gpr_check_dims(h, n, p, d, nlf, lf_min, nstar >= 0 && bytes)) return rc;
    *bytes = pred_layout(h, GprProblem{n, p, d, nlf}, nstar, full_cov).bytes;
    return MFGP_OK;
}
static int lml(mfgp_handle_t h, const GprProblem& P, int lf_min, int want_grad, double* out) {
    if (const int rc = gpr_check(h, P, lf_min, out != nullptr)) return rc;
    return TILE_CALL(h->nb, gpr_value_grad, h, P, want_grad, out, nullptr, nullptr);
}
static int predict(mfgp_handle_t h, const GprProblem& P, int lf_min, const GprPredictIO& io, bool want_cov) {
    if (const int rc = gpr_check(h, P, lf_min, io.nstar >= 0)) return rc;
    if (io.nstar == 0) return MFGP_OK;
    if (!gpr_predict_io_ok(io, want_cov)) return MFGP_ERR_ARG;
    return TILE_CALL(h->nb, predict_impl, h, P, io);
}

}  // namespace mfgp

using namespace mfgp;

extern "C" {

int mfgp_gpr_flow_trace(mfgp_handle_t h, int n, int p, int d, size_t* offset, int* count) {
    if (const int rc = gpr_check_dims(h, n, p, d, 0, 0, offset && count)) return rc;
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);   // any 256-B aligned stand-in
    GprProblem P{n, p, d, 0};
    P.ws = base;
    const GprLayout L = gpr_layout(h->nb, P, gpr_sched(h));
    *offset = (size_t)(reinterpret_cast<char*>(L.trace) - base);
    *count = L.ntrace;
    return MFGP_OK;
}

// ---------------------------------------------------------------- graph kernel (graph.py)
int mfgp_gmf_gpr_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, size_t* bytes) {
    return workspace_size(h, nlf, 1, n, p, d, bytes);
}

int mfgp_gmf_gpr_lml(mfgp_handle_t h, int nlf, int n, int p, int d, const double* X, int ldx, const double* Y,
                     int ldy, const double* theta, int want_grad, void* ws, size_t ws_bytes, double* out, int* info) {
    return lml(h, GprProblem{n, p, d, nlf, X, ldx, Y, ldy, theta, ws, ws_bytes, info}, 1, want_grad, out);
}

int mfgp_gmf_gpr_predict_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, size_t* bytes) {
    return predict_workspace_size(h, nlf, 1, n, p, d, nstar, false, bytes);
}

int mfgp_gmf_gpr_predict(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const double* X, int ldx,
                         const double* Y, int ldy, const double* Xs, int ldxs, const double* theta, void* ws,
                         size_t ws_bytes, double* mean, int ldm, double* var, int* info) {
    return predict(h, GprProblem{n, p, d, nlf, X, ldx, Y, ldy, theta, ws, ws_bytes, info}, 1,
                   GprPredictIO{nstar, Xs, ldxs, mean, ldm, var, nullptr, 0}, false);
}

// ---------------------------------------------------------------- linear multi-fidelity kernel
int mfgp_gpr_workspace_size(mfgp_handle_t h, int n, int p, int d, size_t* bytes) {
    return workspace_size(h, 0, 0, n, p, d, bytes);
}

int mfgp_gpr_lml(mfgp_handle_t h, int n, int p, int d, const double* X, int ldx, const double* Y, int ldy,
                 const double* theta, int want_grad, void* ws, size_t ws_bytes, double* out, int* info) {
    return lml(h, GprProblem{n, p, d, 0, X, ldx, Y, ldy, theta, ws, ws_bytes, info}, 0, want_grad, out);
}

int mfgp_gpr_adam_step(mfgp_handle_t h, int n, int p, int d, const double* X, int ldx, const double* Y, int ldy,
                       double* theta, double* u, double* m, double* v, const unsigned char* trainable,
                       const int* tie, int* step, double lr, double beta1, double beta2, double eps,
                       double* loss_hist, void* ws, size_t ws_bytes, double* out, int* info) {
    return mfgp_gpr_adam_steps(h, n, p, d, X, ldx, Y, ldy, theta, u, m, v, trainable, tie, step, lr, beta1, beta2, eps,
                               loss_hist, ws, ws_bytes, out, info, 1);
}

int mfgp_gpr_adam_steps(mfgp_handle_t h, int n, int p, int d, const double* X, int ldx, const double* Y, int ldy,
                        double* theta, double* u, double* m, double* v, const unsigned char* trainable,
                        const int* tie, int* step, double lr, double beta1, double beta2, double eps,
                        double* loss_hist, void* ws, size_t ws_bytes, double* out, int* info, int nsteps) {
    const GprProblem P{n, p, d, 0, X, ldx, Y, ldy, theta, ws, ws_bytes, info};
    if (const int rc = gpr_check(h, P, 0, nsteps >= 0 && u && m && v && trainable && step && loss_hist && out))
        return rc;
    const FinArgs f = adam_fin(d, theta, u, m, v, trainable, tie, step, lr, beta1, beta2, eps, loss_hist);
    if (nsteps > 1 && adam_steps_fusable(h, P)) return gpr_adam_steps_fused(h, P, out, &f, nsteps);
    for (int t = 0; t < nsteps; ++t) {   // the plain loop of single steps
        const int rc = TILE_CALL(h->nb, gpr_value_grad, h, P, 1, out, &f, nullptr);
        if (rc != MFGP_OK) return rc;
    }
    return MFGP_OK;
}

int mfgp_gpr_lml_phase_times(mfgp_handle_t h, int n, int p, int d, const double* X, int ldx, const double* Y,
                             int ldy, const double* theta, void* ws, size_t ws_bytes, double* out, int* info,
                             float* ms) {
    const GprProblem P{n, p, d, 0, X, ldx, Y, ldy, theta, ws, ws_bytes, info};
    if (const int rc = gpr_check(h, P, 0, out && ms)) return rc;
    PhaseMarks pm;
    for (int i = 0; i < 6; ++i) (void)hipEventCreate(&pm.ev[i]);
    int rc = TILE_CALL(h->nb, gpr_value_grad, h, P, 1, out, nullptr, &pm);
    if (rc == MFGP_OK) {
        (void)hipEventSynchronize(pm.ev[pm.count - 1]);
        for (int i = 0; i + 1 < pm.count; ++i) (void)hipEventElapsedTime(&ms[i], pm.ev[i], pm.ev[i + 1]);
    }
    for (int i = 0; i < 6; ++i) (void)hipEventDestroy(pm.ev[i]);
    return rc;
}

int mfgp_gpr_predict_workspace_size(mfgp_handle_t h, int n, int p, int d, int nstar, size_t* bytes) {
    return predict_workspace_size(h, 0, 0, n, p, d, nstar, false, bytes);
}

int mfgp_gpr_predict(mfgp_handle_t h, int n, int p, int d, int nstar, const double* X, int ldx, const double* Y,
                     int ldy, const double* Xs, int ldxs, const double* theta, void* ws, size_t ws_bytes,
                     double* mean, int ldm, double* var, int* info) {
    return predict(h, GprProblem{n, p, d, 0, X, ldx, Y, ldy, theta, ws, ws_bytes, info}, 0,
                   GprPredictIO{nstar, Xs, ldxs, mean, ldm, var, nullptr, 0}, false);
}

int mfgp_gpr_predict_cov_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, size_t* bytes) {
    return predict_workspace_size(h, nlf, 0, n, p, d, nstar, true, bytes);
}

int mfgp_gpr_predict_cov(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const double* X, int ldx,
                         const double* Y, int ldy, const double* Xs, int ldxs, const double* theta, void* ws,
                         size_t ws_bytes, double* mean, int ldm, double* var, double* cov, int ldc, int* info) {
    return predict(h, GprProblem{n, p, d, nlf, X, ldx, Y, ldy, theta, ws, ws_bytes, info}, 0,
                   GprPredictIO{nstar, Xs, ldxs, mean, ldm, var, cov, ldc}, true);
}

}  // extern "C"
