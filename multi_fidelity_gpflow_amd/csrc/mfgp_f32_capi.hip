// C-ABI entry points of the fp32 GPR path (mfgp_f32.hip) and the dtype-generic *_ex forms (include/mfgp.h):
// the fp32 workspace layout, the two fp32 drivers and the fp32 settings.  The fp64 arm of an *_ex entry is
// the public fp64 entry of the same name.  Host-side orchestration only: no allocation, no synchronisation.
#include <algorithm>

#include "mfgp_device.h"
#include "mfgp_host.h"

namespace mfgp {

using F32Problem = GprProblemT<float>;
using F32PredictIO = GprPredictIOT<float>;

struct F32Layout {
    F32Args a;
    F32Refine r;
    double* items;
    int ntask, G;
    size_t bytes;
};

// ns > 0: predict rows; want_grad: identity rows + alpha + gradient partials; refine (value-only /
// predict): L^T tiles, fp32 work rows, fp64 alpha and residual (mfgp_set_f32_refine)
static F32Layout f32_layout(int n, int p, int d, int ns, int want_grad, int panel, void* ws, int refine = 0) {
    F32Layout L{};
    F32Args& a = L.a;
    const int TB = F32_TILE;
    a.T = ceil_div(n, TB);
    a.Tp = ceil_div(p, TB);
    a.Ts = ns > 0 ? ceil_div(ns, TB) : 0;
    a.Ti = want_grad ? a.T : 0;
    a.W = panel;
    a.ld = (long)a.T * TB;
    a.n = n; a.p = p; a.ns = ns; a.D = d;
    Carve c(ws);
    a.M = c.take<float>((size_t)(a.T + a.Tp + a.Ts + a.Ti) * TB * a.ld);
    a.Dd = c.take<float>((size_t)a.T * TB * TB);
    a.ldiag = c.take<double>((size_t)a.T * TB);
    a.ldal = (long)a.Tp * TB;
    a.alpha = c.take<float>(want_grad ? (size_t)a.ld * a.ldal : 0);
    a.nz = 256;
    a.zpart = c.take<double>((size_t)a.nz);
    L.ntask = a.T * (a.T + 1) / 2;
    L.G = theta_size(d);
    a.gpart = c.take<double>(want_grad ? (size_t)L.G * L.ntask : 0);
    L.items = c.take<double>((size_t)L.G + 8);
    a.cnt = c.take<int>(1);
    if (refine && !want_grad) {
        a.LT = c.take<float>((size_t)a.T * TB * a.ld);
        L.r.XB = c.take<float>((size_t)a.Tp * TB * a.ld);
        L.r.ld64 = (long)ceil_div(a.Tp * TB, 256) * 256;   // k64_kmat reads 256-column blocks
        L.r.A64 = c.take<double>((size_t)a.ld * L.r.ld64);
        L.r.R64 = c.take<double>((size_t)a.ld * L.r.ld64);
    }
    L.bytes = c.off + 256;
    return L;
}

// The problem into the layout's argument block, then the factorization sweep (with the handle's
// look-ahead: the next panel on the side stream beside the capped trailing update).
static void f32_sweep(mfgp_handle_t h, F32Args& a, const F32Problem& P, F32Marks* mk) {
    a.info = P.info; a.X = P.X; a.ldx = P.ldx; a.Y = P.Y; a.ldy = P.ldy; a.theta = P.theta;
    a.upd_slots = (h->f32_reserve > 0 && h->ncu > h->f32_reserve) ? 2 * (h->ncu - h->f32_reserve) : 0;
    if (h->f32_lookahead) launch_f32_sweep(a, h->stream, mk, h->side, h->ev_fork, h->ev_join);
    else launch_f32_sweep(a, h->stream, mk);
}

static int f32_value_grad(mfgp_handle_t h, const F32Problem& P, int want_grad, double* out, const FinArgs* adam,
                          F32Marks* mk) {
    const int refine = h->f32_refine && !want_grad && !adam && !mk;
    F32Layout L = f32_layout(P.n, P.p, P.d, 0, want_grad, h->f32_panel, P.ws, refine);
    if (P.ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    F32Args& a = L.a;
    f32_sweep(h, a, P, mk);
    if (want_grad) launch_f32_grad(a, s, mk);
    if (mk) mk->begin(s, F32_FIN);
    if (refine) launch_f32_refine_lml(a, L.r, s);   // q = Y.a0 + a0.R + |L~^-1 R|^2 partials into zpart
    else launch_f32_zsum(a, s);
    FinArgs f = fin_eval(P, L.G, want_grad, out, adam);
    f.zpart = a.zpart; f.nz = a.nz;
    f.ldiag = a.ldiag;
    f.gpart = a.gpart; f.ng = L.ntask; f.gstride = 0;   // [G][ntask] partials
    f.items = L.items;
    f.cnt = a.cnt;                                      // the arrival counter: no sentinel flag, no abort word
    hipLaunchKernelGGL(k_reduce_items, dim3(2 + (want_grad ? L.G : 0)), dim3(NTHREADS), 0, s, f);
    if (mk) mk->end(s, 0.0);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

static int f32_predict(mfgp_handle_t h, const F32Problem& P, const F32PredictIO& io) {
    F32Layout L = f32_layout(P.n, P.p, P.d, io.nstar, 0, h->f32_panel, P.ws, h->f32_refine);
    if (P.ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    F32Args& a = L.a;
    a.Xs = io.Xs; a.ldxs = io.ldxs;
    f32_sweep(h, a, P, nullptr);
    launch_f32_predict(a, io.mean, io.ldm, io.var, h->stream);   // variance (and the unrefined mean)
    if (h->f32_refine) launch_f32_refine_mean(a, L.r, io.mean, io.ldm, h->f32_refine, h->stream);
    if (io.cov) launch_f32_predict_cov(a, io.cov, io.ldc, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

static F32Problem f32_problem(int n, int p, int d, const void* X, int ldx, const void* Y, int ldy, const double* theta,
                              void* ws, size_t ws_bytes, int* info) {
    return F32Problem{n, p, d, 0, (const float*)X, ldx, (const float*)Y, ldy, theta, ws, ws_bytes, info};
}
static bool f32_ld_ok(const F32Problem& P) { return P.ldx >= P.d + 1 && P.ldy >= P.p; }

// the fp32 arm of mfgp_gpr_predict_ex / mfgp_gpr_predict_cov_ex
static int f32_predict_entry(mfgp_handle_t h, const F32Problem& P, const F32PredictIO& io, bool want_cov) {
    if (const int rc = gpr_check(h, P, 0, io.nstar >= 0)) return rc;
    if (io.nstar == 0) return MFGP_OK;
    if (!gpr_predict_io_ok(io, want_cov) || !f32_ld_ok(P) || io.ldxs < P.d + 1 || io.ldm < P.p) return MFGP_ERR_ARG;
    return f32_predict(h, P, io);
}

}  // namespace mfgp

using namespace mfgp;

extern "C" {

#define CHECK_DT(dt) \
    if ((dt) != MFGP_F64 && (dt) != MFGP_F32) return MFGP_ERR_ARG
// handle, d and dtype of a dtype-generic entry, in this order
#define CHECK_EX(h, d, dt) \
    CHECK_H(h);            \
    CHECK_D(d);            \
    CHECK_DT(dt)

int mfgp_set_f32_refine(mfgp_handle_t h, int enable) {
    CHECK_H(h);
    if (enable < 0 || enable > 2) return MFGP_ERR_ARG;
    h->f32_refine = enable;
    return MFGP_OK;
}

int mfgp_set_f32_panel(mfgp_handle_t h, int tiles) {
    CHECK_H(h);
    if (tiles < 1 || tiles > 64) return MFGP_ERR_ARG;
    h->f32_panel = tiles;
    return MFGP_OK;
}

int mfgp_set_f32_lookahead(mfgp_handle_t h, int enable) {
    CHECK_H(h);
    h->f32_lookahead = enable != 0;
    return MFGP_OK;
}

int mfgp_set_f32_reserve(mfgp_handle_t h, int cus) {
    CHECK_H(h);
    if (cus < 0) return MFGP_ERR_ARG;
    h->f32_reserve = cus;
    return MFGP_OK;
}

int mfgp_mf_gram_ex(mfgp_handle_t h, int dtype, int n1, int n2, int d, const void* X1, int ldx1, const void* X2,
                    int ldx2, const double* theta, double diag_add, void* K, int ldk) {
    CHECK_EX(h, d, dtype);
    if (dtype == MFGP_F64)
        return mfgp_mf_gram(h, n1, n2, d, (const double*)X1, ldx1, (const double*)X2, ldx2, theta, diag_add,
                            (double*)K, ldk);
    if (n1 < 1 || n2 < 1 || !X1 || !X2 || !theta || !K || ldx1 < d + 1 || ldx2 < d + 1 || ldk < n2)
        return MFGP_ERR_ARG;
    launch_f32_gram_dense((const float*)X1, ldx1, n1, (const float*)X2, ldx2, n2, d, theta, (float)diag_add,
                          (float*)K, ldk, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

int mfgp_gpr_workspace_size_ex(mfgp_handle_t h, int dtype, int n, int p, int d, size_t* bytes) {
    CHECK_EX(h, d, dtype);
    if (dtype == MFGP_F64) return mfgp_gpr_workspace_size(h, n, p, d, bytes);
    if (const int rc = gpr_check_dims(h, n, p, d, 0, 0, bytes != nullptr)) return rc;
    *bytes = f32_layout(n, p, d, 0, 1, h->f32_panel, nullptr).bytes;
    if (h->f32_refine) *bytes = std::max(*bytes, f32_layout(n, p, d, 0, 0, h->f32_panel, nullptr, 1).bytes);
    return MFGP_OK;
}

int mfgp_gpr_lml_ex(mfgp_handle_t h, int dtype, int n, int p, int d, const void* X, int ldx, const void* Y, int ldy,
                    const double* theta, int want_grad, void* ws, size_t ws_bytes, double* out, int* info) {
    CHECK_EX(h, d, dtype);
    if (dtype == MFGP_F64)
        return mfgp_gpr_lml(h, n, p, d, (const double*)X, ldx, (const double*)Y, ldy, theta, want_grad, ws, ws_bytes,
                            out, info);
    const F32Problem P = f32_problem(n, p, d, X, ldx, Y, ldy, theta, ws, ws_bytes, info);
    if (const int rc = gpr_check(h, P, 0, out && f32_ld_ok(P))) return rc;
    return f32_value_grad(h, P, want_grad, out, nullptr, nullptr);
}

int mfgp_gpr_adam_step_ex(mfgp_handle_t h, int dtype, int n, int p, int d, const void* X, int ldx, const void* Y,
                          int ldy, double* theta, double* u, double* m, double* v, const unsigned char* trainable,
                          const int* tie, int* step, double lr, double beta1, double beta2, double eps,
                          double* loss_hist, void* ws, size_t ws_bytes, double* out, int* info) {
    CHECK_EX(h, d, dtype);
    if (dtype == MFGP_F64)
        return mfgp_gpr_adam_step(h, n, p, d, (const double*)X, ldx, (const double*)Y, ldy, theta, u, m, v, trainable,
                                  tie, step, lr, beta1, beta2, eps, loss_hist, ws, ws_bytes, out, info);
    const F32Problem P = f32_problem(n, p, d, X, ldx, Y, ldy, theta, ws, ws_bytes, info);
    if (const int rc = gpr_check(h, P, 0, u && m && v && trainable && step && loss_hist && out && f32_ld_ok(P)))
        return rc;
    const FinArgs f = adam_fin(d, theta, u, m, v, trainable, tie, step, lr, beta1, beta2, eps, loss_hist);
    return f32_value_grad(h, P, 1, out, &f, nullptr);
}

int mfgp_gpr_phase_times_ex(mfgp_handle_t h, int dtype, int n, int p, int d, const void* X, int ldx, const void* Y,
                            int ldy, const double* theta, void* ws, size_t ws_bytes, double* out, int* info,
                            float* ms, double* flops, int* launches, int nphase) {
    CHECK_EX(h, d, dtype);
    if (!ms || nphase < 1) return MFGP_ERR_ARG;
    if (dtype == MFGP_F64) {
        float m5[5] = {};
        const int rc = mfgp_gpr_lml_phase_times(h, n, p, d, (const double*)X, ldx, (const double*)Y, ldy, theta, ws,
                                                ws_bytes, out, info, m5);
        for (int i = 0; i < nphase; ++i) {
            ms[i] = i < 5 ? m5[i] : 0.0f;
            if (flops) flops[i] = 0.0;
            if (launches) launches[i] = 0;
        }
        return rc;
    }
    const F32Problem P = f32_problem(n, p, d, X, ldx, Y, ldy, theta, ws, ws_bytes, info);
    if (const int rc = gpr_check(h, P, 0, out != nullptr)) return rc;
    F32Marks* mk = new F32Marks();
    const int rc = f32_value_grad(h, P, 1, out, nullptr, mk);
    float all[F32_NPHASE];
    mk->collect(all);
    for (int i = 0; i < nphase; ++i) {
        ms[i] = i < F32_NPHASE ? all[i] : 0.0f;
        if (flops) flops[i] = i < F32_NPHASE ? mk->flops[i] : 0.0;
        if (launches) launches[i] = i < F32_NPHASE ? mk->launches[i] : 0;
    }
    delete mk;
    return rc;
}

int mfgp_gpr_predict_workspace_size_ex(mfgp_handle_t h, int dtype, int n, int p, int d, int nstar, size_t* bytes) {
    CHECK_EX(h, d, dtype);
    if (dtype == MFGP_F64) return mfgp_gpr_predict_workspace_size(h, n, p, d, nstar, bytes);
    if (const int rc = gpr_check_dims(h, n, p, d, 0, 0, nstar >= 0 && bytes)) return rc;
    *bytes = f32_layout(n, p, d, nstar > 0 ? nstar : 1, 0, h->f32_panel, nullptr, h->f32_refine).bytes;
    return MFGP_OK;
}

int mfgp_gpr_predict_ex(mfgp_handle_t h, int dtype, int n, int p, int d, int nstar, const void* X, int ldx,
                        const void* Y, int ldy, const void* Xs, int ldxs, const double* theta, void* ws,
                        size_t ws_bytes, void* mean, int ldm, void* var, int* info) {
    CHECK_EX(h, d, dtype);
    if (dtype == MFGP_F64)
        return mfgp_gpr_predict(h, n, p, d, nstar, (const double*)X, ldx, (const double*)Y, ldy, (const double*)Xs,
                                ldxs, theta, ws, ws_bytes, (double*)mean, ldm, (double*)var, info);
    return f32_predict_entry(h, f32_problem(n, p, d, X, ldx, Y, ldy, theta, ws, ws_bytes, info),
                             F32PredictIO{nstar, (const float*)Xs, ldxs, (float*)mean, ldm, (float*)var, nullptr, 0},
                             false);
}

int mfgp_gpr_predict_cov_workspace_size_ex(mfgp_handle_t h, int dtype, int nlf, int n, int p, int d, int nstar,
                                           size_t* bytes) {
    CHECK_H(h);
    CHECK_DT(dtype);   // d is left to the entry this one dispatches to
    if (dtype == MFGP_F64) return mfgp_gpr_predict_cov_workspace_size(h, nlf, n, p, d, nstar, bytes);
    if (nlf != 0) return MFGP_ERR_ARG;   // the fp32 path runs the linear multi-fidelity kernel
    return mfgp_gpr_predict_workspace_size_ex(h, dtype, n, p, d, nstar, bytes);
}

int mfgp_gpr_predict_cov_ex(mfgp_handle_t h, int dtype, int nlf, int n, int p, int d, int nstar, const void* X,
                            int ldx, const void* Y, int ldy, const void* Xs, int ldxs, const double* theta, void* ws,
                            size_t ws_bytes, void* mean, int ldm, void* var, void* cov, int ldc, int* info) {
    CHECK_EX(h, d, dtype);
    if (dtype == MFGP_F64)
        return mfgp_gpr_predict_cov(h, nlf, n, p, d, nstar, (const double*)X, ldx, (const double*)Y, ldy,
                                    (const double*)Xs, ldxs, theta, ws, ws_bytes, (double*)mean, ldm, (double*)var,
                                    (double*)cov, ldc, info);
    if (nlf != 0) return MFGP_ERR_ARG;   // the fp32 path runs the linear multi-fidelity kernel
    return f32_predict_entry(h, f32_problem(n, p, d, X, ldx, Y, ldy, theta, ws, ws_bytes, info),
                             F32PredictIO{nstar, (const float*)Xs, ldxs, (float*)mean, ldm, (float*)var, (float*)cov,
                                          ldc},
                             true);
}

}  // extern "C"
