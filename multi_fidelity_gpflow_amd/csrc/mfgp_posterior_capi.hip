// C-ABI entry points of the cached posterior (include/mfgp.h, mfgp_gpr_posterior_size through
// mfgp_svgp_posterior_logdens): the cache and workspace layouts, the argument blocks and the launch
// sequences of mfgp_posterior.hip / mfgp_leave_out.hip / mfgp_design.hip / mfgp_append.hip.  Host-side
// orchestration only, as the other *_capi.hip files: no allocation, no synchronisation.
#include <algorithm>

#include "mfgp_device.h"
#include "mfgp_host.h"

namespace mfgp {

// GPR cache (self-contained, laid out for the tile size it was built with):
//   [X: n x (d + 1), dense][theta: G][LZ: Npad x (Npad + Ppad) = the factor's Xo rows, L^{-1} lower tiles | Z = L^{-1} Y]
struct GprCache {
    int nlf, n, p, d;
    int npad, T, ppad, Tp, G;
    long ldr;
    double *X, *theta, *LZ;
    size_t bytes;
};
static GprCache gpr_cache_layout(int nb, int nlf, int n, int p, int d, const void* base) {
    GprCache c;
    c.nlf = nlf; c.n = n; c.p = p; c.d = d;
    c.T = ceil_div(n, nb);
    c.npad = c.T * nb;
    c.Tp = ceil_div(p, nb);
    c.ppad = c.Tp * nb;
    c.G = kernel_theta_size(nlf, d);
    c.ldr = (long)c.npad + c.ppad;
    Carve cv(const_cast<void*>(base));
    c.X = cv.take<double>((size_t)n * (d + 1));
    c.theta = cv.take<double>((size_t)c.G);
    c.LZ = cv.take<double>((size_t)c.npad * c.ldr);
    c.bytes = cv.off + 256;
    return c;
}

// m-tiles per k_post_a task.  A batch that fills the device with whole rows keeps them whole (no
// partials to re-read); otherwise rows are cut so that the longest task is 8 tile products (a row
// of up to 64 tiles then has at most 8 partials: one batch of loads in k_post_out).
constexpr int POST_CHUNK = 8;
static int post_chunk(int T, int Ts, int batch) { return (long)batch * T * Ts >= 256 ? T : POST_CHUNK; }

struct PostLayout {
    int Ts, nspad, chunk, ntask, ngrp;
    double *Apart, *Bpart, *mpart, *vpart, *Am, *Kss, *Cov;   // GPR; Kss / Cov are null with cov = false
                                                              // (design: launch_post full = 0 never touches them)
    double *pa, *pb, *pm, *gm, *gv;                           // SVGP
    int* cnt;
    size_t bytes;
};
// svgp: batch = latents, T = Tm; gpr: batch = 1
static PostLayout post_layout(int nb, int T, int Tp, int nstar, int batch, bool svgp, void* ws, bool cov = true) {
    PostLayout P{};
    P.Ts = ceil_div(nstar > 0 ? nstar : 1, nb);
    P.nspad = P.Ts * nb;
    P.chunk = post_chunk(T, P.Ts, batch);
    P.ntask = post_ntasks(T, P.chunk, svgp ? 1 : 0);
    P.ngrp = ceil_div(T, post_rg(nb));
    Carve c(ws);
    const size_t part = (size_t)batch * P.ntask * P.Ts * nb * nb;
    P.Apart = c.take<double>(part);
    P.cnt = c.take<int>((size_t)P.Ts);
    if (svgp) {
        P.Bpart = c.take<double>(part);
        const size_t pp = (size_t)batch * P.ngrp * P.nspad;
        P.pa = c.take<double>(pp);
        P.pb = c.take<double>(pp);
        P.pm = c.take<double>(pp);
        P.gm = c.take<double>((size_t)batch * P.nspad);
        P.gv = c.take<double>((size_t)batch * P.nspad);
    } else {
        P.mpart = c.take<double>((size_t)P.ngrp * P.nspad * Tp * nb);
        P.vpart = c.take<double>((size_t)P.ngrp * P.nspad);
        P.Am = c.take<double>((size_t)T * nb * P.nspad);
        if (cov) {   // (the design calls keep A but never form a covariance block)
            P.Kss = c.take<double>((size_t)P.nspad * P.nspad);
            P.Cov = c.take<double>((size_t)P.nspad * P.nspad);
        }
    }
    P.bytes = c.off + 256;
    return P;
}

// The VJP calls' workspace: the predict layout, then the input-gradient partials, k_post_grad's
// counters and (SVGP) the kept A / B of every latent.
struct PostGradIO {
    const double* gmean; long ldgm;
    const double* gvar;
    double* gX; long ldgx;
};
struct PostGradLayout {
    double *gpart, *glat, *Am, *Bm;
    int* gcnt;
    size_t bytes;
};
static PostGradLayout post_grad_layout(int nb, const PostLayout& P, int T, int d, int batch, bool svgp, void* ws) {
    PostGradLayout G{};
    const size_t o = (P.bytes + 255) & ~(size_t)255;
    Carve c(ws ? (char*)ws + o : nullptr);
    G.gpart = c.take<double>((size_t)batch * P.ntask * P.Ts * nb * (d > 0 ? d : 1));
    G.gcnt = c.take<int>((size_t)P.Ts * (1 + batch));
    if (svgp) {
        G.glat = c.take<double>((size_t)batch * P.Ts * nb * (d > 0 ? d : 1));
        G.Am = c.take<double>((size_t)batch * T * nb * P.nspad);
        G.Bm = c.take<double>((size_t)batch * T * nb * P.nspad);
    }
    G.bytes = o + c.off + 256;
    return G;
}
// the upstream gradients and the pass's own buffers into a forward argument block
static void post_grad_args(PostArgs& a, const PostGradLayout& G, const PostGradIO& g) {
    a.gmean = g.gmean; a.ldgm = g.ldgm; a.gvar = g.gvar;
    a.gpart = G.gpart; a.glat = G.glat; a.gcnt = G.gcnt;
    a.gX = g.gX; a.ldgx = g.ldgx;
}

// The forward's argument block from a GPR cache: A = L^{-1} K(X, Xs) over the layout P, mean and var
// of the nstar rows of Xs into the given outputs; keep_a: A stays in P.Am behind the launch.
static PostArgs gpr_post_args(const GprCache& c, const PostLayout& P, const double* Xs, int ldxs, int nstar,
                              double* mean, long ldm, double* var, bool keep_a) {
    PostArgs a{};
    a.Li = c.LZ; a.ldl = c.ldr; a.sL = 0;
    a.X1 = c.X; a.ldx1 = c.d + 1; a.n1 = c.n;
    a.theta = c.theta; a.stheta = 0;
    a.Xs = Xs; a.ldxs = ldxs; a.nstar = nstar;
    a.D = c.d; a.nlf = c.nlf;
    a.T = c.T; a.Ts = P.Ts; a.chunk = P.chunk; a.full = 0; a.ntask = P.ntask; a.ngrp = P.ngrp;
    a.Apart = P.Apart; a.cnt = P.cnt;
    a.Zc = c.LZ + c.npad; a.ldz = c.ldr; a.Tp = c.Tp; a.p = c.p;
    a.Am = keep_a ? P.Am : nullptr; a.ldam = P.nspad;
    a.mpart = P.mpart; a.vpart = P.vpart;
    a.mean = mean; a.ldm = ldm; a.var = var;
    return a;
}

static int gpr_posterior_build_impl(mfgp_handle_t h, const GprProblem& P, void* cache, size_t cache_bytes) {
    const GprLayout L = gpr_layout(h->nb, P, gpr_sched_no_flow(h));
    const GprCache c = gpr_cache_layout(h->nb, P.nlf, P.n, P.p, P.d, cache);
    if (P.ws_bytes < L.bytes || cache_bytes < c.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    gpr_factor(h->nb, s, L, P);
    copy_block(s, P.X, P.ldx, c.X, P.d + 1, P.n, P.d + 1);
    copy_block(s, P.theta, c.G, c.theta, c.G, 1, c.G);
    copy_block(s, L.Xo, c.ldr, c.LZ, c.ldr, c.npad, (int)c.ldr);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

// predict (g == nullptr; cov optional) and predict-VJP (g: upstream gradients in, input gradient out)
template <int NB>
static int gpr_posterior_predict_impl(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                                      size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                      double* mean, int ldm, double* var, double* cov, int ldc,
                                      const PostGradIO* g = nullptr) {
    const GprCache c = gpr_cache_layout(NB, nlf, n, p, d, cache);
    const PostLayout P = post_layout(NB, c.T, c.Tp, nstar, 1, false, ws);
    const PostGradLayout G = post_grad_layout(NB, P, c.T, d, 1, false, ws);
    if (cache_bytes < c.bytes || ws_bytes < (g ? G.bytes : P.bytes)) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    PostArgs a = gpr_post_args(c, P, Xs, ldxs, nstar, mean, ldm, var, cov || g);
    if (g) post_grad_args(a, G, *g);
    launch_post<NB>(a, 1, s);
    if (g) launch_post_grad<NB>(a, 1, s);
    if (cov) cov_from_a<NB>(s, Xs, ldxs, nstar, c.theta, d, nlf, P.Am, P.nspad, c.T, P.Kss, P.Cov, cov, ldc);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

// The log-density calls: the forward, the density launch on its mean / var (mfgp_density.hip), then --
// with an input gradient asked for -- k_post_grad fed the density's own gradients.  Their workspace is the
// predict (value only) or predict-VJP layout, then gmean [nstar x p] and gvar (GPR: [nstar], the sum over
// the outputs that share the one variance; SVGP: [nstar x p]).
struct LogdensIO {
    const double* Y; long y_rs;
    const double* obs_var; long ov_rs;
    const double* obs_cov; int ldc;
    double* logp;
    double* gX; int ldgx;     // nullptr: the value only, the call ends behind the density launch
    int* info;
};
struct LogdensLayout {
    double *gm, *gv;
    size_t bytes;
};
static LogdensLayout logdens_layout(size_t base, int nstar, int p, bool svgp, void* ws) {
    LogdensLayout L{};
    const size_t o = (base + 255) & ~(size_t)255;
    Carve c(ws ? (char*)ws + o : nullptr);
    L.gm = c.take<double>((size_t)nstar * p);
    L.gv = c.take<double>((size_t)nstar * (svgp ? p : 1));
    L.bytes = o + c.off + 256;
    return L;
}
static bool logdens_io_ok(const LogdensIO& q, int nstar, int p, int d) {
    return mvn_logpdf_geometry_ok(nstar, p, q.obs_cov != nullptr, q.ldc, q.y_rs, q.ov_rs) && q.Y && q.logp && q.info &&
           (!q.gX || q.ldgx >= d + 1);
}
// the density launch on the forward's outputs; grad: its gradients into the workspace block L
static void logdens_launch(hipStream_t s, const LogdensIO& q, const LogdensLayout& L, int nstar, int p,
                           const double* mean, long ldm, const double* var, bool svgp) {
    LogpdfArgs a{};
    a.ns = nstar; a.p = p;
    a.mean = mean; a.ldm = ldm;
    a.Y = q.Y; a.y_rs = q.y_rs;
    a.var = var; a.var_rs = svgp ? p : 1; a.var_cs = svgp ? 1 : 0;
    a.obs_var = q.obs_var; a.ov_rs = q.ov_rs;
    a.obs_cov = q.obs_cov; a.ldc = q.ldc;
    a.logp = q.logp; a.info = q.info;
    if (q.gX) {
        a.gmean = L.gm; a.ldgm = p;
        a.gvar = L.gv; a.ldgv = svgp ? p : 1; a.gv_sum = svgp ? 0 : 1;
    }
    launch_mvn_logpdf(a, s);
}

template <int NB>
static int gpr_posterior_logdens_impl(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                                      size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                      double* mean, int ldm, double* var, const LogdensIO& q) {
    const GprCache c = gpr_cache_layout(NB, nlf, n, p, d, cache);
    const PostLayout P = post_layout(NB, c.T, c.Tp, nstar, 1, false, ws);
    const PostGradLayout G = post_grad_layout(NB, P, c.T, d, 1, false, ws);
    const LogdensLayout L = logdens_layout(G.bytes, nstar, p, false, ws);
    if (cache_bytes < c.bytes || ws_bytes < (q.gX ? L.bytes : P.bytes)) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    PostArgs a = gpr_post_args(c, P, Xs, ldxs, nstar, mean, ldm, var, q.gX != nullptr);
    if (q.gX) post_grad_args(a, G, PostGradIO{L.gm, p, L.gv, q.gX, q.ldgx});
    launch_post<NB>(a, 1, s);
    logdens_launch(s, q, L, nstar, p, mean, ldm, var, false);
    if (q.gX) launch_post_grad<NB>(a, 1, s);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

// Leave-group-out workspace: the task table, the arrival counters and the chunk partials.
// Tasks: first fit in order closes a task only when the next group does not fit, so every task but
// the last holds at least 33 - gmax columns, and two consecutive tasks together more than 32.
// Chunks: 4 steps of 32 rows (a task at Goku's 37 steps is spread over 10 workgroups), longer
// beyond 128 steps so that the last workgroup sums at most 32 partials.
struct LoLayout {
    int chunk, nch, ny, ntmax;
    int *tab, *cnt;
    double* part;
    size_t bytes;
};
static LoLayout lo_layout(int n, int p, int ngroups, int nrows, int gmax, void* ws) {
    LoLayout L{};
    const int T32 = ceil_div(n, 32);
    L.chunk = T32 > 128 ? ceil_div(T32, 32) : 4;
    L.nch = ceil_div(T32, L.chunk);
    L.ny = ceil_div(p, 32 * LO_PT);
    L.ntmax = std::min(ngroups, std::min((nrows - 1) / (LO_W + 1 - gmax) + 1, 2 * (nrows / (LO_W + 1)) + 1));
    Carve c(ws);
    L.tab = c.take<int>((size_t)L.ntmax + 2);
    L.cnt = c.take<int>((size_t)L.ntmax * L.ny);
    L.part = c.take<double>((size_t)L.ntmax * L.nch * L.ny * 32 * 32 * (1 + LO_PT));
    L.bytes = c.off + 256;
    return L;
}

// Design workspace: the counters first (one memset per call zeroes exactly that block), then the
// predict layout of the nref + ncand stacked points without its covariance blocks (A is kept there),
// then the forward's outputs (the mean is formed and not used: the forward is the predict call's own)
// and the two kernels' partials.
struct DesignLayout {
    PostLayout P;
    int nall, Tr, Tc, nrun, ncb, nrch;
    int* cnt;            // [Tc] k_design_score, then [ncb] k_design_row
    size_t cnt_bytes;
    double *mean, *var, *dpart, *rpart;
    size_t bytes;
};
static DesignLayout design_layout(int nb, int T, int Tp, int p, int nref, int ncand, void* ws) {
    DesignLayout L{};
    L.nall = nref + ncand;
    L.Tr = ceil_div(nref > 0 ? nref : 1, nb);
    L.Tc = ceil_div(ncand > 0 ? ncand : 1, nb);
    L.nrun = ceil_div(L.Tr, design_run(nb));
    L.ncb = ceil_div(L.nall > 0 ? L.nall : 1, NTHREADS);
    L.nrch = ceil_div(T * nb, DESIGN_RROWS);
    Carve c(ws);
    L.cnt_bytes = (sizeof(int) * ((size_t)L.Tc + L.ncb) + 15) & ~(size_t)15;
    L.cnt = c.take<int>(L.cnt_bytes / sizeof(int));
    const size_t o = (c.off + 255) & ~(size_t)255;
    L.P = post_layout(nb, T, Tp, L.nall, 1, false, ws ? (char*)ws + o : nullptr, false);
    const size_t pb = (L.P.bytes + 255) & ~(size_t)255;
    Carve c2(ws ? (char*)ws + o + pb : nullptr);
    L.mean = c2.take<double>((size_t)L.nall * p);
    L.var = c2.take<double>((size_t)L.nall);
    L.dpart = c2.take<double>((size_t)L.nrun * L.Tc * nb);
    L.rpart = c2.take<double>((size_t)L.nrch * L.ncb * NTHREADS);
    L.bytes = o + pb + c2.off + 256;
    return L;
}

// mode 0: score (refresh: the forward first); mode 1: append row k of E for the picked candidate
template <int NB>
static int gpr_posterior_design_impl(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache,
                                     size_t cache_bytes, const double* Xall, int ldx, int nref, int ncand,
                                     const double* w, double* E, int ldE, int k, void* ws, size_t ws_bytes,
                                     double* score, int refresh, const int* pick) {
    const GprCache c = gpr_cache_layout(NB, nlf, n, p, d, cache);
    const DesignLayout L = design_layout(NB, c.T, c.Tp, p, nref, ncand, ws);
    if (cache_bytes < c.bytes || ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    if (!pick && refresh) launch_post<NB>(gpr_post_args(c, L.P, Xall, ldx, L.nall, L.mean, p, L.var, true), 1, s);
    (void)hipMemsetAsync(L.cnt, 0, L.cnt_bytes, s);
    DesignArgs g{};
    g.Am = L.P.Am; g.ldam = L.P.nspad; g.npad = c.npad;
    g.var = L.var;
    g.Xall = Xall; g.ldx = ldx; g.nref = nref; g.ncand = ncand;
    g.theta = c.theta; g.noise = c.theta + c.G - 1;   // the likelihood variance closes both theta layouts
    g.D = d; g.nlf = nlf;
    g.w = w;
    g.E = E; g.ldE = ldE; g.k = k;
    g.T = c.T; g.Tr = L.Tr; g.Tc = L.Tc; g.nrun = L.nrun;
    g.dpart = L.dpart; g.dcnt = L.cnt; g.score = score;
    g.pick = pick; g.Erow = pick ? E + (size_t)k * ldE : nullptr;
    g.ncb = L.ncb; g.nrch = L.nrch; g.rpart = L.rpart; g.rcnt = L.cnt + L.Tc;
    if (pick) launch_design_row(g, s);
    else launch_design_score<NB>(g, s);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

// Append workspace: the predict layout of the k new rows without its covariance blocks (A is kept
// there), the forward's mean and var, then W, R, the row kernel's counters and its partials.  Tasks: 4
// row tiles of a tile column (at Goku's 37 tiles 190 tasks, the longest four products), longer beyond
// 128 tiles so that a column's last workgroup sums at most 32 partials.
struct AppendLayout {
    PostLayout P;
    int chunk, ntask, nfill;
    double *mean, *var, *W, *Rw, *part;
    int* cnt;
    size_t bytes;
};
static AppendLayout append_layout(int nb, const GprCache& c, int k, void* ws) {
    AppendLayout L{};
    L.P = post_layout(nb, c.T, c.Tp, k, 1, false, ws, false);
    const size_t o = (L.P.bytes + 255) & ~(size_t)255;
    L.chunk = c.T > 128 ? ceil_div(c.T, 32) : 4;
    L.ntask = append_ntasks(c.T, L.chunk);
    L.nfill = std::min(ceil_div(c.n + k, nb) * nb, 256);
    Carve cv(ws ? (char*)ws + o : nullptr);
    L.mean = cv.take<double>((size_t)APPEND_MAXK * c.p);
    L.var = cv.take<double>((size_t)APPEND_MAXK);
    L.W = cv.take<double>((size_t)APPEND_MAXK * c.npad);
    L.Rw = cv.take<double>((size_t)APPEND_MAXK * APPEND_MAXK);
    L.cnt = cv.take<int>((size_t)c.T);
    L.part = cv.take<double>((size_t)L.ntask * APPEND_MAXK * nb);
    L.bytes = o + cv.off + 256;
    return L;
}

template <int NB>
static int gpr_posterior_append_impl(mfgp_handle_t h, int nlf, int n, int p, int d, int k, const void* cache,
                                     size_t cache_bytes, const double* Xadd, int ldxa, const double* Yadd, int ldya,
                                     void* ws, size_t ws_bytes, void* out_cache, size_t out_bytes, double* mean_add,
                                     int ldm, int* info) {
    const GprCache c = gpr_cache_layout(NB, nlf, n, p, d, cache);
    const GprCache o = gpr_cache_layout(NB, nlf, n + k, p, d, out_cache);
    const AppendLayout L = append_layout(NB, c, k, ws);
    if (cache_bytes < c.bytes || out_bytes < o.bytes || ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    double* mean = mean_add ? mean_add : L.mean;
    const long ldmean = mean_add ? ldm : p;
    PostArgs a = gpr_post_args(c, L.P, Xadd, ldxa, k, mean, ldmean, L.var, true);
    a.swap = 1;   // the new rows sit below the cached ones: the cross block has the new row as its row argument
    launch_post<NB>(a, 1, s);
    AppendArgs g{};
    g.LZ = c.LZ; g.ldr = c.ldr; g.X = c.X; g.theta = c.theta;
    g.n = n; g.npad = c.npad; g.T = c.T;
    g.p = p; g.ppad = c.ppad; g.D = d; g.nlf = nlf; g.G = c.G; g.k = k;
    g.diag_add = nlf ? GRAPH_JITTER : 0.0;
    g.Xadd = Xadd; g.ldxa = ldxa; g.Yadd = Yadd; g.ldya = ldya;
    g.Am = L.P.Am; g.ldam = L.P.nspad;
    g.mean = mean; g.ldm = ldmean;
    g.W = L.W; g.Rw = L.Rw; g.cnt = L.cnt; g.part = L.part;
    g.chunk = L.chunk; g.ntask = L.ntask; g.nfill = L.nfill;
    g.LZo = o.LZ; g.ldro = o.ldr; g.npado = o.npad;
    g.Xo = o.X; g.thetao = o.theta;
    g.obase = (unsigned char*)out_cache;
    const char* ob = (const char*)out_cache;
    g.gap0[0] = (const char*)(o.X + (size_t)(n + k) * (d + 1)) - ob; g.gap1[0] = (const char*)o.theta - ob;
    g.gap0[1] = (const char*)(o.theta + o.G) - ob;                   g.gap1[1] = (const char*)o.LZ - ob;
    g.gap0[2] = (const char*)(o.LZ + (size_t)o.npad * o.ldr) - ob;   g.gap1[2] = (long)o.bytes;
    g.info = info;
    launch_append<NB>(g, s);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

// SVGP cache: [Z: m x (d + 1)][thetas: l x G][W: p x l][q_mu^T: l x Mpad, zero padded]
//             [Lm^{-1}: l x Mpad x Mpad][C = Lq^T Lm^{-1}: l x Mpad x Mpad]
struct SvgpCache {
    int Tm, mpad, G;
    double *Z, *thetas, *W, *qmu, *Li, *C;
    size_t bytes;
};
static SvgpCache svgp_cache_layout(int nb, int m, int l, int p, int d, const void* base) {
    SvgpCache c;
    c.Tm = ceil_div(m, nb);
    c.mpad = c.Tm * nb;
    c.G = theta_size(d);
    const size_t mm = (size_t)c.mpad * c.mpad;
    Carve cv(const_cast<void*>(base));
    c.Z = cv.take<double>((size_t)m * (d + 1));
    c.thetas = cv.take<double>((size_t)l * c.G);
    c.W = cv.take<double>((size_t)p * l);
    c.qmu = cv.take<double>((size_t)l * c.mpad);
    c.Li = cv.take<double>(mm * l);
    c.C = cv.take<double>(mm * l);
    c.bytes = cv.off + 256;
    return c;
}

// q_mu [m][L] -> [L][Mpad], zero padded
__global__ void k_post_qmu_pad(const double* q_mu, int m, int L, int mpad, double* out) {
    const long total = (long)L * mpad;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int l = (int)(e / mpad), r = (int)(e % mpad);
        out[e] = r < m ? q_mu[(long)r * L + l] : 0.0;
    }
}

static int svgp_posterior_build_impl(mfgp_handle_t h, int m, int l, int p, int d, const double* Z, int ldz,
                                     const double* thetas, const double* q_mu, const double* q_sqrt, const double* W,
                                     double jitter, void* ws, size_t ws_bytes, void* cache, size_t cache_bytes,
                                     int* info) {
    const SvgpCache c = svgp_cache_layout(h->nb, m, l, p, d, cache);
    if (cache_bytes < c.bytes || ws_bytes < svgp_posterior_factor_bytes(h->nb, m, l)) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    SvgpProblem P{};
    P.m = m; P.l = l; P.p = p; P.d = d;
    P.Z = Z; P.ldz = ldz; P.thetas = thetas; P.q_mu = q_mu; P.q_sqrt = q_sqrt; P.W = W;
    P.jitter = jitter; P.ws = ws; P.ws_bytes = ws_bytes; P.info = info;
    const int rc = svgp_posterior_factor(h->nb, s, P, c.Li, c.C);
    if (rc) return rc == -2 ? MFGP_ERR_WORKSPACE : MFGP_ERR_LAUNCH;
    copy_block(s, Z, ldz, c.Z, d + 1, m, d + 1);
    copy_block(s, thetas, c.G, c.thetas, c.G, l, c.G);
    if (W) copy_block(s, W, l, c.W, l, p, l);
    const long tot = (long)l * c.mpad;
    hipLaunchKernelGGL(k_post_qmu_pad, dim3((int)std::min<long>((tot + 255) / 256, 2048)), dim3(256), 0, s, q_mu, m, l,
                       c.mpad, c.qmu);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

static int svgp_posterior_predict_impl(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed,
                                       const void* cache, size_t cache_bytes, const double* Xs, int ldxs, void* ws,
                                       size_t ws_bytes, double* f_mu, double* f_var,
                                       const PostGradIO* g = nullptr, const LogdensIO* q = nullptr) {
    const SvgpCache c = svgp_cache_layout(h->nb, m, l, p, d, cache);
    const PostLayout P = post_layout(h->nb, c.Tm, 0, nstar, l, true, ws);
    const PostGradLayout G = post_grad_layout(h->nb, P, c.Tm, d, l, true, ws);
    const LogdensLayout Q = logdens_layout(G.bytes, nstar, p, true, ws);
    // the log-density call with an input gradient is the VJP call fed the density's own gradients
    const PostGradIO qg{Q.gm, p, Q.gv, q ? q->gX : nullptr, q ? q->ldgx : 0};
    if (q && q->gX) g = &qg;
    if (cache_bytes < c.bytes || ws_bytes < (q && q->gX ? Q.bytes : g ? G.bytes : P.bytes)) return MFGP_ERR_WORKSPACE;
    const long mm = (long)c.mpad * c.mpad;
    PostArgs a{};
    a.Li = c.Li; a.ldl = c.mpad; a.sL = mm;
    a.C = c.C; a.ldc = c.mpad; a.sC = mm;
    a.X1 = c.Z; a.ldx1 = d + 1; a.n1 = m;
    a.theta = c.thetas; a.stheta = c.G;
    a.Xs = Xs; a.ldxs = ldxs; a.nstar = nstar;
    a.D = d; a.nlf = 0;
    a.T = c.Tm; a.Ts = P.Ts; a.chunk = P.chunk; a.full = 1; a.ntask = P.ntask; a.ngrp = P.ngrp;
    a.Apart = P.Apart; a.Bpart = P.Bpart; a.cnt = P.cnt;
    a.p = p;
    a.qmu = c.qmu; a.pa = P.pa; a.pb = P.pb; a.pm = P.pm; a.gm = P.gm; a.gv = P.gv;
    a.W = mixed ? c.W : nullptr;
    a.f_mu = f_mu; a.f_var = f_var;
    if (g) {
        a.Am = G.Am; a.Bm = G.Bm; a.ldam = P.nspad; a.sAm = (long)c.mpad * P.nspad;
        post_grad_args(a, G, *g);
    }
    TILE_CALL(h->nb, launch_post, a, l, h->stream);
    if (q) logdens_launch(h->stream, *q, Q, nstar, p, f_mu, p, f_var, true);
    if (g) TILE_CALL(h->nb, launch_post_grad, a, l, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

// the GPR entries' shared geometry test
static inline bool nlf_ok(int nlf) { return nlf >= 0 && nlf <= MFGP_MAX_LF; }
static inline bool gpr_geometry_ok(int nlf, int n, int p) { return nlf_ok(nlf) && n >= 1 && p >= 1; }
static inline bool design_geometry_ok(int nlf, int n, int p, int nref, int ncand) {
    return gpr_geometry_ok(nlf, n, p) && nref >= 0 && ncand >= 0 && (long)nref + ncand <= 0x7fffffffL - 4096;
}

static inline bool append_geometry_ok(int nlf, int n, int p, int k) {
    return gpr_geometry_ok(nlf, n, p) && k >= 1 && k <= APPEND_MAXK && (long)n + k <= 0x7fffffffL - 4096;
}

}  // namespace mfgp

using namespace mfgp;

extern "C" {

int mfgp_gpr_posterior_size(mfgp_handle_t h, int nlf, int n, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (!gpr_geometry_ok(nlf, n, p) || !bytes) return MFGP_ERR_ARG;
    *bytes = gpr_cache_layout(h->nb, nlf, n, p, d, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_gpr_posterior_build(mfgp_handle_t h, int nlf, int n, int p, int d, const double* X, int ldx, const double* Y,
                             int ldy, const double* theta, void* ws, size_t ws_bytes, void* cache, size_t cache_bytes,
                             int* info) {
    const GprProblem P{n, p, d, nlf, X, ldx, Y, ldy, theta, ws, ws_bytes, info};
    if (const int rc = gpr_check(h, P, 0, cache && ldx >= d + 1 && ldy >= p)) return rc;
    return gpr_posterior_build_impl(h, P, cache, cache_bytes);
}

int mfgp_gpr_posterior_predict_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                              size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (!gpr_geometry_ok(nlf, n, p) || nstar < 1 || !bytes) return MFGP_ERR_ARG;
    const GprCache c = gpr_cache_layout(h->nb, nlf, n, p, d, nullptr);
    *bytes = post_layout(h->nb, c.T, c.Tp, nstar, 1, false, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_gpr_posterior_predict(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                               size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes, double* mean,
                               int ldm, double* var, double* cov, int ldc) {
    CHECK_H(h);
    CHECK_D(d);
    if (!gpr_geometry_ok(nlf, n, p) || nstar < 1 || !cache || !Xs || !ws || !mean || !var || ldxs < d + 1 || ldm < p)
        return MFGP_ERR_ARG;
    if (cov && ldc < nstar) return MFGP_ERR_ARG;
    return TILE_CALL(h->nb, gpr_posterior_predict_impl, h, nlf, n, p, d, nstar, cache, cache_bytes, Xs, ldxs, ws,
                     ws_bytes, mean, ldm, var, cov, ldc);
}

int mfgp_gpr_posterior_predict_vjp_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                                  size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf != 0 || !gpr_geometry_ok(nlf, n, p) || nstar < 1 || !bytes) return MFGP_ERR_ARG;
    const GprCache c = gpr_cache_layout(h->nb, nlf, n, p, d, nullptr);
    const PostLayout P = post_layout(h->nb, c.T, c.Tp, nstar, 1, false, nullptr);
    *bytes = post_grad_layout(h->nb, P, c.T, d, 1, false, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_gpr_posterior_predict_vjp(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                                   size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                   double* mean, int ldm, double* var, const double* gmean, int ldgm,
                                   const double* gvar, double* gX, int ldgx) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf != 0) return MFGP_ERR_ARG;   // the graph kernel's per-source derivative is not built
    if (nstar == 0) return MFGP_OK;
    if (!gpr_geometry_ok(nlf, n, p) || nstar < 0 || !cache || !Xs || !ws || !mean || !var || !gX || ldxs < d + 1 ||
        ldm < p || ldgx < d + 1)
        return MFGP_ERR_ARG;
    if (gmean && ldgm < p) return MFGP_ERR_ARG;
    const PostGradIO g{gmean, ldgm, gvar, gX, ldgx};
    return TILE_CALL(h->nb, gpr_posterior_predict_impl, h, nlf, n, p, d, nstar, cache, cache_bytes, Xs, ldxs, ws,
                     ws_bytes, mean, ldm, var, nullptr, 0, &g);
}

int mfgp_gpr_posterior_leave_out_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int ngroups, int nrows,
                                                size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (!gpr_geometry_ok(nlf, n, p) || ngroups < 1 || nrows < ngroups || !bytes) return MFGP_ERR_ARG;
    *bytes = lo_layout(n, p, ngroups, nrows, LO_W, nullptr).bytes;   // groups of any size up to 32
    return MFGP_OK;
}

int mfgp_gpr_posterior_leave_out(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache, size_t cache_bytes,
                                 int ngroups, const int* offsets, const int* rows, int nrows, int gmax, void* ws,
                                 size_t ws_bytes, double* resid, int ldr, double* cov, int ldc, double* logdens,
                                 int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (!nlf_ok(nlf) || ngroups < 0 || gmax < 1 || gmax > LO_W) return MFGP_ERR_ARG;
    if (ngroups == 0) return MFGP_OK;
    if (!gpr_geometry_ok(nlf, n, p) || nrows < ngroups || !cache || !offsets || !rows || !ws || !resid || !logdens ||
        !info || ldr < p || (cov && ldc < gmax))
        return MFGP_ERR_ARG;
    const GprCache c = gpr_cache_layout(h->nb, nlf, n, p, d, cache);
    const LoLayout L = lo_layout(n, p, ngroups, nrows, gmax, ws);
    if (cache_bytes < c.bytes || ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    LoArgs a{};
    a.LZ = c.LZ; a.ldr = c.ldr; a.npad = c.npad;
    a.noise = c.theta + c.G - 1;   // the likelihood variance closes both theta layouts
    a.n = n; a.p = p;
    a.ngroups = ngroups; a.nrows = nrows; a.gmax = gmax;
    a.offsets = offsets; a.rows = rows;
    a.ntmax = L.ntmax; a.chunk = L.chunk; a.nch = L.nch; a.ny = L.ny;
    a.tab = L.tab; a.cnt = L.cnt; a.part = L.part;
    a.resid = resid; a.ldres = ldr; a.cov = cov; a.ldc = ldc; a.logdens = logdens; a.info = info;
    launch_leave_out(a, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

int mfgp_gpr_posterior_design_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nref, int ncand,
                                             int qmax, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (!design_geometry_ok(nlf, n, p, nref, ncand) || qmax < 0 || qmax > DESIGN_MAXQ || !bytes) return MFGP_ERR_ARG;
    const GprCache c = gpr_cache_layout(h->nb, nlf, n, p, d, nullptr);
    *bytes = design_layout(h->nb, c.T, c.Tp, p, nref, ncand, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_gpr_posterior_design_score(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache,
                                    size_t cache_bytes, const double* Xall, int ldx, int nref, int ncand,
                                    const double* w, const double* E, int ldE, int k, void* ws, size_t ws_bytes,
                                    double* score, int refresh) {
    CHECK_H(h);
    CHECK_D(d);
    if (!design_geometry_ok(nlf, n, p, nref, ncand) || k < 0 || k > DESIGN_MAXQ) return MFGP_ERR_ARG;
    if (ncand == 0) return MFGP_OK;
    if (!cache || !Xall || !ws || !score || ldx < d + 1 || (k > 0 && (!E || ldE < nref + ncand))) return MFGP_ERR_ARG;
    if (nref == 0) {   // nothing to buy down: zeros, after the same size checks as any other call
        const GprCache c = gpr_cache_layout(h->nb, nlf, n, p, d, nullptr);
        if (cache_bytes < c.bytes || ws_bytes < design_layout(h->nb, c.T, c.Tp, p, nref, ncand, nullptr).bytes)
            return MFGP_ERR_WORKSPACE;
        (void)hipMemsetAsync(score, 0, sizeof(double) * (size_t)ncand, h->stream);
        return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
    }
    double* Em = const_cast<double*>(E);   // (only read in this mode)
    return TILE_CALL(h->nb, gpr_posterior_design_impl, h, nlf, n, p, d, cache, cache_bytes, Xall, ldx, nref, ncand, w,
                     Em, ldE, k, ws, ws_bytes, score, refresh, nullptr);
}

int mfgp_gpr_posterior_design_append(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache,
                                     size_t cache_bytes, const double* Xall, int ldx, int nref, int ncand, void* ws,
                                     size_t ws_bytes, const int* pick, double* E, int ldE, int k) {
    CHECK_H(h);
    CHECK_D(d);
    if (!design_geometry_ok(nlf, n, p, nref, ncand) || k < 0 || k >= DESIGN_MAXQ) return MFGP_ERR_ARG;
    if (ncand == 0) return MFGP_OK;
    if (!cache || !Xall || !ws || !pick || !E || ldx < d + 1 || ldE < nref + ncand) return MFGP_ERR_ARG;
    return TILE_CALL(h->nb, gpr_posterior_design_impl, h, nlf, n, p, d, cache, cache_bytes, Xall, ldx, nref, ncand,
                     nullptr, E, ldE, k, ws, ws_bytes, nullptr, 0, pick);
}

int mfgp_gpr_posterior_append_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int k, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (!append_geometry_ok(nlf, n, p, k) || !bytes) return MFGP_ERR_ARG;
    *bytes = append_layout(h->nb, gpr_cache_layout(h->nb, nlf, n, p, d, nullptr), k, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_gpr_posterior_append(mfgp_handle_t h, int nlf, int n, int p, int d, int k, const void* cache,
                              size_t cache_bytes, const double* Xadd, int ldxa, const double* Yadd, int ldya, void* ws,
                              size_t ws_bytes, void* out_cache, size_t out_bytes, double* mean_add, int ldm,
                              int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (!append_geometry_ok(nlf, n, p, k) || !cache || !Xadd || !ws || !out_cache || !info || out_cache == cache ||
        ldxa < d + 1 || (Yadd && ldya < p) || (mean_add && ldm < p))
        return MFGP_ERR_ARG;
    return TILE_CALL(h->nb, gpr_posterior_append_impl, h, nlf, n, p, d, k, cache, cache_bytes, Xadd, ldxa, Yadd, ldya,
                     ws, ws_bytes, out_cache, out_bytes, mean_add, ldm, info);
}

int mfgp_svgp_posterior_size(mfgp_handle_t h, int m, int l, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (m < 1 || l < 1 || p < 1 || !bytes) return MFGP_ERR_ARG;
    *bytes = svgp_cache_layout(h->nb, m, l, p, d, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_svgp_posterior_build(mfgp_handle_t h, int m, int l, int p, int d, const double* Z, int ldz,
                              const double* thetas, const double* q_mu, const double* q_sqrt, const double* W,
                              double jitter, void* ws, size_t ws_bytes, void* cache, size_t cache_bytes, int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (m < 1 || l < 1 || p < 1 || !Z || !thetas || !q_mu || !q_sqrt || !ws || !cache || !info || ldz < d + 1)
        return MFGP_ERR_ARG;
    if (!W && l != p) return MFGP_ERR_ARG;
    return svgp_posterior_build_impl(h, m, l, p, d, Z, ldz, thetas, q_mu, q_sqrt, W, jitter, ws, ws_bytes, cache,
                                     cache_bytes, info);
}

int mfgp_svgp_posterior_predict_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar < 1 || m < 1 || l < 1 || p < 1 || !bytes) return MFGP_ERR_ARG;
    *bytes = post_layout(h->nb, ceil_div(m, h->nb), 0, nstar, l, true, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_svgp_posterior_predict(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed, const void* cache,
                                size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                double* f_mu, double* f_var) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar < 1 || m < 1 || l < 1 || p < 1 || !cache || !Xs || !ws || !f_mu || !f_var || ldxs < d + 1)
        return MFGP_ERR_ARG;
    if (!mixed && l != p) return MFGP_ERR_ARG;
    return svgp_posterior_predict_impl(h, nstar, m, l, p, d, mixed, cache, cache_bytes, Xs, ldxs, ws, ws_bytes, f_mu,
                                       f_var);
}

int mfgp_svgp_posterior_predict_vjp_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d,
                                                   size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar < 1 || m < 1 || l < 1 || p < 1 || !bytes) return MFGP_ERR_ARG;
    const int T = ceil_div(m, h->nb);
    const PostLayout P = post_layout(h->nb, T, 0, nstar, l, true, nullptr);
    *bytes = post_grad_layout(h->nb, P, T, d, l, true, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_svgp_posterior_predict_vjp(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed,
                                    const void* cache, size_t cache_bytes, const double* Xs, int ldxs, void* ws,
                                    size_t ws_bytes, double* f_mu, double* f_var, const double* gmean, int ldgm,
                                    const double* gvar, double* gX, int ldgx) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar == 0) return MFGP_OK;
    if (nstar < 0 || m < 1 || l < 1 || p < 1 || !cache || !Xs || !ws || !f_mu || !f_var || !gX || ldxs < d + 1 ||
        ldgx < d + 1)
        return MFGP_ERR_ARG;
    if (!mixed && l != p) return MFGP_ERR_ARG;
    if (gmean && ldgm < p) return MFGP_ERR_ARG;
    const PostGradIO g{gmean, ldgm, gvar, gX, ldgx};
    return svgp_posterior_predict_impl(h, nstar, m, l, p, d, mixed, cache, cache_bytes, Xs, ldxs, ws, ws_bytes, f_mu,
                                       f_var, &g);
}

int mfgp_gpr_posterior_logdens_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                              size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (!gpr_geometry_ok(nlf, n, p) || nstar < 1 || !bytes) return MFGP_ERR_ARG;
    const GprCache c = gpr_cache_layout(h->nb, nlf, n, p, d, nullptr);
    const PostLayout P = post_layout(h->nb, c.T, c.Tp, nstar, 1, false, nullptr);
    // (the graph kernel has the value only: the predict layout)
    *bytes = nlf ? P.bytes
                 : logdens_layout(post_grad_layout(h->nb, P, c.T, d, 1, false, nullptr).bytes, nstar, p, false, nullptr)
                       .bytes;
    return MFGP_OK;
}

int mfgp_gpr_posterior_logdens(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                               size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes, double* mean,
                               int ldm, double* var, const double* Y, long y_rs, const double* obs_var, long ov_rs,
                               const double* obs_cov, int ldc, double* logp, double* gX, int ldgx, int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (!nlf_ok(nlf) || (nlf != 0 && gX)) return MFGP_ERR_ARG;   // the graph kernel has no input gradient
    if (nstar == 0) return MFGP_OK;
    const LogdensIO q{Y, y_rs, obs_var, ov_rs, obs_cov, ldc, logp, gX, ldgx, info};
    if (!gpr_geometry_ok(nlf, n, p) || nstar < 0 || !cache || !Xs || !ws || !mean || !var || ldxs < d + 1 || ldm < p ||
        !logdens_io_ok(q, nstar, p, d))
        return MFGP_ERR_ARG;
    return TILE_CALL(h->nb, gpr_posterior_logdens_impl, h, nlf, n, p, d, nstar, cache, cache_bytes, Xs, ldxs, ws,
                     ws_bytes, mean, ldm, var, q);
}

int mfgp_svgp_posterior_logdens_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar < 1 || m < 1 || l < 1 || p < 1 || !bytes) return MFGP_ERR_ARG;
    const int T = ceil_div(m, h->nb);
    const PostLayout P = post_layout(h->nb, T, 0, nstar, l, true, nullptr);
    *bytes = logdens_layout(post_grad_layout(h->nb, P, T, d, l, true, nullptr).bytes, nstar, p, true, nullptr).bytes;
    return MFGP_OK;
}

int mfgp_svgp_posterior_logdens(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed, const void* cache,
                                size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                double* f_mu, double* f_var, const double* Y, long y_rs, const double* obs_var,
                                long ov_rs, const double* obs_cov, int ldc, double* logp, double* gX, int ldgx,
                                int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar == 0) return MFGP_OK;
    const LogdensIO q{Y, y_rs, obs_var, ov_rs, obs_cov, ldc, logp, gX, ldgx, info};
    if (nstar < 0 || m < 1 || l < 1 || p < 1 || !cache || !Xs || !ws || !f_mu || !f_var || ldxs < d + 1 ||
        !logdens_io_ok(q, nstar, p, d))
        return MFGP_ERR_ARG;
    if (!mixed && l != p) return MFGP_ERR_ARG;
    return svgp_posterior_predict_impl(h, nstar, m, l, p, d, mixed, cache, cache_bytes, Xs, ldxs, ws, ws_bytes, f_mu,
                                       f_var, nullptr, &q);
}

}  // extern "C"
