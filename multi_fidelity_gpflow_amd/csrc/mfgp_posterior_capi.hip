// C-ABI entry points of the cached posterior (include/mfgp.h, mfgp_gpr_posterior_size through
// mfgp_svgp_posterior_logdens, and the mfgp_*_jacobian entries): the cache and workspace layouts, the argument
// blocks and the launch sequences of mfgp_posterior.hip / mfgp_leave_out.hip / mfgp_design.hip / mfgp_append.hip /
// mfgp_jacobian.hip.  Host-side
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
    const double* noise() const { return theta + G - 1; }   // the likelihood variance closes both theta layouts
    // the byte ranges [g0[i], g1[i]) of the block that none of its arrays covers (X starts the block)
    void gaps(long* g0, long* g1) const {
        const char* b = (const char*)X;
        g0[0] = (const char*)(X + (size_t)n * (d + 1)) - b; g1[0] = (const char*)theta - b;
        g0[1] = (const char*)(theta + G) - b;               g1[1] = (const char*)LZ - b;
        g0[2] = (const char*)(LZ + (size_t)npad * ldr) - b; g1[2] = (long)bytes;
    }
};
static GprCache gpr_cache_layout(int nb, const GprCacheRef& r) {
    GprCache c;
    c.nlf = r.nlf; c.n = r.n; c.p = r.p; c.d = r.d;
    c.T = ceil_div(c.n, nb);
    c.npad = c.T * nb;
    c.Tp = ceil_div(c.p, nb);
    c.ppad = c.Tp * nb;
    c.G = kernel_theta_size(c.nlf, c.d);
    c.ldr = (long)c.npad + c.ppad;
    Carve cv(const_cast<void*>(r.cache));
    c.X = cv.take<double>((size_t)c.n * (c.d + 1));
    c.theta = cv.take<double>((size_t)c.G);
    c.LZ = cv.take<double>((size_t)c.npad * c.ldr);
    c.bytes = cv.off + 256;
    return c;
}

// A Carve of its own behind the first `bytes` of ws (or of another Behind's part of ws), on the next 256-byte
// boundary: how every layout below that extends another one is placed, and the one place that aligns a
// layout's end.  o: where this carve starts in ws; end(): the bytes of ws up to this carve's end.
struct Behind : Carve {
    size_t o;
    static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
    Behind(void* ws, size_t bytes) : Carve(ws ? (char*)ws + up(bytes) : nullptr), o(up(bytes)) {}
    Behind(const Behind& prev, size_t bytes) : Behind(prev.base, bytes) { o += prev.o; }
    size_t end() const { return o + off + 256; }
};

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

// The workspace of the predict, VJP and log-density calls, each part behind the one before it: the predict
// layout; then the input-gradient partials, k_post_grad's counters and (SVGP) the kept A / B of every latent;
// then gmean [nstar x p] and gvar (GPR: [nstar], the sum over the outputs that share the one variance; SVGP:
// [nstar x p]).  A value-only log-density call needs the predict call's size.  The one place that knows the
// chain: the size queries and the two forward drivers read it here.
struct PostDims { int T, Tp, batch, d, p; bool svgp; };   // what the chain reads of a cache
static PostDims post_dims(const GprCache& c) { return {c.T, c.Tp, 1, c.d, c.p, false}; }
static PostDims post_dims(int nb, const SvgpCacheRef& r) { return {ceil_div(r.m, nb), 0, r.l, r.d, r.p, true}; }
struct PostChain {
    PostLayout P;
    double *gpart, *glat, *Am, *Bm;   // VJP (Am / Bm: SVGP)
    int* gcnt;
    double *gm, *gv;                  // density
    // Jacobian, behind the predict layout (in the VJP part's place): row tiles per chunk, chunks, dimension groups,
    // the chunk partials, the task counters (GPR) and the latents' sums (SVGP; the partials themselves with one chunk)
    int jchunk, jnch, jdgroups;
    double *jpart, *jdgl;
    int* jcnt;
    size_t jcnt_bytes;
    size_t predict, vjp, logdens, jac;   // bytes of a call of that kind
};
// The Jacobian's chunk count from the shapes alone: enough tasks for the device's 256 CUs, never more chunks
// than row tiles.
static int jac_chunks(int T, long tasks) {
    const long want = (256 + tasks - 1) / tasks;
    const int nch = (int)std::max<long>(1, std::min<long>(want, T));
    return ceil_div(T, ceil_div(T, nch));
}
static PostChain post_chain(int nb, const PostDims& s, int nstar, void* ws) {
    PostChain W{};
    const PostLayout& P = W.P = post_layout(nb, s.T, s.Tp, nstar, s.batch, s.svgp, ws);
    Behind g(ws, P.bytes);
    W.gpart = g.take<double>((size_t)s.batch * P.ntask * P.Ts * nb * (s.d > 0 ? s.d : 1));
    W.gcnt = g.take<int>((size_t)P.Ts * (1 + s.batch));
    if (s.svgp) {
        W.glat = g.take<double>((size_t)s.batch * P.Ts * nb * (s.d > 0 ? s.d : 1));
        W.Am = g.take<double>((size_t)s.batch * s.T * nb * P.nspad);
        W.Bm = g.take<double>((size_t)s.batch * s.T * nb * P.nspad);
    }
    Behind q(ws, g.end());
    W.gm = q.take<double>((size_t)nstar * s.p);
    W.gv = q.take<double>((size_t)nstar * (s.svgp ? s.p : 1));
    Behind j(ws, P.bytes);
    const size_t d1 = (size_t)(s.d > 0 ? s.d : 1);
    if (s.svgp) {
        W.jdgroups = 1;
        W.jnch = jac_chunks(s.T, (long)s.batch * P.Ts);
        W.jpart = j.take<double>((size_t)s.batch * W.jnch * P.Ts * d1 * nb);
        W.jdgl = W.jnch > 1 ? j.take<double>((size_t)s.batch * P.Ts * d1 * nb) : W.jpart;
    } else {
        const int dg = nb == 64 ? JacCfg<64>::DG : JacCfg<32>::DG;
        const size_t tp = (size_t)(s.Tp > 0 ? s.Tp : 1);
        W.jdgroups = ceil_div((int)d1, dg);
        W.jnch = jac_chunks(s.T, (long)(P.Ts * tp) * W.jdgroups);
        W.jcnt_bytes = (sizeof(int) * P.Ts * tp * W.jdgroups + 15) & ~(size_t)15;
        W.jcnt = j.take<int>(W.jcnt_bytes / sizeof(int));
        if (W.jnch > 1)
            W.jpart = j.take<double>(P.Ts * tp * W.jdgroups * W.jnch * std::min<size_t>(d1, dg) * nb * nb);
    }
    W.jchunk = ceil_div(s.T, W.jnch);
    W.predict = P.bytes; W.vjp = g.end(); W.logdens = q.end(); W.jac = j.end();
    return W;
}
// The Jacobian weights buffer: GPR alpha = L^{-T} Z [npad x ppad]; SVGP alpha_l = Lm^{-T} q_mu [l][mpad]
static size_t jac_weights_bytes(size_t rows, size_t cols) { return Behind::up(sizeof(double) * rows * cols); }
// What a query asks of a forward driver.  An entry sets at most one of cov, grad and dens: whether the call
// runs k_post_grad, and the bytes of the chain it needs (a value-only log-density ends behind the density launch).
static bool post_wants_grad(const PostQuery& q) { return q.grad || (q.dens && q.dens->gX); }
static size_t post_ws_need(const PostChain& W, const PostQuery& q) {
    if (q.jac) return W.jac;
    if (q.dens) return q.dens->gX ? W.logdens : W.predict;
    return q.grad ? W.vjp : W.predict;
}
// The upstream gradients and the pass's own buffers into a forward argument block.  The log-density
// call with an input gradient is the VJP call fed the density's own gradients.
static void post_grad_args(PostArgs& a, const PostChain& W, const PostQuery& q, int p) {
    const PostGradIO g = q.grad ? *q.grad : PostGradIO{W.gm, p, W.gv, q.dens->gX, q.dens->ldgx};
    a.gmean = g.gmean; a.ldgm = g.ldgm; a.gvar = g.gvar;
    a.gpart = W.gpart; a.glat = W.glat; a.gcnt = W.gcnt;
    a.gX = g.gX; a.ldgx = g.ldgx;
}

// The forward's argument block from a GPR cache: A = L^{-1} K(X, Xs) over the layout P, mean and var
// of the nstar rows of q.Xs into q's outputs; keep_a: A stays in P.Am behind the launch.
static PostArgs gpr_post_args(const GprCache& c, const PostLayout& P, const PostQuery& q, bool keep_a) {
    PostArgs a{};
    a.Li = c.LZ; a.ldl = c.ldr; a.sL = 0;
    a.X1 = c.X; a.ldx1 = c.d + 1; a.n1 = c.n;
    a.theta = c.theta; a.stheta = 0;
    a.Xs = q.Xs; a.ldxs = q.ldxs; a.nstar = q.nstar;
    a.D = c.d; a.nlf = c.nlf;
    a.T = c.T; a.Ts = P.Ts; a.chunk = P.chunk; a.full = 0; a.ntask = P.ntask; a.ngrp = P.ngrp;
    a.Apart = P.Apart; a.cnt = P.cnt;
    a.Zc = c.LZ + c.npad; a.ldz = c.ldr; a.Tp = c.Tp; a.p = c.p;
    a.Am = keep_a ? P.Am : nullptr; a.ldam = P.nspad;
    a.mpart = P.mpart; a.vpart = P.vpart;
    a.mean = q.mean; a.ldm = q.ldm; a.var = q.var;
    return a;
}

// The Jacobian kernels' argument block from a GPR cache and its weights buffer; jac_query_args adds the query
static JacArgs gpr_jac_args(const GprCache& c, double* weights) {
    JacArgs j{};
    j.Li = c.LZ; j.ldl = c.ldr;
    j.Zc = c.LZ + c.npad; j.ldz = c.ldr;
    j.T = c.T; j.Tp = c.Tp;
    j.alpha = weights; j.lda = c.ppad;
    j.X1 = c.X; j.ldx1 = c.d + 1; j.n1 = c.n;
    j.theta = c.theta;
    j.D = c.d; j.p = c.p;
    return j;
}
static void jac_query_args(JacArgs& j, const PostChain& W, const PostQuery& q) {
    j.Xs = q.Xs; j.ldxs = q.ldxs; j.nstar = q.nstar;
    j.Ts = W.P.Ts; j.chunk = W.jchunk; j.nch = W.jnch; j.dgroups = W.jdgroups;
    j.part = W.jpart; j.cnt = W.jcnt; j.dgl = W.jdgl;
    j.J = q.jac->J; j.ldj = q.jac->ldj;
}
template <int NB>
static int gpr_jacobian_weights_impl(mfgp_handle_t h, const GprCacheRef& r, void* weights, size_t weights_bytes) {
    const GprCache c = gpr_cache_layout(NB, r);
    if (r.cache_bytes < c.bytes || weights_bytes < jac_weights_bytes(c.npad, c.ppad)) return MFGP_ERR_WORKSPACE;
    launch_jac_weights<NB>(gpr_jac_args(c, (double*)weights), 1, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

static int gpr_posterior_build_impl(mfgp_handle_t h, const GprProblem& P, const GprCacheRef& r) {
    const GprLayout L = gpr_layout(h->nb, P, gpr_sched_no_flow(h));
    const GprCache c = gpr_cache_layout(h->nb, r);
    if (P.ws_bytes < L.bytes || r.cache_bytes < c.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    gpr_factor(h->nb, s, L, P);
    copy_block(s, P.X, P.ldx, c.X, P.d + 1, P.n, P.d + 1);
    copy_block(s, P.theta, c.G, c.theta, c.G, 1, c.G);
    copy_block(s, L.Xo, c.ldr, c.LZ, c.ldr, c.npad, (int)c.ldr);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

static bool logdens_io_ok(const LogdensIO& q, int nstar, int p, int d) {
    return mvn_logpdf_geometry_ok(nstar, p, q.obs_cov != nullptr, q.ldc, q.y_rs, q.ov_rs) && q.Y && q.logp && q.info &&
           (!q.gX || q.ldgx >= d + 1);
}
// the density launch (mfgp_density.hip) on the forward's outputs; with dens->gX its gradients into W.gm / W.gv
static void logdens_launch(hipStream_t s, const PostChain& W, const PostQuery& q, int p, bool svgp) {
    const LogdensIO& dn = *q.dens;
    LogpdfArgs a{};
    a.ns = q.nstar; a.p = p;
    a.mean = q.mean; a.ldm = q.ldm;
    a.Y = dn.Y; a.y_rs = dn.y_rs;
    a.var = q.var; a.var_rs = svgp ? p : 1; a.var_cs = svgp ? 1 : 0;
    a.obs_var = dn.obs_var; a.ov_rs = dn.ov_rs;
    a.obs_cov = dn.obs_cov; a.ldc = dn.ldc;
    a.logp = dn.logp; a.info = dn.info;
    if (dn.gX) {
        a.gmean = W.gm; a.ldgm = p;
        a.gvar = W.gv; a.ldgv = svgp ? p : 1; a.gv_sum = svgp ? 0 : 1;
    }
    launch_mvn_logpdf(a, s);
}

// The GPR forward calls: predict (q.cov optional), predict-VJP (q.grad: upstream gradients in, input
// gradient out) and log-density (q.dens: the forward, the density launch on its mean / var, then -- with
// an input gradient asked for -- k_post_grad).
template <int NB>
static int gpr_posterior_forward(mfgp_handle_t h, const GprCacheRef& r, const PostQuery& q) {
    const GprCache c = gpr_cache_layout(NB, r);
    const PostChain W = post_chain(NB, post_dims(c), q.nstar, q.ws);
    if (r.cache_bytes < c.bytes || q.ws_bytes < post_ws_need(W, q)) return MFGP_ERR_WORKSPACE;
    if (q.jac && q.jac->weights_bytes < jac_weights_bytes(c.npad, c.ppad)) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    const bool grad = post_wants_grad(q);
    PostArgs a = gpr_post_args(c, W.P, q, q.cov || grad);
    if (grad) post_grad_args(a, W, q, c.p);
    launch_post<NB>(a, 1, s);
    if (q.dens) logdens_launch(s, W, q, c.p, false);
    if (grad) launch_post_grad<NB>(a, 1, s);
    if (q.jac) {
        (void)hipMemsetAsync(W.jcnt, 0, W.jcnt_bytes, s);
        JacArgs j = gpr_jac_args(c, (double*)q.jac->weights);
        jac_query_args(j, W, q);
        launch_jac_gpr<NB>(j, s);
    }
    if (q.cov)
        cov_from_a<NB>(s, q.Xs, q.ldxs, q.nstar, c.theta, c.d, c.nlf, W.P.Am, W.P.nspad, c.T, W.P.Kss, W.P.Cov, q.cov,
                       q.ldc);
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
// One design call: score (pick == nullptr; refresh: the forward first) or append row k of E for the
// candidate *pick.
struct DesignCall {
    const double* Xall; int ldx, nref, ncand;
    const double* w; double* E; int ldE, k;
    void* ws; size_t ws_bytes;
    double* score; int refresh; const int* pick;
};
static DesignLayout design_layout(int nb, const GprCache& c, int nref, int ncand, void* ws) {
    DesignLayout L{};
    L.nall = nref + ncand;
    L.Tr = ceil_div(nref > 0 ? nref : 1, nb);
    L.Tc = ceil_div(ncand > 0 ? ncand : 1, nb);
    L.nrun = ceil_div(L.Tr, design_run(nb));
    L.ncb = ceil_div(L.nall > 0 ? L.nall : 1, NTHREADS);
    L.nrch = ceil_div(c.T * nb, DESIGN_RROWS);
    Carve cn(ws);
    L.cnt_bytes = (sizeof(int) * ((size_t)L.Tc + L.ncb) + 15) & ~(size_t)15;
    L.cnt = cn.take<int>(L.cnt_bytes / sizeof(int));
    Behind cp(ws, cn.off);
    L.P = post_layout(nb, c.T, c.Tp, L.nall, 1, false, cp.base, false);
    Behind co(cp, L.P.bytes);
    L.mean = co.take<double>((size_t)L.nall * c.p);
    L.var = co.take<double>((size_t)L.nall);
    L.dpart = co.take<double>((size_t)L.nrun * L.Tc * nb);
    L.rpart = co.take<double>((size_t)L.nrch * L.ncb * NTHREADS);
    L.bytes = co.end();
    return L;
}

template <int NB>
static int gpr_posterior_design_impl(mfgp_handle_t h, const GprCacheRef& r, const DesignCall& D) {
    const GprCache c = gpr_cache_layout(NB, r);
    const DesignLayout L = design_layout(NB, c, D.nref, D.ncand, D.ws);
    if (r.cache_bytes < c.bytes || D.ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    if (!D.pick && D.nref == 0) {   // nothing to buy down: zeros, after the same size checks as any other call
        (void)hipMemsetAsync(D.score, 0, sizeof(double) * (size_t)D.ncand, s);
        return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
    }
    if (!D.pick && D.refresh)
        launch_post<NB>(
            gpr_post_args(c, L.P, PostQuery{L.nall, D.Xall, D.ldx, D.ws, D.ws_bytes, L.mean, c.p, L.var}, true), 1, s);
    (void)hipMemsetAsync(L.cnt, 0, L.cnt_bytes, s);
    DesignArgs g{};
    g.Am = L.P.Am; g.ldam = L.P.nspad; g.npad = c.npad;
    g.var = L.var;
    g.Xall = D.Xall; g.ldx = D.ldx; g.nref = D.nref; g.ncand = D.ncand;
    g.theta = c.theta; g.noise = c.noise();
    g.D = c.d; g.nlf = c.nlf;
    g.w = D.w;
    g.E = D.E; g.ldE = D.ldE; g.k = D.k;
    g.T = c.T; g.Tr = L.Tr; g.Tc = L.Tc; g.nrun = L.nrun;
    g.dpart = L.dpart; g.dcnt = L.cnt; g.score = D.score;
    g.pick = D.pick; g.Erow = D.pick ? D.E + (size_t)D.k * D.ldE : nullptr;
    g.ncb = L.ncb; g.nrch = L.nrch; g.rpart = L.rpart; g.rcnt = L.cnt + L.Tc;
    if (D.pick) launch_design_row(g, s);
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
    L.chunk = c.T > 128 ? ceil_div(c.T, 32) : 4;
    L.ntask = append_ntasks(c.T, L.chunk);
    L.nfill = std::min(ceil_div(c.n + k, nb) * nb, 256);
    Behind cv(ws, L.P.bytes);
    L.mean = cv.take<double>((size_t)APPEND_MAXK * c.p);
    L.var = cv.take<double>((size_t)APPEND_MAXK);
    L.W = cv.take<double>((size_t)APPEND_MAXK * c.npad);
    L.Rw = cv.take<double>((size_t)APPEND_MAXK * APPEND_MAXK);
    L.cnt = cv.take<int>((size_t)c.T);
    L.part = cv.take<double>((size_t)L.ntask * APPEND_MAXK * nb);
    L.bytes = cv.end();
    return L;
}

// One append call: k rows Xadd (observed at Yadd, or at their own mean) into out_cache.
struct AppendCall {
    int k;
    const double* Xadd; int ldxa; const double* Yadd; int ldya;
    void* ws; size_t ws_bytes; void* out_cache; size_t out_bytes;
    double* mean_add; int ldm; int* info;
};
template <int NB>
static int gpr_posterior_append_impl(mfgp_handle_t h, const GprCacheRef& r, const AppendCall& A) {
    const GprCache c = gpr_cache_layout(NB, r);
    const GprCache o = gpr_cache_layout(NB, GprCacheRef{r.nlf, r.n + A.k, r.p, r.d, A.out_cache, A.out_bytes});
    const AppendLayout L = append_layout(NB, c, A.k, A.ws);
    if (r.cache_bytes < c.bytes || A.out_bytes < o.bytes || A.ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    double* mean = A.mean_add ? A.mean_add : L.mean;
    const int ldmean = A.mean_add ? A.ldm : c.p;
    PostArgs a = gpr_post_args(c, L.P, PostQuery{A.k, A.Xadd, A.ldxa, A.ws, A.ws_bytes, mean, ldmean, L.var}, true);
    a.swap = 1;   // the new rows sit below the cached ones: the cross block has the new row as its row argument
    launch_post<NB>(a, 1, s);
    AppendArgs g{};
    g.LZ = c.LZ; g.ldr = c.ldr; g.X = c.X; g.theta = c.theta;
    g.n = c.n; g.npad = c.npad; g.T = c.T;
    g.p = c.p; g.ppad = c.ppad; g.D = c.d; g.nlf = c.nlf; g.G = c.G; g.k = A.k;
    g.diag_add = c.nlf ? GRAPH_JITTER : 0.0;
    g.Xadd = A.Xadd; g.ldxa = A.ldxa; g.Yadd = A.Yadd; g.ldya = A.ldya;
    g.Am = L.P.Am; g.ldam = L.P.nspad;
    g.mean = mean; g.ldm = ldmean;
    g.W = L.W; g.Rw = L.Rw; g.cnt = L.cnt; g.part = L.part;
    g.chunk = L.chunk; g.ntask = L.ntask; g.nfill = L.nfill;
    g.LZo = o.LZ; g.ldro = o.ldr; g.npado = o.npad;
    g.Xo = o.X; g.thetao = o.theta;
    g.obase = (unsigned char*)A.out_cache;
    o.gaps(g.gap0, g.gap1);
    g.info = A.info;
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
static SvgpCache svgp_cache_layout(int nb, const SvgpCacheRef& r) {
    SvgpCache c;
    c.Tm = ceil_div(r.m, nb);
    c.mpad = c.Tm * nb;
    c.G = theta_size(r.d);
    const size_t mm = (size_t)c.mpad * c.mpad;
    Carve cv(const_cast<void*>(r.cache));
    c.Z = cv.take<double>((size_t)r.m * (r.d + 1));
    c.thetas = cv.take<double>((size_t)r.l * c.G);
    c.W = cv.take<double>((size_t)r.p * r.l);
    c.qmu = cv.take<double>((size_t)r.l * c.mpad);
    c.Li = cv.take<double>(mm * r.l);
    c.C = cv.take<double>(mm * r.l);
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

// P: the variational state and the factorization's workspace (the entry fills it as an SVGP entry does)
static int svgp_posterior_build_impl(mfgp_handle_t h, const SvgpProblem& P, const SvgpCacheRef& r) {
    const SvgpCache c = svgp_cache_layout(h->nb, r);
    if (r.cache_bytes < c.bytes || P.ws_bytes < svgp_posterior_factor_bytes(h->nb, P.m, P.l)) return MFGP_ERR_WORKSPACE;
    hipStream_t s = h->stream;
    const int rc = svgp_posterior_factor(h->nb, s, P, c.Li, c.C);
    if (rc) return rc == -2 ? MFGP_ERR_WORKSPACE : MFGP_ERR_LAUNCH;
    copy_block(s, P.Z, P.ldz, c.Z, P.d + 1, P.m, P.d + 1);
    copy_block(s, P.thetas, c.G, c.thetas, c.G, P.l, c.G);
    if (P.W) copy_block(s, P.W, P.l, c.W, P.l, P.p, P.l);
    const long tot = (long)P.l * c.mpad;
    hipLaunchKernelGGL(k_post_qmu_pad, dim3((int)std::min<long>((tot + 255) / 256, 2048)), dim3(256), 0, s, P.q_mu, P.m,
                       P.l, c.mpad, c.qmu);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

static JacArgs svgp_jac_args(const SvgpCache& c, const SvgpCacheRef& r, double* weights) {
    JacArgs j{};
    j.Li = c.Li; j.ldl = c.mpad; j.sL = (long)c.mpad * c.mpad;
    j.qmu = c.qmu;
    j.T = c.Tm; j.Tp = 0;
    j.alpha = weights; j.sA = c.mpad;
    j.X1 = c.Z; j.ldx1 = r.d + 1; j.n1 = r.m;
    j.theta = c.thetas; j.stheta = c.G;
    j.D = r.d; j.p = r.p;
    j.W = r.mixed ? c.W : nullptr; j.L = r.l;
    return j;
}

// The SVGP forward calls: predict, predict-VJP (q.grad) and log-density (q.dens), as the GPR ones
static int svgp_posterior_forward(mfgp_handle_t h, const SvgpCacheRef& r, const PostQuery& q) {
    const SvgpCache c = svgp_cache_layout(h->nb, r);
    const PostChain W = post_chain(h->nb, post_dims(h->nb, r), q.nstar, q.ws);
    if (r.cache_bytes < c.bytes || q.ws_bytes < post_ws_need(W, q)) return MFGP_ERR_WORKSPACE;
    if (q.jac && q.jac->weights_bytes < jac_weights_bytes(r.l, c.mpad)) return MFGP_ERR_WORKSPACE;
    const PostLayout& P = W.P;
    const bool grad = post_wants_grad(q);
    const long mm = (long)c.mpad * c.mpad;
    PostArgs a{};
    a.Li = c.Li; a.ldl = c.mpad; a.sL = mm;
    a.C = c.C; a.ldc = c.mpad; a.sC = mm;
    a.X1 = c.Z; a.ldx1 = r.d + 1; a.n1 = r.m;
    a.theta = c.thetas; a.stheta = c.G;
    a.Xs = q.Xs; a.ldxs = q.ldxs; a.nstar = q.nstar;
    a.D = r.d; a.nlf = 0;
    a.T = c.Tm; a.Ts = P.Ts; a.chunk = P.chunk; a.full = 1; a.ntask = P.ntask; a.ngrp = P.ngrp;
    a.Apart = P.Apart; a.Bpart = P.Bpart; a.cnt = P.cnt;
    a.p = r.p;
    a.qmu = c.qmu; a.pa = P.pa; a.pb = P.pb; a.pm = P.pm; a.gm = P.gm; a.gv = P.gv;
    a.W = r.mixed ? c.W : nullptr;
    a.f_mu = q.mean; a.f_var = q.var;
    if (grad) {
        a.Am = W.Am; a.Bm = W.Bm; a.ldam = P.nspad; a.sAm = (long)c.mpad * P.nspad;
        post_grad_args(a, W, q, r.p);
    }
    TILE_CALL(h->nb, launch_post, a, r.l, h->stream);
    if (q.dens) logdens_launch(h->stream, W, q, r.p, true);
    if (grad) TILE_CALL(h->nb, launch_post_grad, a, r.l, h->stream);
    if (q.jac) {
        JacArgs j = svgp_jac_args(c, r, (double*)q.jac->weights);
        jac_query_args(j, W, q);
        TILE_CALL(h->nb, launch_jac_svgp, j, r.l, h->stream);
    }
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}
static int svgp_jacobian_weights_impl(mfgp_handle_t h, const SvgpCacheRef& r, void* weights, size_t weights_bytes) {
    const SvgpCache c = svgp_cache_layout(h->nb, r);
    if (r.cache_bytes < c.bytes || weights_bytes < jac_weights_bytes(r.l, c.mpad)) return MFGP_ERR_WORKSPACE;
    const JacArgs j = svgp_jac_args(c, r, (double*)weights);
    TILE_CALL(h->nb, launch_jac_weights, j, r.l, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

static inline bool design_geometry_ok(int nref, int ncand) {
    return nref >= 0 && ncand >= 0 && (long)nref + ncand <= 0x7fffffffL - 4096;
}
static inline bool append_geometry_ok(int n, int k) {
    return k >= 1 && k <= APPEND_MAXK && (long)n + k <= 0x7fffffffL - 4096;
}

// The workspace queries of the forward calls (kind: &PostChain::predict / vjp / logdens).  They reject
// nstar == 0 (the GPR predict queries take it).  The SVGP ones know no mixing flag: mixed = 1, nothing to check.
using PostKind = size_t PostChain::*;
static int gpr_post_ws_size(mfgp_handle_t h, const GprCacheRef& c, int nstar, PostKind kind, size_t* bytes) {
    if (const int rc = gpr_post_check(h, c, nstar >= 1 && bytes)) return rc;
    *bytes = post_chain(h->nb, post_dims(gpr_cache_layout(h->nb, c)), nstar, nullptr).*kind;
    return MFGP_OK;
}
static int svgp_post_ws_size(mfgp_handle_t h, const SvgpCacheRef& c, int nstar, PostKind kind, size_t* bytes) {
    if (const int rc = svgp_post_check(h, c, nstar >= 1 && bytes)) return rc;
    *bytes = post_chain(h->nb, post_dims(h->nb, c), nstar, nullptr).*kind;
    return MFGP_OK;
}

}  // namespace mfgp

using namespace mfgp;

extern "C" {

// Every entry fills its descriptors, then checks (gpr_post_check / svgp_post_check).  Where an entry returns
// MFGP_OK early for an empty call, the checks before that return are its own lines, CHECK_H and CHECK_D among
// them (the helper behind the return then sees a handle and a d that are good): tests/test_capi_codes.py pins
// which side of the return each check is on.

int mfgp_gpr_posterior_size(mfgp_handle_t h, int nlf, int n, int p, int d, size_t* bytes) {
    const GprCacheRef c{nlf, n, p, d};
    if (const int rc = gpr_post_check(h, c, bytes != nullptr)) return rc;
    *bytes = gpr_cache_layout(h->nb, c).bytes;
    return MFGP_OK;
}

int mfgp_gpr_posterior_build(mfgp_handle_t h, int nlf, int n, int p, int d, const double* X, int ldx, const double* Y,
                             int ldy, const double* theta, void* ws, size_t ws_bytes, void* cache, size_t cache_bytes,
                             int* info) {
    const GprProblem P{n, p, d, nlf, X, ldx, Y, ldy, theta, ws, ws_bytes, info};
    if (const int rc = gpr_check(h, P, 0, cache && ldx >= d + 1 && ldy >= p)) return rc;
    return gpr_posterior_build_impl(h, P, GprCacheRef{nlf, n, p, d, cache, cache_bytes});
}

int mfgp_gpr_posterior_predict_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                              size_t* bytes) {
    return gpr_post_ws_size(h, GprCacheRef{nlf, n, p, d}, nstar, &PostChain::predict, bytes);
}

// no nstar == 0 return here: an empty predict is an argument error
int mfgp_gpr_posterior_predict(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                               size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes, double* mean,
                               int ldm, double* var, double* cov, int ldc) {
    const GprCacheRef c{nlf, n, p, d, cache, cache_bytes};
    const PostQuery q{nstar, Xs, ldxs, ws, ws_bytes, mean, ldm, var, cov, ldc};
    if (const int rc = gpr_post_check(h, c, nstar >= 1 && post_query_ok(q, cache, p, d) && !(cov && ldc < nstar)))
        return rc;
    return TILE_CALL(h->nb, gpr_posterior_forward, h, c, q);
}

int mfgp_gpr_posterior_predict_vjp_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                                  size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf != 0) return MFGP_ERR_ARG;
    return gpr_post_ws_size(h, GprCacheRef{nlf, n, p, d}, nstar, &PostChain::vjp, bytes);
}

int mfgp_gpr_posterior_predict_vjp(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                                   size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                   double* mean, int ldm, double* var, const double* gmean, int ldgm,
                                   const double* gvar, double* gX, int ldgx) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf != 0) return MFGP_ERR_ARG;   // the graph kernel's per-source derivative is not built
    if (nstar == 0) return MFGP_OK;      // behind nlf, before the sizes and the pointers
    const GprCacheRef c{nlf, n, p, d, cache, cache_bytes};
    const PostGradIO g{gmean, ldgm, gvar, gX, ldgx};
    const PostQuery q{nstar, Xs, ldxs, ws, ws_bytes, mean, ldm, var, nullptr, 0, &g};
    if (const int rc = gpr_post_check(h, c, nstar > 0 && post_query_ok(q, cache, p, d) && gX && ldgx >= d + 1 &&
                                                !(gmean && ldgm < p)))
        return rc;
    return TILE_CALL(h->nb, gpr_posterior_forward, h, c, q);
}

int mfgp_gpr_posterior_logdens_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                              size_t* bytes) {
    // (the graph kernel has the value only: the predict layout)
    const PostKind kind = nlf ? &PostChain::predict : &PostChain::logdens;
    return gpr_post_ws_size(h, GprCacheRef{nlf, n, p, d}, nstar, kind, bytes);
}

int mfgp_gpr_posterior_logdens(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                               size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes, double* mean,
                               int ldm, double* var, const double* Y, long y_rs, const double* obs_var, long ov_rs,
                               const double* obs_cov, int ldc, double* logp, double* gX, int ldgx, int* info) {
    CHECK_H(h);
    CHECK_D(d);
    // the graph kernel has no input gradient; both before the nstar == 0 return, the sizes and the rest behind it
    if (nlf < 0 || nlf > MFGP_MAX_LF || (nlf != 0 && gX)) return MFGP_ERR_ARG;
    if (nstar == 0) return MFGP_OK;
    const GprCacheRef c{nlf, n, p, d, cache, cache_bytes};
    const LogdensIO dn{Y, y_rs, obs_var, ov_rs, obs_cov, ldc, logp, gX, ldgx, info};
    const PostQuery q{nstar, Xs, ldxs, ws, ws_bytes, mean, ldm, var, nullptr, 0, nullptr, &dn};
    const bool ok = nstar > 0 && post_query_ok(q, cache, p, d) && logdens_io_ok(dn, nstar, p, d);
    if (const int rc = gpr_post_check(h, c, ok)) return rc;
    return TILE_CALL(h->nb, gpr_posterior_forward, h, c, q);
}

int mfgp_gpr_posterior_leave_out_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int ngroups, int nrows,
                                                size_t* bytes) {
    const bool ok = ngroups >= 1 && nrows >= ngroups && bytes;
    if (const int rc = gpr_post_check(h, GprCacheRef{nlf, n, p, d}, ok)) return rc;
    *bytes = lo_layout(n, p, ngroups, nrows, LO_W, nullptr).bytes;   // groups of any size up to 32
    return MFGP_OK;
}

int mfgp_gpr_posterior_leave_out(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache, size_t cache_bytes,
                                 int ngroups, const int* offsets, const int* rows, int nrows, int gmax, void* ws,
                                 size_t ws_bytes, double* resid, int ldr, double* cov, int ldc, double* logdens,
                                 int* info) {
    CHECK_H(h);
    CHECK_D(d);
    // nlf, ngroups < 0 and gmax before the ngroups == 0 return; the sizes and the pointers behind it
    if (nlf < 0 || nlf > MFGP_MAX_LF || ngroups < 0 || gmax < 1 || gmax > LO_W) return MFGP_ERR_ARG;
    if (ngroups == 0) return MFGP_OK;
    const GprCacheRef r{nlf, n, p, d, cache, cache_bytes};
    if (const int rc = gpr_post_check(h, r, nrows >= ngroups && cache && offsets && rows && ws && resid && logdens &&
                                                info && ldr >= p && !(cov && ldc < gmax)))
        return rc;
    const GprCache c = gpr_cache_layout(h->nb, r);
    const LoLayout L = lo_layout(n, p, ngroups, nrows, gmax, ws);
    if (cache_bytes < c.bytes || ws_bytes < L.bytes) return MFGP_ERR_WORKSPACE;
    LoArgs a{};
    a.LZ = c.LZ; a.ldr = c.ldr; a.npad = c.npad;
    a.noise = c.noise();
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
    const GprCacheRef c{nlf, n, p, d};
    const bool ok = design_geometry_ok(nref, ncand) && qmax >= 0 && qmax <= DESIGN_MAXQ && bytes;
    if (const int rc = gpr_post_check(h, c, ok)) return rc;
    *bytes = design_layout(h->nb, gpr_cache_layout(h->nb, c), nref, ncand, nullptr).bytes;
    return MFGP_OK;
}

// Both design entries: the geometry and k's range before the ncand == 0 return, the pointers behind it.
// k <= DESIGN_MAXQ rows of E condition a score, so row k < DESIGN_MAXQ is the last one to append.
int mfgp_gpr_posterior_design_score(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache,
                                    size_t cache_bytes, const double* Xall, int ldx, int nref, int ncand,
                                    const double* w, const double* E, int ldE, int k, void* ws, size_t ws_bytes,
                                    double* score, int refresh) {
    const GprCacheRef c{nlf, n, p, d, cache, cache_bytes};
    if (const int rc = gpr_post_check(h, c, design_geometry_ok(nref, ncand) && k >= 0 && k <= DESIGN_MAXQ)) return rc;
    if (ncand == 0) return MFGP_OK;
    if (!cache || !Xall || !ws || !score || ldx < d + 1 || (k > 0 && (!E || ldE < nref + ncand))) return MFGP_ERR_ARG;
    double* Em = const_cast<double*>(E);   // (only read in this mode)
    const DesignCall D{Xall, ldx, nref, ncand, w, Em, ldE, k, ws, ws_bytes, score, refresh, nullptr};
    return TILE_CALL(h->nb, gpr_posterior_design_impl, h, c, D);
}

int mfgp_gpr_posterior_design_append(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache,
                                     size_t cache_bytes, const double* Xall, int ldx, int nref, int ncand, void* ws,
                                     size_t ws_bytes, const int* pick, double* E, int ldE, int k) {
    const GprCacheRef c{nlf, n, p, d, cache, cache_bytes};
    if (const int rc = gpr_post_check(h, c, design_geometry_ok(nref, ncand) && k >= 0 && k < DESIGN_MAXQ)) return rc;
    if (ncand == 0) return MFGP_OK;
    if (!cache || !Xall || !ws || !pick || !E || ldx < d + 1 || ldE < nref + ncand) return MFGP_ERR_ARG;
    const DesignCall D{Xall, ldx, nref, ncand, nullptr, E, ldE, k, ws, ws_bytes, nullptr, 0, pick};
    return TILE_CALL(h->nb, gpr_posterior_design_impl, h, c, D);
}

int mfgp_gpr_posterior_append_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int k, size_t* bytes) {
    const GprCacheRef c{nlf, n, p, d};
    if (const int rc = gpr_post_check(h, c, append_geometry_ok(n, k) && bytes)) return rc;
    *bytes = append_layout(h->nb, gpr_cache_layout(h->nb, c), k, nullptr).bytes;
    return MFGP_OK;
}

// Yadd and mean_add are optional: their leading dimensions count only when they are given
int mfgp_gpr_posterior_append(mfgp_handle_t h, int nlf, int n, int p, int d, int k, const void* cache,
                              size_t cache_bytes, const double* Xadd, int ldxa, const double* Yadd, int ldya, void* ws,
                              size_t ws_bytes, void* out_cache, size_t out_bytes, double* mean_add, int ldm,
                              int* info) {
    const GprCacheRef c{nlf, n, p, d, cache, cache_bytes};
    if (const int rc = gpr_post_check(h, c, append_geometry_ok(n, k) && cache && Xadd && ws && out_cache && info &&
                                                out_cache != cache && ldxa >= d + 1 && !(Yadd && ldya < p) &&
                                                !(mean_add && ldm < p)))
        return rc;
    const AppendCall A{k, Xadd, ldxa, Yadd, ldya, ws, ws_bytes, out_cache, out_bytes, mean_add, ldm, info};
    return TILE_CALL(h->nb, gpr_posterior_append_impl, h, c, A);
}

int mfgp_svgp_posterior_size(mfgp_handle_t h, int m, int l, int p, int d, size_t* bytes) {
    const SvgpCacheRef c{m, l, p, d, 1};
    if (const int rc = svgp_post_check(h, c, bytes != nullptr)) return rc;
    *bytes = svgp_cache_layout(h->nb, c).bytes;
    return MFGP_OK;
}

int mfgp_svgp_posterior_build(mfgp_handle_t h, int m, int l, int p, int d, const double* Z, int ldz,
                              const double* thetas, const double* q_mu, const double* q_sqrt, const double* W,
                              double jitter, void* ws, size_t ws_bytes, void* cache, size_t cache_bytes, int* info) {
    const SvgpCacheRef c{m, l, p, d, W != nullptr, cache, cache_bytes};   // no W: a latent per output
    if (const int rc = svgp_post_check(h, c, Z && thetas && q_mu && q_sqrt && ws && cache && info && ldz >= d + 1))
        return rc;
    SvgpProblem P{};
    P.m = m; P.l = l; P.p = p; P.d = d;
    P.Z = Z; P.ldz = ldz; P.thetas = thetas; P.q_mu = q_mu; P.q_sqrt = q_sqrt; P.W = W;
    P.jitter = jitter; P.ws = ws; P.ws_bytes = ws_bytes; P.info = info;
    return svgp_posterior_build_impl(h, P, c);
}

int mfgp_svgp_posterior_predict_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes) {
    return svgp_post_ws_size(h, SvgpCacheRef{m, l, p, d, 1}, nstar, &PostChain::predict, bytes);
}
int mfgp_svgp_posterior_predict_vjp_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d,
                                                   size_t* bytes) {
    return svgp_post_ws_size(h, SvgpCacheRef{m, l, p, d, 1}, nstar, &PostChain::vjp, bytes);
}
int mfgp_svgp_posterior_logdens_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes) {
    return svgp_post_ws_size(h, SvgpCacheRef{m, l, p, d, 1}, nstar, &PostChain::logdens, bytes);
}

// no nstar == 0 return here either
int mfgp_svgp_posterior_predict(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed, const void* cache,
                                size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                double* f_mu, double* f_var) {
    const SvgpCacheRef c{m, l, p, d, mixed, cache, cache_bytes};
    const PostQuery q{nstar, Xs, ldxs, ws, ws_bytes, f_mu, p, f_var};
    if (const int rc = svgp_post_check(h, c, nstar >= 1 && post_query_ok(q, cache, p, d))) return rc;
    return svgp_posterior_forward(h, c, q);
}

// Both below: the nstar == 0 return first behind the handle and d, everything else behind it.
int mfgp_svgp_posterior_predict_vjp(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed,
                                    const void* cache, size_t cache_bytes, const double* Xs, int ldxs, void* ws,
                                    size_t ws_bytes, double* f_mu, double* f_var, const double* gmean, int ldgm,
                                    const double* gvar, double* gX, int ldgx) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar == 0) return MFGP_OK;
    const SvgpCacheRef c{m, l, p, d, mixed, cache, cache_bytes};
    const PostGradIO g{gmean, ldgm, gvar, gX, ldgx};
    const PostQuery q{nstar, Xs, ldxs, ws, ws_bytes, f_mu, p, f_var, nullptr, 0, &g};
    if (const int rc = svgp_post_check(h, c, nstar > 0 && post_query_ok(q, cache, p, d) && gX && ldgx >= d + 1 &&
                                                 !(gmean && ldgm < p)))
        return rc;
    return svgp_posterior_forward(h, c, q);
}

int mfgp_svgp_posterior_logdens(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed, const void* cache,
                                size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                double* f_mu, double* f_var, const double* Y, long y_rs, const double* obs_var,
                                long ov_rs, const double* obs_cov, int ldc, double* logp, double* gX, int ldgx,
                                int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar == 0) return MFGP_OK;
    const SvgpCacheRef c{m, l, p, d, mixed, cache, cache_bytes};
    const LogdensIO dn{Y, y_rs, obs_var, ov_rs, obs_cov, ldc, logp, gX, ldgx, info};
    const PostQuery q{nstar, Xs, ldxs, ws, ws_bytes, f_mu, p, f_var, nullptr, 0, nullptr, &dn};
    const bool ok = nstar > 0 && post_query_ok(q, cache, p, d) && logdens_io_ok(dn, nstar, p, d);
    if (const int rc = svgp_post_check(h, c, ok)) return rc;
    return svgp_posterior_forward(h, c, q);
}

// ---- the Jacobian entries (mfgp_jacobian.hip).  The linear multi-fidelity kernel only: nlf > 0 is MFGP_ERR_ARG
// behind the handle and d, as the VJP entries; the nstar == 0 return next, everything else behind it.

int mfgp_gpr_jacobian_weights_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf != 0) return MFGP_ERR_ARG;
    const GprCacheRef c{nlf, n, p, d};
    if (const int rc = gpr_post_check(h, c, bytes != nullptr)) return rc;
    const GprCache g = gpr_cache_layout(h->nb, c);
    *bytes = jac_weights_bytes(g.npad, g.ppad);
    return MFGP_OK;
}

int mfgp_gpr_jacobian_weights(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache, size_t cache_bytes,
                              void* weights, size_t weights_bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf != 0) return MFGP_ERR_ARG;
    const GprCacheRef c{nlf, n, p, d, cache, cache_bytes};
    if (const int rc = gpr_post_check(h, c, cache && weights)) return rc;
    return TILE_CALL(h->nb, gpr_jacobian_weights_impl, h, c, weights, weights_bytes);
}

int mfgp_gpr_jacobian_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf != 0) return MFGP_ERR_ARG;
    return gpr_post_ws_size(h, GprCacheRef{nlf, n, p, d}, nstar, &PostChain::jac, bytes);
}

int mfgp_gpr_jacobian(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache, size_t cache_bytes,
                      const void* weights, size_t weights_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                      double* mean, int ldm, double* var, double* J, int ldj) {
    CHECK_H(h);
    CHECK_D(d);
    if (nlf != 0) return MFGP_ERR_ARG;   // the graph kernel's per-source derivative is not built
    if (nstar == 0) return MFGP_OK;
    const GprCacheRef c{nlf, n, p, d, cache, cache_bytes};
    const JacIO jio{weights, weights_bytes, J, ldj};
    const PostQuery q{nstar, Xs, ldxs, ws, ws_bytes, mean, ldm, var, nullptr, 0, nullptr, nullptr, &jio};
    if (const int rc = gpr_post_check(h, c, nstar > 0 && post_query_ok(q, cache, p, d) && weights && J && ldj >= p))
        return rc;
    return TILE_CALL(h->nb, gpr_posterior_forward, h, c, q);
}

int mfgp_svgp_jacobian_weights_workspace_size(mfgp_handle_t h, int m, int l, int p, int d, size_t* bytes) {
    const SvgpCacheRef c{m, l, p, d, 1};
    if (const int rc = svgp_post_check(h, c, bytes != nullptr)) return rc;
    *bytes = jac_weights_bytes(l, svgp_cache_layout(h->nb, c).mpad);
    return MFGP_OK;
}

int mfgp_svgp_jacobian_weights(mfgp_handle_t h, int m, int l, int p, int d, int mixed, const void* cache,
                               size_t cache_bytes, void* weights, size_t weights_bytes) {
    const SvgpCacheRef c{m, l, p, d, mixed, cache, cache_bytes};
    if (const int rc = svgp_post_check(h, c, cache && weights)) return rc;
    return svgp_jacobian_weights_impl(h, c, weights, weights_bytes);
}

int mfgp_svgp_jacobian_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes) {
    return svgp_post_ws_size(h, SvgpCacheRef{m, l, p, d, 1}, nstar, &PostChain::jac, bytes);
}

int mfgp_svgp_jacobian(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed, const void* cache,
                       size_t cache_bytes, const void* weights, size_t weights_bytes, const double* Xs, int ldxs,
                       void* ws, size_t ws_bytes, double* f_mu, double* f_var, double* J, int ldj) {
    CHECK_H(h);
    CHECK_D(d);
    if (nstar == 0) return MFGP_OK;
    const SvgpCacheRef c{m, l, p, d, mixed, cache, cache_bytes};
    const JacIO jio{weights, weights_bytes, J, ldj};
    const PostQuery q{nstar, Xs, ldxs, ws, ws_bytes, f_mu, p, f_var, nullptr, 0, nullptr, nullptr, &jio};
    if (const int rc = svgp_post_check(h, c, nstar > 0 && post_query_ok(q, cache, p, d) && weights && J && ldj >= p))
        return rc;
    return svgp_posterior_forward(h, c, q);
}

}  // extern "C"
