// Internal (host<->device) argument blocks and launchers of the MI355X GP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// The one tile-size dispatch: fn<64>(args) or fn<32>(args), the argument list written once.
#define TILE_CALL(nb, fn, ...) \
    ((nb) == 64 ? fn<64>(__VA_ARGS__) : fn<32>(__VA_ARGS__))

namespace mfgp {

// Workspace carving: every block starts on a 256-byte boundary; base == nullptr only counts.
struct Carve {
    char* base;
    size_t off = 0;
    explicit Carve(void* b) : base((char*)b) {}
    template <class T>
    T* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

struct GramArgs {
    const double* X1; long ldx1; long sx1; int n1;
    const double* X2; long ldx2; long sx2; int n2;
    const double* theta; long stheta;         // per-batch theta stride (doubles)
    int D;
    int rbf_only;                             // 1: plain SquaredExponential on all D columns
    double* out; long ldo; long so;
    int padded;                               // 1: LML layout (square, lower tiles, identity pad)
    int npad;                                 // padded size (LML layout)
    int tiles_c;                              // number of column tiles (dense layout)
    int add_noise;                            // add theta noise on i==j<n (LML layout)
    double diag_add;                          // extra constant on i==j<n (jitter)
    // fused factor of tile (0,0) (LML layout only)
    double* Dd; long sD; double* ldiag; long sL; int* info;
    // fused RHS init (LML layout only; R == nullptr: skip): R = [I | Y]
    double* R; long ldr; long sR; const double* Y; long ldy; long sY; int p, ppad;
    int nlf;                                  // 0: LinearMultiFidelityKernel; m >= 1: graph kernel, m LF sources
    int* cnt; int ncnt;                       // arrival counters zeroed by workgroup 0 (reduce merge)
    double* isent; int nisent;                // k_reduce_items' items, FLOW_SENTINEL-filled by workgroup 0 (FinArgs::flag)
    // k_grad task order (nullptr: none): one extra LAST workgroup builds it (grad_order)
    int* gorder; int gT, gchunk, gTp;
    // k_chol_flow owner table (nullptr: none): one more extra workgroup builds it and zeroes
    // the flow flags (build_flow_owner); every workgroup fills its share of the publication
    // area with the sentinel
    int* fown; int fW; int* fflags; int nfflags;
    double* fpub; long npub;
    long long* dbg;               // diagnostic per-workgroup timeline (nullptr: off)
    // LML layout: > 0 -> that many tile workgroups, workgroup 0 takes tile (0,0) (and its fused
    // factor) alone on its CU, the others loop over the remaining tiles; 0 -> one tile each
    int tile_wgs;
};

constexpr int FIN_MAXG = 254;   // theta entries finalize_body stages in LDS (graph kernel: <= 186)
// k_reduce_items' sentinel protocol (FinArgs::flag) on the fp64 LML path; 0: arrival counter
#ifndef MFGP_REDUCE_FLAG
#define MFGP_REDUCE_FLAG 1
#endif
struct FinArgs {
    const double* zpart; int nz;
    const double* ldiag; int n;
    const double* gpart; int ng; int gstride;
    const int* info;
    int P, D, want_grad;
    double* out;                      // [lml, grad(G)]
    // Adam (optional, unconstrained parameters)
    int adam;
    double* theta;                    // constrained theta, refreshed after the step
    double* u; double* m; double* v;
    const unsigned char* trainable;
    const int* tie;                   // tie[q]: entries sharing one variable (isotropic lengthscales)
    int* step;
    double lr, b1, b2, eps;
    double* loss_hist;                // loss_hist[step] = -lml (pre-step)
    int noise_index;                  // theta entry using Shift(1e-6) o Softplus
    double* items;                    // [2 + G] stage-1 reduction results
    int G;                            // theta entries (kernel_theta_size)
    int* cnt;                         // arrival counter (zero on entry): last item workgroup finalizes
    int flag;                         // 1: items[] hold FLOW_SENTINEL on entry (the Gram launch filled them):
                                      //    workgroup 0 finalizes once every other item is published
    int* abortw;                      // flow path: k_chol_flow's abort word -- set: the evaluation timed
                                      // out (info := MFGP_FLOW_TIMEOUT); workgroup 0 zeroes it for the next
};

// k_chol_flow (mfgp_flow.hip): persistent dataflow Cholesky + L^{-1} + Z + alpha, NB = 32, batch 1
constexpr int FLOW_MAXOWN = 4;                      // tiles per worker wave
constexpr int FLOW_WAVES = 8;                       // waves per workgroup (two per SIMD)
constexpr int FLOW_THREADS = 64 * FLOW_WAVES;
constexpr int FLOW_FSTRIDE = 32;                    // ints per flag: one 128-B line each (polled lines
                                                    // are not shared, no hot line under 2k pollers)
constexpr size_t FLOW_LDS_BYTES = 128 * 1024;       // > 80 KB: one workgroup per CU
constexpr unsigned long long FLOW_SENTINEL = 0x7FF4DEAD7FF4DEADull;   // signalling NaN: "not yet published"
struct FlowArgs {
    double* A; long lda;          // K + s2 I lower tiles -> L tiles (in place)
    double* R; long ldr;          // [I | Y] accumulators -> X^T tiles (in place)
    double* Xo; long ldx;         // [L^{-1} | Z] (+ alpha^T rows for k_grad)
    double* Dd;                   // T diagonal inverses D_k (NB x NB)
    double* ldiag;
    int* info;
    double* alpha; long ldal;
    double* zpart;
    int* flags;                   // abort word (zeroed by build_flow_owner)
    double* pub;                  // publication area, flow_npub(T, Tp) doubles of FLOW_SENTINEL
    const int* own;               // [W * FLOW_MAXOWN] tile codes (-1: none)
    int T, Tp, n, p;
    long long* trace;             // diagnostic timeline (nullptr: off), flow_trace_count entries
    int nwaves;                   // worker waves (trace layout)
    long long timeout;            // bound of every hand-off wait, 100 MHz ticks (FLOW_TIMEOUT_TICKS)
    // the K + s2 I tiles are formed inside the launch (flow_gram_tile): each A tile by its owner
    // wave before its first item, tile (0,0) and the band tiles of rows 1-2 by the diag
    // workgroup's waves, row 3's by idle worker waves (FT_G); the Y column tiles of R are read
    // from Y on first touch
    const double* X; long ldxi;   // inputs [n, D+1] (fidelity flag in column D)
    const double* Y; long ldy;    // outputs [n, p]
    const double* theta;          // [vL, lL(D), vD, lD(D), rho0, noise]
    int D;
    int gram;                     // 1: the AR1 Gram formed in the launch; 0: A holds K + s2 I already
                                  // (the graph kernel's k_gram ran first)
    // Head phase (mfgp_gpr_adam_steps; flow_head_worker / flow_head_diag): head = 1 -> the launch first
    // finishes the PREVIOUS Adam step from fin (item sums, finalize, theta refresh) in place of
    // that step's k_reduce_items, then runs as usual on the new theta.  head = 0: fin is unused.
    int head;
    FinArgs fin;
};
// the head phase takes at most this many theta entries (its theta slot is the last 64 doubles of
// the publication area, flow_npub)
constexpr int FLOW_HEAD_MAXG = 62;   // G + 2 items, one lane each
constexpr long long FLOW_TIMEOUT_TICKS = 5000000;   // 50 ms (s_memrealtime is 100 MHz)
int flow_trace_count(int T, int nwg);

struct CholArgs {
    double* A; long lda; long sA;        // SPD matrix, lower tiles, updated in place
    double* R; long ldr; long sR;        // RHS [I | Y] (identity tiles 0..T-1, Y tiles T..T+Tp-1)
    double* Xo; long ldx; long sX;       // output [L^{-1} | Z]
    double* Dd; long sD;                 // T inverse diagonal factors (NB x NB each)
    double* ldiag; long sL;              // diag(L)
    int* info;
    int T, Tp, k;
    // Batched steps (k_chol_fused / k_chol_panel): R = [I | ...] is implicit -- the identity tile
    // R_kk and the untouched strictly-lower tiles (zero until the step c == k that first updates
    // R_ic) are formed in the kernels, so R needs no initialisation (the Gram skips writing it)
    int r_implicit;
    // Optional (batch 1, LML path): alpha = L^{-T} Z accumulated row by row as rows of
    // [L^{-1} | Z] become final, and the sum Z^2 partials.  nullptr: skipped.
    double* alpha; long ldal;            // Npad x Ppad
    double* zpart;                       // [T*Tp]
    int n, p;
};


struct GradArgs {
    const double* Xo; long ldx;           // [L^{-1} | Z], then rows [-alpha^T / P ; alpha^T] (Ppad each)
    const double* X; long ldxx;           // inputs [n, D+1]
    const double* theta;
    double* gpart; int gstride;           // per task partial gradient
    int T, Tp, n, P, D;
    int chunk;                            // m-tiles per task
    int nlf;                              // kernel family (GramArgs::nlf)
    const int* order;                     // workgroup -> task (nullptr: identity), see grad_order
    // flow path: the next evaluation's set-up, done here after the flow has ended -- every
    // workgroup sentinel-fills its share of the publication area, workgroup 0 the item slots of
    // k_reduce_items (nullptr: none)
    double* fpub; long npub;
    double* isent; int nisent;
};

struct PredAArgs {
    const double* Xo; long ldx;       // [L^{-1} | Z]
    const double* Kmn; long ldk;      // Npad x Nspad
    double* Am; long ldam;            // Npad x Nspad   A = L^{-1} Kmn
    int Ts;
};

struct PredOutArgs {
    const double* Am; long ldam;
    const double* Xo; long ldx;
    const double* kdiag;              // nstar
    double* mean; long ldm;           // nstar x p
    double* var;                      // nstar
    int T, Tp, nstar, p;
};

// Cached-posterior predict (mfgp_posterior.hip): A = L^{-1} K(X1, X*) against a cached inverse
// factor, K generated tile by tile in LDS.  Two launches: k_post_a (partial row products, one
// task = one row tile x `chunk` m-tiles) and k_post_out (fixed-order sum of a row tile's partials,
// its moment partials, and the last-arriving workgroup of a column tile writes the outputs).
// GPR (Zc != nullptr): mean = A^T Z, var = K_diag(X*) - colsum(A^2).  SVGP (qmu != nullptr), batched
// over latents: also B = C K (C = Lq^T Lm^{-1}, full rows), g_mu = A^T q_mu,
// g_var = Kff - colsum(A^2) + colsum(B^2), then the output mixing.
struct PostArgs {
    const double* Li; long ldl; long sL;      // L^{-1}, lower tiles (row-major), batch stride
    const double* C; long ldc; long sC;       // SVGP: Lq^T Lm^{-1} (all tiles); nullptr: none
    const double* X1; long ldx1; int n1;      // cached training inputs / inducing points [n1, D + 1]
    const double* theta; long stheta;         // cached kernel parameters, per batch entry
    const double* Xs; long ldxs; int nstar;
    int D, nlf;
    int T, Ts, chunk, full;                   // row tiles, column tiles, m-tiles per task, full rows (C)
    int ntask;                                // tasks per batch entry (post_ntasks)
    int ngrp;                                 // k_post_out workgroups per column tile: ceil(T / post_rg(NB)) row groups
    double* Apart; double* Bpart;             // [batch][ntask][Ts][NB * NB]
    int* cnt;                                 // Ts arrival counters (zeroed by k_post_a)
    // GPR outputs
    const double* Zc; long ldz; int Tp, p;    // Z = L^{-1} Y tiles (cached)
    double* Am; long ldam;                    // full_cov: A (Npad x Nspad); nullptr: not kept
    double* mpart;                            // [ngrp][Nspad][Ppad] mean partials
    double* vpart;                            // [ngrp][Nspad] colsum(A^2) partials
    double* mean; long ldm; double* var;
    // SVGP outputs
    const double* qmu;                        // [batch][Mpad] cached q_mu columns (zero padded)
    double *pa, *pb, *pm;                     // [batch][ngrp][Nspad] partials
    double *gm, *gv;                          // [batch][Nspad] latent moments
    const double* W;                          // mixing [p][batch]; nullptr: identity (batch == p)
    double* f_mu; double* f_var;              // [nstar][p]
    // Input-gradient pass (k_post_grad, behind the two forward launches; all unset for a plain predict).
    // GPR keeps A in Am; SVGP keeps A and B per batch entry (stride sAm, rows as Am).
    long sAm; double* Bm;
    const double* gmean; long ldgm;           // upstream d / d mean [nstar x p]; nullptr: zero
    const double* gvar;                       // upstream d / d var: GPR [nstar], SVGP [nstar x p]; nullptr: zero
    double* gpart;                            // [batch][ntask][Ts][D][NB] partial input gradients
    double* glat;                             // [batch][Ts][D][NB] per batch entry sums (batch > 1)
    int* gcnt;                                // k_post_grad's arrival counters: [Ts], then [batch][Ts] (zeroed by k_post_a)
    double* gX; long ldgx;                    // [nstar x (D + 1)], fidelity column written as 0
    // graph kernel: 1 generates K as graph_entry(X* row, cached row), the block a factorization reads when the
    // X* rows are appended BELOW the cached ones (mfgp_append.hip); 0: graph_entry(cached row, X* row)
    int swap;
};
// tasks of one batch entry: row tile i has ceil((full ? T : i + 1) / chunk) of them
int post_ntasks(int T, int chunk, int full);
// row tiles one k_post_out workgroup takes (128 rows: its A tiles stay in LDS across the output tiles)
constexpr int post_rg(int nb) { return nb == 32 ? 4 : 2; }
template <int NB> void launch_post(const PostArgs& a, int batch, hipStream_t s);
// The VJP of the predict outputs w.r.t. X* (linear MF kernel only): k_post_grad, after launch_post
// with A (B) kept.  One task = one row tile j x `chunk` i-tiles of U_j = sum_i (L^{-1})_ij^T R_i
// (+ C_ij^T R_B,i); the same task count as the forward by symmetry (row tile j has T - j steps).
template <int NB> void launch_post_grad(const PostArgs& a, int batch, hipStream_t s);
// Leave-group-out prediction from the GPR cache (mfgp_leave_out.hip): k_lo_pack packs whole
// consecutive groups into tasks of at most LO_W columns, k_lo accumulates C^T [C | Z] of a task's
// gathered columns C = L^{-1}[:, S] over chunks of 32-row steps and its last workgroup factors the
// block-diagonal G = C^T C and writes the outputs.
constexpr int LO_W = 32;    // columns of a task = the largest group
constexpr int LO_PT = 3;    // 32-column blocks of Z one workgroup carries (96 outputs)
struct LoArgs {
    const double* LZ; long ldr; int npad;     // cached [L^{-1} | Z] rows (read-only)
    const double* noise;                      // the cached likelihood variance
    int n, p;
    int ngroups, nrows, gmax;
    const int* offsets; const int* rows;      // group g: rows[offsets[g] .. offsets[g + 1])
    int ntmax;                                // task slots (lo_layout's bound on the packing)
    int chunk, nch;                           // 32-row steps per chunk, chunks of n rows
    int ny;                                   // blocks of 32 LO_PT outputs
    int* tab;                                 // [ntmax + 2]: task count, then each task's first group, then ngroups
    int* cnt;                                 // [ntmax][ny] arrival counters (zeroed by k_lo_pack)
    double* part;                             // [ntmax][nch][ny][32][32 (1 + LO_PT)] chunk partials
    double* resid; long ldres;                // [nrows x p]  E = y_S - mu
    double* cov; long ldc;                    // [nrows x gmax] rows of the groups' Sigma_f (nullptr: skipped)
    double* logdens;                          // [ngroups x p]
    int* info;                                // [ngroups]
};
void launch_leave_out(const LoArgs& a, hipStream_t s);

// Block append to the GPR cache (mfgp_append.hip): k <= 32 rows Xadd under the cached factors.  The forward
// (launch_post with PostArgs::swap, A kept) has run on Xadd; k_append_head forms S = K(Xadd, Xadd) + s2 I - A^T A,
// factors it (R = L22^{-1}), writes W = -R A^T, the new rows of Z and info; k_append_rows copies the old
// block's L^{-1} tiles to the new block's row stride and multiplies them into the new bottom rows W L^{-1}.
constexpr int APPEND_MAXK = 32;
struct AppendArgs {
    const double* LZ; long ldr;               // old block: [L^{-1} | Z] rows (read-only)
    const double* X; const double* theta;     // old block: inputs [n x (D + 1)], kernel parameters [G]
    int n, npad, T;                           // old rows, padded rows, row tiles
    int p, ppad, D, nlf, G, k;
    double diag_add;                          // the graph kernel's jitter on the diagonal of K (0: linear kernel)
    const double* Xadd; long ldxa;            // [k x (D + 1)]
    const double* Yadd; long ldya;            // [k x p]; nullptr: the rows are observed at their own mean
    const double* Am; long ldam;              // A = L^{-1} K(X, Xadd), npad x ldam (kept by the forward)
    const double* mean; long ldm;             // the forward's mean at Xadd [k x p]
    double* W;                                // [32][npad]  -R A^T (rows >= k zero)
    double* Rw;                               // [32][32]    R, zero above the diagonal, identity beyond k
    int* cnt;                                 // [T] arrival counters of k_append_rows (zeroed by the head)
    double* part;                             // [ntask][32 * NB] partial bottom products
    int chunk, ntask, nfill;                  // row tiles per task, tasks, workgroups of the fill pass
    double* LZo; long ldro; int npado;        // new block: [L^{-1} | Z], n + k rows padded to npado
    double* Xo; double* thetao;
    unsigned char* obase; long gap0[3], gap1[3];   // new block: the bytes no array covers (zeroed)
    int* info;
};
int append_ntasks(int T, int chunk);
template <int NB> void launch_append(const AppendArgs& a, hipStream_t s);

// Simulation design from the GPR cache (mfgp_design.hip).  The forward (launch_post, A kept) has run on
// the stacked points [Xref ; Xcand]; k_design_score forms C = K(Xref, Xcand) - A_ref^T A_cand -
// E_ref^T E_cand tile pair by tile pair in LDS and reduces sum_r w_r C(r, c)^2 / (v'(c) + s2);
// k_design_row appends the conditioning row of one picked candidate to E.
constexpr int DESIGN_MAXQ = 32;      // rows of E (picks a batch conditions on)
constexpr int DESIGN_RROWS = 128;    // rows of A one k_design_row workgroup takes
constexpr int design_run(int nb) { return nb == 32 ? 4 : 2; }   // reference row tiles per k_design_score task (128 rows)
struct DesignArgs {
    const double* Am; long ldam; int npad;    // A = L^{-1} K(X, [Xref ; Xcand]), npad x nspad (kept by the forward)
    const double* var;                        // [nref + ncand] marginal variances (the forward's)
    const double* Xall; long ldx;             // stacked inputs [nref + ncand, D + 1]
    int nref, ncand;
    const double* theta; const double* noise; // cached kernel parameters; their last entry, the likelihood variance
    int D, nlf;
    const double* w;                          // [nref] reference weights; nullptr: ones
    const double* E; long ldE; int k;         // k conditioning rows over the stacked columns
    int T, Tr, Tc, nrun;                      // row tiles of A, reference / candidate tiles, ceil(Tr / design_run)
    double* dpart;                            // [nrun][Tc * NB] partial column sums
    int* dcnt;                                // [Tc] arrival counters (zero on entry)
    double* score;                            // [ncand]
    // k_design_row: row k of E = C'(x, c*) / sqrt(v'(c*) + s2) over the stacked columns x
    const int* pick;                          // device: the picked candidate (outside 0..ncand-1: a zero row)
    double* Erow;                             // E + k ldE
    int ncb, nrch;                            // blocks of NTHREADS columns, chunks of DESIGN_RROWS rows
    double* rpart;                            // [nrch][ncb * NTHREADS] partial products
    int* rcnt;                                // [ncb] arrival counters (zero on entry)
};
template <int NB> void launch_design_score(const DesignArgs& a, hipStream_t s);
void launch_design_row(const DesignArgs& a, hipStream_t s);

// Batched fp64 MFMA GEMM (k_bgemm, mfgp_svgp_grad.hip), NB x NB output tiles:
// D = (alpha * op(A) diag(s) op(B) + beta * Cin) [* diag(colscale)] + x y^T   (tril: zero j > i)
struct BgemmArgs {
    const double* A; long lda; long sA;
    const double* B; long ldb; long sB;
    const double* s; long ss;              // k scaling (nullptr: none)
    const double* colscale; long scs;      // output column scaling (nullptr: none)
    const double* Cin; long ldc; long sC; double beta;
    const double* x; long sx; const double* y; long sy;   // rank-1 term (nullptr: none)
    double* D; long ldd; long sD;
    double alpha;
    int Mt, Nt, Kt, tril;
    // sym (k_bgemm2 only, with tril; a symmetric product formed from its lower tiles): 1 stores
    // Psi(D) = (tril D + tril D^T - diag D) / 2, the lower tiles' values halved and mirrored
    // across the diagonal; 2 stores tril D mirrored (D itself, exactly symmetric)
    int sym;
    // known-zero triangles of the operands, so their k-tiles are skipped (never read):
    // amask 1: op(A) lower (k-tile <= row tile), 2: op(A) upper (k-tile >= row tile);
    // bmask 1: op(B) lower (k-tile >= column tile), 2: op(B) upper (k-tile <= column tile)
    int amask, bmask;
    // column statistics of the output (NB = 32, k_bgemm2 only; nullptr: none), one partial per
    // 32-row output tile: csq[(b Mt + ti) ldcs + j] = sum over the tile's rows of D^2, and with
    // qv, csq2 likewise of D[i][j] qv[i qs + b] over rows i < qn (the SVGP conditional's moments)
    double* csq; double* csq2; long ldcs;
    const double* qv; long qs; int qn;
};
void launch_bgemm(int nb, hipStream_t st, int ta, int tb, const BgemmArgs& a, int batch);

// ---------------------------------------------------------------- SVGP host layer (mfgp_svgp.hip, mfgp_svgp_grad.hip)
// One SVGP call is described by plain structs that the C-ABI entry fills once and every driver takes
// by const reference: a driver's signature names everything it reads, and nothing else does.

// The caller's stream, and the handle's side stream with its fork / join events for the calls'
// independent branches (the K_uu factorization beside the K_uf Gram; the reverse pass's dE/dm, dE/dLq
// and K_diag terms beside the gA -> Sigma_bar / K_bar -> kernel-derivative chain).  Without a side
// stream everything stays on main.
struct SvgpStreams {
    hipStream_t main, side;
    hipEvent_t ev_fork, ev_join;
    bool has_side() const { return side && ev_fork && ev_join; }
    // fork the side stream off main; returns the stream to launch the branch on
    hipStream_t fork() const {
        if (!has_side()) return main;
        (void)hipEventRecord(ev_fork, main);
        (void)hipStreamWaitEvent(side, ev_fork, 0);
        return side;
    }
    void join() const {
        if (!has_side()) return;
        (void)hipEventRecord(ev_join, side);
        (void)hipStreamWaitEvent(main, ev_join, 0);
    }
};

// The likelihood of an ELBO call.  The kernels take the Gaussian / heteroscedastic variance as the
// pair (noise, noise_dev), noise_dev winning when set: the value entries give the host value alone,
// the gradient entries the device scalar alone (noise stays 0).
struct SvgpLik {
    enum Kind {
        GAUSSIAN,   // one variance for every observation
        HET,        // variance + Yunc^2 per observation (Yunc [n][ldu])
        MASKED      // NaN targets are missing; noise_dev holds pn = 1 or p variances
    } kind = GAUSSIAN;
    double noise = 0.0;
    const double* noise_dev = nullptr;
    const double* Yunc = nullptr; int ldu = 0;
    int pn = 0;
};

// What every SVGP driver reads.  The predict drivers leave Y unset (X holds the test inputs, n their count).
struct SvgpProblem {
    int n, m, l, p, d;
    const double* X; int ldx;
    const double* Y; int ldy;
    const double* Z; int ldz;
    const double* thetas; const double* q_mu; const double* q_sqrt;
    int qs_packed;            // q_sqrt (and gq_sqrt) as packed lower triangles [l][m(m+1)/2]
    const double* W;          // mixing [p][l]; nullptr: identity (l == p)
    double scale, kl_mult, jitter;
    void* ws; size_t ws_bytes;
    int* info;
};

// What the forward writes: out = [elbo, KL, VE] and the latent moments; with f_mu / f_var set it is a
// predict (mixed moments only, no likelihood); Aout / Bout keep A = Li Kuf and B = Lq^T A
// ([l][Mpad][Npad] each) for the gradient pass.
struct SvgpFwdOut {
    double *out, *g_mu, *g_var;
    double *f_mu = nullptr, *f_var = nullptr;
    double *Aout = nullptr, *Bout = nullptr;
};
struct SvgpGradOut { double *gZ, *gtheta, *gq_mu, *gq_sqrt, *gW, *gnoise; };
struct SvgpCovOut { int mode; double* f_cov; };   // mode: 1 full_cov, 2 full_output_cov, 3 both

struct SvgpLayout {
    int nb, Tm, mpad, Tn, npad, G;
    double *Kuu, *R, *Xo, *Dd, *ldiag, *Lq, *C, *Kuf, *pa, *pb, *pm, *ve_part, *kl_part;
    size_t bytes;
};
SvgpLayout svgp_layout(int nb, int n, int m, int l, int p, int d, void* ws);
size_t svgp_workspace_bytes(int nb, int n, int m, int l, int p, int d);
size_t svgp_grad_workspace_bytes(int nb, int n, int m, int l, int p, int d);
size_t svgp_predict_cov_workspace_bytes(int nb, int ns, int m, int l, int p, int d);

// Return codes of the drivers: 0, -2 workspace too small, -3 launch error, -4 the VE reverse kernel's
// row state does not fit (svgp_ve_*_rows == 0).
int svgp_elbo_impl(int nb, const SvgpStreams& st, const SvgpProblem& P, const SvgpLik& lik, const SvgpFwdOut& o);
int svgp_predict_impl(int nb, const SvgpStreams& st, const SvgpProblem& P, const SvgpFwdOut& o);
int svgp_grad_impl(int nb, const SvgpStreams& st, const SvgpProblem& P, const SvgpLik& lik, const SvgpFwdOut& o,
                   const SvgpGradOut& go);
int svgp_predict_cov_impl(int nb, const SvgpStreams& st, const SvgpProblem& P, const SvgpFwdOut& o,
                          const SvgpCovOut& co);
// Lm^{-1} zero padded / C = Lq^T Lm^{-1} of the SVGP K_uu pipeline into the caller's cache blocks
// ([l][Mpad][Mpad] each), on s alone; reads m, l, d, Z, thetas, q_sqrt, jitter, ws and info of P
int svgp_posterior_factor(int nb, hipStream_t s, const SvgpProblem& P, double* Li, double* C);
size_t svgp_posterior_factor_bytes(int nb, int m, int l);

// rows a workgroup of the heteroscedastic VE reverse kernel takes (k_ve_bwd_het) for p outputs and
// l latents; 0: the row state of one row does not fit its LDS budget (MFGP_ERR_DIM)
int svgp_ve_het_rows(int p, int l);
// the same for the masked VE reverse kernel (k_ve_bwd_masked), whose row state has a third [rb][p|1] tile
int svgp_ve_masked_rows(int p, int l);

constexpr int MAXD_HOST = 32;

// fp32 path (mfgp_f32.hip): one tall row-major matrix M, 128 x 128 tiles, ld = Npad; row tiles
// [A = K + s2 I: T][Y^T: Tp][K(X*, X): Ts][I: Ti] (see the file header).
constexpr int F32_TILE = 128;
struct F32Args {
    float* M; long ld;                    // tall matrix, ld = Npad
    int T, Tp, Ts, Ti;                    // row-tile counts of the four regions
    int W;                                // tile columns per outer panel
    float* Dd;                            // T diagonal inverses D_k = L_kk^-1 (128 x 128, upper zero)
    double* ldiag;                        // diag(L), Npad
    int* info;                            // LAPACK-style, zeroed by k32_gram
    const float* X; long ldx; int n;      // inputs [n, D+1]
    const float* Y; long ldy; int p;      // targets [n, p]
    const float* Xs; long ldxs; int ns;   // predict inputs [ns, D+1] (Ts > 0)
    const double* theta; int D;           // constrained theta (fp64, include/mfgp.h layout)
    float* alpha; long ldal;              // K^-1 Y, Npad x Ppad (gradient)
    double* zpart; int nz;                // sum Z^2 partials (nz workgroups)
    double* gpart;                        // [G][T(T+1)/2] gradient partials
    int* cnt;                             // k_reduce_items arrival counter, zeroed by k32_gram
    int upd_slots;                        // lookahead: cap on resident trailing-update workgroups (0: none)
    float* LT;                            // refinement: L^T tiles (L(r,k)^T at tile (k,r), D_k^T at (k,k)), or nullptr
};
// fp64 refinement of the fp32 solve (value-only LML and predict mean, mfgp_set_f32_refine)
struct F32Refine {
    double* A64;                          // alpha (Npad x Ppad, fp64)
    double* R64;                          // R = Y - K alpha (Npad x Ppad, fp64)
    long ld64;                            // = Ppad
    float* XB;                            // work rows (Ppad x Npad, fp32, ld = Npad)
};
size_t f32_gemm_smem();
// Diagnostic timing of the fp32 launches (never on the hot path): events around every launch,
// summed per category after a sync; flops = the tile work each category performed.
enum F32Phase { F32_GRAM = 0, F32_DIAG, F32_PANEL, F32_UPD_IN, F32_UPD_OUT, F32_ALPHA, F32_GRAD, F32_FIN, F32_NPHASE };
struct F32Marks {
    static constexpr int MAXEV = 4096;
    hipEvent_t ev[MAXEV];
    int cat[MAXEV / 2];
    int n = 0;
    double flops[F32_NPHASE] = {};
    int launches[F32_NPHASE] = {};
    void begin(hipStream_t s, int c) {
        if (n + 2 > MAXEV) return;
        (void)hipEventCreate(&ev[n]);
        (void)hipEventCreate(&ev[n + 1]);
        cat[n / 2] = c;
        (void)hipEventRecord(ev[n], s);
    }
    void end(hipStream_t s, double fl) {
        if (n + 2 > MAXEV) return;
        (void)hipEventRecord(ev[n + 1], s);
        flops[cat[n / 2]] += fl;
        launches[cat[n / 2]] += 1;
        n += 2;
    }
    void collect(float* ms) {   // synchronises; ms[F32_NPHASE]
        for (int c = 0; c < F32_NPHASE; ++c) ms[c] = 0.0f;
        if (n) (void)hipEventSynchronize(ev[n - 1]);
        for (int i = 0; i < n; i += 2) {
            float t = 0.0f;
            (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
            ms[cat[i / 2]] += t;
        }
        for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
        n = 0;
    }
};
void launch_f32_sweep(const F32Args& a, hipStream_t s, F32Marks* mk = nullptr, hipStream_t side = nullptr,
                      hipEvent_t fork = nullptr, hipEvent_t join = nullptr);
void launch_f32_grad(const F32Args& a, hipStream_t s, F32Marks* mk = nullptr);
void launch_f32_zsum(const F32Args& a, hipStream_t s);
void launch_f32_predict(const F32Args& a, float* mean, long ldm, float* var, hipStream_t s);
void launch_f32_predict_cov(const F32Args& a, float* cov, long ldc, hipStream_t s);
void launch_f32_gram_dense(const float* X1, long ldx1, int n1, const float* X2, long ldx2, int n2, int D,
                           const double* theta, float diag_add, float* K, long ldk, hipStream_t s);
void launch_f32_refine_lml(const F32Args& a, const F32Refine& r, hipStream_t s);
void launch_f32_refine_mean(const F32Args& a, const F32Refine& r, float* mean, long ldm, int steps, hipStream_t s);

size_t gram_smem_bytes(int nb);
size_t chol_smem_bytes(int nb);
size_t grad_smem_bytes(int nb, int G, int nil2);
int chol_step_blocks(int T, int Tp, int k, bool alpha = false);
__host__ __device__ int grad_tasks(int T, int chunk);


int flow_nflags(int T, int Tp);
long flow_npub(int T, int Tp);
void launch_chol_flow(const FlowArgs& a, int nwg, hipStream_t s);

// LML layout (padded) or graph kernel: k_gram; dense layout of the linear MF / RBF kernel: k_gram_dense
template <int NB> void launch_gram(const GramArgs& g, int nblocks, int batch, hipStream_t s);
template <int NB> void launch_first_factor(const double* A, long lda, long sA, double* Dd, long sD, double* ldiag,
                                           long sL, int* info, int batch, hipStream_t s);
// dense layout, write extents wr1 x wr2 (>= n1 x n2; the excess is written 0.0)
void launch_gram_dense(const GramArgs& g, int batch, int wr1, int wr2, hipStream_t s);
void launch_flow_prep(const GramArgs& g, int nwg, hipStream_t s);    // set-up launch of k_chol_flow
// one-launch value + gradient (+ Adam) of the AR1 GPR LML for small problems (k_gpr_tiny)
bool gpr_tiny_fits(int n, int p, int d, int nlf);
bool gpr_tiny_pred_fits(int n, int p, int d, int nstar);
void launch_gpr_tiny_pred(const double* X, long ldx, const double* Y, long ldy, const double* Xs, long ldxs, int nstar,
                          const double* theta, int n, int p, int d, double* mean, long ldm, double* var, int* info,
                          hipStream_t s);
void launch_gpr_tiny(const double* X, long ldx, const double* Y, long ldy, const double* theta, int n, int p, int d,
                     int want_grad, int* info, const FinArgs& f, hipStream_t s);
template <int NB> void launch_chol_steps(CholArgs c, int batch, hipStream_t s);
template <int NB> void launch_grad(const GradArgs& g, hipStream_t s);
template <int NB> void launch_pred(const PredAArgs& pa, const PredOutArgs& po, int T, hipStream_t s);

__global__ void k_rhs_init(double* R, long ldr, long sR, int npad, int ppad, const double* Y, long ldy, long sY,
                           int n, int p);
__global__ void k_reduce_items(FinArgs a);
__global__ void k_theta_from_u(const double* u, double* theta, int G, int noise_index);
__global__ void k_kdiag(const double* X, long ldx, int n, int D, const double* theta, double* out, int nlf);
__global__ void k_selftest_mfma(double* out);

// mfgp_mvn_sample (mfgp_sample.hip): out(b, s, i, c) = mean(b, i, c) + sum_{j <= i} L_b[i][j] eps(b, s, j, c),
// L_b = chol(cov_b + jitter I); the addressing is include/mfgp.h's.
struct SampleArgs {
    const double* cov; long ldc, sC;
    double jitter;
    const double* mean; long mean_rs, mean_bs;
    const double* eps;
    double* out; long rs, ss, bs;
    double* Lw; long ldl, sL;   // the factor's 32-tiles in the workspace (set by launch_mvn_sample)
    int* info;
    int n, batch, nsamp, ncol;
};
size_t mvn_sample_ws_bytes(int n, int batch);
void launch_mvn_sample(SampleArgs a, void* ws, hipStream_t s);

// mfgp_mvn_logpdf (mfgp_density.hip): the Gaussian log-density of row s of Y under N(mean_s, obs_cov +
// diag(var_s + obs_var_s)) and its gradients w.r.t. mean and var; the addressing is include/mfgp.h's.
constexpr int MVN_DENSE_MAXP = 128;            // the dense form's LDS image: 129 x 129 doubles
constexpr size_t MVN_LOGPDF_WS_BYTES = 256;    // reserved: the kernels keep everything on chip
struct LogpdfArgs {
    int ns, p;
    const double* mean; long ldm;
    const double* Y; long y_rs;
    const double* var; long var_rs, var_cs;
    const double* obs_var; long ov_rs;        // nullptr: none
    const double* obs_cov; long ldc;          // nullptr: the diagonal form
    double* logp;
    double* gmean; long ldgm;                 // nullptr: not wanted
    double* gvar; long ldgv;                  // nullptr: not wanted
    int gv_sum;                               // 1 (var_cs == 0 only): gvar is [ns], summed over the outputs
    int* info;
};
void launch_mvn_logpdf(const LogpdfArgs& a, hipStream_t s);
bool mvn_logpdf_geometry_ok(int ns, int p, bool dense, int ldc, long y_rs, long ov_rs);

// Emulator Jacobian from the cached posterior (mfgp_jacobian.hip), linear multi-fidelity kernel only:
//   J[s][k][c] = d mean[s][c] / d Xs[s][k] = sum_i alpha[i][c] dK(x_i, xs_s) / d xs[s][k],
//   dK / d xs[s][k] = (wL / lL_k^2 + wD / lD_k^2)(x_ik - xs_sk), wL = cL vL kL, wD = cD vD kD.
// k_jac_weights  alpha = L^{-T} Z (GPR, [T NB x Tp NB]) or Lm^{-T} q_mu per latent (SVGP, [batch][T NB]):
//                one workgroup per output tile, U_j = sum_{i >= j} (L^{-1})_ij^T Z_i on the matrix core.
// k_jac_gpr      per (column tile of Xs, output tile, chunk of row tiles, group of JacCfg::DG dimensions): the
//                wL / wD tiles generated in LDS, G_k formed as the MFMA's A operand, acc_k += G_k^T alpha_tile;
//                chunk partials in `part`, summed in chunk order by the last workgroup to arrive at `cnt`.
// k_jac_svgp     per (latent, column tile, chunk): dg_l[s][k] partials, the VJP epilogue's contraction with
//                U = alpha_l (x) 1; k_jac_svgp_sum adds the chunks in order, k_jac_svgp_mix the latents.
struct JacArgs {
    const double* Li; long ldl; long sL;      // L^{-1}, lower tiles, batch stride
    const double* Zc; long ldz;               // GPR: Z tiles; nullptr: SVGP
    const double* qmu;                        // SVGP: [batch][T NB] cached q_mu columns
    int T, Tp;
    double* alpha; long lda; long sA;         // the weights (see k_jac_weights); sA: batch stride
    const double* X1; long ldx1; int n1;      // cached inputs / inducing points
    const double* theta; long stheta;
    const double* Xs; long ldxs; int nstar;
    int D, p;
    int Ts, chunk, nch, dgroups;              // column tiles, row tiles per chunk, chunks, dimension groups
    double* part; int* cnt;                   // GPR: [Ts][Tp][dgroups][nch][dw][NB][NB] (dw = min(DG, D)), [Ts][Tp][dgroups]
                                              // SVGP: part [batch][nch][Ts][D][NB]
    double* dgl;                              // SVGP: [batch][Ts][D][NB] (part itself when nch == 1)
    const double* W; int L;                   // SVGP mixing [p][L]; nullptr: a latent per output
    double* J; long ldj;                      // [nstar][D][ldj], outputs fastest
};
template <int NB> struct JacCfg { static constexpr int DG = NB == 32 ? 16 : 4; };   // accumulators a thread carries
template <int NB> void launch_jac_weights(const JacArgs& a, int batch, hipStream_t s);
template <int NB> void launch_jac_gpr(const JacArgs& a, hipStream_t s);
template <int NB> void launch_jac_svgp(const JacArgs& a, int batch, hipStream_t s);

// mfgp_mvn_fisher (mfgp_density.hip): F_s = J_s^T (obs_cov + diag(var_s + obs_var_s))^{-1} J_s per row s.
constexpr size_t FISHER_LDS_BYTES = 160 * 1024;     // the dense form's image must fit one CU's LDS
constexpr size_t MVN_FISHER_WS_BYTES = 256;         // reserved: the kernels keep everything on chip
struct FisherArgs {
    int ns, p, d;
    const double* J; long ldj;                // [ns][d][ldj]
    const double* var; long var_rs, var_cs;
    const double* obs_var; long ov_rs;        // nullptr: none
    const double* obs_cov; long ldc;          // nullptr: the diagonal form
    double* F;                                // [ns][d][d]
    int* info;
};
size_t fisher_dense_smem(int p, int d);
bool mvn_fisher_geometry_ok(int ns, int p, int d, bool dense, int ldc, long ov_rs);
void launch_mvn_fisher(const FisherArgs& a, hipStream_t s);

}  // namespace mfgp
