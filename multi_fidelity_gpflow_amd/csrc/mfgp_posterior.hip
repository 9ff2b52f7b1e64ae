// Cached-posterior predict (GPflow model.posterior()): the work of predict_f that depends on X*.
//
//   k_post_a    partial products of A = L^{-1} K(X, X*) against the CACHED inverse factor.  The
//               K(X, X*) tile of every step is generated in LDS from the cached X rows and the X*
//               rows (linear MF / graph entry function, theta from the cache): K_mn never exists in
//               HBM.  One task = one row tile x `chunk` consecutive m-tiles, so the long last rows
//               of the triangular product are spread over workgroups (PostArgs, mfgp_internal.h).
//   k_post_out  per (group of 128 rows, column tile): each row tile's partials summed in task order,
//               then the group's moment partials (sum_i A_i^T Z_i, colsum(A_i^2); SVGP:
//               colsum(B_i^2), A_i^T q_mu).  The last workgroup to arrive at a column tile's counter
//               sums the group partials in group order, folds in K_diag(X*) and writes the outputs
//               (SVGP: latent moments, mixing).
//   k_post_grad the VJP of those outputs w.r.t. X* (linear MF kernel), behind the two launches above
//               with A (B) kept: see "input gradients" below.
//
// Every sum has a fixed order and there are no floating-point atomics: two calls with the same
// inputs give the same bits.  Cross-workgroup data inside k_post_out goes through sc1 stores /
// loads (st_coherent / ld_coherent), the producer drains its stores before the arrival atomic.
#include "mfgp_device.h"
#include "mfgp_internal.h"
#include "mfgp_post_device.h"

namespace mfgp {

int post_ntasks(int T, int chunk, int full) {
    int n = 0;
    for (int i = 0; i < T; ++i) n += ((full ? T : i + 1) + chunk - 1) / chunk;
    return n;
}

// row tile i: its first task and its task count
__device__ __forceinline__ void post_row_tasks(int T, int chunk, int full, int i, int& base, int& nch) {
    base = 0;
    for (int j = 0; j < i; ++j) base += ((full ? T : j + 1) + chunk - 1) / chunk;
    nch = ((full ? T : i + 1) + chunk - 1) / chunk;
}

template <int NB>
constexpr size_t post_a_smem() {
    return sizeof(double) * (3 * (size_t)TileCfg<NB>::ELEMS + 2 * NB * PXS + 2 * NB + 2 * PMAXD + PTHETA);
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_post_a(PostArgs a) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int E = TileCfg<NB>::ELEMS;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* Ls = smem;
    double* Cs = Ls + E;
    double* Ks = Cs + E;
    double* x1 = Ks + E;            // NB x PXS: cached rows of the m-tile
    double* xs = x1 + NB * PXS;     // NB x PXS: X* rows of the column tile
    double* f1 = xs + NB * PXS;     // NB fidelity flags (-1: padding)
    double* fs = f1 + NB;
    double* il = fs + NB;           // [1 / lL | 1 / lD]
    double* ths = il + 2 * PMAXD;   // theta
    const int t = threadIdx.x, l = blockIdx.z;
    const int task = blockIdx.x / a.Ts, cs = blockIdx.x % a.Ts;
    if (blockIdx.x == 0 && l == 0) {
        // k_post_out's arrival counters; k_post_grad's: Ts column-tile counters, then Ts per batch entry
        for (int e = t; e < a.Ts; e += NTHREADS) a.cnt[e] = 0;
        if (a.gcnt)
            for (int e = t; e < a.Ts * (1 + (int)gridDim.z); e += NTHREADS) a.gcnt[e] = 0;
    }
    // task -> (row tile i, chunk ch)
    int i = 0, ch = task;
    for (; i < a.T; ++i) {
        const int nch = ((a.full ? a.T : i + 1) + a.chunk - 1) / a.chunk;
        if (ch < nch) break;
        ch -= nch;
    }
    if (i >= a.T) return;   // (never: the grid is post_ntasks x Ts)
    const int m0 = ch * a.chunk;
    const int mend = a.full ? a.T : i + 1;
    const int m1 = m0 + a.chunk < mend ? m0 + a.chunk : mend;
    const int D = a.D;
    const double* tp = a.theta + l * a.stheta;
    const int G = kernel_theta_size(a.nlf, D);
    for (int e = t; e < G; e += NTHREADS) ths[e] = tp[e];
    if (!a.nlf && t < D) {
        il[t] = rcp_nr(tp[1 + t]);
        il[PMAXD + t] = rcp_nr(tp[2 + D + t]);
    }
    for (int e = t; e < NB * D; e += NTHREADS) {
        const int r = e / D, d = e % D, gs = cs * NB + r;
        xs[r * PXS + d] = gs < a.nstar ? a.Xs[(long)gs * a.ldxs + d] : 0.0;
    }
    if (t < NB) {
        const int gs = cs * NB + t;
        fs[t] = gs < a.nstar ? a.Xs[(long)gs * a.ldxs + D] : -1.0;
    }
    const double* Li = a.Li + l * a.sL;
    const double* Cm = a.C ? a.C + l * a.sC : nullptr;
    const GraphTheta gth{ths, D, a.nlf};
    Acc<NB> accA, accB;
    acc_zero(accA);
    acc_zero(accB);
    // One memory round trip a step, hidden behind the previous step's tile generation and product:
    // the next step's L^{-1} (C) tile, cached rows and flags are fetched into registers before the
    // current step computes (a step that waited for its own loads took ~2x as long).
    constexpr int PER = NB * PMAXD / NTHREADS;
    TileRegs<NB> rl, rc;
    double rx[PER], rf = -1.0;
    auto fetch = [&](int m) {
        if (m <= i) tile_fetch<NB>(rl, Li + (long)i * NB * a.ldl + (long)m * NB, a.ldl);
        if (Cm) tile_fetch<NB>(rc, Cm + (long)i * NB * a.ldc + (long)m * NB, a.ldc);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = t + q * NTHREADS;
            rx[q] = 0.0;
            if (e < NB * D) {
                const int gr = m * NB + e / D;
                if (gr < a.n1) rx[q] = a.X1[(long)gr * a.ldx1 + e % D];
            }
        }
        if (t < NB) {
            const int gr = m * NB + t;
            rf = gr < a.n1 ? a.X1[(long)gr * a.ldx1 + D] : -1.0;
        }
    };
    if (m0 < m1) fetch(m0);
    for (int m = m0; m < m1; ++m) {
        __syncthreads();   // the previous step's readers of x1 / Ls / Cs / Ks are done
        if (m <= i) tile_put<NB>(Ls, rl);
        if (Cm) tile_put<NB>(Cs, rc);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = t + q * NTHREADS;
            if (e < NB * D) x1[(e / D) * PXS + e % D] = rx[q];
        }
        if (t < NB) f1[t] = rf;
        if (m + 1 < m1) fetch(m + 1);
        __syncthreads();
        if (a.nlf) {
            for (int e = t; e < NB * NB; e += NTHREADS) {
                const int r = e / NB, c = e % NB;
                const int s1 = graph_source(f1[r], a.nlf), s2 = graph_source(fs[c], a.nlf);
                Ks[r * S + c] = a.swap ? graph_entry(xs + c * PXS, x1 + r * PXS, s2, s1, gth)
                                       : graph_entry(x1 + r * PXS, xs + c * PXS, s1, s2, gth);
            }
        } else {
            post_mf_tile<NB>(Ks, x1, f1, xs, fs, D, il, ths);
        }
        __syncthreads();
        if (m <= i) tile_mma<NB, false, false>(accA, Ls, Ks, 1.0);
        if (Cm) tile_mma<NB, false, false>(accB, Cs, Ks, 1.0);
    }
    const long o = (((long)l * a.ntask + task) * a.Ts + cs) * (NB * NB);
    acc_store(accA, a.Apart + o, NB);
    if (Cm) acc_store(accB, a.Bpart + o, NB);
}

template <int NB>
constexpr size_t post_out_smem() {
    return sizeof(double) * 2 * post_rg(NB) * (size_t)TileCfg<NB>::ELEMS;
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_post_out(PostArgs a) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int E = TileCfg<NB>::ELEMS;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int RG = post_rg(NB);
    double* As = smem;            // RG tiles: the group's A_i, kept across the output tiles
    double* Bs = As + RG * E;     // RG tiles: the group's Z_i of one output tile (SVGP: the first holds B_i)
    __shared__ int last;
    const int t = threadIdx.x, l = blockIdx.z;
    const int g = blockIdx.x / a.Ts, cs = blockIdx.x % a.Ts;
    const int nspad = a.Ts * NB;
    const int i0 = g * RG, i1 = i0 + RG < a.T ? i0 + RG : a.T;
    double va = 0.0, vb = 0.0, pm = 0.0;   // thread c < NB: column c of the group's rows
    for (int i = i0; i < i1; ++i) {
        double* Ai = As + (i - i0) * E;
        int base, nch;
        post_row_tasks(a.T, a.chunk, a.full, i, base, nch);
        // A_i (B_i) = the row's partials in task order
        for (int e = t; e < NB * NB; e += NTHREADS) {
            const int r = e / NB, c = e % NB;
            const long o =(((long)l * a.ntask + base) * a.Ts + cs) * (NB * NB) + e;
            const long st = (long)a.Ts * (NB * NB);
            const double sa = post_sum(a.Apart + o, st, nch);
            const double sb = a.C ? post_sum(a.Bpart + o, st, nch) : 0.0;
            Ai[r * S + c] = sa;
            if (a.C) Bs[r * S + c] = sb;
            if (a.Am) a.Am[l * a.sAm + ((long)i * NB + r) * a.ldam + cs * NB + c] = sa;
            if (a.Bm) a.Bm[l * a.sAm + ((long)i * NB + r) * a.ldam + cs * NB + c] = sb;
        }
        __syncthreads();
        if (t < NB) {
            const double* q = a.qmu ? a.qmu + (long)l * a.T * NB + (long)i * NB : nullptr;
            for (int r = 0; r < NB; ++r) {
                const double v = Ai[r * S + t];
                va += v * v;
                if (q) pm += v * q[r];
                if (a.C) { const double w = Bs[r * S + t]; vb += w * w; }
            }
        }
        __syncthreads();   // Bs is rewritten by the next row tile
    }
    if (t < NB) {
        if (a.Zc) {
            st_coherent(a.vpart + (long)g * nspad + cs * NB + t, va);
        } else {
            const long o = ((long)l * a.ngrp + g) * nspad + cs * NB + t;
            st_coherent(a.pa + o, va);
            st_coherent(a.pb + o, vb);
            st_coherent(a.pm + o, pm);
        }
    }
    const int ppad = a.Tp * NB;
    if (a.Zc) {   // mean partial of the row group: sum_i A_i^T Z_i
        for (int cy = 0; cy < a.Tp; ++cy) {
            Acc<NB> acc;
            acc_zero(acc);
            __syncthreads();
            for (int i = i0; i < i1; ++i)   // the group's Z tiles in one memory round trip
                tile_load<NB>(Bs + (i - i0) * E, a.Zc + (long)i * NB * a.ldz + (long)cy * NB, a.ldz);
            __syncthreads();
            for (int i = i0; i < i1; ++i) tile_mma<NB, true, false>(acc, As + (i - i0) * E, Bs + (i - i0) * E, 1.0);
            acc_store_coherent(acc, a.mpart + ((long)g * nspad + cs * NB) * ppad + cy * NB, ppad);
        }
    }
    drain_stores();
    __syncthreads();
    if (t == 0) last = arrive(a.cnt + cs) == a.ngrp * (int)gridDim.z - 1;
    __syncthreads();
    if (!last) return;
    // ---- the column tile's outputs, by its last workgroup (row partials in row order)
    if (a.Zc) {
        for (int e = t; e < NB * a.p; e += NTHREADS) {
            const int r = e / a.p, c = e % a.p, s = cs * NB + r;
            if (s >= a.nstar) break;
            a.mean[(long)s * a.ldm + c] = post_sum_coherent(a.mpart + (long)s * ppad + c, (long)nspad * ppad, a.ngrp);
        }
        const int s = cs * NB + t;
        if (t < NB && s < a.nstar) {
            const double v = post_sum_coherent(a.vpart + s, nspad, a.ngrp);
            a.var[s] = post_kdiag(a.Xs[(long)s * a.ldxs + a.D], a.theta, a.D, a.nlf) - v;
        }
        return;
    }
    const int L = (int)gridDim.z;
    for (int e = t; e < L * NB; e += NTHREADS) {
        const int ll = e / NB, s = cs * NB + e % NB;
        if (s >= a.nstar) continue;
        const long o = (long)ll * a.ngrp * nspad + s;
        const double sa = post_sum_coherent(a.pa + o, nspad, a.ngrp);
        const double sb = post_sum_coherent(a.pb + o, nspad, a.ngrp);
        const double sm = post_sum_coherent(a.pm + o, nspad, a.ngrp);
        const double kff = post_kdiag(a.Xs[(long)s * a.ldxs + a.D], a.theta + ll * a.stheta, a.D, 0);
        st_coherent(a.gm + (long)ll * nspad + s, sm);
        st_coherent(a.gv + (long)ll * nspad + s, kff - sa + sb);
    }
    drain_stores();
    __syncthreads();
    for (int e = t; e < NB * a.p; e += NTHREADS) {   // mixing f = g W^T, f_var = g_var (W o W)^T (k_svgp_mix)
        const int r = e / a.p, c = e % a.p, s = cs * NB + r;
        if (s >= a.nstar) break;
        double fm = 0.0, fv = 0.0;
        if (a.W) {
            for (int l0 = 0; l0 < L; l0 += 8) {   // (the sc1 loads issued eight at a time, summed in latent order)
                double gmv[8], gvv[8], w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool in = l0 + j < L;
                    gmv[j] = in ? ld_coherent(a.gm + (long)(l0 + j) * nspad + s) : 0.0;
                    gvv[j] = in ? ld_coherent(a.gv + (long)(l0 + j) * nspad + s) : 0.0;
                    w[j] = in ? a.W[(long)c * L + l0 + j] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    fm += gmv[j] * w[j];
                    fv += gvv[j] * (w[j] * w[j]);
                }
            }
        } else {
            fm = ld_coherent(a.gm + (long)c * nspad + s);
            fv = ld_coherent(a.gv + (long)c * nspad + s);
        }
        a.f_mu[(long)s * a.p + c] = fm;
        a.f_var[(long)s * a.p + c] = fv;
    }
}

template <int NB>
void launch_post(const PostArgs& a, int batch, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_post_a<NB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)post_a_smem<NB>());
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_post_out<NB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)post_out_smem<NB>());
        attr = true;
    }
    hipLaunchKernelGGL(k_post_a<NB>, dim3(a.ntask * a.Ts, 1, batch), dim3(NTHREADS), post_a_smem<NB>(), s, a);
    hipLaunchKernelGGL(k_post_out<NB>, dim3(a.ngrp * a.Ts, 1, batch), dim3(NTHREADS), post_out_smem<NB>(), s, a);
}

template void launch_post<32>(const PostArgs&, int, hipStream_t);
template void launch_post<64>(const PostArgs&, int, hipStream_t);

// ---------------------------------------------------------------- input gradients (VJP w.r.t. X*)
// With upstream gm (d / d mean) and gv (d / d var), and A (B) kept by the forward:
//   GPR   R = Z gm^T - 2 A diag(gv),                         U = L^{-T} R
//   SVGP  R_A = q_mu ggm^T - 2 A diag(ggv), R_B = 2 B diag(ggv),   U = Lm^{-T} R_A + C^T R_B   (per latent)
//   gX[s, d] = sum_i U[i, s] dK(x_i, x*_s) / dx*_{s, d}
//   dK / dx*_{s, d} = cL kL (x_{i, d} - x*_{s, d}) / lL_d^2 + cD kD (x_{i, d} - x*_{s, d}) / lD_d^2
// One task = (row tile j, `chunk` consecutive i-tiles, column tile): the R tiles are formed on the
// fly, the partial U_j is accumulated on the matrix core, the K(X_j, X*) tile is generated in LDS as
// post_mf_tile does (its two terms kept apart) and U_j o K_j is contracted with the scaled
// differences into D partial sums per column.  U and dK never exist in HBM.  The contraction is
// linear in U, so a row tile's chunks contract independently.  Reduction in two stages, each by the
// last workgroup to arrive at a counter: a batch entry's tasks of a column tile in task order (GPR:
// that is gX), then the latents' sums in latent order.  (One stage over latents x tasks left a
// single workgroup with 640 dependent-latency terms per output at Goku's single-bin SVGP.)

// post_mf_tile with the entry split into its lL and lD terms, each multiplied by U:
// KLs = U o cL kL, KDs = U o cD kD (cL = 1 | rho | rho^2, cD = 1 for HF x HF, else 0; masks as post_mf_tile)
template <int NB>
__device__ __forceinline__ void post_mf_tile_grad(double* KLs, double* KDs, const double* Us, const double* x1,
                                                  const double* f1, const double* xs, const double* fs, int D,
                                                  const double* il, const double* th) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int RSTEP = NTHREADS / NB;
    constexpr int NE = NB * NB / NTHREADS;
    const int t = threadIdx.x, c = t % NB, rb = t / NB;
    const double* xb = xs + c * PXS;
    const double fb = fs[c];
    const bool Lb = (fb == 0.0), Hb = (fb == 1.0);
    const double vL = th[0], vD = th[1 + D], rho = th[2 + 2 * D];
    for (int g = 0; g < NE; g += 4) {
        const int r0 = rb + g * RSTEP;
        const double* xa = x1 + r0 * PXS;
        double kl[4] = {0.0, 0.0, 0.0, 0.0}, kd[4] = {0.0, 0.0, 0.0, 0.0};
        for (int d = 0; d < D; ++d) {
            const double b = xb[d], lL = il[d], lD = il[PMAXD + d];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double df = xa[j * RSTEP * PXS + d] - b;
                const double qL = df * lL, qD = df * lD;
                kl[j] += qL * qL;
                kd[j] += qD * qD;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { kl[j] *= -0.5; kd[j] *= -0.5; }
        exp4(kl);
        exp4(kd);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double fa = f1[r0 + j * RSTEP];
            const bool La = (fa == 0.0), Ha = (fa == 1.0);
            const double kL = vL * kl[j];
            double wl = (La && Lb) ? kL : (!(Ha && Hb) ? kL * rho : kL * (rho * rho));
            double wd = (Ha && Hb) ? vD * kd[j] : 0.0;
            if (!(La || Ha) || !(Lb || Hb)) wl = wd = 0.0;
            const int o = (r0 + j * RSTEP) * S + c;
            const double u = Us[o];
            KLs[o] = u * wl;
            KDs[o] = u * wd;
        }
    }
}

// 4 tiles (L^{-1} | C or Z | R | R_B or gm), the staged inputs of the epilogue, flags, upstream
// vectors, 1 / l, theta.  NB = 64: the staged inputs take the fourth tile's place (free by then);
// four tiles and the inputs side by side would pass the 160 KB of a CU.
template <int NB>
constexpr size_t post_grad_smem() {
    return sizeof(double) * (4 * (size_t)TileCfg<NB>::ELEMS + (NB == 64 ? 0 : 2 * NB * PXS) + 4 * NB + 2 * PMAXD + PTHETA);
}
static_assert(2 * 64 * PXS <= TileCfg<64>::ELEMS, "k_post_grad<64> stages its inputs in the fourth tile");

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_post_grad(PostArgs a) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int E = TileCfg<NB>::ELEMS;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* Ls = smem;              // (L^{-1})_ij; epilogue: U o cL kL
    double* Cs = Ls + E;            // SVGP C_ij, GPR Z_i tile; epilogue: U o cD kD
    double* Rs = Cs + E;            // R_i (R_A,i); epilogue: U_j
    double* Gs = Rs + E;            // SVGP R_B,i, GPR gm tile
    double* x1 = NB == 64 ? Gs : Gs + E;   // NB x PXS: cached rows of tile j (epilogue)
    double* xs = x1 + NB * PXS;            // NB x PXS: X* rows of the column tile (epilogue)
    double* f1 = smem + 4 * E + (NB == 64 ? 0 : 2 * NB * PXS);
    double* fs = f1 + NB;
    double* gms = fs + NB;          // SVGP: ggm_l of the column tile
    double* gvs = gms + NB;         // gv (SVGP: ggv_l) of the column tile
    double* il = gvs + NB;          // [1 / lL | 1 / lD]
    double* ths = il + 2 * PMAXD;
    __shared__ int last;
    const int t = threadIdx.x, l = blockIdx.z, L = (int)gridDim.z;
    const int task = blockIdx.x / a.Ts, cs = blockIdx.x % a.Ts;
    // task -> (row tile j, chunk ch): row tile j has T - j steps (all T with C), the forward's counts mirrored
    int jj = 0, ch = task;
    for (; jj < a.T; ++jj) {
        const int nch = ((a.full ? a.T : jj + 1) + a.chunk - 1) / a.chunk;
        if (ch < nch) break;
        ch -= nch;
    }
    if (jj >= a.T) return;   // (never: the grid is post_ntasks x Ts)
    const int j = a.full ? jj : a.T - 1 - jj;
    const int m0 = ch * a.chunk;
    const int mend = a.full ? a.T : jj + 1;
    const int m1 = m0 + a.chunk < mend ? m0 + a.chunk : mend;
    const int D = a.D;
    const double* tp = a.theta + l * a.stheta;
    for (int e = t; e < theta_size(D); e += NTHREADS) ths[e] = tp[e];
    if (t < D) {
        il[t] = rcp_nr(tp[1 + t]);
        il[PMAXD + t] = rcp_nr(tp[2 + D + t]);
    }
    if (t < NB) {   // the column tile's upstream vectors (rows beyond nstar: zero)
        const int s = cs * NB + t;
        double vm = 0.0, vv = 0.0;
        if (s < a.nstar) {
            if (a.Zc) {
                if (a.gvar) vv = a.gvar[s];
            } else if (a.W) {   // ggm = gm W, ggv = gv (W o W), summed in output order
                for (int c = 0; c < a.p; ++c) {
                    const double w = a.W[(long)c * L + l];
                    if (a.gmean) vm += a.gmean[(long)s * a.ldgm + c] * w;
                    if (a.gvar) vv += a.gvar[(long)s * a.p + c] * (w * w);
                }
            } else {
                if (a.gmean) vm = a.gmean[(long)s * a.ldgm + l];
                if (a.gvar) vv = a.gvar[(long)s * a.p + l];
            }
        }
        gms[t] = vm;
        gvs[t] = vv;
    }
    __syncthreads();
    const double* Li = a.Li + l * a.sL;
    const double* Cm = a.C ? a.C + l * a.sC : nullptr;
    const double* Am = a.Am + l * a.sAm;
    // One memory round trip a step, hidden behind the previous step's products (k_post_a's scheme):
    // every tile and vector of the next product is fetched into registers before the current one runs.
    constexpr int NP = NB * NB / 2 / NTHREADS;   // 16-byte pairs of a tile per thread
    constexpr int NBLK = TileCfg<NB>::NBLK;
    Acc<NB> accU;
    acc_zero(accU);
    if (a.Zc) {
        // GPR: R_i = Z_i gm^T - 2 A_i diag(gv) in the accumulator layout, then U_j += (L^{-1})_ij^T R_i
        const bool hasM = a.gmean != nullptr, hasV = a.gvar != nullptr;
        TileRegs<NB> rl, rz;
        double rg[2 * NP], ra[NBLK][4];
        auto fetch_zg = [&](int i, int cy, bool g) {   // Z tile (i, cy) and, with g, the gm tile cy
            tile_fetch<NB>(rz, a.Zc + (long)i * NB * a.ldz + (long)cy * NB, a.ldz);
            if (g) {
#pragma unroll
                for (int q = 0; q < 2 * NP; ++q) {
                    const int e = t + q * NTHREADS, r = e / NB, c = e % NB, s = cs * NB + r, cc = cy * NB + c;
                    rg[q] = (s < a.nstar && cc < a.p) ? a.gmean[(long)s * a.ldgm + cc] : 0.0;
                }
            }
        };
        auto fetch_la = [&](int i) {   // (L^{-1})_ij and A_i's entries of this thread's accumulator slots
            tile_fetch<NB>(rl, Li + (long)i * NB * a.ldl + (long)j * NB, a.ldl);
            if (hasV) {
#pragma unroll
                for (int q = 0; q < NBLK; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        ra[q][r] = Am[((long)i * NB + acc_row<NB>(q, r)) * a.ldam + cs * NB + acc_col<NB>(q)];
            }
        };
        if (m0 < m1) {
            const int i = a.full ? m0 : j + m0;
            if (hasM) fetch_zg(i, 0, true);
            fetch_la(i);
        }
        for (int m = m0; m < m1; ++m) {
            const int i = a.full ? m : j + m;
            Acc<NB> accR;
            acc_zero(accR);
            if (hasM)
                for (int cy = 0; cy < a.Tp; ++cy) {
                    __syncthreads();   // the previous products' readers of Cs / Gs (and of Ls / Rs)
                    tile_put<NB>(Cs, rz);
                    if (a.Tp > 1 || m == m0) {   // one gm tile: staged once
#pragma unroll
                        for (int q = 0; q < 2 * NP; ++q) {
                            const int e = t + q * NTHREADS;
                            Gs[(e / NB) * S + e % NB] = rg[q];
                        }
                    }
                    if (cy + 1 < a.Tp) fetch_zg(i, cy + 1, true);
                    else if (m + 1 < m1) fetch_zg(i + 1, 0, a.Tp > 1);
                    __syncthreads();
                    tile_mma<NB, false, true>(accR, Cs, Gs, 1.0);
                }
            if (hasV) {
#pragma unroll
                for (int q = 0; q < NBLK; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) accR.v[q][r] -= 2.0 * ra[q][r] * gvs[acc_col<NB>(q)];
            }
            if (!hasM) __syncthreads();   // the previous step's readers of Ls / Rs
            tile_put<NB>(Ls, rl);
            acc_to_lds<NB>(accR, Rs);
            if (m + 1 < m1) fetch_la(i + 1);
            __syncthreads();
            tile_mma<NB, true, false>(accU, Ls, Rs, 1.0);
        }
    } else {
        // SVGP: R_A,i = q_mu_i ggm^T - 2 A_i diag(ggv) (i >= j: Lm^{-1} is lower), R_B,i = 2 B_i diag(ggv);
        // U_j += (Lm^{-1})_ij^T R_A,i + C_ij^T R_B,i
        const bool hasB = a.gvar != nullptr;
        const double* Bm = hasB ? a.Bm + l * a.sAm : nullptr;
        const double* qm = a.qmu + (long)l * a.T * NB;
        TileRegs<NB> rl, rc, ra, rb;
        double rq[NP];
        auto fetch = [&](int i) {
            if (i >= j) {
                tile_fetch<NB>(rl, Li + (long)i * NB * a.ldl + (long)j * NB, a.ldl);
                tile_fetch<NB>(ra, Am + (long)i * NB * a.ldam + cs * NB, a.ldam);
#pragma unroll
                for (int q = 0; q < NP; ++q) rq[q] = qm[i * NB + (t + q * NTHREADS) / (NB / 2)];
            }
            if (hasB) {
                tile_fetch<NB>(rc, Cm + (long)i * NB * a.ldc + (long)j * NB, a.ldc);
                tile_fetch<NB>(rb, Bm + (long)i * NB * a.ldam + cs * NB, a.ldam);
            }
        };
        if (m0 < m1) fetch(a.full ? m0 : j + m0);
        for (int m = m0; m < m1; ++m) {
            const int i = a.full ? m : j + m;
            const bool lower = i >= j;
            __syncthreads();   // the previous step's readers
            if (lower) tile_put<NB>(Ls, rl);
            if (hasB) tile_put<NB>(Cs, rc);
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int pr = t + q * NTHREADS, row = pr / (NB / 2), c = 2 * (pr % (NB / 2));
                const double g0 = gvs[c], g1 = gvs[c + 1];
                if (lower) {
                    f64x2 v;
                    v[0] = rq[q] * gms[c] - 2.0 * ra.v[q][0] * g0;
                    v[1] = rq[q] * gms[c + 1] - 2.0 * ra.v[q][1] * g1;
                    *reinterpret_cast<f64x2*>(Rs + row * S + c) = v;
                }
                if (hasB) {
                    f64x2 v;
                    v[0] = 2.0 * rb.v[q][0] * g0;
                    v[1] = 2.0 * rb.v[q][1] * g1;
                    *reinterpret_cast<f64x2*>(Gs + row * S + c) = v;
                }
            }
            if (m + 1 < m1) fetch(i + 1);
            __syncthreads();
            if (lower) tile_mma<NB, true, false>(accU, Ls, Rs, 1.0);
            if (hasB) tile_mma<NB, true, false>(accU, Cs, Gs, 1.0);
        }
    }
    // ---- epilogue: U_j o K(X_j, X*) contracted with (x_i - x*_s) / l^2
    __syncthreads();   // the last product's readers
    acc_to_lds<NB>(accU, Rs);
    for (int e = t; e < NB * D; e += NTHREADS) {
        const int r = e / D, d = e % D, gr = j * NB + r, gs = cs * NB + r;
        x1[r * PXS + d] = gr < a.n1 ? a.X1[(long)gr * a.ldx1 + d] : 0.0;
        xs[r * PXS + d] = gs < a.nstar ? a.Xs[(long)gs * a.ldxs + d] : 0.0;
    }
    if (t < NB) {
        const int gr = j * NB + t, gs = cs * NB + t;
        f1[t] = gr < a.n1 ? a.X1[(long)gr * a.ldx1 + D] : -1.0;
        fs[t] = gs < a.nstar ? a.Xs[(long)gs * a.ldxs + D] : -1.0;
    }
    __syncthreads();
    post_mf_tile_grad<NB>(Ls, Cs, Rs, x1, f1, xs, fs, D, il, ths);
    __syncthreads();
    // thread (column sl, dimension group dg): dimensions dg, dg + NG, ..; rows in row order
    constexpr int NG = NTHREADS / NB, ND = PMAXD / NG;
    const int sl = t % NB, dg = t / NB;
    double acc[ND], wl[ND], wd[ND], xv[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        const int d = dg + k * NG;
        const bool in = d < D;
        acc[k] = 0.0;
        wl[k] = in ? il[d] * il[d] : 0.0;
        wd[k] = in ? il[PMAXD + d] * il[PMAXD + d] : 0.0;
        xv[k] = in ? xs[sl * PXS + d] : 0.0;
    }
    for (int r = 0; r < NB; ++r) {
        const double pl = Ls[r * S + sl], pd = Cs[r * S + sl];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const int d = dg + k * NG;
            if (d < D) acc[k] += (pl * wl[k] + pd * wd[k]) * (x1[r * PXS + d] - xv[k]);
        }
    }
    const long pstride = (long)a.Ts * D * NB;
    double* gp = a.gpart + ((long)l * a.ntask + task) * pstride + (long)cs * D * NB;
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        const int d = dg + k * NG;
        if (d < D) st_coherent(gp + d * NB + sl, acc[k]);
    }
    drain_stores();
    __syncthreads();
    if (t == 0) last = arrive(a.gcnt + (1 + l) * a.Ts + cs) == a.ntask - 1;
    __syncthreads();
    if (!last) return;
    // ---- the batch entry's gradient of this column tile, by its last workgroup: partials in task order
    const double* gl = a.gpart + (long)l * a.ntask * pstride + (long)cs * D * NB;
    for (int e = t; e < NB * D; e += NTHREADS) {
        const double v = post_sum_coherent<32>(gl + e, pstride, a.ntask);
        if (L == 1) {
            const int s = cs * NB + e % NB;
            if (s < a.nstar) a.gX[(long)s * a.ldgx + e / NB] = v;
        } else {
            st_coherent(a.glat + ((long)l * a.Ts + cs) * D * NB + e, v);
        }
    }
    if (L > 1) {
        drain_stores();
        __syncthreads();
        if (t == 0) last = arrive(a.gcnt + cs) == L - 1;
        __syncthreads();
        if (!last) return;
        // ---- gX, by the column tile's last batch entry: the latents' gradients in latent order
        for (int e = t; e < NB * D; e += NTHREADS) {
            const int s = cs * NB + e % NB;
            if (s >= a.nstar) continue;
            a.gX[(long)s * a.ldgx + e / NB] =
                post_sum_coherent<32>(a.glat + (long)cs * D * NB + e, (long)a.Ts * D * NB, L);
        }
    }
    if (t < NB && cs * NB + t < a.nstar) a.gX[(long)(cs * NB + t) * a.ldgx + D] = 0.0;   // the fidelity column
}

template <int NB>
void launch_post_grad(const PostArgs& a, int batch, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_post_grad<NB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)post_grad_smem<NB>());
        attr = true;
    }
    hipLaunchKernelGGL(k_post_grad<NB>, dim3(a.ntask * a.Ts, 1, batch), dim3(NTHREADS), post_grad_smem<NB>(), s, a);
}

template void launch_post_grad<32>(const PostArgs&, int, hipStream_t);
template void launch_post_grad<64>(const PostArgs&, int, hipStream_t);

}  // namespace mfgp
