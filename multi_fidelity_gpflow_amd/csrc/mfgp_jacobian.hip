// Emulator Jacobian from the cached posterior (include/mfgp.h mfgp_gpr_jacobian / mfgp_svgp_jacobian):
//   J[s][k][c] = d mean[s][c] / d X*[s][k] over the D input columns, linear multi-fidelity kernel.
//
//   k_jac_weights   alpha = L^{-T} Z (GPR) / Lm^{-T} q_mu (SVGP, per latent), once per cache block: one
//                   workgroup per output tile, U_j = sum_{i >= j} (L^{-1})_ij^T Z_i on the matrix core
//                   (k_post_grad's product), the next step's tiles fetched behind the current product.
//   k_jac_gpr       J = sum_i alpha[i][c] dK(x_i, x*_s) / dx*[s][k] with dK generated on chip.  One task =
//                   (column tile of X*, output tile, chunk of row tiles, group of DG input dimensions).  Per row
//                   tile the two terms of the kernel entry (wL = cL vL kL, wD = cD vD kD: post_mf_tile_grad's
//                   split) are generated in LDS; G_k[i][s] = (wL / lL_k^2 + wD / lD_k^2)(x_ik - x*_sk) is formed
//                   elementwise from them AS the matrix core's A operand (no G tile, no barrier per dimension)
//                   and acc_k += G_k^T alpha_tile with v_mfma_f64_16x16x4: DG accumulators a thread, one read of
//                   the wL / wD / alpha elements serves all of them.  Chunk partials go to the workspace and the
//                   last workgroup to arrive at the task's counter adds them in chunk order (k_post_grad's
//                   arrive / st_coherent / post_sum_coherent; no spin-wait, no floating-point atomics).
//   k_jac_svgp      dg_l[s][k] = sum_i alpha_l[i] dK_l(z_i, x*_s) / dx*[s][k]: k_post_grad's epilogue contraction
//                   with U = alpha_l (x) 1, batched over latents with the theta stride; chunk partials.
//   k_jac_svgp_sum  the chunks of a latent in chunk order;  k_jac_svgp_mix  J[s][k][c] = sum_l W[c][l] dg_l[s][k]
//                   in latent order (no W: J[s][k][l] = dg_l[s][k]).
//
// Every sum has a fixed order that depends on the shapes alone: two calls with the same inputs give the same
// bits.  The fidelity column enters through exact == 0 / == 1 tests: a row of either side whose fidelity is
// neither has wL = wD = 0 and adds exactly 0.
#include "mfgp_device.h"
#include "mfgp_internal.h"
#include "mfgp_post_device.h"

namespace mfgp {

namespace {

constexpr int JTHETA = 72;   // theta entries of the linear kernel staged in LDS (2 D + 4 <= 68)

// post_mf_tile_grad's two terms of the K(x1 rows, xs rows) tile without the U factor: KLs = aw cL vL kL,
// KDs = aw cD vD kD (cL = 1 | rho | rho^2, cD = 1 for HF x HF, else 0; aw: one weight per row, nullptr: 1)
template <int NB>
__device__ __forceinline__ void jac_mf_tile(double* KLs, double* KDs, const double* aw, const double* x1,
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
            const int r = r0 + j * RSTEP;
            const double fa = f1[r];
            const bool La = (fa == 0.0), Ha = (fa == 1.0);
            const double kL = vL * kl[j];
            double wl = (La && Lb) ? kL : (!(Ha && Hb) ? kL * rho : kL * (rho * rho));
            double wd = (Ha && Hb) ? vD * kd[j] : 0.0;
            if (!(La || Ha) || !(Lb || Hb)) wl = wd = 0.0;
            const double u = aw ? aw[r] : 1.0;
            KLs[r * S + c] = u * wl;
            KDs[r * S + c] = u * wd;
        }
    }
}

// theta, [1 / l] and [1 / l^2] of one batch entry, the X* rows and flags of column tile cs (rows beyond nstar:
// zeros, flag -1) into LDS; the caller's barrier follows
template <int NB>
__device__ __forceinline__ void jac_stage(const JacArgs& a, const double* tp, int cs, double* ths, double* il,
                                          double* il2, double* xs, double* fs) {
    const int t = threadIdx.x, D = a.D;
    for (int e = t; e < theta_size(D); e += NTHREADS) ths[e] = tp[e];
    if (t < D) {
        const double rl = rcp_nr(tp[1 + t]), rd = rcp_nr(tp[2 + D + t]);
        il[t] = rl;
        il[PMAXD + t] = rd;
        il2[t] = rl * rl;
        il2[PMAXD + t] = rd * rd;
    }
    for (int e = t; e < NB * D; e += NTHREADS) {
        const int r = e / D, d = e % D, gs = cs * NB + r;
        xs[r * PXS + d] = gs < a.nstar ? a.Xs[(long)gs * a.ldxs + d] : 0.0;
    }
    if (t < NB) {
        const int gs = cs * NB + t;
        fs[t] = gs < a.nstar ? a.Xs[(long)gs * a.ldxs + D] : -1.0;
    }
}

template <int NB>
constexpr size_t jac_weights_smem() {
    return sizeof(double) * 2 * (size_t)TileCfg<NB>::ELEMS;
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_jac_weights(JacArgs a) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int E = TileCfg<NB>::ELEMS;
    constexpr int NBLK = TileCfg<NB>::NBLK;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* Ls = smem;        // (L^{-1})_ij
    double* Zs = Ls + E;      // Z_i tile; SVGP: q_mu_i in column 0, zeros beside it
    const int t = threadIdx.x, l = blockIdx.z;
    const int tpx = a.Zc ? a.Tp : 1;
    const int j = blockIdx.x / tpx, cy = blockIdx.x % tpx;
    const double* Li = a.Li + l * a.sL;
    const double* qm = a.qmu ? a.qmu + (long)l * a.T * NB : nullptr;
    if (qm)
        for (int e = t; e < E; e += NTHREADS) Zs[e] = 0.0;
    TileRegs<NB> rl, rz;
    double rq = 0.0;
    auto fetch = [&](int i) {
        tile_fetch<NB>(rl, Li + (long)i * NB * a.ldl + (long)j * NB, a.ldl);
        if (qm) {
            if (t < NB) rq = qm[i * NB + t];
        } else {
            tile_fetch<NB>(rz, a.Zc + (long)i * NB * a.ldz + (long)cy * NB, a.ldz);
        }
    };
    Acc<NB> acc;
    acc_zero(acc);
    fetch(j);
    for (int i = j; i < a.T; ++i) {
        __syncthreads();   // the previous product's readers (first step: the zero fill of Zs)
        tile_put<NB>(Ls, rl);
        if (qm) {
            if (t < NB) Zs[t * S] = rq;
        } else {
            tile_put<NB>(Zs, rz);
        }
        if (i + 1 < a.T) fetch(i + 1);
        __syncthreads();
        tile_mma<NB, true, false>(acc, Ls, Zs, 1.0);
    }
    if (qm) {
        double* out = a.alpha + l * a.sA + (long)j * NB;
#pragma unroll
        for (int q = 0; q < NBLK; ++q)
            if (acc_col<NB>(q) == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[acc_row<NB>(q, r)] = acc.v[q][r];
            }
    } else {
        acc_store(acc, a.alpha + (long)j * NB * a.lda + (long)cy * NB, a.lda);
    }
}

// 3 tiles (wL | wD | alpha), the staged rows of both sides, flags, [1 / l], [1 / l^2], theta
template <int NB>
constexpr size_t jac_gpr_smem() {
    return sizeof(double) * (3 * (size_t)TileCfg<NB>::ELEMS + 2 * NB * PXS + 2 * NB + 4 * PMAXD + JTHETA);
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_jac_gpr(JacArgs a) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int E = TileCfg<NB>::ELEMS;
    constexpr int BPW = TileCfg<NB>::BPW;
    constexpr int NBLK = TileCfg<NB>::NBLK;
    constexpr int DG = JacCfg<NB>::DG;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* KLs = smem;
    double* KDs = KLs + E;
    double* As = KDs + E;             // alpha tile (row tile m, output tile cy)
    double* x1 = As + E;              // NB x PXS: cached rows of tile m
    double* xs = x1 + NB * PXS;       // NB x PXS: X* rows of the column tile
    double* f1 = xs + NB * PXS;
    double* fs = f1 + NB;
    double* il = fs + NB;             // [1 / lL | 1 / lD]
    double* il2 = il + 2 * PMAXD;     // [1 / lL^2 | 1 / lD^2]
    double* ths = il2 + 2 * PMAXD;
    __shared__ int last;
    const int t = threadIdx.x, D = a.D;
    int bx = blockIdx.x;
    const int ch = bx % a.nch;
    bx /= a.nch;
    const int cy = bx % a.Tp, cs = bx / a.Tp;
    const int gy = blockIdx.y, d0 = gy * DG;
    const int nd = D - d0 < DG ? D - d0 : DG;
    const int dw = D < DG ? D : DG;   // dimensions a partial holds
    const int m0 = ch * a.chunk;
    const int m1 = m0 + a.chunk < a.T ? m0 + a.chunk : a.T;
    jac_stage<NB>(a, a.theta, cs, ths, il, il2, xs, fs);
    __syncthreads();
    const int lane = t & 63, w = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int rb = 16 * BPW * (w >> 1), cb = 16 * BPW * (w & 1);
    double xsv[BPW][DG];   // this lane's X* columns of the operand, per dimension
#pragma unroll
    for (int ti = 0; ti < BPW; ++ti)
#pragma unroll
        for (int k = 0; k < DG; ++k) xsv[ti][k] = k < nd ? xs[(rb + 16 * ti + li) * PXS + d0 + k] : 0.0;
    Acc<NB> acc[DG];
#pragma unroll
    for (int k = 0; k < DG; ++k) acc_zero(acc[k]);
    // One memory round trip a step, hidden behind the previous step's tile generation and products
    // (k_post_a's scheme): the next alpha tile, cached rows and flags are fetched into registers first.
    constexpr int PER = NB * PMAXD / NTHREADS;
    TileRegs<NB> ra;
    double rx[PER], rf = -1.0;
    auto fetch = [&](int m) {
        tile_fetch<NB>(ra, a.alpha + (long)m * NB * a.lda + (long)cy * NB, a.lda);
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
    fetch(m0);
    for (int m = m0; m < m1; ++m) {
        __syncthreads();   // the previous step's readers of As / x1 / KLs / KDs
        tile_put<NB>(As, ra);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = t + q * NTHREADS;
            if (e < NB * D) x1[(e / D) * PXS + e % D] = rx[q];
        }
        if (t < NB) f1[t] = rf;
        if (m + 1 < m1) fetch(m + 1);
        __syncthreads();
        jac_mf_tile<NB>(KLs, KDs, nullptr, x1, f1, xs, fs, D, il, ths);
        __syncthreads();
#pragma unroll 2
        for (int k0 = 0; k0 < NB; k0 += 4) {
            const int r = k0 + lk;   // cached row of the tile: the product's inner index
            double kl[BPW], kd[BPW], b[BPW];
#pragma unroll
            for (int ti = 0; ti < BPW; ++ti) {
                kl[ti] = KLs[r * S + rb + 16 * ti + li];
                kd[ti] = KDs[r * S + rb + 16 * ti + li];
                b[ti] = As[r * S + cb + 16 * ti + li];
            }
#pragma unroll
            for (int k = 0; k < DG; ++k) {
                if (k < nd) {
                    const double x = x1[r * PXS + d0 + k];
                    const double wl = il2[d0 + k], wd = il2[PMAXD + d0 + k];
#pragma unroll
                    for (int ti = 0; ti < BPW; ++ti) {
                        const double g = (kl[ti] * wl + kd[ti] * wd) * (x - xsv[ti][k]);
#pragma unroll
                        for (int tj = 0; tj < BPW; ++tj)
                            acc[k].v[ti * BPW + tj] =
                                __builtin_amdgcn_mfma_f64_16x16x4f64(g, b[tj], acc[k].v[ti * BPW + tj], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (a.nch == 1) {   // whole rows: the accumulators are the result
#pragma unroll
        for (int k = 0; k < DG; ++k)
            if (k < nd) {
#pragma unroll
                for (int q = 0; q < NBLK; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int s = cs * NB + acc_row<NB>(q, r), c = cy * NB + acc_col<NB>(q);
                        if (s < a.nstar && c < a.p) a.J[((long)s * D + d0 + k) * a.ldj + c] = acc[k].v[q][r];
                    }
            }
        return;
    }
    const long task = ((long)cs * a.Tp + cy) * a.dgroups + gy;
    const long pstride = (long)dw * NB * NB;
    double* pp = a.part + (task * a.nch + ch) * pstride;
#pragma unroll
    for (int k = 0; k < DG; ++k)
        if (k < nd) acc_store_coherent<NB>(acc[k], pp + (long)k * NB * NB, NB);
    drain_stores();
    __syncthreads();
    if (t == 0) last = arrive(a.cnt + task) == a.nch - 1;
    __syncthreads();
    if (!last) return;
    // ---- the task's block of J, by its last workgroup: the chunk partials in chunk order
    const double* pl = a.part + task * a.nch * pstride;
    for (int e = t; e < nd * NB * NB; e += NTHREADS) {
        const int k = e / (NB * NB), rc = e % (NB * NB);
        const int s = cs * NB + rc / NB, c = cy * NB + rc % NB;
        if (s >= a.nstar || c >= a.p) continue;
        a.J[((long)s * D + d0 + k) * a.ldj + c] = post_sum_coherent(pl + e, pstride, a.nch);
    }
}

// 2 tiles (alpha_l o wL | alpha_l o wD), the staged rows, flags, the row weights, [1 / l], [1 / l^2], theta
template <int NB>
constexpr size_t jac_svgp_smem() {
    return sizeof(double) * (2 * (size_t)TileCfg<NB>::ELEMS + 2 * NB * PXS + 3 * NB + 4 * PMAXD + JTHETA);
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_jac_svgp(JacArgs a) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int E = TileCfg<NB>::ELEMS;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* KLs = smem;
    double* KDs = KLs + E;
    double* x1 = KDs + E;
    double* xs = x1 + NB * PXS;
    double* f1 = xs + NB * PXS;
    double* fs = f1 + NB;
    double* al = fs + NB;             // alpha_l rows of tile m
    double* il = al + NB;
    double* il2 = il + 2 * PMAXD;
    double* ths = il2 + 2 * PMAXD;
    const int t = threadIdx.x, l = blockIdx.z, D = a.D;
    const int ch = blockIdx.x / a.Ts, cs = blockIdx.x % a.Ts;
    const int m0 = ch * a.chunk;
    const int m1 = m0 + a.chunk < a.T ? m0 + a.chunk : a.T;
    jac_stage<NB>(a, a.theta + l * a.stheta, cs, ths, il, il2, xs, fs);
    const double* alpha = a.alpha + l * a.sA;
    // thread (column sl, dimension group dg): dimensions dg, dg + NG, ..; rows in row order (k_post_grad's epilogue)
    constexpr int NG = NTHREADS / NB, ND = PMAXD / NG;
    const int sl = t % NB, dg = t / NB;
    double acc[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) acc[k] = 0.0;
    for (int m = m0; m < m1; ++m) {
        __syncthreads();   // the previous step's readers (first step: jac_stage's writes are ordered below)
        for (int e = t; e < NB * D; e += NTHREADS) {
            const int r = e / D, d = e % D, gr = m * NB + r;
            x1[r * PXS + d] = gr < a.n1 ? a.X1[(long)gr * a.ldx1 + d] : 0.0;
        }
        if (t < NB) {
            const int gr = m * NB + t;
            f1[t] = gr < a.n1 ? a.X1[(long)gr * a.ldx1 + D] : -1.0;
            al[t] = alpha[gr];   // (zero beyond m: q_mu is zero padded, Lm^{-1} block diagonal there)
        }
        __syncthreads();
        jac_mf_tile<NB>(KLs, KDs, al, x1, f1, xs, fs, D, il, ths);
        __syncthreads();
        for (int r = 0; r < NB; ++r) {
            const double pl = KLs[r * S + sl], pd = KDs[r * S + sl];
#pragma unroll
            for (int k = 0; k < ND; ++k) {
                const int d = dg + k * NG;
                if (d < D) acc[k] += (pl * il2[d] + pd * il2[PMAXD + d]) * (x1[r * PXS + d] - xs[sl * PXS + d]);
            }
        }
    }
    double* gp = a.part + (((long)l * a.nch + ch) * a.Ts + cs) * D * NB;
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        const int d = dg + k * NG;
        if (d < D) gp[d * NB + sl] = acc[k];
    }
}

// dgl[l][cs][d][s] = the latent's chunk partials in chunk order
__global__ void k_jac_svgp_sum(JacArgs a, long per_latent, int batch) {
    const long total = per_latent * batch;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long l = e / per_latent, o = e % per_latent;
        a.dgl[e] = post_sum(a.part + l * a.nch * per_latent + o, per_latent, a.nch);
    }
}

// J[s][k][c] = sum_l W[c][l] dg_l[s][k] in latent order (no W: J[s][k][l] = dg_l[s][k]); one thread per entry
template <int NB>
__global__ void k_jac_svgp_mix(JacArgs a) {
    const long total = (long)a.nstar * a.D * a.p;
    const long per_latent = (long)a.Ts * a.D * NB;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % a.p);
        const long sk = e / a.p;
        const int k = (int)(sk % a.D), s = (int)(sk / a.D);
        const double* g = a.dgl + ((long)(s / NB) * a.D + k) * NB + s % NB;
        double v = 0.0;
        if (a.W) {
            for (int l = 0; l < a.L; ++l) v += a.W[(long)c * a.L + l] * g[l * per_latent];
        } else {
            v = g[c * per_latent];
        }
        a.J[((long)s * a.D + k) * a.ldj + c] = v;
    }
}

template <class K>
void jac_smem_attr(K kernel, size_t bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
}

}  // namespace

template <int NB>
void launch_jac_weights(const JacArgs& a, int batch, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        jac_smem_attr(&k_jac_weights<NB>, jac_weights_smem<NB>());
        attr = true;
    }
    hipLaunchKernelGGL(k_jac_weights<NB>, dim3(a.T * (a.Zc ? a.Tp : 1), 1, batch), dim3(NTHREADS),
                       jac_weights_smem<NB>(), s, a);
}

template <int NB>
void launch_jac_gpr(const JacArgs& a, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        jac_smem_attr(&k_jac_gpr<NB>, jac_gpr_smem<NB>());
        attr = true;
    }
    hipLaunchKernelGGL(k_jac_gpr<NB>, dim3(a.Ts * a.Tp * a.nch, a.dgroups, 1), dim3(NTHREADS), jac_gpr_smem<NB>(), s, a);
}

template <int NB>
void launch_jac_svgp(const JacArgs& a, int batch, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        jac_smem_attr(&k_jac_svgp<NB>, jac_svgp_smem<NB>());
        attr = true;
    }
    hipLaunchKernelGGL(k_jac_svgp<NB>, dim3(a.Ts * a.nch, 1, batch), dim3(NTHREADS), jac_svgp_smem<NB>(), s, a);
    const long per_latent = (long)a.Ts * a.D * NB;
    if (a.nch > 1) {
        const long tot = per_latent * batch;
        hipLaunchKernelGGL(k_jac_svgp_sum, dim3((unsigned)((tot + 255) / 256 < 1024 ? (tot + 255) / 256 : 1024)), dim3(256),
                           0, s, a, per_latent, batch);
    }
    const long tot = (long)a.nstar * a.D * a.p;
    hipLaunchKernelGGL(k_jac_svgp_mix<NB>, dim3((unsigned)((tot + 255) / 256 < 2048 ? (tot + 255) / 256 : 2048)), dim3(256),
                       0, s, a);
}

template void launch_jac_weights<32>(const JacArgs&, int, hipStream_t);
template void launch_jac_weights<64>(const JacArgs&, int, hipStream_t);
template void launch_jac_gpr<32>(const JacArgs&, hipStream_t);
template void launch_jac_gpr<64>(const JacArgs&, hipStream_t);
template void launch_jac_svgp<32>(const JacArgs&, int, hipStream_t);
template void launch_jac_svgp<64>(const JacArgs&, int, hipStream_t);

}  // namespace mfgp
