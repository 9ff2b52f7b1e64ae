// Leave-group-out cross-validation from the cached GPR posterior (GPRPosterior.leave_out).
//
// For a set S of training rows, at the snapshot's hyper-parameters, with C = L^{-1}[:, S] and Z = L^{-1} Y:
//   G = C^T C = [K_y^{-1}]_SS,   H = C^T Z = [K_y^{-1} Y]_S,
//   E = y_S - mu_{S|-S} = G^{-1} H,   Sigma_f = G^{-1} - s2 I,
//   log p(y_S | y_-S)[c] = -1/2 H[:, c]^T G^{-1} H[:, c] + 1/2 log det G - |S| / 2 log 2 pi.
// Nothing but the cache's LZ rows and its noise entry is read: no Gram, no kernel function, no X.
//
//   k_lo_pack  one workgroup: checks the group table (sizes in 1..gmax, rows in 0..n-1), zeroes the
//              arrival counters and packs whole consecutive groups into tasks of at most 32 columns
//              (first fit in order: a group is never split).  A task's columns are then one
//              contiguous stretch of `rows`, so the table is one first-group index per task.
//   k_lo       one workgroup per (task, chunk of 32-row steps, block of 96 outputs): per step the
//              gathered 32 x 32 block of C and the 32 x 96 block of Z are staged in LDS and
//              C^T [C | Z] is accumulated on v_mfma_f64_16x16x4.  The last workgroup to arrive at a
//              task's counter sums the chunk partials in chunk order, zeroes the cross-group entries
//              of G (1 on the padding diagonal), factors and inverts the block-diagonal 32 x 32 matrix
//              with the single-wave factor and writes E, Sigma_f, the log density and info.
//
// The steps are 32 rows whatever tile size the cache was laid out for (its tile size enters through
// npad and the row stride only), and every entry is masked by its own indices (row >= column, row < n,
// output < p): the kernel relies neither on what the build left above the diagonal of L^{-1} nor on
// the padded rows n..npad.  Every sum has a fixed order and there are no floating-point atomics: two
// calls with the same inputs give the same bits.
#include "mfgp_device.h"
#include "mfgp_internal.h"

namespace mfgp {

constexpr int LO_STAGE = 2048;   // group offsets k_lo_pack stages in LDS at a time
constexpr double LO_LOG2PI = 1.8378770664093453;

__global__ __launch_bounds__(NTHREADS) void k_lo_pack(LoArgs a) {
    __shared__ int so[LO_STAGE + 1];
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t == 0) bad = 0;
    __syncthreads();
    int b = 0;
    for (int g = t; g < a.ngroups; g += NTHREADS) {
        const int o0 = a.offsets[g], o1 = a.offsets[g + 1];
        if (o0 < 0 || o1 > a.nrows || o1 - o0 < 1 || o1 - o0 > a.gmax) b = 1;
    }
    if (t == 0 && (a.offsets[0] != 0 || a.offsets[a.ngroups] != a.nrows)) b = 1;
    for (int r = t; r < a.nrows; r += NTHREADS) {
        const int v = a.rows[r];
        if (v < 0 || v >= a.n) b = 1;
    }
    if (b) bad = 1;   // (every writer stores the same value)
    for (int e = t; e < a.ntmax * a.ny; e += NTHREADS) a.cnt[e] = 0;
    __syncthreads();
    int nt = 0, cur = LO_W + 1;   // thread 0: tasks so far, columns of the open task (none open yet)
    if (!bad) {
        for (int base = 0; base < a.ngroups; base += LO_STAGE) {
            const int m = a.ngroups - base < LO_STAGE ? a.ngroups - base : LO_STAGE;
            for (int e = t; e <= m; e += NTHREADS) so[e] = a.offsets[base + e];
            __syncthreads();
            if (t == 0) {
                for (int k = 0; k < m; ++k) {
                    const int sz = so[k + 1] - so[k];
                    if (cur + sz > LO_W) {   // the group opens the next task
                        if (nt < a.ntmax) a.tab[1 + nt] = base + k;
                        ++nt;
                        cur = 0;
                    }
                    cur += sz;
                }
            }
            __syncthreads();
        }
        if (t == 0) {
            if (nt > a.ntmax) bad = 1;   // (never: lo_layout's bound holds for sizes in 1..gmax)
            else a.tab[1 + nt] = a.ngroups;
        }
        __syncthreads();
    }
    if (bad) {   // a malformed table: nothing runs, every group reports -1
        for (int g = t; g < a.ngroups; g += NTHREADS) a.info[g] = -1;
        nt = 0;
    }
    if (t == 0) a.tab[0] = nt;
}

// sum over k < n of base[k * stride] in k order, the sc1 loads issued eight at a time
__device__ __forceinline__ double lo_sum_coherent(const double* base, long stride, int n) {
    double s = 0.0;
    for (int k0 = 0; k0 < n; k0 += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = k0 + j < n ? ld_coherent(base + (long)(k0 + j) * stride) : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    return s;
}

__global__ __launch_bounds__(NTHREADS) void k_lo(LoArgs a) {
    constexpr int S = TileCfg<32>::S;
    constexpr int E = TileCfg<32>::ELEMS;
    constexpr long PW = 32 * 32 * (1 + LO_PT);   // doubles of one partial: G, then LO_PT blocks of H
    __shared__ __attribute__((aligned(16))) double Cs[E];           // gathered C block; epilogue: G, then G^{-1}
    __shared__ __attribute__((aligned(16))) double Rs[E];           // epilogue: the inverse factor of G
    __shared__ __attribute__((aligned(16))) double Zs[LO_PT * E];   // Z blocks; epilogue: H, then W = R H
    __shared__ double dg[32];
    __shared__ int cols[LO_W], cgs[LO_W], cgn[LO_W], sgo[LO_W + 1];
    __shared__ int last, bad;
    const int t = threadIdx.x;
    const int task = blockIdx.x / a.nch, c = blockIdx.x % a.nch, y = blockIdx.y;
    if (task >= a.tab[0]) return;
    const int g0 = a.tab[1 + task], ng = a.tab[2 + task] - g0;   // 1 <= ng <= 32 groups
    const int c0 = a.offsets[g0], ncols = a.offsets[g0 + ng] - c0;
    if (t < LO_W) cols[t] = t < ncols ? a.rows[c0 + t] : -1;
    if (t <= ng) sgo[t] = a.offsets[g0 + t] - c0;
    __syncthreads();
    int minr = a.n - 1;
    for (int j = 0; j < ncols; ++j) minr = cols[j] < minr ? cols[j] : minr;
    // the task's columns are zero above row minr: its first step, and the first chunk with work
    const int T32 = (a.n + 31) / 32;
    const int s0 = minr / 32, cfirst = s0 / a.chunk;
    if (c < cfirst) return;
    const int sb = s0 > c * a.chunk ? s0 : c * a.chunk;
    const int se = (c + 1) * a.chunk < T32 ? (c + 1) * a.chunk : T32;
    const int pc0 = y * 32 * LO_PT;
    const int nh = (a.p - pc0 + 31) / 32 < LO_PT ? (a.p - pc0 + 31) / 32 : LO_PT;
    const double* Zc = a.LZ + a.npad + pc0;
    Acc<32> accG, accH[LO_PT];
    acc_zero(accG);
#pragma unroll
    for (int h = 0; h < LO_PT; ++h) acc_zero(accH[h]);
    // One memory round trip a step, hidden behind the previous step's products (k_post_a's scheme)
    double rc[4];
    f64x2 rz[LO_PT][2];
    auto fetch = [&](int s) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + q * NTHREADS, gr = s * 32 + (e >> 5), col = cols[e & 31];
            rc[q] = (col >= 0 && gr >= col && gr < a.n) ? a.LZ[(long)gr * a.ldr + col] : 0.0;
        }
#pragma unroll
        for (int h = 0; h < LO_PT; ++h) {
            if (h >= nh) continue;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int pr = t + q * NTHREADS, gr = s * 32 + (pr >> 4), cc = h * 32 + 2 * (pr & 15);
                f64x2 v = {0.0, 0.0};
                if (gr < a.n) v = *reinterpret_cast<const f64x2*>(Zc + (long)gr * a.ldr + cc);
                if (pc0 + cc >= a.p) v[0] = 0.0;
                if (pc0 + cc + 1 >= a.p) v[1] = 0.0;
                rz[h][q] = v;
            }
        }
    };
    fetch(sb);
    for (int s = sb; s < se; ++s) {
        __syncthreads();   // the previous step's readers of Cs / Zs are done
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + q * NTHREADS;
            Cs[(e >> 5) * S + (e & 31)] = rc[q];
        }
#pragma unroll
        for (int h = 0; h < LO_PT; ++h) {
            if (h >= nh) continue;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int pr = t + q * NTHREADS;
                *reinterpret_cast<f64x2*>(Zs + h * E + (pr >> 4) * S + 2 * (pr & 15)) = rz[h][q];
            }
        }
        if (s + 1 < se) fetch(s + 1);
        __syncthreads();
        tile_mma<32, true, false>(accG, Cs, Cs, 1.0);
#pragma unroll
        for (int h = 0; h < LO_PT; ++h)
            if (h < nh) tile_mma<32, true, false>(accH[h], Cs, Zs + h * E, 1.0);
    }
    double* mine = a.part + (((long)task * a.nch + c) * a.ny + y) * PW;
    acc_store_coherent<32>(accG, mine, 32);
#pragma unroll
    for (int h = 0; h < LO_PT; ++h)
        if (h < nh) acc_store_coherent<32>(accH[h], mine + 1024 * (1 + h), 32);
    drain_stores();
    __syncthreads();
    if (t == 0) last = arrive(a.cnt + task * a.ny + y) == a.nch - cfirst - 1;
    __syncthreads();
    if (!last) return;
    // ---- the task's outputs, by its last workgroup: G and H = the chunk partials in chunk order
    const double* first = a.part + (((long)task * a.nch + cfirst) * a.ny + y) * PW;
    for (int e = t; e < 1024 * (1 + nh); e += NTHREADS) {
        const int blk = e >> 10, r = (e >> 5) & 31, cc = e & 31;
        const double v = lo_sum_coherent(first + e, (long)a.ny * PW, a.nch - cfirst);
        (blk ? Zs + (blk - 1) * E : Cs)[r * S + cc] = v;
    }
    if (t < LO_W) {   // column -> first column and size of its group (a padding column: a group of its own)
        int gs = t, gn = 1;
        for (int k = 0; k < ng; ++k)
            if (sgo[k] <= t && t < sgo[k + 1]) { gs = sgo[k]; gn = sgo[k + 1] - sgo[k]; }
        cgs[t] = gs;
        cgn[t] = gn;
    }
    __syncthreads();
    // block-diagonal G: cross-group entries zeroed, 1 on the padding diagonal (its sums are exact zeros)
    for (int e = t; e < 1024; e += NTHREADS) {
        const int r = e >> 5, cc = e & 31;
        if (cgs[r] != cgs[cc]) Cs[r * S + cc] = 0.0;
        else if (r >= ncols) Cs[r * S + cc] = 1.0;
    }
    __syncthreads();
    tile_potrf_inv_w1(Cs, Rs, dg, &bad);   // Rs = R with R^T R = G^{-1}, dg = diag(chol G)
    // W = R H (the groups' blocks of R are independent: R is block diagonal)
#pragma unroll
    for (int h = 0; h < LO_PT; ++h) {
        acc_zero(accH[h]);
        if (h < nh) tile_mma<32, false, false>(accH[h], Rs, Zs + h * E, 1.0);
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < LO_PT; ++h)
        if (h < nh) acc_to_lds<32>(accH[h], Zs + h * E);
    __syncthreads();
    const int ncy = a.p - pc0 < 32 * LO_PT ? a.p - pc0 : 32 * LO_PT;
    for (int e = t; e < ng * ncy; e += NTHREADS) {
        const int k = e / ncy, cc = e % ncy;
        const double* w = Zs + (cc >> 5) * E + (cc & 31);
        double quad = 0.0, ld = 0.0;
        for (int i = sgo[k]; i < sgo[k + 1]; ++i) {
            quad += w[i * S] * w[i * S];
            ld += log(dg[i]);
        }
        a.logdens[(long)(g0 + k) * a.p + pc0 + cc] = -0.5 * quad + ld - 0.5 * (sgo[k + 1] - sgo[k]) * LO_LOG2PI;
    }
    if (y == 0 && t < ng) {   // first non-positive / non-finite pivot of the group (1-based), 0: none
        int bi = 0;
        for (int i = sgo[t + 1] - 1; i >= sgo[t]; --i)
            if (!(dg[i] > 0.0 && dg[i] < INFINITY)) bi = i - sgo[t] + 1;
        a.info[g0 + t] = bi;
    }
    // E = R^T W
#pragma unroll
    for (int h = 0; h < LO_PT; ++h) {
        if (h >= nh) continue;
        Acc<32> acc;
        acc_zero(acc);
        tile_mma<32, true, false>(acc, Rs, Zs + h * E, 1.0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = acc_row<32>(0, r), oc = pc0 + h * 32 + acc_col<32>(0);
            if (row < ncols && oc < a.p) a.resid[(long)(c0 + row) * a.ldres + oc] = acc.v[0][r];
        }
    }
    if (y != 0 || !a.cov) return;
    // Sigma_f = R^T R - s2 I: row r of the output holds its row of its group's block
    acc_zero(accG);
    tile_mma<32, true, false>(accG, Rs, Rs, 1.0);
    acc_to_lds<32>(accG, Cs);   // (the factor is done with its panel)
    __syncthreads();
    const double s2 = a.noise[0];
    for (int e = t; e < ncols * a.gmax; e += NTHREADS) {
        const int j = e / a.gmax, k = e % a.gmax;
        double v = 0.0;
        if (k < cgn[j]) v = Cs[j * S + cgs[j] + k] - (cgs[j] + k == j ? s2 : 0.0);
        a.cov[(long)(c0 + j) * a.ldc + k] = v;
    }
}

void launch_leave_out(const LoArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_lo_pack, dim3(1), dim3(NTHREADS), 0, s, a);
    hipLaunchKernelGGL(k_lo, dim3(a.ntmax * a.nch, a.ny, 1), dim3(NTHREADS), 0, s, a);
}

}  // namespace mfgp
