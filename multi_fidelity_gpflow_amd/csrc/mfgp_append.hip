// Block append to the cached GPR posterior (GPRPosterior.condition_on / fantasize).
//
// K_y = K + s2 I = L L^T of the n cached rows, with L^{-1} and Z = L^{-1} Y in the cache.  For k <= 32 new
// rows Xadd under them, with B the k x n cross block as the factorization reads it (the new row is the
// row argument of the kernel's entry function):
//   A = L^{-1} B^T,   S = K(Xadd, Xadd) + s2 I - A^T A = L22 L22^T,   R = L22^{-1}
//   L'^{-1} = [ L^{-1}         0 ]      Z' = [ Z               ]
//             [ -R A^T L^{-1}  R ]           [ R (Yadd - A^T Z) ]
// A and the mean A^T Z come from the cached predict's forward on Xadd (launch_post, A kept).
//
//   k_append_head  one workgroup: checks the fidelities, G = A^T A over 32-row steps on v_mfma_f64_16x16x4,
//                  S from G and the generated lower triangle of K(Xadd, Xadd), the single-wave factor
//                  (R), info, the new rows of Z, then W = -R A^T step by step into the workspace.  It
//                  also zeroes k_append_rows' counters and writes theta, Xadd and the bytes between the
//                  arrays of the new block.
//   k_append_rows  one task = one tile column j of the old block x `chunk` consecutive row tiles i >= j.
//                  Every L^{-1} tile is fetched once (the next one into registers while the current one
//                  is multiplied): its rows < n are stored to the new block at the new row stride, and
//                  W[:, tile i] L^{-1}[i, j] is accumulated on the matrix core.  The last workgroup to
//                  arrive at a column's counter sums the column's partials in task order and writes the
//                  bottom rows.  Behind the tasks, fill workgroups write every word no task owns: zeros
//                  right of the diagonal tiles, R, the identity padding, Z and X.
//
// Every word of the new block is written exactly once, every sum has a fixed order and there are no
// floating-point atomics: two calls with the same inputs give the same bits.  The old block's padding
// rows n..npad-1 are never copied: each tile entry is masked by its own indices (row < n, column <= row).
#include "mfgp_device.h"
#include "mfgp_internal.h"
#include "mfgp_post_device.h"

namespace mfgp {

int append_ntasks(int T, int chunk) {
    int n = 0;
    for (int j = 0; j < T; ++j) n += (T - j + chunk - 1) / chunk;
    return n;
}

__global__ __launch_bounds__(NTHREADS) void k_append_head(AppendArgs a) {
    constexpr int S = TileCfg<32>::S;
    constexpr int E = TileCfg<32>::ELEMS;
    __shared__ __attribute__((aligned(16))) double As[E];   // a 32-row step of A; then S (the factor's panel)
    __shared__ __attribute__((aligned(16))) double Gs[E];   // G = A^T A; then a 32-column block of Yadd - mean
    __shared__ __attribute__((aligned(16))) double Rs[E];   // R
    __shared__ double dg[32];
    __shared__ int bad, badf;
    const int t = threadIdx.x;
    const int D = a.D, k = a.k, n = a.n;
    // ---- what the row kernel and the new block need besides the factors
    for (int e = t; e < a.T; e += NTHREADS) a.cnt[e] = 0;
    for (int e = t; e < a.G; e += NTHREADS) a.thetao[e] = a.theta[e];
    for (int e = t; e < k * (D + 1); e += NTHREADS)
        a.Xo[(long)(n + e / (D + 1)) * (D + 1) + e % (D + 1)] = a.Xadd[(long)(e / (D + 1)) * a.ldxa + e % (D + 1)];
    for (int g = 0; g < 3; ++g)
        for (long b = a.gap0[g] + t; b < a.gap1[g]; b += NTHREADS) a.obase[b] = 0;
    // ---- the first row whose fidelity is no source of the kernel (wave 0: k <= 32)
    if (t < 64) {
        bool no = false;
        if (t < k) {
            const double f = a.Xadd[(long)t * a.ldxa + D];
            no = a.nlf ? graph_source(f, a.nlf) < 0 : !(f == 0.0 || f == 1.0);
        }
        const unsigned long long m = __ballot(no);
        if (t == 0) badf = m ? __ffsll((long long)m) : 0;
    }
    // ---- G = A^T A, one memory round trip a step hidden behind the previous step's product
    const int nst = a.npad / 32;
    TileRegs<32> ra;
    Acc<32> acc;
    acc_zero(acc);
    tile_fetch<32>(ra, a.Am, a.ldam);
    for (int s = 0; s < nst; ++s) {
        __syncthreads();   // the previous step's readers of As
        tile_put<32>(As, ra);
        if (s + 1 < nst) tile_fetch<32>(ra, a.Am + (long)(s + 1) * 32 * a.ldam, a.ldam);
        __syncthreads();
        tile_mma<32, true, false>(acc, As, As, 1.0);
    }
    __syncthreads();
    acc_to_lds<32>(acc, Gs);
    __syncthreads();
    // ---- S: the lower triangle of K(Xadd, Xadd) (row i is the row argument) + s2 (+ jitter) - G; identity beyond k
    const double dadd = a.theta[a.G - 1] + a.diag_add;
    for (int e = t; e < 32 * 32; e += NTHREADS) {
        const int r = e / 32, c = e % 32;
        double v = (r == c) ? 1.0 : 0.0;
        if (c <= r && r < k) {
            v = design_entry(a.Xadd + (long)r * a.ldxa, a.Xadd + (long)c * a.ldxa, D, a.nlf, a.theta);
            if (r == c) v += dadd;
            v -= Gs[r * S + c];
        }
        As[r * S + c] = v;
    }
    __syncthreads();
    tile_potrf_inv_w1(As, Rs, dg, &bad);
    if (t == 0) a.info[0] = badf ? -badf : bad;
    for (int e = t; e < 32 * 32; e += NTHREADS) a.Rw[e] = Rs[(e / 32) * S + e % 32];
    // ---- the new rows of Z: R (Yadd - mean), 32 outputs at a time (a fantasy row is exactly zero)
    for (int c0 = 0; c0 < a.ppad; c0 += 32) {
        __syncthreads();   // the previous block's readers of Gs
        for (int e = t; e < 32 * 32; e += NTHREADS) {
            const int r = e / 32, c = c0 + e % 32;
            Gs[r * S + e % 32] =
                (a.Yadd && r < k && c < a.p) ? a.Yadd[(long)r * a.ldya + c] - a.mean[(long)r * a.ldm + c] : 0.0;
        }
        __syncthreads();
        for (int e = t; e < 32 * 32; e += NTHREADS) {
            const int r = e / 32, c = e % 32;
            if (r >= k) continue;
            double v = 0.0;
            if (a.Yadd && c0 + c < a.p)
                for (int q = 0; q <= r; ++q) v += Rs[r * S + q] * Gs[q * S + c];
            a.LZo[(long)(n + r) * a.ldro + a.npado + c0 + c] = v;
        }
    }
    // ---- W = -R A^T, step by step (A is re-read from L2)
    tile_fetch<32>(ra, a.Am, a.ldam);
    for (int s = 0; s < nst; ++s) {
        __syncthreads();
        tile_put<32>(As, ra);
        if (s + 1 < nst) tile_fetch<32>(ra, a.Am + (long)(s + 1) * 32 * a.ldam, a.ldam);
        __syncthreads();
        Acc<32> w;
        acc_zero(w);
        tile_mma<32, false, true>(w, Rs, As, -1.0);
        acc_store(w, a.W + (long)s * 32, a.npad);
    }
}

// the words of the new block no task owns, by the fill workgroup fb of nf
template <int NB>
__device__ __forceinline__ void append_fill(const AppendArgs& a, int fb, int nf) {
    const int t = threadIdx.x, n = a.n, k = a.k;
    const long nx = (long)n * (a.D + 1);
    for (long e = (long)fb * NTHREADS + t; e < nx; e += (long)nf * NTHREADS) a.Xo[e] = a.X[e];
    for (int r = fb; r < a.npado; r += nf) {
        double* row = a.LZo + (long)r * a.ldro;
        if (r < n) {            // right of the row's diagonal tile: zero; Z: the old row
            for (int c = (r / NB + 1) * NB + t; c < a.npado; c += NTHREADS) row[c] = 0.0;
            const double* zr = a.LZ + (long)r * a.ldr + a.npad;
            for (int c = t; c < a.ppad; c += NTHREADS) row[a.npado + c] = c < a.p ? zr[c] : 0.0;
        } else if (r < n + k) { // R, lower triangular; Z is the head kernel's
            const int rr = r - n;
            for (int c = n + t; c < a.npado; c += NTHREADS) row[c] = (c - n <= rr) ? a.Rw[rr * 32 + (c - n)] : 0.0;
        } else {                // identity padding, zero Z
            for (int c = t; c < a.npado; c += NTHREADS) row[c] = (c == r) ? 1.0 : 0.0;
            for (int c = t; c < a.ppad; c += NTHREADS) row[a.npado + c] = 0.0;
        }
    }
}

template <int NB>
constexpr size_t append_smem() {
    return sizeof(double) * 2 * (size_t)TileCfg<NB>::ELEMS;
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_append_rows(AppendArgs a) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int E = TileCfg<NB>::ELEMS;
    constexpr int NP = NB * NB / 2 / NTHREADS;   // 16-byte pairs of an L^{-1} tile per thread
    constexpr int NW = 32 * NB / 2 / NTHREADS;   // of a 32 x NB block of W
    constexpr int NBLK = TileCfg<NB>::NBLK;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* Ls = smem;        // (L^{-1})_ij, masked
    double* Ws = Ls + E;      // W[:, tile i] in rows 0..31 (NB = 64: rows 32..63 stay zero)
    __shared__ int last;
    const int t = threadIdx.x;
    if ((int)blockIdx.x >= a.ntask) {
        append_fill<NB>(a, (int)blockIdx.x - a.ntask, (int)gridDim.x - a.ntask);
        return;
    }
    // task -> (tile column j, chunk ch): column j has T - j row tiles
    int j = 0, ch = (int)blockIdx.x, nch = 0;
    for (; j < a.T; ++j) {
        nch = (a.T - j + a.chunk - 1) / a.chunk;
        if (ch < nch) break;
        ch -= nch;
    }
    if (j >= a.T) return;   // (never: the grid is append_ntasks + nfill)
    const int base = (int)blockIdx.x - ch;
    const int i0 = j + ch * a.chunk;
    const int i1 = i0 + a.chunk < a.T ? i0 + a.chunk : a.T;
    if (NB > 32)
        for (int e = t; e < (NB - 32) * S; e += NTHREADS) Ws[32 * S + e] = 0.0;
    Acc<NB> acc;
    acc_zero(acc);
    TileRegs<NB> rl;
    f64x2 rw[NW];
    auto fetch = [&](int i) {
        tile_fetch<NB>(rl, a.LZ + (long)i * NB * a.ldr + (long)j * NB, a.ldr);
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const int pr = t + q * NTHREADS, row = pr / (NB / 2), c = 2 * (pr % (NB / 2));
            rw[q] = *reinterpret_cast<const f64x2*>(a.W + (long)row * a.npad + (long)i * NB + c);
        }
    };
    fetch(i0);
    for (int i = i0; i < i1; ++i) {
        __syncthreads();   // the previous step's readers of Ls / Ws
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int pr = t + q * NTHREADS, row = pr / (NB / 2), c = 2 * (pr % (NB / 2));
            const int gr = i * NB + row, gc = j * NB + c;
            f64x2 v = rl.v[q];
            if (!(gr < a.n && gc <= gr)) v[0] = 0.0;
            if (!(gr < a.n && gc + 1 <= gr)) v[1] = 0.0;
            *reinterpret_cast<f64x2*>(Ls + row * S + c) = v;
            if (gr < a.n) *reinterpret_cast<f64x2*>(a.LZo + (long)gr * a.ldro + gc) = v;
        }
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const int pr = t + q * NTHREADS, row = pr / (NB / 2), c = 2 * (pr % (NB / 2));
            *reinterpret_cast<f64x2*>(Ws + row * S + c) = rw[q];
        }
        if (i + 1 < i1) fetch(i + 1);
        __syncthreads();
        tile_mma<NB, false, false>(acc, Ws, Ls, 1.0);
    }
    // ---- the task's partial of bottom[:, tile j] (rows 0..31 of the accumulator)
    const long pw = 32L * NB;
    double* pt = a.part + (long)blockIdx.x * pw;
#pragma unroll
    for (int q = 0; q < NBLK; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = acc_row<NB>(q, r);
            if (row < 32) st_coherent(pt + row * NB + acc_col<NB>(q), acc.v[q][r]);
        }
    drain_stores();
    __syncthreads();
    if (t == 0) last = arrive(a.cnt + j) == nch - 1;
    __syncthreads();
    if (!last) return;
    // ---- the bottom rows of this tile column, by its last workgroup: the partials in task order
    for (int e = t; e < 32 * NB; e += NTHREADS) {
        const int r = e / NB, gc = j * NB + e % NB;
        if (r < a.k && gc < a.n)
            a.LZo[(long)(a.n + r) * a.ldro + gc] = post_sum_coherent(a.part + (long)base * pw + e, pw, nch);
    }
}

template <int NB>
void launch_append(const AppendArgs& a, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_append_rows<NB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)append_smem<NB>());
        attr = true;
    }
    hipLaunchKernelGGL(k_append_head, dim3(1), dim3(NTHREADS), 0, s, a);
    hipLaunchKernelGGL(k_append_rows<NB>, dim3(a.ntask + a.nfill), dim3(NTHREADS), append_smem<NB>(), s, a);
}

template void launch_append<32>(const AppendArgs&, hipStream_t);
template void launch_append<64>(const AppendArgs&, hipStream_t);

}  // namespace mfgp
