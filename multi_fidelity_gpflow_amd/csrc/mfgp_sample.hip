// Joint Gaussian draws (GPflow GPModel.predict_f_samples / conditionals.util.sample_mvn):
// out = mean + chol(cov + jitter I) eps for a batch of dense covariances.
//
//   k_sample_factor  left-looking tile Cholesky that KEEPS L, one launch per tile column k.  Workgroup
//                    i >= k forms S_ik - sum_{m<k} L_im L_km^T on the matrix core, and every workgroup of
//                    the launch forms the diagonal tile S_kk - sum_{m<k} L_km L_km^T as well, factors it
//                    in LDS itself and solves its own panel tile against it: a launch needs nothing from
//                    another workgroup of the same launch, launch boundaries are the only ordering.  The
//                    jitter is added while the tile is loaded; only the lower triangle of cov is read.
//                    (The existing steps -- launch_chol_steps, k_chol_flow -- hand back L^{-1}: their
//                    diagonal tiles are factored in registers and only the inverse tile is stored, so L's
//                    diagonal tiles cannot be taken from CholArgs::A.)
//   k_sample_apply   out tile (row tile i) x (32 columns q = s * ncol + c) = mean + sum_{j<=i} L_ij E_j,
//                    the E_j tile gathered through the caller's strides into LDS, the next L / E tile
//                    fetched into registers before the current product (k_post_a's scheme).
//
// Tiles are 32 x 32 whatever the handle's tile size: the covariance is dense with its own leading
// dimension.  Rows and columns beyond n (the ragged last tile) are an identity block in the factor and
// zero rows of E: they add exact zeros and are never stored.  Every sum has a fixed order and there are
// no atomics: the same inputs give the same bits.  A failed pivot (non-positive or non-finite) is
// recorded in info and the NaNs run through the remaining launches like any other number.
#include "mfgp_device.h"
#include "mfgp_internal.h"

namespace mfgp {

namespace {

constexpr int SNB = 32;
constexpr int SS = TileCfg<SNB>::S;
constexpr int SE = TileCfg<SNB>::ELEMS;

// Cholesky of the SPD 32 x 32 LDS tile A (stride SS, lower triangle valid, upper never read) in
// 8-column blocks, the factor left in A's lower triangle (tile_potrf_inv_b8's factor phase):
//   1. every thread factors the 8 x 8 pivot block redundantly in registers;
//   2. one thread per row below substitutes its panel row, L_rb = A_rb L_bb^{-T};
//   3. barrier; all threads apply the rank-8 update of the trailing lower part; barrier.
// Returns the first non-positive / non-finite pivot (1-based, 0: none), the same in every thread.
__device__ int sample_potrf32(double* __restrict__ A) {
    const int t = threadIdx.x;
    int badloc = 0;
#pragma unroll
    for (int b = 0; b < SNB / 8; ++b) {
        const int r0 = 8 * b;
        double l[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) l[i][j] = A[(r0 + i) * SS + r0 + j];
        double rinv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double akk = l[k][k];
            if (badloc == 0 && !(akk > 0.0 && akk < INFINITY)) badloc = r0 + k + 1;
            const double lkk = sqrt(akk);
            const double rk = 1.0 / lkk;
            l[k][k] = lkk;
            rinv[k] = rk;
#pragma unroll
            for (int i = k + 1; i < 8; ++i) l[i][k] *= rk;
#pragma unroll
            for (int j = k + 1; j < 8; ++j)
#pragma unroll
                for (int i = j; i < 8; ++i) l[i][j] -= l[i][k] * l[j][k];
        }
        const int rows = SNB - r0 - 8;
        double x[8];
        if (t < rows) {
            const int r = r0 + 8 + t;
#pragma unroll
            for (int c = 0; c < 8; ++c) x[c] = A[r * SS + r0 + c];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                double v = x[c];
#pragma unroll
                for (int m = 0; m < c; ++m) v -= x[m] * l[c][m];
                x[c] = v * rinv[c];
            }
        }
        __syncthreads();   // every thread has read the pivot block and its panel row
        if (t < rows) {
            const int r = r0 + 8 + t;
#pragma unroll
            for (int c = 0; c < 8; ++c) A[r * SS + r0 + c] = x[c];
        }
        if (t == NTHREADS - 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) A[(r0 + i) * SS + r0 + j] = l[i][j];
        }
        __syncthreads();
        if (rows > 0) {
            for (int e = t; e < rows * rows; e += NTHREADS) {
                const int ii = e / rows, jj = e - ii * rows;
                if (jj > ii) continue;
                const int i = r0 + 8 + ii, j = r0 + 8 + jj;
                double acc = A[i * SS + j];
#pragma unroll
                for (int m = 0; m < 8; ++m) acc -= A[i * SS + r0 + m] * A[j * SS + r0 + m];
                A[i * SS + j] = acc;
            }
        }
        __syncthreads();
    }
    return badloc;
}

__global__ __launch_bounds__(NTHREADS) void k_sample_factor(SampleArgs a, int k) {
    __shared__ __attribute__((aligned(16))) double Ak[SE];   // L_km
    __shared__ __attribute__((aligned(16))) double Ai[SE];   // L_im
    __shared__ __attribute__((aligned(16))) double Ds[SE];   // the diagonal tile, then L_kk
    __shared__ __attribute__((aligned(16))) double Ps[SE];   // the panel tile, then L_ik
    const int t = threadIdx.x, b = blockIdx.z, i = k + (int)blockIdx.x;
    const bool panel = i > k;   // (uniform over the workgroup)
    const double* __restrict__ C = a.cov + (long)b * a.sC;
    double* __restrict__ L = a.Lw + (long)b * a.sL;
    const int n = a.n;
    Acc<SNB> accD, accP;
    acc_zero(accP);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int lr = acc_row<SNB>(0, r), lc = acc_col<SNB>(0);
        const int gr = k * SNB + lr, gc = k * SNB + lc;
        double v = 0.0;
        if (gr < n) {
            if (gc <= gr) v = C[(long)gr * a.ldc + gc] + (gc == gr ? a.jitter : 0.0);
        } else if (gc == gr) {
            v = 1.0;   // beyond n: an identity block
        }
        accD.v[0][r] = v;
        if (panel) {
            const int pr = i * SNB + lr;   // (its columns k * 32 + lc are < n: k < i <= T - 1)
            accP.v[0][r] = pr < n ? C[(long)pr * a.ldc + gc] : 0.0;
        }
    }
    // the next step's two tiles are fetched into registers before the current products
    TileRegs<SNB> rk, ri;
    auto fetch = [&](int m) {
        tile_fetch<SNB>(rk, L + (long)k * SNB * a.ldl + (long)m * SNB, a.ldl);
        if (panel) tile_fetch<SNB>(ri, L + (long)i * SNB * a.ldl + (long)m * SNB, a.ldl);
    };
    if (k > 0) fetch(0);
    for (int m = 0; m < k; ++m) {
        __syncthreads();   // the previous step's readers of Ak / Ai are done
        tile_put<SNB>(Ak, rk);
        if (panel) tile_put<SNB>(Ai, ri);
        if (m + 1 < k) fetch(m + 1);
        __syncthreads();
        tile_mma<SNB, false, true>(accD, Ak, Ak, -1.0);
        if (panel) tile_mma<SNB, false, true>(accP, Ai, Ak, -1.0);
    }
    acc_to_lds<SNB>(accD, Ds);
    if (panel) acc_to_lds<SNB>(accP, Ps);
    __syncthreads();
    const int bad = sample_potrf32(Ds);   // (ends with a barrier)
    if (!panel) {
        if (t == 0) {
            const int prev = k > 0 ? a.info[b] : 0;
            a.info[b] = prev ? prev : (bad ? k * SNB + bad : 0);
        }
        for (int e = t; e < SNB * SNB; e += NTHREADS) {
            const int r = e / SNB, c = e % SNB;
            L[((long)k * SNB + r) * a.ldl + (long)k * SNB + c] = c <= r ? Ds[r * SS + c] : 0.0;
        }
        return;
    }
    // L_ik = P L_kk^{-T}: one thread per row, forward substitution in column order
    if (t < SNB) {
        double x[SNB];
#pragma unroll
        for (int c = 0; c < SNB; ++c) x[c] = Ps[t * SS + c];
#pragma unroll
        for (int c = 0; c < SNB; ++c) {
            double v = x[c];
#pragma unroll
            for (int m = 0; m < c; ++m) v = fma(-x[m], Ds[c * SS + m], v);
            x[c] = v / Ds[c * SS + c];
        }
#pragma unroll
        for (int c = 0; c < SNB; ++c) Ps[t * SS + c] = x[c];
    }
    __syncthreads();
    tile_store<SNB>(L + (long)i * SNB * a.ldl + (long)k * SNB, a.ldl, Ps);
}

__global__ __launch_bounds__(NTHREADS) void k_sample_apply(SampleArgs a) {
    __shared__ __attribute__((aligned(16))) double Ls[SE];
    __shared__ __attribute__((aligned(16))) double Es[SE];
    const int t = threadIdx.x, i = blockIdx.y, b = blockIdx.z;
    const long q0 = (long)blockIdx.x * SNB;
    const long Q = (long)a.nsamp * a.ncol;
    const int n = a.n;
    const double* __restrict__ L = a.Lw + (long)b * a.sL + (long)i * SNB * a.ldl;
    // gather: this thread's column of the E tile and its four rows r0 + 8 u
    const int cq = t & (SNB - 1), r0 = t >> 5;
    const long q = q0 + cq;
    const bool qok = q < Q;
    const double* __restrict__ ep = a.eps + (long)b * a.bs + (qok ? (q / a.ncol) * a.ss + (q % a.ncol) : 0L);
    TileRegs<SNB> rl;
    double re[4];
    auto fetch = [&](int j) {
        tile_fetch<SNB>(rl, L + (long)j * SNB, a.ldl);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = j * SNB + r0 + 8 * u;
            re[u] = (qok && row < n) ? ep[(long)row * a.rs] : 0.0;
        }
    };
    Acc<SNB> acc;
    acc_zero(acc);
    fetch(0);
    for (int j = 0; j <= i; ++j) {
        __syncthreads();   // the previous step's readers of Ls / Es are done
        tile_put<SNB>(Ls, rl);
#pragma unroll
        for (int u = 0; u < 4; ++u) Es[(r0 + 8 * u) * SS + cq] = re[u];
        if (j < i) fetch(j + 1);
        __syncthreads();
        tile_mma<SNB, false, false>(acc, Ls, Es, 1.0);
    }
    const long oq = q0 + acc_col<SNB>(0);
    if (oq >= Q) return;
    const long s = oq / a.ncol, c = oq % a.ncol;
    const double* __restrict__ mp = a.mean + (long)b * a.mean_bs + c;
    double* __restrict__ op = a.out + (long)b * a.bs + s * a.ss + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = i * SNB + acc_row<SNB>(0, r);
        if (row < n) op[(long)row * a.rs] = mp[(long)row * a.mean_rs] + acc.v[0][r];
    }
}

}  // namespace

size_t mvn_sample_ws_bytes(int n, int batch) {
    const size_t npad = (size_t)((n + SNB - 1) / SNB) * SNB;
    return npad * npad * sizeof(double) * (size_t)batch + 256;
}

void launch_mvn_sample(SampleArgs a, void* ws, hipStream_t s) {
    const int T = (a.n + SNB - 1) / SNB;
    const long npad = (long)T * SNB;
    a.Lw = reinterpret_cast<double*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    a.ldl = npad;
    a.sL = npad * npad;
    for (int k = 0; k < T; ++k)
        hipLaunchKernelGGL(k_sample_factor, dim3(T - k, 1, a.batch), dim3(NTHREADS), 0, s, a, k);
    const long Q = (long)a.nsamp * a.ncol;
    hipLaunchKernelGGL(k_sample_apply, dim3((unsigned)((Q + SNB - 1) / SNB), T, a.batch), dim3(NTHREADS), 0, s, a);
}

}  // namespace mfgp
