// Batched Gaussian log-density with its gradients (include/mfgp.h mfgp_mvn_logpdf) and, on the same covariance
// and the same LDS factorization, the batched Fisher matrix (mfgp_mvn_fisher, further down): per row s,
//   Sigma_s = obs_cov + diag(var_s + obs_var_s),  r = y_s - mean_s,
//   logp_s  = -1/2 r^T Sigma_s^{-1} r - 1/2 log det Sigma_s - (P / 2) log 2 pi,
//   gmean_s = a = Sigma_s^{-1} r,  gvar_s[c] = 1/2 (a_c^2 - (Sigma_s^{-1})_cc).
//
//   k_mvn_dense  (obs_cov given, P <= 128) one workgroup per row; everything lives in LDS.  The image is
//                (P8 + 1) x (P8 + 1) doubles, P8 = P rounded up to 8: the lower triangle of Sigma_s (the
//                diagonal terms added while obs_cov's lower triangle is loaded, an identity block beyond P)
//                and r^T as one more ROW under it.  The Cholesky runs in 8-column blocks (sample_potrf32's
//                scheme at any size: the 8 x 8 pivot block redundantly in every thread's registers, one
//                thread per row below substitutes its panel row, all threads apply the rank-8 update:
//                3 barriers per 8 columns instead of 2 per column).  Because r^T is a row of the image,
//                its panel steps ARE the forward solve z = L^{-1} r, and the trailing update leaves
//                -z^T z in the corner element: the quadratic form costs no pass of its own.  With a
//                gradient asked for, L is inverted in place from the last 8-column block to the first
//                (X21 = -X22 L21 X11, 3 barriers per block), and one thread per column c takes
//                a_c = sum_i X_ic z_i and (Sigma^{-1})_cc = sum_i X_ic^2 in row order.
//                The LDS size is dynamic, chosen by P: 34.4 KB at P = 64 (four workgroups share a CU's
//                160 KiB), 134.2 KB at P = 128.
//   k_mvn_diag   (obs_cov == NULL, any P) one wave per row, four rows per workgroup: lane l takes the
//                outputs l, l + 64, ... in order, then a fixed butterfly over the wave.  An output whose
//                target is NaN is left out: no term, both gradients 0.
//
// Every sum has a fixed order that depends on P alone, there are no floating-point atomics and a row
// reads nothing of another row: a row's bits do not depend on ns or on its neighbours.  info[s] is the
// 1-based index of the first output with a non-positive / non-finite pivot (dense) or total variance
// (diagonal) or with a non-finite residual, 0 if none.
#include "mfgp_device.h"
#include "mfgp_host.h"

namespace mfgp {

namespace {

constexpr double LOG2PI = 1.8378770664093453;
constexpr int MVN_ROWS_PER_WG = NTHREADS / 64;   // k_mvn_diag: one wave per row

__host__ __device__ constexpr int mvn_p8(int p) { return (p + 7) & ~7; }
// the dense kernel's LDS: the (P8 + 1)^2 image, P8 staged gradients, 8 words of scalars
static size_t mvn_dense_smem(int p) {
    const size_t p8 = (size_t)mvn_p8(p);
    return ((p8 + 1) * (p8 + 1) + p8 + 8) * sizeof(double);
}

// fixed-order sum over the 64 lanes of a wave (the same tree whatever the values)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// Cholesky of the leading n8 x n8 block (n8 a multiple of 8) of the LDS image A (stride S, lower
// triangle valid, upper never read), with the `extra` rows under it carried along as panel rows
// (row n8 + e becomes A_row L^{-T}; its own trailing elements take the rank-8 updates too).  The
// factor is left in the lower triangle.  Returns the first non-positive / non-finite pivot (1-based,
// 0: none), the same in every thread.  Ends with a barrier.
__device__ int dense_potrf(double* __restrict__ A, int n8, int S, int extra) {
    const int t = threadIdx.x;
    const int R = n8 + extra;
    int badloc = 0;
    for (int r0 = 0; r0 < n8; r0 += 8) {
        double l[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) l[i][j] = A[(r0 + i) * S + r0 + j];
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
        const int rows = R - r0 - 8;   // (<= 121 < NTHREADS)
        double x[8];
        if (t < rows) {
            const int r = r0 + 8 + t;
#pragma unroll
            for (int c = 0; c < 8; ++c) x[c] = A[r * S + r0 + c];
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
            for (int c = 0; c < 8; ++c) A[r * S + r0 + c] = x[c];
        }
        if (t == NTHREADS - 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) A[(r0 + i) * S + r0 + j] = l[i][j];
        }
        __syncthreads();
        for (int e = t; e < rows * rows; e += NTHREADS) {
            const int ii = e / rows, jj = e - ii * rows;
            if (jj > ii) continue;
            const int i = r0 + 8 + ii, j = r0 + 8 + jj;
            double acc = A[i * S + j];
#pragma unroll
            for (int m = 0; m < 8; ++m) acc -= A[i * S + r0 + m] * A[j * S + r0 + m];
            A[i * S + j] = acc;
        }
        __syncthreads();
    }
    return badloc;
}

// In-place inverse of the lower-triangular n8 x n8 factor in A, 8-column blocks from the last to the
// first: with the trailing block X22 already inverted, X11 = L11^{-1} (registers, every thread),
// W = X22 L21 (one thread per element, written over L21 behind a barrier), X21 = -W X11 (one thread
// per row).  Ends with a barrier.
__device__ void dense_trtri(double* __restrict__ A, int n8, int S) {
    const int t = threadIdx.x;
    for (int r0 = n8 - 8; r0 >= 0; r0 -= 8) {
        double l[8][8], x[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) l[i][j] = A[(r0 + i) * S + r0 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j][j] = 1.0 / l[j][j];
#pragma unroll
            for (int i = j + 1; i < 8; ++i) {
                double v = 0.0;
#pragma unroll
                for (int k = j; k < i; ++k) v += l[i][k] * x[k][j];
                x[i][j] = -v / l[i][i];
            }
        }
        const int m = n8 - r0 - 8;     // rows below the block (<= 120)
        double w[4];                   // m * 8 <= 960 elements over 256 threads
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = t + u * NTHREADS;
            w[u] = 0.0;
            if (e < m * 8) {
                const int i = r0 + 8 + (e >> 3), c = r0 + (e & 7);
                double acc = 0.0;
                for (int k = r0 + 8; k <= i; ++k) acc += A[i * S + k] * A[k * S + c];
                w[u] = acc;
            }
        }
        __syncthreads();   // every read of L21 and of the pivot block is done
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = t + u * NTHREADS;
            if (e < m * 8) A[(r0 + 8 + (e >> 3)) * S + r0 + (e & 7)] = w[u];
        }
        if (t == NTHREADS - 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) A[(r0 + i) * S + r0 + j] = x[i][j];
        }
        __syncthreads();
        if (t < m) {   // row r0 + 8 + t of W is read and overwritten by this thread alone
            double* __restrict__ row = A + (r0 + 8 + t) * S + r0;
            double wr[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) wr[c] = row[c];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                double v = 0.0;
#pragma unroll
                for (int cc = c; cc < 8; ++cc) v += wr[cc] * x[cc][c];
                row[c] = -v;
            }
        }
        __syncthreads();
    }
}

// (four waves per SIMD: the four workgroups a CU's LDS holds at P <= 64 need 128 VGPRs or fewer each)
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_mvn_dense(LogpdfArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int t = threadIdx.x;
    const long s = blockIdx.x;
    const int P = a.p, n8 = mvn_p8(P), S = n8 + 1;
    double* __restrict__ A = smem;
    double* __restrict__ stage = smem + (n8 + 1) * S;            // [n8]
    int* __restrict__ rbad = reinterpret_cast<int*>(stage + n8); // first non-finite residual
    if (t == 0) *rbad = 0x7fffffff;
    const double* __restrict__ vp = a.var + s * a.var_rs;
    const double* __restrict__ op = a.obs_var ? a.obs_var + s * a.ov_rs : nullptr;
    for (int e = t; e < n8 * n8; e += NTHREADS) {
        const int i = e / n8, j = e - i * n8;
        if (j > i) continue;
        double v;
        if (i < P) {
            v = a.obs_cov[(long)i * a.ldc + j];
            if (i == j) v += vp[(long)i * a.var_cs] + (op ? op[i] : 0.0);
        } else {
            v = i == j ? 1.0 : 0.0;   // beyond P: an identity block
        }
        A[i * S + j] = v;
    }
    __syncthreads();   // (rbad is initialised)
    for (int c = t; c <= n8; c += NTHREADS) {
        double r = 0.0;
        if (c < P) {
            r = a.Y[s * a.y_rs + c] - a.mean[s * a.ldm + c];
            if (!(fabs(r) < INFINITY)) atomicMin(rbad, c + 1);
        }
        A[n8 * S + c] = r;   // (c == n8: the corner that collects -z^T z)
    }
    __syncthreads();
    const int bad = dense_potrf(A, n8, S, 1);
    if (t < 64) {   // logp from the factor's diagonal and the corner, one wave, fixed order
        double v = 0.0;
        for (int c = t; c < P; c += 64) v += log(A[c * S + c]);
        const double logdet_half = wave_sum(v);
        if (t == 0) {
            const int rb = *rbad;
            int inf = bad;
            if (rb != 0x7fffffff && (inf == 0 || rb < inf)) inf = rb;
            a.info[s] = inf;
            a.logp[s] = 0.5 * A[n8 * S + n8] - logdet_half - 0.5 * (double)P * LOG2PI;
        }
    }
    if (!a.gmean && !a.gvar) return;   // (uniform over the workgroup)
    dense_trtri(A, n8, S);
    if (t < P) {
        double ac = 0.0, dc = 0.0;
        for (int i = t; i < P; ++i) {
            const double x = A[i * S + t];
            ac += x * A[n8 * S + i];
            dc += x * x;
        }
        const double gv = 0.5 * (ac * ac - dc);
        if (a.gmean) a.gmean[s * a.ldgm + t] = ac;
        if (a.gvar && !a.gv_sum) a.gvar[s * a.ldgv + t] = gv;
        stage[t] = gv;
    }
    if (a.gvar && a.gv_sum) {   // one variance per row: its derivative is the sum over the outputs
        __syncthreads();
        if (t < 64) {
            double v = 0.0;
            for (int c = t; c < P; c += 64) v += stage[c];
            v = wave_sum(v);
            if (t == 0) a.gvar[s] = v;
        }
    }
}

__global__ __launch_bounds__(NTHREADS) void k_mvn_diag(LogpdfArgs a) {
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * MVN_ROWS_PER_WG + (threadIdx.x >> 6);
    if (s >= a.ns) return;   // (uniform over the wave; the kernel has no barrier)
    const int P = a.p;
    const double* __restrict__ yp = a.Y + s * a.y_rs;
    const double* __restrict__ mp = a.mean + s * a.ldm;
    const double* __restrict__ vp = a.var + s * a.var_rs;
    const double* __restrict__ op = a.obs_var ? a.obs_var + s * a.ov_rs : nullptr;
    double acc = 0.0, gvs = 0.0;
    int bad = 0x7fffffff;
    for (int c = lane; c < P; c += 64) {
        const double y = yp[c];
        double gm = 0.0, gv = 0.0;
        if (y == y) {   // a NaN target is a missing output: no term, no gradient
            const double v = vp[(long)c * a.var_cs] + (op ? op[c] : 0.0);
            const double r = y - mp[c];
            if (bad == 0x7fffffff && !(v > 0.0 && v < INFINITY && fabs(r) < INFINITY)) bad = c + 1;
            const double iv = 1.0 / v;
            gm = r * iv;
            gv = 0.5 * (gm * gm - iv);
            acc += r * gm + log(v) + LOG2PI;
        }
        if (a.gmean) a.gmean[s * a.ldgm + c] = gm;
        if (a.gvar && !a.gv_sum) a.gvar[s * a.ldgv + c] = gv;
        gvs += gv;
    }
    acc = wave_sum(acc);
    bad = wave_min(bad);
    if (a.gvar && a.gv_sum) gvs = wave_sum(gvs);
    if (lane == 0) {
        a.logp[s] = 0.0 - 0.5 * acc;   // (a row with no target at all: +0)
        a.info[s] = bad == 0x7fffffff ? 0 : bad;
        if (a.gvar && a.gv_sum) a.gvar[s] = gvs;
    }
}

// ---------------------------------------------------------------- Fisher matrix (mfgp_mvn_fisher)
// F_s = J_s^T Sigma_s^{-1} J_s, Sigma_s as above, J_s [P x D] read from the Jacobian's device layout
// J[s][k][c] (row k of J_s^T, outputs fastest).
//   k_fisher_dense  (obs_cov given) one workgroup per row.  The LDS image is (P8 + D) rows of stride
//                   (P8 + D) | 1 doubles: the lower triangle of Sigma_s exactly as k_mvn_dense builds it, and the
//                   D rows of J_s^T under it, their last D columns zero.  dense_potrf carries those rows along:
//                   they become J^T L^{-T}, and their own trailing updates leave -J^T Sigma^{-1} J in the
//                   D x D corner, so the Fisher matrix costs no pass of its own.  The lower triangle of the
//                   corner is negated and mirrored: F is exactly symmetric.  The LDS size is chosen at launch
//                   (fisher_dense_smem): 44.4 KB at P = 64, D = 10; the image must fit the 160 KiB of a CU.
//   k_fisher_diag   (obs_cov == NULL, any P) one workgroup per row, outputs staged 64 at a time; a thread
//                   owns up to three (a, b <= a) pairs and adds J[c][a] J[c][b] / (var_c + ov_c) in output order.
// A row reads nothing of another row: its bits do not depend on ns or on its neighbours.  info[s] is the
// 1-based index of the first output with a non-positive / non-finite pivot (dense) or total variance
// (diagonal), 0 if none.
constexpr int FISHER_MAXD = 32;
constexpr int FISHER_PAIRS = (FISHER_MAXD * (FISHER_MAXD + 1) / 2 + NTHREADS - 1) / NTHREADS;

__global__ __launch_bounds__(NTHREADS) void k_fisher_dense(FisherArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int t = threadIdx.x;
    const long s = blockIdx.x;
    const int P = a.p, D = a.d, n8 = mvn_p8(P), R = n8 + D, S = R | 1;
    double* __restrict__ A = smem;
    const double* __restrict__ vp = a.var + s * a.var_rs;
    const double* __restrict__ op = a.obs_var ? a.obs_var + s * a.ov_rs : nullptr;
    for (int e = t; e < n8 * n8; e += NTHREADS) {
        const int i = e / n8, j = e - i * n8;
        if (j > i) continue;
        double v;
        if (i < P) {
            v = a.obs_cov[(long)i * a.ldc + j];
            if (i == j) v += vp[(long)i * a.var_cs] + (op ? op[i] : 0.0);
        } else {
            v = i == j ? 1.0 : 0.0;   // beyond P: an identity block
        }
        A[i * S + j] = v;
    }
    const double* __restrict__ Jp = a.J + s * D * a.ldj;
    for (int e = t; e < D * R; e += NTHREADS) {
        const int k = e / R, c = e - k * R;
        A[(n8 + k) * S + c] = c < P ? Jp[(long)k * a.ldj + c] : 0.0;   // (c >= n8: the corner that collects -F)
    }
    __syncthreads();
    const int bad = dense_potrf(A, n8, S, D);
    double* __restrict__ Fp = a.F + s * D * D;
    for (int e = t; e < D * D; e += NTHREADS) {
        const int i = e / D, j = e - i * D;
        const int lo = i > j ? i : j, hi = i > j ? j : i;
        Fp[e] = 0.0 - A[(n8 + lo) * S + n8 + hi];
    }
    if (t == 0) a.info[s] = bad;
}

__global__ __launch_bounds__(NTHREADS) void k_fisher_diag(FisherArgs a) {
    __shared__ double Js[FISHER_MAXD][65];
    __shared__ double wv[64];
    __shared__ int sbad;
    const int t = threadIdx.x;
    const long s = blockIdx.x;
    const int P = a.p, D = a.d, npair = D * (D + 1) / 2;
    const double* __restrict__ vp = a.var + s * a.var_rs;
    const double* __restrict__ op = a.obs_var ? a.obs_var + s * a.ov_rs : nullptr;
    const double* __restrict__ Jp = a.J + s * D * a.ldj;
    if (t == 0) sbad = 0x7fffffff;
    int pa[FISHER_PAIRS], pb[FISHER_PAIRS];
    double acc[FISHER_PAIRS];
#pragma unroll
    for (int u = 0; u < FISHER_PAIRS; ++u) {   // pair e -> (a, b <= a), row by row of the lower triangle
        int e = t + u * NTHREADS, i = 0;
        if (e >= npair) e = 0;
        while (e > i) { e -= i + 1; ++i; }
        pa[u] = i;
        pb[u] = e;
        acc[u] = 0.0;
    }
    for (int c0 = 0; c0 < P; c0 += 64) {
        __syncthreads();   // the previous block's readers (first block: sbad is initialised)
        for (int e = t; e < D * 64; e += NTHREADS) {
            const int k = e >> 6, c = c0 + (e & 63);
            Js[k][e & 63] = c < P ? Jp[(long)k * a.ldj + c] : 0.0;
        }
        if (t < 64) {
            const int c = c0 + t;
            double w = 0.0;
            if (c < P) {
                const double v = vp[(long)c * a.var_cs] + (op ? op[c] : 0.0);
                if (!(v > 0.0 && v < INFINITY)) atomicMin(&sbad, c + 1);
                w = 1.0 / v;
            }
            wv[t] = w;
        }
        __syncthreads();
        const int nc = P - c0 < 64 ? P - c0 : 64;
#pragma unroll
        for (int u = 0; u < FISHER_PAIRS; ++u) {
            if (t + u * NTHREADS >= npair) continue;
            double v = acc[u];
            for (int c = 0; c < nc; ++c) v += Js[pa[u]][c] * Js[pb[u]][c] * wv[c];
            acc[u] = v;
        }
    }
    double* __restrict__ Fp = a.F + s * D * D;
#pragma unroll
    for (int u = 0; u < FISHER_PAIRS; ++u) {
        if (t + u * NTHREADS >= npair) continue;
        Fp[pa[u] * D + pb[u]] = acc[u];
        Fp[pb[u] * D + pa[u]] = acc[u];
    }
    __syncthreads();
    if (t == 0) a.info[s] = sbad == 0x7fffffff ? 0 : sbad;
}

}  // namespace

void launch_mvn_logpdf(const LogpdfArgs& a, hipStream_t s) {
    if (a.ns <= 0) return;
    if (a.obs_cov) {
        static bool attr = false;
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mvn_dense),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)mvn_dense_smem(MVN_DENSE_MAXP));
            attr = true;
        }
        hipLaunchKernelGGL(k_mvn_dense, dim3((unsigned)a.ns), dim3(NTHREADS), mvn_dense_smem(a.p), s, a);
    } else {
        hipLaunchKernelGGL(k_mvn_diag, dim3((unsigned)ceil_div(a.ns, MVN_ROWS_PER_WG)), dim3(NTHREADS), 0, s, a);
    }
}

// the shared argument test of mfgp_mvn_logpdf and the fused posterior entries
bool mvn_logpdf_geometry_ok(int ns, int p, bool dense, int ldc, long y_rs, long ov_rs) {
    if (ns < 0 || p < 1 || y_rs < 0 || ov_rs < 0) return false;
    if (dense && (p > MVN_DENSE_MAXP || ldc < p)) return false;
    return (y_rs == 0 || y_rs >= p) && (ov_rs == 0 || ov_rs >= p);
}

// the dense Fisher kernel's LDS: the (P8 + D) x ((P8 + D) | 1) image
size_t fisher_dense_smem(int p, int d) {
    const size_t r = (size_t)mvn_p8(p) + (size_t)d;
    return r * (r | 1) * sizeof(double);
}

void launch_mvn_fisher(const FisherArgs& a, hipStream_t s) {
    if (a.ns <= 0) return;
    if (a.obs_cov) {
        static bool attr = false;
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fisher_dense),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)FISHER_LDS_BYTES);
            attr = true;
        }
        hipLaunchKernelGGL(k_fisher_dense, dim3((unsigned)a.ns), dim3(NTHREADS), fisher_dense_smem(a.p, a.d), s, a);
    } else {
        hipLaunchKernelGGL(k_fisher_diag, dim3((unsigned)a.ns), dim3(NTHREADS), 0, s, a);
    }
}

// the argument test of mfgp_mvn_fisher; dense: P <= 128 and the image within the LDS of a CU
bool mvn_fisher_geometry_ok(int ns, int p, int d, bool dense, int ldc, long ov_rs) {
    if (ns < 0 || p < 1 || d < 1 || d > FISHER_MAXD || ov_rs < 0) return false;
    if (dense && (p > MVN_DENSE_MAXP || ldc < p || fisher_dense_smem(p, d) > FISHER_LDS_BYTES)) return false;
    return ov_rs == 0 || ov_rs >= p;
}

}  // namespace mfgp

using namespace mfgp;

extern "C" {

int mfgp_mvn_logpdf_workspace_size(mfgp_handle_t h, int ns, int p, size_t* bytes) {
    CHECK_H(h);
    if (ns < 0 || p < 1 || !bytes) return MFGP_ERR_ARG;
    *bytes = MVN_LOGPDF_WS_BYTES;
    return MFGP_OK;
}

int mfgp_mvn_logpdf(mfgp_handle_t h, int ns, int p, const double* mean, int ldm, const double* Y, long y_rs,
                    const double* var, long var_rs, long var_cs, const double* obs_var, long ov_rs,
                    const double* obs_cov, int ldc, void* ws, size_t ws_bytes, double* logp, double* gmean, int ldgm,
                    double* gvar, int ldgv, int* info) {
    CHECK_H(h);
    if (!mvn_logpdf_geometry_ok(ns, p, obs_cov != nullptr, ldc, y_rs, ov_rs) || ldm < p || var_rs < 0 ||
        (var_cs != 0 && var_cs != 1))
        return MFGP_ERR_ARG;
    const bool gv_sum = gvar && var_cs == 0 && ldgv == 1;
    if ((gmean && ldgm < p) || (gvar && ldgv < p && !gv_sum)) return MFGP_ERR_ARG;
    if (ns == 0) return MFGP_OK;
    if (!mean || !Y || !var || !ws || !logp || !info) return MFGP_ERR_ARG;
    if (ws_bytes < MVN_LOGPDF_WS_BYTES) return MFGP_ERR_WORKSPACE;
    LogpdfArgs a{};
    a.ns = ns; a.p = p;
    a.mean = mean; a.ldm = ldm;
    a.Y = Y; a.y_rs = y_rs;
    a.var = var; a.var_rs = var_rs; a.var_cs = var_cs;
    a.obs_var = obs_var; a.ov_rs = ov_rs;
    a.obs_cov = obs_cov; a.ldc = ldc;
    a.logp = logp; a.gmean = gmean; a.ldgm = ldgm; a.gvar = gvar; a.ldgv = ldgv; a.gv_sum = gv_sum ? 1 : 0;
    a.info = info;
    launch_mvn_logpdf(a, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

int mfgp_mvn_fisher_workspace_size(mfgp_handle_t h, int ns, int p, int d, size_t* bytes) {
    CHECK_H(h);
    CHECK_D(d);
    if (ns < 0 || p < 1 || !bytes) return MFGP_ERR_ARG;
    *bytes = MVN_FISHER_WS_BYTES;
    return MFGP_OK;
}

int mfgp_mvn_fisher(mfgp_handle_t h, int ns, int p, int d, const double* J, int ldj, const double* var, long var_rs,
                    long var_cs, const double* obs_var, long ov_rs, const double* obs_cov, int ldc, void* ws,
                    size_t ws_bytes, double* F, int* info) {
    CHECK_H(h);
    CHECK_D(d);
    if (!mvn_fisher_geometry_ok(ns, p, d, obs_cov != nullptr, ldc, ov_rs) || ldj < p || var_rs < 0 ||
        (var_cs != 0 && var_cs != 1))
        return MFGP_ERR_ARG;
    if (ns == 0) return MFGP_OK;
    if (!J || !var || !ws || !F || !info) return MFGP_ERR_ARG;
    if (ws_bytes < MVN_FISHER_WS_BYTES) return MFGP_ERR_WORKSPACE;
    FisherArgs a{};
    a.ns = ns; a.p = p; a.d = d;
    a.J = J; a.ldj = ldj;
    a.var = var; a.var_rs = var_rs; a.var_cs = var_cs;
    a.obs_var = obs_var; a.ov_rs = ov_rs;
    a.obs_cov = obs_cov; a.ldc = ldc;
    a.F = F; a.info = info;
    launch_mvn_fisher(a, h->stream);
    return last() == hipSuccess ? MFGP_OK : MFGP_ERR_LAUNCH;
}

}  // extern "C"
