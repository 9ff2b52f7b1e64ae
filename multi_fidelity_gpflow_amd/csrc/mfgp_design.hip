// Simulation design from the cached GPR posterior (GPRPosterior.variance_reduction / select).
//
// At the snapshot's hyper-parameters, observing y at a candidate x_c lowers the posterior variance of
// f at a reference x_r by cov(f(x_r), f(x_c))^2 / (var f(x_c) + s2).  With A = L^{-1} K(X, [Xref ; Xcand])
// kept by the cached predict's forward (launch_post) and its marginal variances v:
//   C(r, c)  = K(x_r, x_c) - A_r^T A_c - E_r^T E_c        (the [ref, cand] block of the full covariance)
//   v'(c)    = v(c) - colsum(E_c^2)
//   score[c] = sum_r w_r C(r, c)^2 / (v'(c) + s2)
// E holds one row per candidate already picked in the batch: conditioning on a pick c* is one more
// row under A, e(x) = C'(x, c*) / sqrt(v'(c*) + s2) over all stacked columns x.
//
//   k_design_score  one task = one candidate column tile x a run of reference row tiles (128 rows).
//                   Per step the A (then E) rows of the run's reference tiles and of the candidate tile
//                   are staged in LDS and A_i^T A_j is accumulated on v_mfma_f64_16x16x4, one
//                   accumulator per reference tile: the candidate tile is read once per run.  Then, per
//                   reference tile, K(Xref_i, Xcand_j) is generated in LDS (post_mf_tile / graph_entry,
//                   as k_post_a), the product is subtracted in place, and the squared entries are
//                   weighted and summed down the rows in row order.  The Nr x Nc block never exists in
//                   HBM.  The last workgroup to arrive at a column tile's counter sums the runs'
//                   partials in run order, divides and writes score.
//   k_design_row    one workgroup = 256 stacked columns x 128 rows of A: partial A_x^T A_c* for the picked
//                   candidate (its index read from a device int); the last workgroup of a column block
//                   sums the partials in chunk order, adds K and E's rows and writes row k of E.
//
// Every sum has a fixed order and there are no floating-point atomics: two calls with the same inputs
// give the same bits.  Cross-workgroup partials go through sc1 stores / loads, the producer drains its
// stores before the arrival atomic (k_post_out's pattern); the counters are zeroed by the caller.
// Rows and columns beyond nref / ncand read as zero and carry weight zero; a row whose fidelity is no
// source has an exactly zero kernel row, hence an exactly zero column of A, of C and of E.
#include "mfgp_device.h"
#include "mfgp_internal.h"
#include "mfgp_post_device.h"

namespace mfgp {

// design_run + 1 tiles (the run's reference tiles, the candidate tile), the staged inputs of one
// reference tile and of the candidate tile, flags / weights / the `last` word, 1 / l, theta.
// NB = 64: 3 tiles + inputs = 136 KB of the CU's 160.
template <int NB>
constexpr size_t design_smem() {
    return sizeof(double) *
           ((design_run(NB) + 1) * (size_t)TileCfg<NB>::ELEMS + 2 * NB * PXS + 4 * NB + 2 * PMAXD + PTHETA);
}
static_assert(design_smem<64>() <= 160 * 1024, "k_design_score<64> fits one CU's LDS");

template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_design_score(DesignArgs a) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int EL = TileCfg<NB>::ELEMS;
    constexpr int R = design_run(NB);
    constexpr int PER = NB * NB / NTHREADS;
    constexpr int NBLK = TileCfg<NB>::NBLK;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* As = smem;               // R tiles: rows of A (E) x the run's reference columns
    double* Bs = As + R * EL;        // rows of A (E) x the candidate columns; epilogue: K_ij, then C_ij
    double* xr = Bs + EL;            // NB x PXS: the reference rows of one tile (epilogue)
    double* xc = xr + NB * PXS;      // NB x PXS: the candidate rows of the column tile
    double* fr = xc + NB * PXS;      // fidelity flags (-1: padding)
    double* fc = fr + NB;
    double* wr = fc + NB;            // weights of the reference tile (0: padding)
    int* last = reinterpret_cast<int*>(wr + NB);   // (NB doubles kept for it)
    double* il = wr + 2 * NB;        // [1 / lL | 1 / lD]
    double* ths = il + 2 * PMAXD;    // theta
    const int t = threadIdx.x;
    const int j = blockIdx.x % a.Tc, run = blockIdx.x / a.Tc;
    const int i0 = run * R;
    const int nr = a.Tr - i0 < R ? a.Tr - i0 : R;   // reference tiles of this run (>= 1)
    const int D = a.D, nall = a.nref + a.ncand;
    const int G = kernel_theta_size(a.nlf, D);
    for (int e = t; e < G; e += NTHREADS) ths[e] = a.theta[e];
    if (!a.nlf && t < D) {
        il[t] = rcp_nr(a.theta[1 + t]);
        il[PMAXD + t] = rcp_nr(a.theta[2 + D + t]);
    }
    for (int e = t; e < NB * D; e += NTHREADS) {
        const int r = e / D, d = e % D, c = j * NB + r;
        xc[r * PXS + d] = c < a.ncand ? a.Xall[(long)(a.nref + c) * a.ldx + d] : 0.0;
    }
    if (t < NB) {
        const int c = j * NB + t;
        fc[t] = c < a.ncand ? a.Xall[(long)(a.nref + c) * a.ldx + D] : -1.0;
    }
    Acc<NB> acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc_zero(acc[r]);
    // Steps 0..T-1: the row tiles of A; one more for the k rows of E (zero padded to a tile).  One
    // memory round trip a step, hidden behind the previous step's products (k_post_a's scheme).
    const int nsteps = a.T + (a.k > 0 ? 1 : 0);
    double ra[R][PER], rb[PER];
    auto fetch = [&](int s) {
        const bool ex = s >= a.T;
        const double* src = ex ? a.E : a.Am + (long)s * NB * a.ldam;
        const long ld = ex ? a.ldE : a.ldam;
        const int rows = ex ? a.k : NB;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = t + q * NTHREADS, row = e / NB, col = e % NB;
            const bool in = row < rows;
            const int gc = a.nref + j * NB + col;
            rb[q] = (in && gc < nall) ? src[(long)row * ld + gc] : 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int gr = (i0 + r) * NB + col;
                ra[r][q] = (in && r < nr && gr < a.nref) ? src[(long)row * ld + gr] : 0.0;
            }
        }
    };
    fetch(0);
    for (int s = 0; s < nsteps; ++s) {
        __syncthreads();   // the previous step's readers of As / Bs are done
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = t + q * NTHREADS, o = (e / NB) * S + e % NB;
            Bs[o] = rb[q];
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r < nr) As[r * EL + o] = ra[r][q];
        }
        if (s + 1 < nsteps) fetch(s + 1);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < nr) tile_mma<NB, true, false>(acc[r], As + r * EL, Bs, 1.0);
    }
    // ---- per reference tile: C_ij = K(Xref_i, Xcand_j) - product, then sum_r w_r C^2 down the rows
    const GraphTheta gth{ths, D, a.nlf};
    double colsum = 0.0;   // thread c < NB: column c over the run's rows, in row order
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r >= nr) continue;
        const int i = i0 + r;
        __syncthreads();   // the products' / the previous tile's readers of Bs, xr, fr, wr
        for (int e = t; e < NB * D; e += NTHREADS) {
            const int row = e / D, d = e % D, g = i * NB + row;
            xr[row * PXS + d] = g < a.nref ? a.Xall[(long)g * a.ldx + d] : 0.0;
        }
        if (t < NB) {
            const int g = i * NB + t;
            fr[t] = g < a.nref ? a.Xall[(long)g * a.ldx + D] : -1.0;
            wr[t] = g < a.nref ? (a.w ? a.w[g] : 1.0) : 0.0;
        }
        __syncthreads();
        if (a.nlf) {
            for (int e = t; e < NB * NB; e += NTHREADS) {
                const int row = e / NB, c = e % NB;
                Bs[row * S + c] = graph_entry(xr + row * PXS, xc + c * PXS, graph_source(fr[row], a.nlf),
                                              graph_source(fc[c], a.nlf), gth);
            }
        } else {
            post_mf_tile<NB>(Bs, xr, fr, xc, fc, D, il, ths);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NBLK; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int o = acc_row<NB>(q, u) * S + acc_col<NB>(q);
                Bs[o] = Bs[o] - acc[r].v[q][u];
            }
        __syncthreads();
        if (t < NB) {
            for (int row = 0; row < NB; ++row) {
                const double v = Bs[row * S + t];
                colsum += wr[row] * (v * v);
            }
        }
    }
    const long ncpad = (long)a.Tc * NB;
    if (t < NB) st_coherent(a.dpart + (long)run * ncpad + j * NB + t, colsum);
    drain_stores();
    __syncthreads();
    if (t == 0) *last = arrive(a.dcnt + j) == a.nrun - 1;
    __syncthreads();
    if (!*last) return;
    // ---- the column tile's scores, by its last workgroup: the runs' partials in run order
    const int c = j * NB + t;
    if (t < NB && c < a.ncand) {
        const double sum = post_sum_coherent(a.dpart + j * NB + t, ncpad, a.nrun);
        double vp = a.var[a.nref + c];
        for (int q = 0; q < a.k; ++q) {
            const double e = a.E[(long)q * a.ldE + a.nref + c];
            vp -= e * e;
        }
        a.score[c] = sum / (vp + a.noise[0]);
    }
}

__global__ __launch_bounds__(NTHREADS) void k_design_row(DesignArgs a) {
    __shared__ double ac[DESIGN_RROWS];   // the picked candidate's column of A, this chunk's rows
    __shared__ int last;
    const int t = threadIdx.x;
    const int cb = blockIdx.x % a.ncb, rc = blockIdx.x / a.ncb;
    const int nall = a.nref + a.ncand, x = cb * NTHREADS + t;
    const int pk = a.pick[0];
    if (pk < 0 || pk >= a.ncand) {   // no such candidate: a zero row (conditions on nothing)
        if (rc == 0 && x < nall) a.Erow[x] = 0.0;
        return;
    }
    const int xc = a.nref + pk;
    const int r0 = rc * DESIGN_RROWS;
    const int nrow = a.npad - r0 < DESIGN_RROWS ? a.npad - r0 : DESIGN_RROWS;   // a multiple of 32
    if (t < DESIGN_RROWS) ac[t] = t < nrow ? a.Am[(long)(r0 + t) * a.ldam + xc] : 0.0;
    __syncthreads();
    double s = 0.0;
    if (x < nall) {
        const double* col = a.Am + (long)r0 * a.ldam + x;
        for (int r = 0; r < nrow; r += 8) {   // eight loads in flight, summed in row order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = col[(long)(r + u) * a.ldam];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u] * ac[r + u];
        }
    }
    const long stride = (long)a.ncb * NTHREADS;
    st_coherent(a.rpart + rc * stride + x, s);
    drain_stores();
    __syncthreads();
    if (t == 0) last = arrive(a.rcnt + cb) == a.nrch - 1;
    __syncthreads();
    if (!last || x >= nall) return;
    // ---- row k of E over this block's columns, by its last workgroup: the chunks' partials in chunk order
    double p = post_sum_coherent(a.rpart + x, stride, a.nrch);
    double vp = a.var[xc];
    for (int q = 0; q < a.k; ++q) {
        const double ec = a.E[(long)q * a.ldE + xc];
        p += a.E[(long)q * a.ldE + x] * ec;
        vp -= ec * ec;
    }
    const double kx = design_entry(a.Xall + (long)x * a.ldx, a.Xall + (long)xc * a.ldx, a.D, a.nlf, a.theta);
    a.Erow[x] = (kx - p) / sqrt(vp + a.noise[0]);
}

template <int NB>
void launch_design_score(const DesignArgs& a, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_design_score<NB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)design_smem<NB>());
        attr = true;
    }
    hipLaunchKernelGGL(k_design_score<NB>, dim3(a.Tc * a.nrun), dim3(NTHREADS), design_smem<NB>(), s, a);
}

template void launch_design_score<32>(const DesignArgs&, hipStream_t);
template void launch_design_score<64>(const DesignArgs&, hipStream_t);

void launch_design_row(const DesignArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_design_row, dim3(a.ncb * a.nrch), dim3(NTHREADS), 0, s, a);
}

}  // namespace mfgp
