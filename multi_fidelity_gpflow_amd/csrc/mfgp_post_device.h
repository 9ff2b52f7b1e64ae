// Device helpers shared by the kernels that work on the cached posterior's A = L^{-1} K(X, X*)
// (mfgp_posterior.hip, mfgp_design.hip, mfgp_append.hip): the LDS staging constants, the K(X, X*) tile generator of the
// linear multi-fidelity kernel, the kernel entry of one pair of rows, K_diag of one row and the fixed-order
// sums of cross-workgroup partials.
#pragma once
#include "mfgp_device.h"

namespace mfgp {

constexpr int PMAXD = 32;
constexpr int PXS = PMAXD + 1;   // LDS row stride of staged inputs (odd: distinct banks over rows)
constexpr int PTHETA = 192;      // theta entries staged in LDS (graph kernel, 4 sources, D = 32: 186)

// The NB x NB tile K(x1 rows, xs rows) of the linear multi-fidelity kernel into Ks.  A thread owns
// column c = t % NB of rows t / NB + (NTHREADS / NB) q and works on four of its entries at a time:
// the four distance sums share the column's reads and run as independent chains, the exponentials
// go through exp4.  A product workgroup is often alone on its CU (one wave per SIMD, nothing to
// hide a latency behind), where the entry-at-a-time form left every LDS read and every step of the
// exp polynomial exposed.  Exact == 0 / == 1 fidelity masks (anything else: a zero row / column,
// linear.py:67-70); r^2 in direct-difference form, il = [1 / lL | 1 / lD].
template <int NB>
__device__ __forceinline__ void post_mf_tile(double* Ks, const double* x1, const double* f1, const double* xs,
                                             const double* fs, int D, const double* il, const double* th) {
    constexpr int S = TileCfg<NB>::S;
    constexpr int RSTEP = NTHREADS / NB;           // rows between a thread's consecutive entries
    constexpr int NE = NB * NB / NTHREADS;         // entries per thread (a multiple of 4)
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
            double v = (La && Lb) ? kL : (!(Ha && Hb) ? kL * rho : kL * (rho * rho) + vD * kd[j]);
            if (!(La || Ha) || !(Lb || Hb)) v = 0.0;
            Ks[(r0 + j * RSTEP) * S + c] = v;
        }
    }
}

// K_diag of one X* row (k_kdiag's expressions)
__device__ __forceinline__ double post_kdiag(double f, const double* theta, int D, int nlf) {
    if (nlf) {
        const GraphTheta th{theta, D, nlf};
        const int s = graph_source(f, nlf);
        double v = 0.0;
        if (s >= 0 && s < nlf) v = th.v(s);
        else if (s == nlf) {
            for (int k = 0; k < nlf; ++k) v += th.v(k) * (th.rho(k) * th.rho(k));
            v += th.v(nlf);
        }
        return v;
    }
    const MFTheta th{theta, D};
    const double rho = th.rho();
    return (f == 0.0) ? th.vL() : ((f == 1.0) ? th.vL() * (rho * rho) + th.vD() : 0.0);
}

// K(xa, xb) of one pair of stacked rows (fidelity in column D): post_mf_tile's expressions for the
// linear multi-fidelity kernel, the graph entry function (row source first) for nlf > 0
__device__ __forceinline__ double design_entry(const double* xa, const double* xb, int D, int nlf,
                                               const double* theta) {
    if (nlf) {
        const GraphTheta th{theta, D, nlf};
        return graph_entry(xa, xb, graph_source(xa[D], nlf), graph_source(xb[D], nlf), th);
    }
    const double fa = xa[D], fb = xb[D];
    const bool La = (fa == 0.0), Ha = (fa == 1.0), Lb = (fb == 0.0), Hb = (fb == 1.0);
    if (!(La || Ha) || !(Lb || Hb)) return 0.0;
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < D; ++d) {
        const double df = xa[d] - xb[d];
        const double qL = df * rcp_nr(theta[1 + d]), qD = df * rcp_nr(theta[2 + D + d]);
        e[0] += qL * qL;
        e[1] += qD * qD;
    }
    e[0] *= -0.5;
    e[1] *= -0.5;
    exp4(e);
    const double vL = theta[0], vD = theta[1 + D], rho = theta[2 + 2 * D];
    const double kL = vL * e[0];
    return (La && Lb) ? kL : (!(Ha && Hb) ? kL * rho : kL * (rho * rho) + vD * e[1]);
}

// sum over k < n of base[k * stride] in k order; the sc1 loads are issued eight at a time (one at a
// time, a thread's sum cost a memory round trip per term; W = 32 for k_post_grad's long task lists)
template <int W = 8>
__device__ __forceinline__ double post_sum_coherent(const double* base, long stride, int n) {
    double s = 0.0;
    for (int k0 = 0; k0 < n; k0 += W) {
        double v[W];
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = k0 + j < n ? ld_coherent(base + (long)(k0 + j) * stride) : 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) s += v[j];
    }
    return s;
}

// the same for data of an earlier launch (plain loads)
__device__ __forceinline__ double post_sum(const double* base, long stride, int n) {
    double s = 0.0;
    for (int k0 = 0; k0 < n; k0 += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = k0 + j < n ? base[(long)(k0 + j) * stride] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    return s;
}

}  // namespace mfgp
