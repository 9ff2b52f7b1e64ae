// The step reduction's device functions, shared by k_reduce_items (mfgp_kernels.hip) and the head
// phase of k_chol_flow (mfgp_flow.hip): the per-thread part of an item sum and the finalize
// (LML, gradient output, Keras-Adam step).  Both kernels compile THIS text, so the head phase
// reproduces k_reduce_items bit for bit: the same operations in the same order.
//
// NT is the size of the group that runs a function: NTHREADS (k_reduce_items' workgroup, tid =
// threadIdx.x) or 64 (one wave of k_chol_flow, tid = lane; G <= 64 there).
#pragma once
#include "../../include/mfgp.h"
#include "mfgp_device.h"
#include "mfgp_internal.h"

namespace mfgp {

// A poll that exceeds this many 100 MHz ticks marks the evaluation failed: NaN LML, no Adam step.
constexpr long long REDUCE_TIMEOUT_TICKS = 5000000;   // 50 ms

// Adam inputs of theta entry tid, loaded before the items are polled (sentinel protocol)
struct FinPre {
    double u, m, v;
    int tr;
    // head phase: the step's theta-gradient-independent factors, computed under the poll too
    int ready = 0;
    double alpha = 0.0, den = 0.0;
};
// Keras-Adam's step size at step s, and the SoftplusGrad denominator of entry u
__device__ __forceinline__ double adam_alpha(const FinArgs& a, int s) {
    const double t = (double)(s + 1);
    return a.lr * sqrt(1.0 - pow(a.b2, t)) / (1.0 - pow(a.b1, t));
}
__device__ __forceinline__ double adam_den(double uq) { return exp(-uq) + 1.0; }

template <int NT>
__device__ __forceinline__ void fin_group_sync() {
    if constexpr (NT == NTHREADS) {
        __syncthreads();
    } else {   // one wave: its DS operations complete in issue order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// Thread tid's (of 256) share of item `it` of [sum Z^2, sum log L_ii, grad_0 .. grad_{G-1}]
// (partials stored [item][task]); deterministic order.
__device__ __forceinline__ double reduce_item_thread(const FinArgs& a, int it, int tid) {
    double s = 0.0;
    if (it == 0) {
        for (int e = tid; e < a.nz; e += NTHREADS) s += a.zpart[e];
    } else if (it == 1) {   // 8 loads in flight per thread before the logs
        for (int e0 = tid; e0 < a.n; e0 += 8 * NTHREADS) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = (e0 + u * NTHREADS < a.n) ? a.ldiag[e0 + u * NTHREADS] : 1.0;
#pragma unroll
            for (int u = 0; u < 8; ++u)   // a batch past the end is 1.0 in every lane: s + log(1.0) is s
                if (__ballot(v[u] != 1.0) != 0) s += log(v[u]);
        }
    } else {
        const double* src = a.gpart + (long)(it - 2) * a.ng;
        double s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int e = tid;
        for (; e + 3 * NTHREADS < a.ng; e += 4 * NTHREADS) {
            s += src[e];
            s1 += src[e + NTHREADS];
            s2 += src[e + 2 * NTHREADS];
            s3 += src[e + 3 * NTHREADS];
        }
        for (; e < a.ng; e += NTHREADS) s += src[e];
        s = (s + s1) + (s2 + s3);
    }
    return s;
}

// th_lds (head phase only): the refreshed theta entries are also left there for the launch's own Gram
template <int NT>
__device__ __forceinline__ void adam_body(const FinArgs& a, int G, int s, const double* gsh, const int* tsh,
                                          const FinPre* pre, int tid, double* th_lds = nullptr) {
    const bool ready = pre && pre->ready;
    const double alpha = ready ? pre->alpha : adam_alpha(a, s);
    for (int q = tid; q < G; q += NT) {
        if (pre ? pre->tr : a.trainable[q]) {
            const double uq = pre ? pre->u : a.u[q];
            double gc = gsh[q];
            if (tsh) {   // a variable shared by several theta entries gets the summed gradient
                gc = 0.0;
                for (int r = 0; r < G; ++r)
                    if (tsh[r] == tsh[q]) gc += gsh[r];
            }
            const double g = (-gc) / (ready ? pre->den : adam_den(uq));   // loss = -lml; TF SoftplusGrad form
            double mq = pre ? pre->m : a.m[q], vq = pre ? pre->v : a.v[q];
            mq += (g - mq) * (1.0 - a.b1);
            vq += (g * g - vq) * (1.0 - a.b2);
            const double un = uq - (mq * alpha) / (sqrt(vq) + a.eps);
            a.m[q] = mq;
            a.v[q] = vq;
            a.u[q] = un;
            const double thq = tf_softplus(un) + (q == a.noise_index ? 1e-6 : 0.0);
            a.theta[q] = thq;
            if (th_lds) th_lds[q] = thq;
        }
    }
}

// Stage 2: LML, gradient output and the optional Keras-Adam step.
// gsh = [sum Z^2, sum log L_ii, grad_0 .. grad_{G-1}] in LDS (read after a barrier)
template <int NT>
__device__ __forceinline__ void finalize_from(const FinArgs& a, int G, const double* gsh, const int* tsh, int info0,
                                              int s, const FinPre* pre, int tid, double* th_lds = nullptr) {
    const double LOG2PI = 1.8378770664093453;
    // -0.5 gsh[0] - P gsh[1] - 0.5 n P LOG2PI, with the fused multiply-adds written out: left to the
    // compiler, the contraction of this line depends on the code around it, and it came out
    // differently in k_chol_flow than in k_reduce_items once (1 ulp in the loss history).  This is
    // the form k_reduce_items has always had.
    double lml;
    {
#pragma clang fp contract(off)
        const double c = ((double)a.n * -0.5) * (double)a.P;
        lml = __builtin_fma(LOG2PI, c, __builtin_fma(gsh[0], -0.5, -((double)a.P * gsh[1])));
    }
    if (info0 != 0) lml = NAN;
    if (a.adam && info0 == 0) adam_body<NT>(a, G, s, gsh + 2, a.tie ? tsh : nullptr, pre, tid, th_lds);
    if (tid == 0) a.out[0] = lml;
    if (a.want_grad)
        for (int q = tid; q < G; q += NT) a.out[1 + q] = gsh[2 + q];
    if (!a.adam) return;
    if (tid == 0) a.loss_hist[s] = -lml;
    fin_group_sync<NT>();   // every wave has read *a.step
    if (tid == 0 && info0 == 0) *a.step = s + 1;
}

}  // namespace mfgp
