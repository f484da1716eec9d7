// Server step on the device: rule() (main.py:23-25) + Central.update_model (agents.py:9-21).
//
//   rule(weight_ups) = torch.stack(entries).mean(0) per parameter tensor, entries = the aliased
//   S_t of every fast worker (main.py:172) and the popped stale FIFO entries (main.py:161-165) in
//   append order; update_model = torch.optim.Adam (main.py:106).
//
// Arithmetic is bit-exact with torch 2.10 CPU: the sum over the stacked dim follows ATen's cascade
// (cascade.h: a host-built program per step, interpreted per element; multi_row_sum on whole
// 32-element column blocks of each tensor, row_sum on its last numel % 32 elements); mean =
// sum / (float)k; Adam m = fma(1-b1, g-m, m), v = fma((1-b2)*g, g, v*b2),
// den = sqrt(v)/sqrt(bc2) + eps, p += (-lr/bc1 * m) / den (correctly rounded sqrt; torch CPU's
// sqrt is not).  Compiled with -ffp-contract=off: the only fmas are explicit.
// Central(model, optim) takes other optimizers too: the kernels are instantiated per update rule
// (OptKind, slabstep.h: Adam, Adam with weight decay / AdamW, SGD with and without momentum,
// Adagrad, Yogi; see opt_update), each streaming only the state arrays its rule owns.
// Agg(rule) takes other rules too: every rule-carrying kernel also has a weighted form (W), the
// staleness-weighted rule sum_j w_j * entry_j / W with w = 1 for the S_t entries (a stale value is
// multiplied by its array's fp32 weight where it is loaded, the same cascade sums the products,
// one IEEE division follows); bit-exact with torch.stack([x * w ...]).sum(0) / W.
// On top of the weighted form every rule-carrying kernel has a delay-compensated form (C): a stale
// value with a snapshot theta_src is first corrected to x + ((x*x)*lam) * (p - theta_src) with the
// p the kernel holds (compensate()), and a launch that writes S_out can write that pre-update p to
// theta_out, the snapshot of the entry being pushed.
// Global-norm clipping (torch.nn.utils.clip_grad_norm_ between `.grad = ...` and optim.step())
// runs as three launches: the stream in a fifth kind, OK_GOUT, stores g = rule() to G and one fp64
// sum of squares per block; k_clip_finish adds those in index order and writes the correctly
// rounded norm and torch's coefficient; k_clip_apply runs the update on g * coef.
//
// Two kernels:
//   k_agg_stream  S_t already in a buffer (after the all-reduce at world > 1, or the facade):
//                 one float4 group per thread, 7 + distinct-array streams, HBM-bound;
//   k_slab_step   world = 1: the epoch's weight-gradient slabs are reduced to S_t in the same
//                 launch (slabstep.h), S_t never round-trips through HBM.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "attack.h"
#include "attack_opt.h"
#include "bulyan.h"
#include "cclip.h"
#include "common.h"
#include "flsim.h"
#include "geomed.h"
#include "krum.h"
#include "nnm.h"
#include "probe.h"
#include "robust.h"
#include "slabstep.h"

#ifndef FLSIM_SEQ_EARLY_EXIT
#define FLSIM_SEQ_EARLY_EXIT 1
#endif

namespace flsim {

constexpr int NYR = 8;          // entry arrays staged per thread (LDS); the rest load on demand
constexpr int MAX_TAILS = 8;    // tensor tails per streaming launch (host splits longer lists)
constexpr int AGG_GMAX = 2;     // float4 groups per thread of the register-array stream
constexpr int MAX_EDGE = 4 * AGG_GMAX * (2 * MAX_TAILS + 2);   // 256-element edge pieces per launch

// ---- element arithmetic -----------------------------------------------------------------------
// Correctly rounded fp32 sqrt.  v_sqrt_f32 is within 1 ulp; the exact residuals x - s'*s of the
// two neighbours s' = s -/+ 1 ulp (single-rounding fma: its sign is exact) pick the correctly
// rounded root.  Tiny inputs are scaled by 2^32 (root by 2^-16) so the residuals stay normal.
__device__ __forceinline__ float sqrt_rn(float x) {
    const bool tiny = x < 0x1p-96f;
    const float xs = tiny ? x * 0x1p+32f : x;
    float s = __builtin_amdgcn_sqrtf(xs);
    const int si = __float_as_int(s);
    const float s_dn = __int_as_float(si - 1);
    const float s_up = __int_as_float(si + 1);
    const float r_dn = __fmaf_rn(-s_dn, s, xs);
    const float r_up = __fmaf_rn(-s_up, s, xs);
    s = (r_dn <= 0.f) ? s_dn : s;
    s = (r_up > 0.f) ? s_up : s;
    s = tiny ? s * 0x1p-16f : s;
    // 0, +inf and NaN pass through unchanged (the correction above is only for finite x > 0)
    return (xs == 0.f || xs == __builtin_inff() || xs != xs) ? x : s;
}

// Correctly rounded a / b for a launch-constant divisor b with rb = RN(1/b) (Markstein: q0
// within 1 ulp, exact residual by fma, one correction).  Zero, tiny (near-subnormal) and
// non-finite quotients take the IEEE division so signs and subnormals stay exact.
__device__ __forceinline__ float div_const(float a, float b, float rb) {
    const float q0 = a * rb;
    const float r = __fmaf_rn(-q0, b, a);
    const float q = __fmaf_rn(r, rb, q0);
    const float aq = fabsf(q0);
    return (aq >= 0x1p-124f && aq <= 0x1p+124f) ? q : __fdiv_rn(a, b);
}

// torch.optim.Adam's update for the gradient g (_single_tensor_adam, no weight decay)
__device__ __forceinline__ void adam_update(const AdamConst& A, float g, float& p, float& m,
                                            float& v) {
    const float mi = __fmaf_rn(A.w1, g - m, m);
    float vi = v * A.b2;
    vi = __fmaf_rn(A.w2 * g, g, vi);
    const float den = div_const(sqrt_rn(vi), A.bc2s, A.rbc2s) + A.eps;
    p = p + __fdiv_rn(A.neg_ss * mi, den);
    m = mi;
    v = vi;
}

// rule()'s division.  Unweighted: the divisor is the entry count k, an integer, where div_const is
// correctly rounded.  Weighted (W): the divisor is any positive fp32 (a sum of discounts), where
// a * RN(1/b) can be 2 ulp off and one correction is then not enough: the IEEE division.
template <bool W>
__device__ __forceinline__ float rule_div(const AdamConst& A, float s) {
    if constexpr (W) return __fdiv_rn(s, A.fk);
    else return div_const(s, A.fk, A.rk);
}

// Delay compensation (DC-ASGD) of a stale value x pushed when the model was th and popped when it
// is p (the pre-update parameter): x + ((x*x) * lam) * (p - th), five fp32 roundings in the rule
// text's order (no contraction: -ffp-contract=off).  T = float or a float vector.
template <class T>
__host__ __device__ __forceinline__ T compensate(T x, T p, T th, float lam) {
    const T h = (x * x) * lam;
    const T d = p - th;
    return x + h * d;
}

template <bool W = false>
__device__ __forceinline__ void adam_elem(const AdamConst& A, float s, float& p, float& m,
                                          float& v) {
    const float g = rule_div<W>(A, s);                      // rule(): mean = sum / k
    adam_update(A, g, p, m, v);
}

// The other update rules, in torch 2.10's CPU op order (every add(x, alpha=a) there is one fma):
//   Adam, weight_decay w  g = fma(p, w, g), then Adam                  (_single_tensor_adam)
//   AdamW                 p = p * f32(1 - lr * w), then Adam on g
//   SGD                   g = fma(p, w, g) if w != 0;                  (_single_tensor_sgd)
//                         momentum mu != 0: buf = g at step 1, else fma(g, 1 - dampening, buf * mu);
//                                           g = nesterov ? fma(buf, mu, g) : buf;
//                         p = fma(g, -lr, p)
//   Adagrad               g = fma(p, w, g) if w != 0;  sum = fma(g, g, sum);       (_single_tensor_adagrad)
//                         p = p + (f32(-clr) * g) / (sqrt(sum) + eps)   (sum lives in m)
//   Yogi (FedYogi form)   g = fma(p, w, g) if w != 0;  m = fma(1 - b1, g - m, m);  g2 = g * g;
//                         v = fma(f32(-(1 - b2)) * sign(v - g2), g2, v);
//                         p = p + (f32(-lr) * m) / (sqrt(v) + eps)
//   (addcmul_(a, b, value=c) is fma(f32(c) * a, b, x); addcdiv_ is x + (f32(c) * a) / b)
// The flags are launch-uniform (scalar branches).  m is SGD's momentum buffer; a kind never
// touches an argument it does not own (the callers pass dummies).
// opt_update: the update for a gradient g (what follows rule()'s division; the clipped step's
// k_clip_apply enters here with g * coef); opt_elem: rule()'s division, then the update.
template <int OK>
__device__ __forceinline__ void opt_update(const AdamConst& A, const OptConst& X, float g,
                                           float& p, float& m, float& v) {
    if constexpr (OK == OK_ADAM) {
        adam_update(A, g, p, m, v);
    } else if constexpr (OK == OK_ADAMD) {
        if (X.flags & OF_DECOUPLED) p = p * X.wd;
        else g = __fmaf_rn(p, X.wd, g);
        adam_update(A, g, p, m, v);
    } else if constexpr (OK == OK_ADAGRAD) {
        if (X.flags & OF_WD) g = __fmaf_rn(p, X.wd, g);
        const float sum = __fmaf_rn(g, g, m);                   // addcmul_(g, g, value=1)
        p = p + __fdiv_rn(X.neg_lr * g, sqrt_rn(sum) + A.eps);  // addcdiv_(g, std, value=-clr)
        m = sum;
    } else if constexpr (OK == OK_YOGI) {
        if (X.flags & OF_WD) g = __fmaf_rn(p, X.wd, g);
        const float mi = __fmaf_rn(A.w1, g - m, m);             // lerp_(g, 1 - beta1)
        const float g2 = g * g;
        const float d = v - g2;
        const float sg = (float)(d > 0.f) - (float)(d < 0.f);   // torch.sign: 0 for a NaN
        // addcmul_(sign, g2, value=-(1 - beta2)), literally: -+0 * inf is the NaN torch gives
        const float vi = __fmaf_rn(-A.w2 * sg, g2, v);
        p = p + __fdiv_rn(X.neg_lr * mi, sqrt_rn(vi) + A.eps);  // addcdiv_(m, std, value=-lr)
        m = mi;
        v = vi;
    } else {
        if (X.flags & OF_WD) g = __fmaf_rn(p, X.wd, g);
        if constexpr (OK == OK_SGDM) {
            const float buf = (X.flags & OF_FIRST) ? g : __fmaf_rn(g, X.omd, m * X.mu);
            g = (X.flags & OF_NESTEROV) ? __fmaf_rn(buf, X.mu, g) : buf;
            m = buf;
        }
        p = __fmaf_rn(g, X.neg_lr, p);
    }
}

template <int OK, bool W = false>
__device__ __forceinline__ void opt_elem(const AdamConst& A, const OptConst& X, float s, float& p,
                                         float& m, float& v) {
    static_assert(OK != OK_GOUT, "OK_GOUT has no update (gout_store)");
    opt_update<OK>(A, X, rule_div<W>(A, s), p, m, v);      // rule(): mean = sum / k
}

// Deterministic block sum (256 threads) of one double per thread: the 64 lanes of a wave by a
// butterfly (every lane adds the same pairs: one result in all lanes), then the four waves as
// (w0 + w1) + (w2 + w3) through red[4] in LDS.  Every thread of the block must call it (one
// barrier); every thread gets the sum.
__device__ __forceinline__ double block_sum_f64(double a, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The leading elements of a tensor of `numel` elements that rule()'s sum takes as multi_row_sum
// columns (the main program); the rest are row_sum columns (the tail program).  ATen sums 32
// columns at a time with multi_row_sum and what is left with row_sum.  A tensor of fewer than 8
// elements takes ATen's scalar path instead, which still sums 4 columns at a time with
// multi_row_sum: the weighted kernels follow it (they are pinned to torch itself); the
// unweighted ones keep the 32-column rule for every tensor, as the oracle states it (no
// supported model has a tensor of 4 .. 7 elements, where the two differ).
// The compensated kernels (C) exist in the weighted form only, which keeps the instantiation count
// down; without a discount they run with weights 1.0 and the divisor k.  That is exact: x * 1.0f
// is x, and the IEEE division by an integer k is what div_const gives.
__host__ __device__ inline long rule_body(int numel, bool weighted) {
    return (weighted && numel < 8) ? (long)(numel / 4 * 4) : (long)(numel / 32) * 32;
}

// Program access.  The interpreter reads one macro word (two dwords) per step at a uniform address,
// so the words must
// come through the scalar cache: the reference-order program rides in the kernel arguments; a
// general-order program is copied (device to device, stream-ordered, right before the launch)
// into this constant-address-space buffer.  A plain global buffer would be read with vector loads
// (the compiler cannot prove the kernel does not write it) and every op would wait on one.
constexpr int CASC_CONST_WORDS = 16384;
__constant__ int32_t g_casc_prog[CASC_CONST_WORDS];

template <bool INL>
struct ProgRef {
    const RuleProg& R;
    __device__ __forceinline__ uint32_t lo(int i) const {
        if constexpr (INL) return (uint32_t)R.iprog[2 * i];
        else return (uint32_t)g_casc_prog[2 * i];
    }
    __device__ __forceinline__ uint32_t hi(int i) const {
        if constexpr (INL) return (uint32_t)R.iprog[2 * i + 1];
        else return (uint32_t)g_casc_prog[2 * i + 1];
    }
};

// stage a general-order program into g_casc_prog on `stream` (no-op for inline programs)
static int stage_program(const RuleProg& R, hipStream_t stream) {
    if (R.prog == nullptr) return 0;
    FLSIM_REQUIRE(2 * (R.info.len + 1) <= CASC_CONST_WORDS, "rule program of %d macro words (max %d)",
                  R.info.len, CASC_CONST_WORDS / 2 - 1);
    static void* dst = nullptr;
    if (!dst) FLSIM_CHECK_HIP(hipGetSymbolAddress(&dst, HIP_SYMBOL(g_casc_prog)));
    FLSIM_CHECK_HIP(hipMemcpyAsync(dst, R.prog, (size_t)(R.info.len + 1) * 8,
                                   hipMemcpyDeviceToDevice, stream));
    return 0;
}

// ================================================================================================
// k_agg_stream: S_t from a buffer
// ================================================================================================
struct AggArgs {
    const float* S;
    float* S_out;                   // nullable: S_t also written here (the FIFO slot at a tick)
    float* p;
    float* m;
    float* v;
    long g0;                        // first float4 group of this launch
    long lo, hi;                    // element range [lo, hi)
    int ntail;
    int tail_lo[MAX_TAILS];         // [lo, hi) element ranges summed with row_sum
    int tail_hi[MAX_TAILS];
    int nedge;                      // blocks 0..nedge-1: 256-element edge pieces at edge_lo[b]
    long edge_lo[MAX_EDGE];
    AdamConst ac;
    RuleProg R;
    OptConst oc;                    // after R: the OK_ADAM kernels' argument offsets stay as they were
    float w[RULE_MAX_ARR];          // weighted rule (W kernels only): the weight of R.arr[q]
    float* theta_out;               // C kernels only, nullable: the pre-update p also written here
    const float* snap[RULE_MAX_ARR];   // C kernels only: theta_src of R.arr[q]; nullptr = as it is
    float* G;                       // OK_GOUT kernels only: g = rule() is stored here
    double* partials;               // OK_GOUT kernels only: block b's sum of g * g (fp64) goes to
    long part0;                     //   partials[part0 + b]
};
static_assert(sizeof(AggArgs) <= 4096, "kernel argument block");

// OK_GOUT: the block's sum of squares, one double per block (every thread of the block calls).
// k_agg_stream_reg has no LDS of its own: the four wave sums get 32 B here.  k_agg_stream lends
// the head of its staging array (one more barrier first: wave 0 may still be reading it), so its
// 32 KB per block stay 32 KB and five blocks still fit a CU.
__device__ __forceinline__ void gout_block(const AggArgs& A, double sq, double* red) {
    const double t = block_sum_f64(sq, red);
    if (threadIdx.x == 0) A.partials[A.part0 + blockIdx.x] = t;
}
__device__ __forceinline__ void gout_block(const AggArgs& A, double sq) {
    __shared__ double red[4];
    gout_block(A, sq, red);
}
__device__ __forceinline__ void gout_block_lent(const AggArgs& A, double sq, f32x4* staging) {
    __syncthreads();
    gout_block(A, sq, reinterpret_cast<double*>(staging));
}

__device__ __forceinline__ bool in_tail(const AggArgs& A, long e) {
    bool r = false;
#pragma unroll
    for (int t = 0; t < MAX_TAILS; ++t)
        r |= (t < A.ntail) && e >= A.tail_lo[t] && e < A.tail_hi[t];
    return r;
}

__device__ __forceinline__ bool block_touch(const AggArgs& A, long blo, long span = 1024) {
    const long bhi = blo + span;
    bool touch = blo < A.lo || bhi > A.hi;
#pragma unroll
    for (int t = 0; t < MAX_TAILS; ++t)
        touch |= (t < A.ntail) && A.tail_lo[t] < bhi && A.tail_hi[t] > blo;
    return touch;
}

// Blocks [0, nedge) are 256-element edge pieces (launch edges, tensor tails): one element per
// thread; they run first and overlap the stream.  The other blocks stream one aligned float4 group
// per thread; a streaming block that is also an edge block returns at once.  Every load of a
// thread (S_t, the staged entry arrays, p, m, v) is issued before the arithmetic; loads and
// stores are non-temporal (each byte is touched once).
//
// W: the staleness-weighted rule, sum_j w_j * entry_j / divisor.  A stale value is multiplied by
// its array's weight once, where it is loaded (before the staging, and in the on-demand path); the
// program then runs on the products as it runs on the values.  The multiply is a plain fp32
// multiply (no contraction), a null array stays 0.
//
// C (on W only): delay compensation.  The snapshot of a stale array is loaded with the array; once
// p is there the value becomes compensate(value, p, snapshot) -- before its weight, so the staging
// and the program see it as they see any weighted value.  theta_out receives the pre-update p.
template <bool INL, int OK = OK_ADAM, bool W = false, bool C = false>
__global__ void __launch_bounds__(256) k_agg_stream(AggArgs A) {
    static_assert(W || !C, "the compensated form is built on the weighted one");
    constexpr bool HAS_M = opt_n_state(OK) >= 1, HAS_V = opt_n_state(OK) == 2;
    __shared__ f32x4 ys_lds[NYR * 256];
    const ProgRef<INL> prog{A.R};
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < A.nedge) {
        long e = A.edge_lo[blockIdx.x] + tid;
        bool live = true;
        if constexpr (OK == OK_GOUT) {
            // every thread stays for the block's sum: one out of range works on element lo and
            // stores nothing
            live = e >= A.lo && e < A.hi;
            if (!live) e = A.lo;
        } else if (e < A.lo || e >= A.hi) return;
        const float x = A.S[e];
        float p = 0.f, m = 0.f, v = 0.f;
        if constexpr (OK != OK_GOUT || C) p = A.p[e];
        if constexpr (HAS_M) m = A.m[e];
        if constexpr (HAS_V) v = A.v[e];
        const float p0 = p;             // the pre-update p (C)
        auto yf = [&](int q) -> float {
            if (!A.R.arr[q]) return 0.f;
            if constexpr (C) {
                float y = A.R.arr[q][e];
                if (A.snap[q]) y = compensate(y, p0, A.snap[q][e], A.ac.lam);
                return y * A.w[q];
            } else if constexpr (W) return A.R.arr[q][e] * A.w[q];
            else return A.R.arr[q][e];
        };
        const CascVals<float> cv = casc_values(x, A.R.info.need, A.R.info.lp);
        const bool tail = in_tail(A, e);
        float s = 0.f;
        if (!tail) s = casc_run_macro(prog, 0, cv, yf);
        if (tail) s = casc_run_macro(prog, A.R.info.tail_off, cv, yf);
        if constexpr (OK == OK_GOUT) {
            const float g = rule_div<W>(A.ac, s);
            if (live) {
                A.G[e] = g;
                if (A.S_out) A.S_out[e] = x;
                if constexpr (C) {
                    if (A.theta_out) A.theta_out[e] = p0;
                }
            }
            gout_block_lent(A, live ? (double)g * (double)g : 0.0, ys_lds);
            return;
        } else {
            opt_elem<OK, W>(A.ac, A.oc, s, p, m, v);
            A.p[e] = p;
        }
        if constexpr (HAS_M) A.m[e] = m;
        if constexpr (HAS_V) A.v[e] = v;
        if (A.S_out) A.S_out[e] = x;
        if constexpr (C) {
            if (A.theta_out) A.theta_out[e] = p0;
        }
        return;
    }
    const long e0 = 4 * (A.g0 + (long)(blockIdx.x - A.nedge) * 256) + 4 * tid;
    if (block_touch(A, e0 - 4 * tid)) {
        if constexpr (OK == OK_GOUT) {
            if (tid == 0) A.partials[A.part0 + blockIdx.x] = 0.0;      // its edge pieces hold the sum
        }
        return;
    }
    auto ld = [](const float* ptr) -> f32x4 {
        return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ptr));
    };
    auto st = [](float* ptr, f32x4 val) {
        __builtin_nontemporal_store(val, reinterpret_cast<f32x4*>(ptr));
    };
    const int nst = A.R.narr < NYR ? A.R.narr : NYR;
    f32x4 ys[NYR];
#pragma unroll
    for (int q = 0; q < NYR; ++q)
        ys[q] = (q < nst && A.R.arr[q]) ? ld(A.R.arr[q] + e0) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ts[C ? NYR : 1];
    if constexpr (C) {
#pragma unroll
        for (int q = 0; q < NYR; ++q)
            ts[q] = (q < nst && A.R.arr[q] && A.snap[q]) ? ld(A.snap[q] + e0)
                                                         : f32x4{0.f, 0.f, 0.f, 0.f};
    } else if constexpr (W) {
#pragma unroll
        for (int q = 0; q < NYR; ++q)
            if (q < nst) ys[q] = ys[q] * A.w[q];
    }
    const f32x4 x = ld(A.S + e0);
    f32x4 p = {0.f, 0.f, 0.f, 0.f}, m = p, v = p;
    if constexpr (OK != OK_GOUT || C) p = ld(A.p + e0);
    if constexpr (HAS_M) m = ld(A.m + e0);
    if constexpr (HAS_V) v = ld(A.v + e0);
    const f32x4 p0 = p;                 // the pre-update p (C)
    if constexpr (C) {
#pragma unroll
        for (int q = 0; q < NYR; ++q)
            if (q < nst) {
                if (A.R.arr[q] && A.snap[q]) ys[q] = compensate(ys[q], p0, ts[q], A.ac.lam);
                ys[q] = ys[q] * A.w[q];
            }
    }
#pragma unroll
    for (int q = 0; q < NYR; ++q)
        if (q < nst) ys_lds[q * 256 + tid] = ys[q];
    auto yf = [&](int q) -> f32x4 {
        if (q < NYR) return ys_lds[q * 256 + tid];
        if (!A.R.arr[q]) return f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (C) {
            f32x4 y = ld(A.R.arr[q] + e0);
            if (A.snap[q]) y = compensate(y, p0, ld(A.snap[q] + e0), A.ac.lam);
            return y * A.w[q];
        } else if constexpr (W) return ld(A.R.arr[q] + e0) * A.w[q];
        else return ld(A.R.arr[q] + e0);
    };
    const f32x4 sum = casc_run_macro<true>(
        prog, 0, casc_values(x, A.R.info.need, A.R.info.lp), yf);
    if constexpr (OK == OK_GOUT) {
        f32x4 g;
        double sq = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            g[u] = rule_div<W>(A.ac, sum[u]);
            sq += (double)g[u] * (double)g[u];
        }
        st(A.G + e0, g);
        gout_block_lent(A, sq, ys_lds);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float pp = p[u], mm = m[u], vv = v[u];
            opt_elem<OK, W>(A.ac, A.oc, sum[u], pp, mm, vv);
            p[u] = pp;
            m[u] = mm;
            v[u] = vv;
        }
        st(A.p + e0, p);
    }
    if constexpr (HAS_M) st(A.m + e0, m);
    if constexpr (HAS_V) st(A.v + e0, v);
    if (A.S_out) st(A.S_out + e0, x);
    if constexpr (C) {
        if (A.theta_out) st(A.theta_out + e0, p0);
    }
}

// The reference-order stream with its few entry arrays (NY <= 2: the popped FIFO entries of the
// reference's one slow worker) held in registers instead of LDS, and G float4 groups per thread
// (block = 256 * G groups, group j of thread t at 256 j + t: each j is one coalesced sweep).  All
// of a thread's loads are issued before any arithmetic; no LDS, so 8 blocks of 4 waves fit a CU
// (the LDS-staged form above holds 32 KB per block: 5).  The interpreter runs once per thread on
// G * 4 elements in lock step (T = a 4G-wide vector; the program is uniform).  Edge pieces as
// k_agg_stream (a streaming block covers 1024 G elements).
template <int G>
struct AggVec;
template <>
struct AggVec<1> { typedef float T __attribute__((ext_vector_type(4))); };
template <>
struct AggVec<2> { typedef float T __attribute__((ext_vector_type(8))); };

template <int G, int NY, int OK = OK_ADAM, bool W = false, bool C = false>
__global__ void __launch_bounds__(256) k_agg_stream_reg(AggArgs A) {
    static_assert(W || !C, "the compensated form is built on the weighted one");
    constexpr bool HAS_M = opt_n_state(OK) >= 1, HAS_V = opt_n_state(OK) == 2;
    typedef typename AggVec<G>::T T;
    const ProgRef<true> prog{A.R};
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < A.nedge) {
        long e = A.edge_lo[blockIdx.x] + tid;
        bool live = true;
        if constexpr (OK == OK_GOUT) {
            // every thread stays for the block's sum: one out of range works on element lo and
            // stores nothing
            live = e >= A.lo && e < A.hi;
            if (!live) e = A.lo;
        } else if (e < A.lo || e >= A.hi) return;
        const float x = A.S[e];
        float p = 0.f, m = 0.f, v = 0.f;
        if constexpr (OK != OK_GOUT || C) p = A.p[e];
        if constexpr (HAS_M) m = A.m[e];
        if constexpr (HAS_V) v = A.v[e];
        const float p0 = p;             // the pre-update p (C)
        auto yf = [&](int q) -> float {
            if (!A.R.arr[q]) return 0.f;
            if constexpr (C) {
                float y = A.R.arr[q][e];
                if (A.snap[q]) y = compensate(y, p0, A.snap[q][e], A.ac.lam);
                return y * A.w[q];
            } else if constexpr (W) return A.R.arr[q][e] * A.w[q];
            else return A.R.arr[q][e];
        };
        const CascVals<float> cv = casc_values(x, A.R.info.need, A.R.info.lp);
        const bool tail = in_tail(A, e);
        float s = 0.f;
        if (!tail) s = casc_run_macro(prog, 0, cv, yf);
        if (tail) s = casc_run_macro(prog, A.R.info.tail_off, cv, yf);
        if constexpr (OK == OK_GOUT) {
            const float g = rule_div<W>(A.ac, s);
            if (live) {
                A.G[e] = g;
                if (A.S_out) A.S_out[e] = x;
                if constexpr (C) {
                    if (A.theta_out) A.theta_out[e] = p0;
                }
            }
            gout_block(A, live ? (double)g * (double)g : 0.0);
            return;
        } else {
            opt_elem<OK, W>(A.ac, A.oc, s, p, m, v);
            A.p[e] = p;
        }
        if constexpr (HAS_M) A.m[e] = m;
        if constexpr (HAS_V) A.v[e] = v;
        if (A.S_out) A.S_out[e] = x;
        if constexpr (C) {
            if (A.theta_out) A.theta_out[e] = p0;
        }
        return;
    }
    const long b0 = 4 * (A.g0 + (long)(blockIdx.x - A.nedge) * 256 * G);   // block's first element
    if (block_touch(A, b0, 1024L * G)) {
        if constexpr (OK == OK_GOUT) {
            if (tid == 0) A.partials[A.part0 + blockIdx.x] = 0.0;      // its edge pieces hold the sum
        }
        return;
    }
    auto ld = [](const float* ptr) -> f32x4 {
        return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ptr));
    };
    auto st = [](float* ptr, f32x4 val) {
        __builtin_nontemporal_store(val, reinterpret_cast<f32x4*>(ptr));
    };
    long e[G];
#pragma unroll
    for (int j = 0; j < G; ++j) e[j] = b0 + 1024L * j + 4 * tid;
    f32x4 xs[G], ps[G], ms[G], vs[G], ys[NY > 0 ? NY : 1][G];
#pragma unroll
    for (int q = 0; q < NY; ++q)
#pragma unroll
        for (int j = 0; j < G; ++j)
            ys[q][j] = A.R.arr[q] ? ld(A.R.arr[q] + e[j]) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ts[C && NY > 0 ? NY : 1][G];
    if constexpr (C) {
#pragma unroll
        for (int q = 0; q < NY; ++q)
#pragma unroll
            for (int j = 0; j < G; ++j)
                ts[q][j] = (A.R.arr[q] && A.snap[q]) ? ld(A.snap[q] + e[j])
                                                     : f32x4{0.f, 0.f, 0.f, 0.f};
    } else if constexpr (W) {
#pragma unroll
        for (int q = 0; q < NY; ++q)
#pragma unroll
            for (int j = 0; j < G; ++j) ys[q][j] = ys[q][j] * A.w[q];
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
        xs[j] = ld(A.S + e[j]);
        if constexpr (OK != OK_GOUT || C) ps[j] = ld(A.p + e[j]);
        else ps[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (HAS_M) ms[j] = ld(A.m + e[j]);
        else ms[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (HAS_V) vs[j] = ld(A.v + e[j]);
        else vs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (C) {                  // ps is still the pre-update p
#pragma unroll
        for (int q = 0; q < NY; ++q)
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (A.R.arr[q] && A.snap[q])
                    ys[q][j] = compensate(ys[q][j], ps[j], ts[q][j], A.ac.lam);
                ys[q][j] = ys[q][j] * A.w[q];
            }
    }
    auto widen = [](const f32x4 (&a)[G]) -> T {
        T t;
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int u = 0; u < 4; ++u) t[4 * j + u] = a[j][u];
        return t;
    };
    T yw[NY > 0 ? NY : 1];
#pragma unroll
    for (int q = 0; q < NY; ++q) yw[q] = widen(ys[q]);
    auto yf = [&](int q) -> T {
        if constexpr (NY == 0) return T(0.f);
        else if constexpr (NY == 1) return yw[0];
        else return q == 0 ? yw[0] : yw[1];
    };
    const T sum = casc_run_macro<true>(prog, 0, casc_values(widen(xs), A.R.info.need, A.R.info.lp),
                                       yf);
    double sq = 0.0;                    // OK_GOUT: this thread's squares, group by group
#pragma unroll
    for (int j = 0; j < G; ++j) {
        if constexpr (C) {
            if (A.theta_out) st(A.theta_out + e[j], ps[j]);
        }
        if constexpr (OK == OK_GOUT) {
            f32x4 g;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                g[u] = rule_div<W>(A.ac, sum[4 * j + u]);
                sq += (double)g[u] * (double)g[u];
            }
            st(A.G + e[j], g);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float pp = ps[j][u], mm = ms[j][u], vv = vs[j][u];
                opt_elem<OK, W>(A.ac, A.oc, sum[4 * j + u], pp, mm, vv);
                ps[j][u] = pp;
                ms[j][u] = mm;
                vs[j][u] = vv;
            }
            st(A.p + e[j], ps[j]);
        }
        if constexpr (HAS_M) st(A.m + e[j], ms[j]);
        if constexpr (HAS_V) st(A.v + e[j], vs[j]);
        if (A.S_out) st(A.S_out + e[j], xs[j]);
    }
    if constexpr (OK == OK_GOUT) gout_block(A, sq);
}

// ================================================================================================
// The clipped step's second and third launches (include/flsim.h)
// ================================================================================================
// One block: thread t adds partials[t], partials[t + 256], ... in index order, block_sum_f64 adds
// the 256 threads; thread 0 writes out[0] = total_norm = (float)sqrt(sum) and out[1] = coef =
// min(RN(1 / (total_norm + f32(1e-6))) * max_norm, 1.0f).  The comparison keeps a NaN (fminf
// would drop it); the reciprocal is the IEEE division 1 / x, as torch's reciprocal().
__global__ void __launch_bounds__(256) k_clip_finish(const double* partials, long n, float max_norm,
                                                     float* out) {
    double a = 0.0;
    long i = threadIdx.x;
    for (; i + 7 * 256 < n; i += 8 * 256) {     // eight loads in flight, added in index order
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = partials[i + 256 * u];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += x[u];
    }
    for (; i < n; i += 256) a += partials[i];
    __shared__ double red[4];
    const double tot = block_sum_f64(a, red);
    if (threadIdx.x == 0) {
        const float t = (float)sqrt(tot);
        float c = __fdiv_rn(1.0f, t + 1e-6f) * max_norm;
        c = c > 1.0f ? 1.0f : c;
        out[0] = t;
        out[1] = c;
    }
}

struct ClipApplyArgs {
    const float* G;
    const float* coef;              // the device scalar k_clip_finish wrote
    float* p;
    float* m;
    float* v;
    long P;
    AdamConst ac;
    OptConst oc;
};

// g' = G * coef (one fp32 multiply, always applied), then the update of kind OK on g' (opt_update:
// no cascade program in between, so a -0 gradient stays -0).  One float4 group per thread,
// non-temporal like the stream; the last P % 4 elements one by one.
template <int OK>
__global__ void __launch_bounds__(256) k_clip_apply(ClipApplyArgs A) {
    constexpr bool HAS_M = opt_n_state(OK) >= 1, HAS_V = opt_n_state(OK) == 2;
    const long e0 = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
    if (e0 >= A.P) return;
    const float coef = *A.coef;
    if (e0 + 4 <= A.P) {
        auto ld = [](const float* ptr) -> f32x4 {
            return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ptr));
        };
        auto st = [](float* ptr, f32x4 val) {
            __builtin_nontemporal_store(val, reinterpret_cast<f32x4*>(ptr));
        };
        const f32x4 g = ld(A.G + e0);
        f32x4 p = ld(A.p + e0), m = {0.f, 0.f, 0.f, 0.f}, v = m;
        if constexpr (HAS_M) m = ld(A.m + e0);
        if constexpr (HAS_V) v = ld(A.v + e0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float pp = p[u], mm = m[u], vv = v[u];
            opt_update<OK>(A.ac, A.oc, g[u] * coef, pp, mm, vv);
            p[u] = pp;
            m[u] = mm;
            v[u] = vv;
        }
        st(A.p + e0, p);
        if constexpr (HAS_M) st(A.m + e0, m);
        if constexpr (HAS_V) st(A.v + e0, v);
        return;
    }
    for (long e = e0; e < A.P; ++e) {
        float p = A.p[e], m = 0.f, v = 0.f;
        if constexpr (HAS_M) m = A.m[e];
        if constexpr (HAS_V) v = A.v[e];
        opt_update<OK>(A.ac, A.oc, A.G[e] * coef, p, m, v);
        A.p[e] = p;
        if constexpr (HAS_M) A.m[e] = m;
        if constexpr (HAS_V) A.v[e] = v;
    }
}

// ================================================================================================
// k_slab_step: slabs -> S_t [-> S_out] [-> rule() + Adam], one launch
// ================================================================================================
struct StepArgs {
    float* base;                    // gradstate
    long cnt_off, part_off;         // tile counters (int32) / unit partials, floats from base
    float* S_out;
    float* p;
    float* m;
    float* v;
    int nseg, units;
    int u_lo;                       // first unit of this launch (block b runs unit u_lo + b)
    int il_lo, il_w, il_n;          // interleave units [il_lo, il_lo + il_n): il_w wide, then conv
    AdamConst ac;
    RuleProg R;
    SlabSeg seg[STEP_MAX_SEG];
    OptConst oc;                    // after seg: the OK_ADAM kernels' argument offsets stay as they were
    float w[STEP_MAX_WARR];         // weighted rule (W kernels only): the weight of R.arr[q]
    float* theta_out;               // C kernels only, nullable: the pre-update p also written here
    // (C kernels: lambda is ac.lam, the snapshot of R.arr[q] is R.arr[STEP_SNAP0 + q]; slabstep.h)
};
static_assert(sizeof(StepArgs) <= 4096, "kernel argument block");

// LDS map (ONE __shared__ array, cdna_hip_programming.md §5 item 4(a)): z-lane partials f32x4[256]
// at 0, the tile's 256 sums at 1024, the last-arriver flag at 1280, staged entry arrays at 1536
constexpr int L_RED = 0, L_SUM = 1024, L_FLAG = 1280, L_Y = 1536;
// general-order tiles also stage x, p, m, v for the one-wave interpreter
constexpr int L_S = L_Y + NYR * 256, L_P = L_S + 256, L_M = L_P + 256, L_V = L_M + 256,
              L_END = L_V + 256;

// one unit's z-range of 256 slab columns -> this thread's column sum (thread t owns column t)
__device__ __forceinline__ float reduce_cols(const float* slab, const SlabSeg& g, int tile, int z0,
                                             int z1, float* lds) {
    const int tid = threadIdx.x;
    if ((g.n & 3) == 0) {
        const int tx = tid & 63, tz = tid >> 6;
        const long col = (long)tile * 256 + 4 * tx;
        f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (col < g.n) {
            const float* pz = slab + col;
            int z = z0 + tz;
            for (; z + 28 < z1; z += 32) {        // eight rows in flight per thread
                f32x4 x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    x[u] = __builtin_nontemporal_load(
                        reinterpret_cast<const f32x4*>(pz + (long)(z + 4 * u) * g.n));
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u & 3] += x[u];
            }
            for (; z + 12 < z1; z += 16) {
                f32x4 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    x[u] = __builtin_nontemporal_load(
                        reinterpret_cast<const f32x4*>(pz + (long)(z + 4 * u) * g.n));
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] += x[u];
            }
            // at most three z-lanes rows left
            if (z < z1) acc[0] += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pz + (long)z * g.n));
            if (z + 4 < z1) acc[1] += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pz + (long)(z + 4) * g.n));
            if (z + 8 < z1) acc[2] += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pz + (long)(z + 8) * g.n));
        }
        f32x4 t = acc[0];
        t += acc[1];
        t += acc[2];
        t += acc[3];
        f32x4* red = reinterpret_cast<f32x4*>(lds + L_RED);
        red[tid] = t;
        __syncthreads();
        if (tz == 0) {
            t += red[64 + tx];
            t += red[128 + tx];
            t += red[192 + tx];
            reinterpret_cast<f32x4*>(lds + L_SUM)[tx] = t;
        }
        __syncthreads();
        return lds[L_SUM + tid];
    }
    // rows not a multiple of 4 floats (tiny tensors): one column per thread
    const long col = (long)tile * 256 + tid;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (col < g.n) {
        const float* pz = slab + col;
        int z = z0;
        for (; z + 3 < z1; z += 4) {
            a0 += pz[(long)z * g.n];
            a1 += pz[(long)(z + 1) * g.n];
            a2 += pz[(long)(z + 2) * g.n];
            a3 += pz[(long)(z + 3) * g.n];
        }
        if (z < z1) a0 += pz[(long)z * g.n];
        if (z + 1 < z1) a1 += pz[(long)(z + 1) * g.n];
        if (z + 2 < z1) a2 += pz[(long)(z + 2) * g.n];
    }
    a0 += a1;
    a0 += a2;
    a0 += a3;
    return a0;
}

// finish-phase addressing of a slab column: packed conv [co][khkw*CIP + ci] -> torch
// [co][ci][kh][kw]; padding columns (ci >= CI, khkw >= 9, col >= n) carry nothing
__device__ __forceinline__ bool col_to_param(const SlabSeg& g, long col, long& tl) {
    tl = col;
    bool valid = col < g.n;
    if (g.CO) {
        const int co = (int)(col / g.KP);
        const int k = (int)(col - (long)co * g.KP);
        const int khkw = k / g.CIP, ci = k - khkw * g.CIP;
        valid = valid && khkw < 9 && ci < g.CI;
        tl = ((long)co * g.CI + ci) * 9 + khkw;
    }
    return valid;
}

// Identity-layout segments (the linear layers): tiles of 1024 elements, thread t owns the float4
// column 4t; it sums its Z slab rows itself (small Z, four accumulators) and finishes with 16-B
// parameter-side loads and stores; the parameter loads are issued before the slab reads.
template <bool ADAM, bool INL, int OK, bool W, bool C>
__device__ __forceinline__ void slab_step_wide(const StepArgs& A, const SlabSeg& g, int u, int ul,
                                               float* lds) {
    constexpr bool HAS_M = opt_n_state(OK) >= 1, HAS_V = opt_n_state(OK) == 2;
    // entry arrays held in registers (the rest load on demand): all of a general-order program's
    // arrays up to 8 (configs[3] uses 6), so no Y word of the interpreter waits on a global load
    constexpr int NYW = 8;
    const int tid = threadIdx.x;
    const float* slab = A.base + g.slab_off;
    const ProgRef<INL> prog{A.R};
    int tile, t_end, j;
    if (g.nz == 1) {
        tile = ul * g.tpu;
        t_end = tile + g.tpu < g.tiles ? tile + g.tpu : g.tiles;
        j = 0;
    } else {
        tile = ul / g.nz;
        j = ul - tile * g.nz;
        t_end = tile + 1;
    }
    const int z0 = j * g.zc;
    int z1 = z0 + g.zc < g.Z ? z0 + g.zc : g.Z;
    if (z1 > g.zlim) z1 = g.zlim > z0 ? g.zlim : z0;     // rows past zlim are stale this epoch
    auto ld = [](const float* ptr) -> f32x4 {
        return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ptr));
    };
    for (; tile < t_end; ++tile) {
        const long c = (long)tile * 1024 + 4 * tid;
        const bool valid = c < g.n;
        const long e = g.toff + c;
        f32x4 p, m, v, ys[NYW];
        auto load_param_side = [&]() {
#pragma unroll
            for (int q = 0; q < NYW; ++q)
                ys[q] = (q < A.R.narr && A.R.arr[q]) ? ld(A.R.arr[q] + e) : f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 ts[C ? NYW : 1];
            if constexpr (C) {
#pragma unroll
                for (int q = 0; q < NYW; ++q)
                    ts[q] = (q < A.R.narr && A.R.arr[q] && A.R.arr[STEP_SNAP0 + q])
                                ? ld(A.R.arr[STEP_SNAP0 + q] + e) : f32x4{0.f, 0.f, 0.f, 0.f};
            } else if constexpr (W) {
#pragma unroll
                for (int q = 0; q < NYW; ++q)
                    if (q < A.R.narr) ys[q] = ys[q] * A.w[q];
            }
            p = ld(A.p + e);
            if constexpr (HAS_M) m = ld(A.m + e);
            else m = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (HAS_V) v = ld(A.v + e);
            else v = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (C) {              // p is the pre-update p
#pragma unroll
                for (int q = 0; q < NYW; ++q)
                    if (q < A.R.narr) {
                        if (A.R.arr[q] && A.R.arr[STEP_SNAP0 + q])
                            ys[q] = compensate(ys[q], p, ts[q], A.ac.lam);
                        ys[q] = ys[q] * A.w[q];
                    }
            }
        };
        // reference order: the parameter side is loaded ahead of the slab rows (both round trips
        // overlap); general order: after them, so the registers are free during the reduction and
        // more waves fit (the interpreter that follows hides the exposed load behind the other
        // resident waves)
        if (ADAM && INL && valid && g.nz == 1) load_param_side();
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
        if (valid) {
            const float* pz = slab + c;
            int z = z0;
            for (; z + 7 < z1; z += 8) {               // eight rows in flight
                f32x4 x[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) x[r] = ld(pz + (long)(z + r) * g.n);
                a0 += x[0];
                a1 += x[1];
                a2 += x[2];
                a3 += x[3];
                a0 += x[4];
                a1 += x[5];
                a2 += x[6];
                a3 += x[7];
            }
            for (; z + 3 < z1; z += 4) {
                const f32x4 x0 = ld(pz + (long)z * g.n), x1 = ld(pz + (long)(z + 1) * g.n);
                const f32x4 x2 = ld(pz + (long)(z + 2) * g.n), x3 = ld(pz + (long)(z + 3) * g.n);
                a0 += x0;
                a1 += x1;
                a2 += x2;
                a3 += x3;
            }
            if (z < z1) a0 += ld(pz + (long)z * g.n);
            if (z + 1 < z1) a1 += ld(pz + (long)(z + 1) * g.n);
            if (z + 2 < z1) a2 += ld(pz + (long)(z + 2) * g.n);
        }
        a0 += a1;
        a0 += a2;
        a0 += a3;
        if (ADAM && !INL && valid && g.nz == 1) load_param_side();
        if (g.nz > 1) {
            // the conv path's hand-off with 1024 floats per unit (sc1 stores / loads)
            float* part = A.base + A.part_off;
            float* mine = part + (long)u * 1024 + 4 * tid;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                __hip_atomic_store(mine + k, a0[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            int* cnt = reinterpret_cast<int*>(A.base + A.cnt_off) + g.tile0 + tile;
            if (tid == 0) {
                const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
                lds[L_FLAG] = __int_as_float(old);
            }
            __syncthreads();
            if (__float_as_int(lds[L_FLAG]) != g.nz - 1) return;
            if (ADAM && valid) load_param_side();
            float* pt = part + (long)(g.unit0 + tile * g.nz) * 1024 + 4 * tid;
            for (int jj = 0; jj < g.nz; ++jj) {
                f32x4 x;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    x[k] = __hip_atomic_load(pt + (long)jj * 1024 + k, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
                if (jj == 0) a0 = x;
                else a0 += x;
            }
            if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!valid) continue;
        if (A.S_out) *reinterpret_cast<f32x4*>(A.S_out + e) = a0;
        if constexpr (C) {
            if (A.theta_out) *reinterpret_cast<f32x4*>(A.theta_out + e) = p;
        }
        if constexpr (ADAM) {
            const f32x4 p0 = p;             // the pre-update p (C)
            auto yf = [&](int q) -> f32x4 {
                // q is uniform: a scalar switch picks the register, no indexed access
                static_assert(NYW == 8, "one case per register-held entry array");
                switch (q) {
                    case 0: return ys[0];
                    case 1: return ys[1];
                    case 2: return ys[2];
                    case 3: return ys[3];
                    case 4: return ys[4];
                    case 5: return ys[5];
                    case 6: return ys[6];
                    case 7: return ys[7];
                    default:
                        if (!A.R.arr[q]) return f32x4{0.f, 0.f, 0.f, 0.f};
                        if constexpr (C) {
                            f32x4 y = ld(A.R.arr[q] + e);
                            if (A.R.arr[STEP_SNAP0 + q])
                                y = compensate(y, p0, ld(A.R.arr[STEP_SNAP0 + q] + e), A.ac.lam);
                            return y * A.w[q];
                        } else if constexpr (W) return ld(A.R.arr[q] + e) * A.w[q];
                        else return ld(A.R.arr[q] + e);
                }
            };
            const f32x4 sum = casc_run_macro<true>(
                prog, 0, casc_values(a0, A.R.info.need, A.R.info.lp), yf);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pp = p[k], mm = m[k], vv = v[k];
                opt_elem<OK, W>(A.ac, A.oc, sum[k], pp, mm, vv);
                p[k] = pp;
                m[k] = mm;
                v[k] = vv;
            }
            __builtin_nontemporal_store(p, reinterpret_cast<f32x4*>(A.p + e));
            if constexpr (HAS_M) __builtin_nontemporal_store(m, reinterpret_cast<f32x4*>(A.m + e));
            if constexpr (HAS_V) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(A.v + e));
        }
    }
}

// Units are dispatched round-robin (block b -> unit b): consecutive units, hence every segment's
// mix of cheap and heavy units, are spread over all XCDs.  The partial hand-off uses sc1 stores /
// loads, whose cost does not depend on which XCD the last arriver sits on.  Each thread's
// parameter-side loads (p, m, v, staged entry arrays) are issued before the slab reduction (whole
// tiles) or together with the partial loads (split tiles), so the two memory round trips overlap.
template <bool ADAM, bool INL, int OK, bool W, bool C>
__device__ __forceinline__ void slab_step_body(const StepArgs& A, float* lds) {
    constexpr bool HAS_M = opt_n_state(OK) >= 1, HAS_V = opt_n_state(OK) == 2;
    const int tid = threadIdx.x;
    // runs of XG consecutive units (a tile's z-units, neighbouring tiles: one parameter region)
    // share an XCD (blocks b and b + 8 do), the runs themselves go round-robin over the XCDs so
    // every XCD gets the same mix of segments
    constexpr int XG = 8;
    const int nb = (int)gridDim.x;
    const int b = (int)blockIdx.x;
    const int nfull = nb / (8 * XG) * (8 * XG);
    const int lb = b < nfull ? ((b >> 3) / XG * 8 + (b & 7)) * XG + (b >> 3) % XG : b;
    int u = A.u_lo + lb;
    if (u >= A.units) return;
    if (u >= A.il_lo && A.il_n > 0) {
        // position i of the interleaved run: wide unit f(i) when f steps, else conv unit i - f(i),
        // f(i) = floor(i * W / N) (the wide units spread evenly over the run)
        const long i = u - A.il_lo;
        const long f0 = i * A.il_w / A.il_n, f1 = (i + 1) * A.il_w / A.il_n;
        u = A.il_lo + (f1 > f0 ? (int)f0 : A.il_w + (int)(i - f0));
    }
    int si = 0;
    while (si + 1 < A.nseg && A.seg[si + 1].unit0 <= u) ++si;
    const SlabSeg& g = A.seg[si];
    const int ul = u - g.unit0;
    if (g.wide) {
        slab_step_wide<ADAM, INL, OK, W, C>(A, g, u, ul, lds);
        return;
    }
    int tile, t_end, j;
    if (g.nz == 1) {
        tile = ul * g.tpu;
        t_end = tile + g.tpu < g.tiles ? tile + g.tpu : g.tiles;
        j = 0;
    } else {
        tile = ul / g.nz;
        j = ul - tile * g.nz;
        t_end = tile + 1;
    }
    const float* slab = A.base + g.slab_off;
    const int z0 = j * g.zc;
    int z1 = z0 + g.zc < g.Z ? z0 + g.zc : g.Z;
    if (z1 > g.zlim) z1 = g.zlim > z0 ? g.zlim : z0;     // rows past zlim are stale this epoch
    const ProgRef<INL> prog{A.R};
    const int nst = A.R.narr < NYR ? A.R.narr : NYR;
    for (; tile < t_end; ++tile) {
        long tl;
        const bool valid = col_to_param(g, (long)tile * 256 + tid, tl);
        const long e = g.toff + tl;
        float p = 0.f, m = 0.f, v = 0.f, ys[NYR];
        auto load_param_side = [&]() {
#pragma unroll
            for (int q = 0; q < NYR; ++q)
                ys[q] = (q < nst && A.R.arr[q]) ? A.R.arr[q][e] : 0.f;
            float ts[C ? NYR : 1];
            if constexpr (C) {
#pragma unroll
                for (int q = 0; q < NYR; ++q)
                    ts[q] = (q < nst && A.R.arr[q] && A.R.arr[STEP_SNAP0 + q])
                                ? A.R.arr[STEP_SNAP0 + q][e] : 0.f;
            } else if constexpr (W) {
#pragma unroll
                for (int q = 0; q < NYR; ++q)
                    if (q < nst) ys[q] = ys[q] * A.w[q];
            }
            p = A.p[e];
            if constexpr (HAS_M) m = A.m[e];
            if constexpr (HAS_V) v = A.v[e];
            if constexpr (C) {              // p is the pre-update p
#pragma unroll
                for (int q = 0; q < NYR; ++q)
                    if (q < nst) {
                        if (A.R.arr[q] && A.R.arr[STEP_SNAP0 + q])
                            ys[q] = compensate(ys[q], p, ts[q], A.ac.lam);
                        ys[q] = ys[q] * A.w[q];
                    }
            }
        };
        if (ADAM && valid && g.nz == 1) load_param_side();
        __syncthreads();                       // LDS reuse across the unit's tiles
        float s = reduce_cols(slab, g, tile, z0, z1, lds);
        if (g.nz > 1) {
            // hand the partial to the tile's last-arriving unit: sc1 stores, every wave's vmcnt
            // drained, one agent-scope ticket; the last arriver reads all partials with sc1 loads
            float* part = A.base + A.part_off;
            __hip_atomic_store(part + (long)u * 1024 + tid, s, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            int* cnt = reinterpret_cast<int*>(A.base + A.cnt_off) + g.tile0 + tile;
            if (tid == 0) {
                const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
                lds[L_FLAG] = __int_as_float(old);
            }
            __syncthreads();
            if (__float_as_int(lds[L_FLAG]) != g.nz - 1) return;
            if (ADAM && valid) load_param_side();
            // the nz partials in z order, eight loads in flight
            float* pt = part + (long)(g.unit0 + tile * g.nz) * 1024 + tid;
            s = 0.f;
            bool first = true;
            for (int j0 = 0; j0 < g.nz; j0 += 8) {
                float pv[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                    pv[jj] = j0 + jj < g.nz ? __hip_atomic_load(pt + (long)(j0 + jj) * 1024,
                                                                __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_AGENT)
                                            : 0.f;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    if (j0 + jj < g.nz) {
                        s = first ? pv[jj] : s + pv[jj];
                        first = false;
                    }
                }
            }
            if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if constexpr (ADAM && !INL) {
            // general order: the tile's 256 elements go through the program as float4 lanes of
            // ONE wave (a quarter of the interpreter's scalar work per element); the tile is
            // staged in LDS (x, p, m, v, entry arrays) and written back by its owning threads.
            // Tiles holding row_sum tail elements, or more arrays than NYR, take the per-element
            // path below.
            if (valid && A.S_out) A.S_out[e] = s;
            if constexpr (C) {
                if (valid && A.theta_out) A.theta_out[e] = p;
            }
            const bool tail = valid && tl >= rule_body(g.numel, W);
            lds[L_S + tid] = valid ? s : 0.f;
            lds[L_P + tid] = p;
            if constexpr (HAS_M) lds[L_M + tid] = m;
            if constexpr (HAS_V) lds[L_V + tid] = v;
#pragma unroll
            for (int q = 0; q < NYR; ++q)
                if (q < nst) lds[L_Y + q * 256 + tid] = valid ? ys[q] : 0.f;
            if (!__syncthreads_or(tail) && A.R.narr <= NYR) {
#if FLSIM_SEQ_EARLY_EXIT
                if (tile + 1 == t_end) {
                    // the unit's last tile: waves 1..3 leave now (their slots go to the next
                    // streaming blocks instead of idling at a barrier through the program); wave
                    // 0 interprets and stores its four elements per lane itself
                    if (tid >= 64) return;
                    const f32x4* l4 = reinterpret_cast<const f32x4*>(lds);
                    auto yf4 = [&](int q) -> f32x4 { return l4[(L_Y + q * 256) / 4 + tid]; };
                    const f32x4 sum = casc_run_macro<true>(
                        prog, 0, casc_values(l4[L_S / 4 + tid], A.R.info.need, A.R.info.lp), yf4);
                    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
                    const f32x4 pp = l4[L_P / 4 + tid], mm = HAS_M ? l4[L_M / 4 + tid] : zero4,
                                vv = HAS_V ? l4[L_V / 4 + tid] : zero4;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        long tk;
                        if (!col_to_param(g, (long)tile * 256 + 4 * tid + k, tk)) continue;
                        float p1 = pp[k], m1 = mm[k], v1 = vv[k];
                        opt_elem<OK, W>(A.ac, A.oc, sum[k], p1, m1, v1);
                        const long ek = g.toff + tk;
                        A.p[ek] = p1;
                        if constexpr (HAS_M) A.m[ek] = m1;
                        if constexpr (HAS_V) A.v[ek] = v1;
                    }
                    return;
                }
#endif
                if (tid < 64) {
                    const f32x4* l4 = reinterpret_cast<const f32x4*>(lds);
                    auto yf4 = [&](int q) -> f32x4 { return l4[(L_Y + q * 256) / 4 + tid]; };
                    const f32x4 sum = casc_run_macro<true>(
                        prog, 0, casc_values(l4[L_S / 4 + tid], A.R.info.need, A.R.info.lp), yf4);
                    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
                    f32x4 pp = l4[L_P / 4 + tid], mm = HAS_M ? l4[L_M / 4 + tid] : zero4,
                          vv = HAS_V ? l4[L_V / 4 + tid] : zero4;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float p1 = pp[k], m1 = mm[k], v1 = vv[k];
                        opt_elem<OK, W>(A.ac, A.oc, sum[k], p1, m1, v1);
                        pp[k] = p1;
                        mm[k] = m1;
                        vv[k] = v1;
                    }
                    f32x4* w4 = reinterpret_cast<f32x4*>(lds);
                    w4[L_P / 4 + tid] = pp;
                    if constexpr (HAS_M) w4[L_M / 4 + tid] = mm;
                    if constexpr (HAS_V) w4[L_V / 4 + tid] = vv;
                }
                __syncthreads();
                if (valid) {
                    A.p[e] = lds[L_P + tid];
                    if constexpr (HAS_M) A.m[e] = lds[L_M + tid];
                    if constexpr (HAS_V) A.v[e] = lds[L_V + tid];
                }
                continue;
            }
        }
        if (!valid) continue;
        if (A.S_out && (INL || !ADAM)) A.S_out[e] = s;
        if constexpr (C && INL) {
            if (A.theta_out) A.theta_out[e] = p;
        }
        if constexpr (ADAM) {
            const float p0 = p;             // the pre-update p (C)
#pragma unroll
            for (int q = 0; q < NYR; ++q)
                if (q < nst) lds[L_Y + q * 256 + tid] = ys[q];
            auto yf = [&](int q) -> float {
                if (q < NYR) return lds[L_Y + q * 256 + tid];
                if (!A.R.arr[q]) return 0.f;
                if constexpr (C) {
                    float y = A.R.arr[q][e];
                    if (A.R.arr[STEP_SNAP0 + q])
                        y = compensate(y, p0, A.R.arr[STEP_SNAP0 + q][e], A.ac.lam);
                    return y * A.w[q];
                } else if constexpr (W) return A.R.arr[q][e] * A.w[q];
                else return A.R.arr[q][e];
            };
            const CascVals<float> cv = casc_values(s, A.R.info.need, A.R.info.lp);
            const bool tail = tl >= rule_body(g.numel, W);
            float sum = 0.f;
            if (!tail) sum = casc_run_macro(prog, 0, cv, yf);
            if (tail) sum = casc_run_macro(prog, A.R.info.tail_off, cv, yf);
            opt_elem<OK, W>(A.ac, A.oc, sum, p, m, v);
            A.p[e] = p;
            if constexpr (HAS_M) A.m[e] = m;
            if constexpr (HAS_V) A.v[e] = v;
        }
    }
}

template <bool ADAM, bool INL, int OK = OK_ADAM, bool W = false, bool C = false>
__global__ void __launch_bounds__(256) k_slab_step(StepArgs A) {
    static_assert((W && ADAM) || !C, "the compensated form is built on the weighted one");
    __shared__ float lds[L_Y + NYR * 256];
    slab_step_body<ADAM, INL, OK, W, C>(A, lds);
}

// General-order programs: the interpreter's chains of dependent adds want many resident waves to
// hide their latency, so this instantiation is held to SEQ_WAVES waves per SIMD (register budget)
#ifndef SEQ_WAVES
#define SEQ_WAVES 4
#endif
template <int OK = OK_ADAM, bool W = false, bool C = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SEQ_WAVES, 8)))
k_slab_step_seq(StepArgs A) {
    static_assert(W || !C, "the compensated form is built on the weighted one");
    __shared__ float lds[L_END];
    slab_step_body<true, false, OK, W, C>(A, lds);
}

// ================================================================================================
// host
// ================================================================================================
// rule()'s divisor in launch form: the entry count k (an integer below 2^24, exact in fp32) or a
// weighted rule's divisor, rounded to fp32 once
static int make_divisor(double divisor, AdamConst* ac) {
    FLSIM_REQUIRE(divisor > 0 && divisor < (double)(1 << 24), "divisor %g out of range", divisor);
    ac->fk = (float)divisor;                         // rule(): mean = sum / k
    FLSIM_REQUIRE(ac->fk > 0.f, "ZeroDivisionError: divisor %g rounds to 0 in fp32", divisor);
    {
        volatile float one = 1.f, fk = ac->fk;       // RN(1/k) in fp32, not via double
        ac->rk = one / fk;
    }
    return 0;
}

int make_adam_const(double divisor, long step, double lr, double beta1, double beta2, double eps,
                    AdamConst* ac) {
    RC(make_divisor(divisor, ac));
    FLSIM_REQUIRE(step >= 1, "step must be >= 1");
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    ac->w1 = (float)(1.0 - beta1);
    ac->b2 = (float)beta2;
    ac->w2 = (float)(1.0 - beta2);
    ac->bc2s = (float)sqrt(bc2);
    {
        volatile float one = 1.f, b = ac->bc2s;
        ac->rbc2s = one / b;
    }
    ac->eps = (float)eps;
    ac->neg_ss = (float)(-(lr / bc1));
    return 0;
}

int check_optim(const flsim_optim* o) {
    FLSIM_REQUIRE(o, "null optimizer");
    FLSIM_REQUIRE(o->kind == FLSIM_OPT_ADAM || o->kind == FLSIM_OPT_ADAMW ||
                  o->kind == FLSIM_OPT_SGD || o->kind == FLSIM_OPT_ADAGRAD ||
                  o->kind == FLSIM_OPT_YOGI, "unknown optimizer kind %d", o->kind);
    // negated comparisons: a NaN is refused too
    FLSIM_REQUIRE(o->lr >= 0.0, "Invalid learning rate: %g", o->lr);
    FLSIM_REQUIRE(o->weight_decay >= 0.0, "Invalid weight_decay value: %g", o->weight_decay);
    // (momentum, dampening and nesterov act for FLSIM_OPT_SGD only; they are checked for every kind)
    FLSIM_REQUIRE(o->momentum >= 0.0, "Invalid momentum value: %g", o->momentum);
    FLSIM_REQUIRE(!o->nesterov || (o->momentum > 0.0 && o->dampening == 0.0),
                  "Nesterov momentum requires a momentum and zero dampening");
    // the two kinds of Adaptive Federated Optimization (lr_decay is read for Adagrad only)
    if (o->kind == FLSIM_OPT_ADAGRAD)
        FLSIM_REQUIRE(o->lr_decay >= 0.0, "Invalid lr_decay value: %g", o->lr_decay);
    if (o->kind == FLSIM_OPT_ADAGRAD || o->kind == FLSIM_OPT_YOGI)
        FLSIM_REQUIRE(o->eps >= 0.0, "Invalid epsilon value: %g", o->eps);
    if (o->kind == FLSIM_OPT_YOGI) {
        FLSIM_REQUIRE(o->beta1 >= 0.0 && o->beta1 < 1.0, "Invalid beta parameter at index 0: %g",
                      o->beta1);
        FLSIM_REQUIRE(o->beta2 >= 0.0 && o->beta2 < 1.0, "Invalid beta parameter at index 1: %g",
                      o->beta2);
    }
    return 0;
}

// A weighted rule's weights and divisor (the cases where the rule text would divide by zero or
// average with a negative or non-finite weight); before any pointer check, like check_optim.
// Negated comparisons: a NaN is refused too.
int check_weights(const flsim_rule_weights* w) {
    if (!w) return 0;
    FLSIM_REQUIRE(w->n >= 0 && w->n <= RULE_MAX_ARR, "weights for %d arrays (max %d)", w->n,
                  RULE_MAX_ARR);
    for (int q = 0; q < w->n; ++q)
        FLSIM_REQUIRE(w->w[q] >= 0.0 && w->w[q] <= 3.0e38, "Invalid weight %g of array %d",
                      w->w[q], q);
    FLSIM_REQUIRE(w->divisor == w->divisor && w->divisor <= 3.0e38, "Invalid divisor %g",
                  w->divisor);
    FLSIM_REQUIRE(w->divisor > 0.0, "ZeroDivisionError: weighted rule divisor %g", w->divisor);
    return 0;
}

// the weights in launch form (fp32, rounded once) for a rule whose arrays they belong to; an
// array that is S_t itself (`alias`: the buffer S_t is read from or written to) must weigh 1.0:
// the cascade program's blocks of pure S_t entries stand for x added as it is
int make_weights(const flsim_rule* r, const flsim_rule_weights* w, const float* alias0,
                 const float* alias1, float* out, int cap) {
    FLSIM_REQUIRE(w->n == r->n_arrays, "weights for %d arrays, the rule has %d", w->n,
                  r->n_arrays);
    FLSIM_REQUIRE(w->n <= cap, "NotImplementedError: weighted rule with %d arrays in this step "
                  "(max %d)", w->n, cap);
    for (int q = 0; q < w->n; ++q) {
        const bool alias = r->arrays[q] && (r->arrays[q] == alias0 || r->arrays[q] == alias1);
        FLSIM_REQUIRE(!alias || w->w[q] == 1.0, "NotImplementedError: array %d is S_t itself, its "
                      "weight must be 1.0 (is %g)", q, w->w[q]);
        out[q] = (float)w->w[q];
    }
    return 0;
}

// Delay compensation's lambda and array count; before any pointer check, like check_weights.
// Negated comparisons: a NaN is refused too.
int check_comp(const flsim_rule_comp* c, const flsim_rule* r) {
    if (!c) return 0;
    FLSIM_REQUIRE(c->lambda >= 0.0 && c->lambda <= 3.0e38, "Invalid delay compensation lambda %g",
                  c->lambda);
    FLSIM_REQUIRE(r, "null rule");
    FLSIM_REQUIRE(c->n == r->n_arrays, "snapshots for %d arrays, the rule has %d", c->n,
                  r->n_arrays);
    return 0;
}

int make_comp(const flsim_rule* r, const flsim_rule_comp* comp, const float* S, const float* S_out,
              float* theta_out, const float* p, int cap, CompLaunch* out) {
    memset(out, 0, sizeof(*out));
    out->theta_out = theta_out;
    FLSIM_REQUIRE(((uintptr_t)theta_out & 15) == 0, "theta_out must be 16-byte aligned");
    FLSIM_REQUIRE(!theta_out || theta_out != p, "theta_out aliases p");
    if (!comp) return 0;
    out->lam = (float)comp->lambda;                  // rounded to fp32 once
    int n_comp = 0;
    for (int q = 0; q < comp->n; ++q) {
        const float* t = comp->theta_src[q];
        if (!t) continue;
        FLSIM_REQUIRE(((uintptr_t)t & 15) == 0, "snapshots must be 16-byte aligned");
        const bool alias = r->arrays[q] && (r->arrays[q] == S || r->arrays[q] == S_out);
        FLSIM_REQUIRE(!alias, "array %d is S_t itself: it takes no snapshot", q);
        FLSIM_REQUIRE(t != theta_out, "theta_out aliases the snapshot of array %d", q);
        out->snap[q] = t;
        ++n_comp;
        bool seen = false;
        for (int s = 0; s < q && !seen; ++s) seen = comp->theta_src[s] == t;
        out->nsnap += !seen;
    }
    FLSIM_REQUIRE(n_comp <= cap, "NotImplementedError: compensated rule with %d snapshots in this "
                  "step (max %d)", n_comp, cap);
    return 0;
}

int make_opt_launch(const flsim_optim* o, double divisor, long step, OptLaunch* ol) {
    RC(check_optim(o));
    memset(ol, 0, sizeof(*ol));
    if (o->kind == FLSIM_OPT_SGD) {
        RC(make_divisor(divisor, &ol->ac));
        FLSIM_REQUIRE(step >= 1, "step must be >= 1");
        ol->ok = o->momentum != 0.0 ? OK_SGDM : OK_SGD;
        ol->oc.wd = (float)o->weight_decay;
        ol->oc.mu = (float)o->momentum;
        ol->oc.omd = (float)(1.0 - o->dampening);
        ol->oc.neg_lr = (float)(-o->lr);
        ol->oc.flags = (o->weight_decay != 0.0 ? OF_WD : 0) | (o->nesterov ? OF_NESTEROV : 0) |
                       (step == 1 ? OF_FIRST : 0);
        return 0;
    }
    if (o->kind == FLSIM_OPT_ADAGRAD || o->kind == FLSIM_OPT_YOGI) {
        // the constants ride in fields the argument blocks already carry (slabstep.h), each
        // formed in double and rounded to fp32 once
        RC(make_divisor(divisor, &ol->ac));
        FLSIM_REQUIRE(step >= 1, "step must be >= 1");
        ol->ac.eps = (float)o->eps;
        ol->oc.wd = (float)o->weight_decay;
        ol->oc.flags = o->weight_decay != 0.0 ? OF_WD : 0;
        if (o->kind == FLSIM_OPT_ADAGRAD) {
            ol->ok = OK_ADAGRAD;
            ol->oc.neg_lr = (float)(-(o->lr / (1.0 + (double)(step - 1) * o->lr_decay)));
        } else {
            ol->ok = OK_YOGI;
            ol->ac.w1 = (float)(1.0 - o->beta1);
            ol->ac.w2 = (float)(1.0 - o->beta2);     // the device negates it (exact)
            ol->oc.neg_lr = (float)(-o->lr);
        }
        return 0;
    }
    RC(make_adam_const(divisor, step, o->lr, o->beta1, o->beta2, o->eps, &ol->ac));
    // no decay: the Adam kernels as they were (AdamW's p * f32(1 - lr * 0) = p exactly)
    ol->ok = o->weight_decay != 0.0 ? OK_ADAMD : OK_ADAM;
    if (o->kind == FLSIM_OPT_ADAMW) {
        ol->oc.wd = (float)(1.0 - o->lr * o->weight_decay);
        ol->oc.flags = OF_DECOUPLED | OF_WD;
    } else {
        ol->oc.wd = (float)o->weight_decay;
        ol->oc.flags = OF_WD;
    }
    return 0;
}

int make_rule(const flsim_rule* r, RuleProg* R) {
    FLSIM_REQUIRE(r, "null rule");
    FLSIM_REQUIRE(r->n_arrays >= 0 && r->n_arrays <= RULE_MAX_ARR, "n_arrays = %d (max %d)",
                  r->n_arrays, RULE_MAX_ARR);
    memset(R, 0, sizeof(*R));
    R->narr = r->n_arrays;
    int distinct = 0;
    for (int q = 0; q < r->n_arrays; ++q) {
        R->arr[q] = r->arrays[q];
        bool seen = r->arrays[q] == nullptr;
        for (int s = 0; s < q && !seen; ++s) seen = r->arrays[s] == r->arrays[q];
        distinct += !seen;
    }
    R->distinct = distinct;
    if (r->prog == nullptr) {
        // reference order: [S] * c + arrays in order (main.py:161-172: the slow worker is last)
        FLSIM_REQUIRE(r->c >= 0 && r->c + r->n_arrays > 0,
                      "empty weight_ups (reference: IndexError in rule, main.py:25)");
        const int k = r->c + r->n_arrays;
        int32_t pos[RULE_MAX_ARR], arr[RULE_MAX_ARR];
        for (int q = 0; q < r->n_arrays; ++q) {
            pos[q] = r->c + q;
            arr[q] = q;
        }
        int32_t ops[RULE_INL_PROG];
        CascInfo oi;
        int len = build_cascade_program(k, pos, arr, r->n_arrays, ops, RULE_INL_PROG, &oi);
        FLSIM_REQUIRE(len > 0, "rule program for k = %d entries failed (%d)", k, len);
        len = build_macro_program(ops, oi, reinterpret_cast<uint32_t*>(R->iprog),
                                  RULE_INL_PROG / 2, &R->info);
        FLSIM_REQUIRE(len > 0, "rule macro program for k = %d entries failed (%d)", k, len);
        R->prog = nullptr;
    } else {
        R->prog = r->prog;
        R->info = CascInfo{r->info[0], r->info[1], r->info[2], r->info[3]};
        FLSIM_REQUIRE(R->info.len > 0 && R->info.tail_off > 0 && R->info.tail_off < R->info.len &&
                      R->info.lp >= 4, "bad program info");
    }
    return 0;
}

int slab_step_launch(float* gradstate, const StepPlan& plan, long cnt_off, long part_off,
                     float* S_out, const RuleProg* rule, const AdamConst* ac, float* p, float* m,
                     float* v, long P, hipStream_t stream) {
    OptLaunch ol{};
    ol.ok = OK_ADAM;
    if (rule) {
        FLSIM_REQUIRE(ac, "null pointer");
        ol.ac = *ac;
    }
    return slab_step_launch_optim(gradstate, plan, cnt_off, part_off, S_out, rule, ol, p, m, v, P,
                                  stream);
}

// the fused step's two rule() + update launches of one kind
template <int OK, bool W, bool C>
static void launch_slab_rule(bool seq, unsigned nblk, hipStream_t stream, const ProbeSlot& ps,
                             const StepArgs& A) {
    if (!seq)
        hipExtLaunchKernelGGL((k_slab_step<true, true, OK, W, C>), dim3(nblk), dim3(256), 0, stream,
                              ps.start, ps.stop, 0, A);
    else
        hipExtLaunchKernelGGL((k_slab_step_seq<OK, W, C>), dim3(nblk), dim3(256), 0, stream,
                              ps.start, ps.stop, 0, A);
}

// The two dispatches from a runtime value to a template argument.  f is a generic lambda called
// with a std::integral_constant; `decltype(x)::value` is the constant.
// with_kind: the update kind.  GOUT says whether the site has an OK_GOUT instantiation; a site
// without one takes OK_SGD for it, like any value that is no case.
template <int K>
using IntC = std::integral_constant<int, K>;

template <bool GOUT, class F>
static void with_kind(int ok, F&& f) {
    switch (ok) {
        case OK_ADAM: f(IntC<OK_ADAM>{}); break;
        case OK_ADAMD: f(IntC<OK_ADAMD>{}); break;
        case OK_SGDM: f(IntC<OK_SGDM>{}); break;
        case OK_ADAGRAD: f(IntC<OK_ADAGRAD>{}); break;
        case OK_YOGI: f(IntC<OK_YOGI>{}); break;
        case OK_GOUT:
            if constexpr (GOUT) {
                f(IntC<OK_GOUT>{});
                break;
            }
            [[fallthrough]];
        default: f(IntC<OK_SGD>{}); break;
    }
}

// with_kpad: a padded entry count, a power of two from KMIN to 64 (anything else takes 64)
template <int KMIN, class F>
static void with_kpad(int kpad, F&& f) {
    if constexpr (KMIN < 64) {
        if (kpad == KMIN) f(IntC<KMIN>{});
        else with_kpad<2 * KMIN>(kpad, f);
    } else {
        f(IntC<64>{});
    }
}

template <bool W, bool C = false>
static void launch_slab_kind(int ok, bool seq, unsigned nblk, hipStream_t stream,
                             const ProbeSlot& ps, const StepArgs& A) {
    with_kind<false>(ok, [&](auto k) {
        launch_slab_rule<decltype(k)::value, W, C>(seq, nblk, stream, ps, A);
    });
}

int slab_step_launch_optim(float* gradstate, const StepPlan& plan, long cnt_off, long part_off,
                           float* S_out, const RuleProg* rule, const OptLaunch& ol, float* p,
                           float* m, float* v, long P, hipStream_t stream, const float* weights,
                           const CompLaunch* comp) {
    const int nstate = opt_n_state(ol.ok);
    StepArgs A{};
    A.base = gradstate;
    A.cnt_off = cnt_off;
    A.part_off = part_off;
    A.S_out = S_out;
    A.p = p;
    A.m = m;
    A.v = v;
    A.nseg = plan.nseg;
    A.units = plan.units;
    for (int i = 0; i < plan.nseg; ++i) A.seg[i] = plan.seg[i];
    if (rule) {
        FLSIM_REQUIRE(p && (m || nstate < 1) && (v || nstate < 2), "null pointer");
        A.R = *rule;
        A.ac = ol.ac;
        A.oc = ol.oc;
        if (weights) {
            FLSIM_REQUIRE(rule->narr <= STEP_MAX_WARR, "weighted rule with %d arrays", rule->narr);
            for (int q = 0; q < rule->narr; ++q) A.w[q] = weights[q];
        }
        if (comp) {
            FLSIM_REQUIRE(weights, "the compensated step is built on the weighted one");
            A.ac.lam = comp->lam;
            A.theta_out = comp->theta_out;
            for (int q = 0; q < rule->narr; ++q) A.R.arr[STEP_SNAP0 + q] = comp->snap[q];
        }
    }
    // FLSIM_STEP_UNITS="lo,hi" (measurement only): run units [lo, hi) of the plan -- whole
    // segments, so every split tile completes and resets its counter
    A.u_lo = 0;
    int u_hi = plan.units;
    // general order only: interleave the wide and conv units (measured: reference order and
    // reduce-only steps are faster in plan order, profiles/r02f/step_bench_*.txt)
    A.il_lo = plan.u_wide;
    A.il_w = plan.u_conv - plan.u_wide;
    A.il_n = (rule && rule->prog != nullptr) ? plan.units - plan.u_wide : 0;
    if (const char* env = lab_env("FLSIM_STEP_UNITS")) {
        int lo = 0, hi = 0;
        if (sscanf(env, "%d,%d", &lo, &hi) == 2 && 0 <= lo && lo < hi && hi <= plan.units) {
            A.u_lo = lo;
            u_hi = hi;
            A.il_n = 0;             // measurement of a unit range: plan order, no interleave
        }
    }
    if (const char* env = lab_env("FLSIM_STEP_NO_INTERLEAVE"))
        if (atoi(env)) A.il_n = 0;
    const unsigned nblk = (unsigned)(u_hi - A.u_lo);
    // algorithmic HBM bytes: every slab byte once; S_out written; p and the kind's state arrays
    // (m, v: 2, 1 or 0 of them) read + written; each distinct entry array read once
    double slab_read = 0.0;
    for (int i = 0; i < plan.nseg; ++i)
        slab_read += (double)(plan.seg[i].zlim < plan.seg[i].Z ? plan.seg[i].zlim : plan.seg[i].Z) *
                     plan.seg[i].n;
    double bytes = 4.0 * slab_read + (S_out ? 4.0 * P : 0.0);
    if (rule) bytes += 4.0 * (double)P * (2 + 2 * nstate + rule->distinct);
    // ... each distinct snapshot read once, theta_out written
    if (rule && comp) bytes += 4.0 * (double)P * (comp->nsnap + (comp->theta_out ? 1 : 0));
    const ProbeSlot ps = probe_begin();
    if (!rule) {
        hipExtLaunchKernelGGL(k_slab_step<false, true>, dim3(nblk), dim3(256), 0, stream, ps.start,
                              ps.stop, 0, A);
    } else {
        const bool seq = rule->prog != nullptr;
        if (seq) RC(stage_program(*rule, stream));
        if (comp) launch_slab_kind<true, true>(ol.ok, seq, nblk, stream, ps, A);
        else if (weights) launch_slab_kind<true>(ol.ok, seq, nblk, stream, ps, A);
        else launch_slab_kind<false>(ol.ok, seq, nblk, stream, ps, A);
    }
    FLSIM_LAUNCH_CHECK();
    const int kid = !rule ? K_SLABSUM : (rule->prog == nullptr ? K_STEP : K_STEP_SEQ);
    return probe_end(ps, kid, bytes);
}

// the streaming launch of one kind: the register-array form (reference order, <= 2 entry arrays,
// G groups per thread) or the LDS-staged one (inline or staged program)
template <int OK, bool W, bool C>
static void launch_agg(bool reg, int G, dim3 grid, hipStream_t stream, const ProbeSlot& ps,
                       const AggArgs& A) {
    if (reg) {
        auto k = G == 2 ? (A.R.narr == 0 ? k_agg_stream_reg<2, 0, OK, W, C>
                           : A.R.narr == 1 ? k_agg_stream_reg<2, 1, OK, W, C>
                                           : k_agg_stream_reg<2, 2, OK, W, C>)
                        : (A.R.narr == 0 ? k_agg_stream_reg<1, 0, OK, W, C>
                           : A.R.narr == 1 ? k_agg_stream_reg<1, 1, OK, W, C>
                                           : k_agg_stream_reg<1, 2, OK, W, C>);
        hipExtLaunchKernelGGL(k, grid, dim3(256), 0, stream, ps.start, ps.stop, 0, A);
    } else if (A.R.prog == nullptr)
        hipExtLaunchKernelGGL((k_agg_stream<true, OK, W, C>), grid, dim3(256), 0, stream, ps.start,
                              ps.stop, 0, A);
    else
        hipExtLaunchKernelGGL((k_agg_stream<false, OK, W, C>), grid, dim3(256), 0, stream,
                              ps.start, ps.stop, 0, A);
}

template <bool W, bool C = false>
static void launch_agg_kind(int ok, bool reg, int G, dim3 grid, hipStream_t stream,
                            const ProbeSlot& ps, const AggArgs& A) {
    with_kind<true>(ok, [&](auto k) {
        launch_agg<decltype(k)::value, W, C>(reg, G, grid, stream, ps, A);
    });
}

// Clipping's max_norm (the values for which torch's clip would flip or zero the gradient, or
// turn it into NaN); before any pointer check, like check_optim.  Negated: a NaN is refused too.
static int check_clip(const flsim_clip* c) {
    if (!c) return 0;
    FLSIM_REQUIRE(c->max_norm > 0.f, "Invalid clipping max_norm %g: it must be > 0",
                  (double)c->max_norm);
    return 0;
}

// [a, a + na) and [b, b + nb) bytes share a byte; [a, a + n) and [b, b + n) floats share an element
static bool overlaps(const void* a, long na, const void* b, long nb) {
    return a && b && (uintptr_t)a < (uintptr_t)b + (uintptr_t)nb &&
           (uintptr_t)b < (uintptr_t)a + (uintptr_t)na;
}
static bool overlaps(const float* a, const float* b, long n) { return overlaps(a, 4 * n, b, 4 * n); }

// the clipped step's second and third launches
static int clip_finish_apply(const flsim_clip* clip, long n_part, const OptLaunch& ol, float* p,
                             float* m, float* v, long P, hipStream_t stream) {
    {
        const ProbeSlot ps = probe_begin();
        hipExtLaunchKernelGGL(k_clip_finish, dim3(1), dim3(256), 0, stream, ps.start, ps.stop, 0,
                              (const double*)clip->partials, n_part, clip->max_norm, clip->out);
        FLSIM_LAUNCH_CHECK();
        if (probe_end(ps, K_CLIP_FIN, 8.0 * (double)n_part + 8.0)) return 2;
    }
    ClipApplyArgs A{};
    A.G = clip->G;
    A.coef = clip->out + 1;
    A.p = p;
    A.m = m;
    A.v = v;
    A.P = P;
    A.ac = ol.ac;
    A.oc = ol.oc;
    const dim3 grid((unsigned)((P + 1023) / 1024));
    const ProbeSlot ps = probe_begin();
    with_kind<false>(ol.ok, [&](auto k) {
        hipExtLaunchKernelGGL(k_clip_apply<decltype(k)::value>, grid, dim3(256), 0, stream,
                              ps.start, ps.stop, 0, A);
    });
    FLSIM_LAUNCH_CHECK();
    // algorithmic HBM bytes: G read; p and the kind's state arrays read + written
    return probe_end(ps, K_CLIP_APPLY, 4.0 * (double)P * (3 + 2 * opt_n_state(ol.ok)));
}

// ================================================================================================
// What the rules over bucket means share (k_robust, Krum, the geometric median, centered clipping):
// the entry table, the apply kernels' outputs and their per-element head and tail
// ================================================================================================
struct EntryTable {
    const float* ent[RULE_MAX_ARR];     // bucket / class sums; nullptr = an all-zero entry
    float cnt[RULE_MAX_ARR];            // (float)count[j] and RN(1 / that): x_j = ent[j][e] / cnt[j]
    float rcnt[RULE_MAX_ARR];
};

struct ApplyOut {
    float* g_out;                       // nullable: g is also written here
    float* G;                           // OK_GOUT, nullable: the clipped step's G
    double* partials;                   // OK_GOUT, nullable: block b's sum of g * g (fp64)
    float* p;
    float* m;
    float* v;
    long P;
    AdamConst ac;
    OptConst oc;
};

// One element of an apply kernel (one thread owns one element; 256 threads per block).
// begin(): the index and `live`; false when the thread has nothing to do.  load_state(): p and the
// m / v the kind owns.  finish(): g goes to g_out, then the update of kind OK and its stores.
// OK_GOUT has no update: g goes to g_out and / or G, and with `partials` every thread of the block
// stays for the block's fp64 sum of squares (one out of range adds 0).
template <int OK>
struct ApplyElem {
    static constexpr bool HAS_M = opt_n_state(OK) >= 1, HAS_V = opt_n_state(OK) == 2;
    long e;
    bool live;
    float p = 0.f, m = 0.f, v = 0.f;

    __device__ __forceinline__ bool begin(const ApplyOut& O) {
        e = (long)blockIdx.x * 256 + threadIdx.x;
        live = e < O.P;
        return OK == OK_GOUT || live;
    }
    __device__ __forceinline__ void load_state(const ApplyOut& O) {
        if constexpr (OK != OK_GOUT) p = __builtin_nontemporal_load(O.p + e);
        if constexpr (HAS_M) m = __builtin_nontemporal_load(O.m + e);
        if constexpr (HAS_V) v = __builtin_nontemporal_load(O.v + e);
    }
    __device__ __forceinline__ void finish(const ApplyOut& O, float g) {
        if constexpr (OK == OK_GOUT) {
            if (live) {
                if (O.g_out) __builtin_nontemporal_store(g, O.g_out + e);
                if (O.G) __builtin_nontemporal_store(g, O.G + e);
            }
            if (O.partials) {
                __shared__ double red[4];
                const double s = block_sum_f64(live ? (double)g * (double)g : 0.0, red);
                if (threadIdx.x == 0) O.partials[blockIdx.x] = s;
            }
        } else {
            if (O.g_out) __builtin_nontemporal_store(g, O.g_out + e);
            opt_update<OK>(O.ac, O.oc, g, p, m, v);
            __builtin_nontemporal_store(p, O.p + e);
            if constexpr (HAS_M) __builtin_nontemporal_store(m, O.m + e);
            if constexpr (HAS_V) __builtin_nontemporal_store(v, O.v + e);
        }
    }
};

// the entry counts (the end of every bucketed rule's hyper-parameter check)
static int check_counts(const int32_t* count, int k) {
    for (int j = 0; j < k; ++j)
        FLSIM_REQUIRE(count[j] >= 1, "Invalid count %d of entry %d: it must be >= 1", count[j], j);
    return 0;
}

// a bucket mean on the host twins: one fp32 division (volatile: one rounding whatever the flags); a
// null entry is all zero
static float bucket_mean(const float* const* entries, const int32_t* count, int j, long e) {
    volatile float x = entries[j] ? entries[j][e] : 0.f;
    volatile float c = (float)count[j];
    return x / c;
}

// ---- the host side of a bucketed step: the stages the four entry points run, in this order ------
// (after the rule's own hyper-parameter check; a rule's checks of its center and of its scratch
// pointers come between step_begin and check_scratch)
// what the entries and the scratch are checked against (check_scratch, fill_entries); a call with
// no p / m / v / clip (NNM) has P alone: StepBuffers{} and P
struct StepBuffers {
    const float* outs[4];               // p, m, v, g_out
    const flsim_clip* clip;
    long P, nblk;                       // nblk: the apply launch's blocks = the clip partials
};

struct BucketStep : StepBuffers {
    OptLaunch ol;                       // OK_GOUT without an optimizer
    int nstate;
    float *g_out, *p, *m, *v;           // p / m / v: null where the kind does not own them
};

struct Span {                           // a scratch buffer
    const void* ptr;
    long bytes;
};

// a bucketed call's scratch pointers, before check_scratch: sc[0] is the partials, n_partials
// doubles of which this step writes n_dist (a null scratch struct: the caller passes an empty one)
static int check_scratch_pointers(const char* name, const Span* sc, int ns, long n_partials,
                                  long n_dist) {
    uintptr_t all = 0;
    for (int a = 0; a < ns; ++a) {
        FLSIM_REQUIRE(sc[a].ptr, "null %s scratch", name);
        all |= (uintptr_t)sc[a].ptr;
    }
    FLSIM_REQUIRE((all & 15) == 0, "%s scratch must be 16-byte aligned", name);
    FLSIM_REQUIRE(n_partials >= n_dist, "%s n_partials = %ld, this step writes %ld", name,
                  n_partials, n_dist);
    return 0;
}

// the optimizer's and the clip's hyper-parameters (before any pointer), then p / m / v / g_out / P
static int step_begin(const flsim_optim* optim, const flsim_clip* clip, float* g_out, float* p,
                      float* m, float* v, long P, long step, BucketStep* B) {
    if (optim) RC(check_optim(optim));
    RC(check_clip(clip));
    FLSIM_REQUIRE(optim || (g_out && !clip), "null optimizer (only a step that writes g_out alone, "
                  "unclipped, takes none)");
    B->ol = OptLaunch{};
    B->ol.ok = OK_GOUT;
    int nstate = 0;
    if (optim) {
        nstate = optim_n_state(optim);
        RC(make_opt_launch(optim, 1.0, step, &B->ol));
        FLSIM_REQUIRE(p && (m || nstate < 1) && (v || nstate < 2), "null pointer");
    } else {
        p = nullptr;
    }
    if (nstate < 2) v = nullptr;
    if (nstate < 1) m = nullptr;
    FLSIM_REQUIRE(P > 0 && P < (1L << 31), "P = %ld out of range", P);
    FLSIM_REQUIRE((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g_out) & 15) == 0,
                  "p/m/v/g_out must be 16-byte aligned");
    const float* const outs[] = {p, m, v, g_out};
    for (int a = 0; a < 4; ++a) {
        for (int b = a + 1; b < 4; ++b)
            FLSIM_REQUIRE(!overlaps(outs[a], outs[b], P), "p/m/v/g_out overlap each other");
        B->outs[a] = outs[a];
    }
    B->nstate = nstate;
    B->g_out = g_out;
    B->p = p;
    B->m = m;
    B->v = v;
    B->clip = clip;
    B->P = P;
    B->nblk = (P + 255) / 256;
    return 0;
}

// the rule's scratch buffers against each other, the outputs, clip G and the rule's center
// (nullable); `name` is the rule's in the messages; a buffer of no bytes overlaps nothing
static int check_scratch(const StepBuffers& B, const char* name, const Span* sc, int ns,
                         const float* center) {
    for (int a = 0; a < ns; ++a) {
        if (!sc[a].bytes) continue;
        for (int b = a + 1; b < ns; ++b)
            FLSIM_REQUIRE(!sc[b].bytes ||
                          !overlaps(sc[a].ptr, sc[a].bytes, sc[b].ptr, sc[b].bytes),
                          "%s scratch buffers overlap each other", name);
        for (const float* o : B.outs)
            FLSIM_REQUIRE(!overlaps(sc[a].ptr, sc[a].bytes, o, 4 * B.P),
                          "%s scratch overlaps p/m/v/g_out", name);
        FLSIM_REQUIRE(!B.clip || !overlaps(sc[a].ptr, sc[a].bytes, B.clip->G, 4 * B.P),
                      "%s scratch overlaps clip G", name);
        FLSIM_REQUIRE(!overlaps(sc[a].ptr, sc[a].bytes, center, 4 * B.P),
                      "%s center overlaps the %s scratch", name, name);
    }
    return 0;
}

// the clip buffers (center: centered clipping's, nullable)
static int check_clip_buffers(const StepBuffers& B, const float* center) {
    const flsim_clip* clip = B.clip;
    if (!clip) return 0;
    FLSIM_REQUIRE(clip->G && clip->partials && clip->out, "null clip buffer");
    FLSIM_REQUIRE((((uintptr_t)clip->G | (uintptr_t)clip->partials | (uintptr_t)clip->out) & 15) ==
                  0, "clip G/partials/out must be 16-byte aligned");
    for (const float* o : B.outs)
        FLSIM_REQUIRE(!overlaps(clip->G, o, B.P), "clip G overlaps p/m/v/g_out");
    FLSIM_REQUIRE(!overlaps(clip->G, center, B.P), "centered-clipping center overlaps clip G");
    return 0;
}

// the entries: their alignment and their overlap with the outputs, clip G, the scratch (sc
// nullable) and the center (nullable); fills T; *distinct: the entry arrays read (not NULL, each
// counted once).  Then the size of the clip partials, the last check before the first launch.
static int fill_entries(const StepBuffers& B, const float* const* entries, const int32_t* count,
                        int k, const char* name, const Span* sc, int ns, const float* center,
                        EntryTable* T, int* distinct) {
    *distinct = 0;
    for (int j = 0; j < k; ++j) {
        const float* e = entries[j];
        FLSIM_REQUIRE(((uintptr_t)e & 3) == 0, "entry %d must be 4-byte aligned", j);
        for (const float* o : B.outs)
            FLSIM_REQUIRE(!overlaps(e, o, B.P), "entry %d overlaps p/m/v/g_out", j);
        FLSIM_REQUIRE(!B.clip || !overlaps(e, B.clip->G, B.P), "entry %d overlaps clip G", j);
        for (int a = 0; a < ns; ++a)
            FLSIM_REQUIRE(!sc[a].bytes || !overlaps(e, 4 * B.P, sc[a].ptr, sc[a].bytes),
                          "entry %d overlaps the %s scratch", j, name);
        FLSIM_REQUIRE(!overlaps(e, center, B.P), "entry %d overlaps the %s center", j, name);
        volatile float one = 1.f, c = (float)count[j];    // RN(1 / count) in fp32
        T->ent[j] = e;
        T->cnt[j] = c;
        T->rcnt[j] = one / c;
        bool seen = e == nullptr;
        for (int q = 0; q < j && !seen; ++q) seen = entries[q] == e;
        *distinct += !seen;
    }
    FLSIM_REQUIRE(!B.clip || B.clip->n_partials >= B.nblk,
                  "clip n_partials = %ld, this step writes %ld", B.clip->n_partials, B.nblk);
    return 0;
}

// The apply launch (kernel id `kid`), then the clipped step's two: fills A.O, picks the launch's
// kind (OK_GOUT under clipping) and calls launch(kind constant, grid, probe slot).  `arrays`: the
// P-element arrays the rule itself reads and writes, for the probe's algorithmic HBM bytes; to
// them come g_out / G written, and p and the kind's state arrays read + written (not by a launch
// that only writes g).
template <class Args, class F>
static int launch_apply(const BucketStep& B, Args& A, int kid, int arrays, hipStream_t stream,
                        F&& launch) {
    const flsim_clip* clip = B.clip;
    A.O = ApplyOut{B.g_out, clip ? clip->G : nullptr, clip ? clip->partials : nullptr, B.p, B.m,
                   B.v, B.P, B.ol.ac, B.ol.oc};
    const int ok_launch = clip ? (int)OK_GOUT : B.ol.ok;
    const int nst_launch = ok_launch == OK_GOUT ? 0 : B.nstate;
    const double bytes = 4.0 * (double)B.P * (arrays + (B.g_out ? 1 : 0) + (clip ? 1 : 0) +
                                              (ok_launch == OK_GOUT ? 0 : 2 + 2 * nst_launch));
    const ProbeSlot ps = probe_begin();
    with_kind<true>(ok_launch, [&](auto ok) { launch(ok, dim3((unsigned)B.nblk), ps); });
    FLSIM_LAUNCH_CHECK();
    if (probe_end(ps, kid, bytes)) return 2;
    if (!clip) return 0;
    return clip_finish_apply(clip, B.nblk, B.ol, B.p, B.m, B.v, B.P, stream);
}

// ================================================================================================
// k_robust: coordinate-wise median / trimmed mean over k <= 64 bucket means + the update
// (include/flsim.h: flsim_robust; csrc/robust.h: the network and select / sum, shared with the host)
// ================================================================================================
struct RobustArgs {
    EntryTable T;
    ApplyOut O;
    int k, kind, trim;
    float fn;                           // (float)(k - 2 * trim): the trimmed mean's divisor
};
static_assert(sizeof(RobustArgs) <= 4096, "kernel argument block");

// One thread owns one element (a float4 group per thread was measured too, at k = 2 .. 16: it
// needs four times the registers and is slower at every k, profiles/robust/README.md).  All k loads
// of a thread are issued before any arithmetic, non-temporally (each byte is read once; a wave's
// load is one coalesced 256 B row); then p / m / v; then the k divisions, the keys, the network,
// select / sum and the update of kind OK.  KPAD is the network's size, not k: the runtime k, kind
// and trim are launch-uniform (scalar branches skip the loads past k).  OK_GOUT: ApplyElem.
template <int KPAD, int OK>
__global__ void __launch_bounds__(256) k_robust(RobustArgs A) {
    ApplyElem<OK> el;
    if (!el.begin(A.O)) return;
    const long e = el.e;
    float x[KPAD];
#pragma unroll
    for (int j = 0; j < KPAD; ++j)
        x[j] = (j < A.k && A.T.ent[j] && el.live) ? __builtin_nontemporal_load(A.T.ent[j] + e) : 0.f;
    el.load_state(A.O);
    uint32_t key[KPAD];
#pragma unroll
    for (int j = 0; j < KPAD; ++j)
        key[j] = j < A.k ? robust_key(div_const(x[j], A.T.cnt[j], A.T.rcnt[j])) : ROBUST_PAD;
    float g = robust_select<KPAD>(key, A.kind, A.trim, A.k);
    if (A.kind != FLSIM_ROBUST_MEDIAN) g = __fdiv_rn(g, A.fn);
    el.finish(A.O, g);
}

// flsim_robust's hyper-parameters; before any pointer check, like check_optim
static int check_robust(const flsim_robust* r) {
    FLSIM_REQUIRE(r, "null robust rule");
    FLSIM_REQUIRE(r->kind == FLSIM_ROBUST_MEDIAN || r->kind == FLSIM_ROBUST_TRIMMED_MEAN,
                  "unknown robust rule kind %d", r->kind);
    FLSIM_REQUIRE(r->k >= 1 && r->k <= RULE_MAX_ARR, "robust rule over k = %d entries (1 .. %d)",
                  r->k, RULE_MAX_ARR);
    FLSIM_REQUIRE(r->trim >= 0 && r->trim <= RULE_MAX_ARR && 2 * r->trim < r->k,
                  "Invalid trim %d for k = %d entries: 0 <= 2 * trim < k", r->trim, r->k);
    FLSIM_REQUIRE(r->kind != FLSIM_ROBUST_MEDIAN || r->trim == 0,
                  "the median takes no trim (trim = %d)", r->trim);
    return check_counts(r->count, r->k);
}

// the host twin's element: the same divisions, keys, network and select / sum as k_robust
template <int KPAD>
static void robust_eval_host(const flsim_robust* r, long P, float* g_out) {
    for (long e = 0; e < P; ++e) {
        uint32_t key[KPAD];
        for (int j = 0; j < KPAD; ++j) {
            if (j >= r->k) {
                key[j] = ROBUST_PAD;
                continue;
            }
            key[j] = robust_key(bucket_mean(r->entries, r->count, j, e));
        }
        float g = robust_select<KPAD>(key, r->kind, r->trim, r->k);
        if (r->kind != FLSIM_ROBUST_MEDIAN) {
            volatile float s = g, n = (float)(r->k - 2 * r->trim);
            g = s / n;
        }
        g_out[e] = g;
    }
}

// ================================================================================================
// Krum / Multi-Krum: all-pairs distances, score + selection, apply (include/flsim.h: flsim_krum;
// csrc/krum.h: the geometry and the score / selection code shared with the host)
// ================================================================================================
struct KrumDistArgs {
    EntryTable T;                       // x_j = ent[j][e] / cnt[j], as k_robust forms it
    double* partials;                  // [NPB * 16][grid]
    long P;
    int k;
    int ntiles;
};
static_assert(sizeof(KrumDistArgs) <= 4096, "kernel argument block");

template <int KPAD>
struct KrumGeom {
    static constexpr int NB = KPAD / 4, NPB = krum_npb(KPAD);
    static constexpr int E = krum_tile_elems(KPAD), Q = E / 4;      // Q: float4 groups per row
    // thread groups that split a tile's float4 groups; each holds one thread per 4 x 4 pair block
    static constexpr int G = KPAD == 64 ? 3 : 256 / NPB;
    static constexpr int NT = (G * NPB + 63) / 64 * 64;
    static constexpr int LOADS = (KPAD * Q + NT - 1) / NT;
    // row r of the tile starts at r * E + 4 * (r / 4) floats: the rows 4t of the 16 pair-block
    // columns then start in 16 different 16-byte slots of the 256-byte bank row, so the
    // ds_read_b128 of lanes that differ in their block column is conflict-free
    static constexpr int LDS_FLOATS = KPAD * E + KPAD;
    __host__ __device__ static constexpr int row(int r) { return r * E + 4 * (r >> 2); }
};

// One block stages a tile (E elements of all KPAD rows, the bucket means x = ent / cnt) in LDS:
// coalesced 16-byte non-temporal loads (scalar loads for an entry that is not 16-byte aligned and
// at the end of the array), one 16-byte LDS store each; the elements past P and the rows past k
// are zero, which adds nothing to any sum.  (Issuing the next tile's loads before the current
// tile is computed was measured and is slower at every k: profiles/krum/README.md.)  Thread (grp, pb) owns the 4 x 4 pairs of block pb and
// walks the float4 groups grp, grp + G, ...: eight 16-byte LDS reads give four elements of its
// eight rows, and every pair takes one fp64 subtract and one fp64 fma per element.  A block
// grid-strides over the tiles; at the end the groups are added by a fixed halving tree through
// LDS, and group 0 writes the block's NPB * 16 sums.
template <int KPAD>
__global__ void __launch_bounds__(KrumGeom<KPAD>::NT) k_krum_dist(KrumDistArgs A) {
    using Gm = KrumGeom<KPAD>;
    constexpr int E = Gm::E, Q = Gm::Q, G = Gm::G, NPB = Gm::NPB, NT = Gm::NT;
    __shared__ __attribute__((aligned(16))) float tile[Gm::LDS_FLOATS];
    // (a step of the tree has at most G / 2 writing groups)
    static_assert(sizeof(double) * 16 * (G / 2) * NPB <= sizeof(float) * Gm::LDS_FLOATS,
                  "the group tree's scratch fits the tile");
    const int t = threadIdx.x;
    const int grp = t / NPB, pb = t - grp * NPB;
    const bool worker = grp < G;
    int ti = 0, tj = pb;
    while (tj >= Gm::NB - ti) {
        tj -= Gm::NB - ti;
        ++ti;
    }
    tj += ti;
    for (int idx = A.k * Q + t; idx < KPAD * Q; idx += NT) {       // the rows past k: zero, once
        const int j = idx / Q, q = idx - j * Q;
        *reinterpret_cast<f32x4*>(&tile[Gm::row(j) + 4 * q]) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int tl = blockIdx.x; tl < A.ntiles; tl += gridDim.x) {
        const long e0 = (long)tl * E;
        __syncthreads();                    // the previous tile has been read by every thread
        f32x4 x[Gm::LOADS];
#pragma unroll
        for (int u = 0; u < Gm::LOADS; ++u) {
            const int idx = u * NT + t;
            x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx < A.k * Q) {
                const int j = idx / Q, q = idx - j * Q;
                const float* src = A.T.ent[j];
                const long e = e0 + 4 * q;
                if (src) {
                    if ((((uintptr_t)src & 15) == 0) && e + 4 <= A.P) {
                        x[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + e));
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (e + c < A.P) x[u][c] = __builtin_nontemporal_load(src + e + c);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < Gm::LOADS; ++u) {
            const int idx = u * NT + t;
            if (idx < A.k * Q) {
                const int j = idx / Q, q = idx - j * Q;
                const float c = A.T.cnt[j], rc = A.T.rcnt[j];
                f32x4 y;
#pragma unroll
                for (int w = 0; w < 4; ++w) y[w] = div_const(x[u][w], c, rc);
                *reinterpret_cast<f32x4*>(&tile[Gm::row(j) + 4 * q]) = y;
            }
        }
        __syncthreads();
        if (worker) {
            for (int q = grp; q < Q; q += G) {
                f32x4 xi[4], xj[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    xi[a] = *reinterpret_cast<const f32x4*>(&tile[Gm::row(4 * ti + a) + 4 * q]);
                    xj[a] = *reinterpret_cast<const f32x4*>(&tile[Gm::row(4 * tj + a) + 4 * q]);
                }
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    double di[4], dj[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        di[a] = (double)xi[a][w];
                        dj[a] = (double)xj[a][w];
                    }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const double d = di[a] - dj[b];
                            acc[a][b] = __builtin_fma(d, d, acc[a][b]);
                        }
                }
            }
        }
    }
    // the groups, by a halving tree in a fixed order: group g + s is added into group g
    double* red = reinterpret_cast<double*>(tile);
    int top = 1;
    while (top < G) top <<= 1;
    for (int s = top >> 1; s > 0; s >>= 1) {
        __syncthreads();
        if (worker && grp >= s && grp < 2 * s) {
            double* dst = red + ((grp - s) * NPB + pb) * 16;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) dst[a * 4 + b] = acc[a][b];
        }
        __syncthreads();
        if (worker && grp < s && grp + s < G) {
            const double* src = red + (grp * NPB + pb) * 16;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] += src[a * 4 + b];
        }
    }
    // slot-major, partials[slot][block]: the finish launch reads a pair's sums as one run
    if (grp == 0) {
        double* dst = A.partials + (long)pb * 16 * gridDim.x + blockIdx.x;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) dst[(long)(a * 4 + b) * gridDim.x] = acc[a][b];
    }
}

// The pairwise-distance stage's matrix, for one block of KRUM_FIN_THREADS = 16 waves (k_krum_finish,
// k_nnm_finish: the two rules read one matrix, bit for bit, because this is its only text).  Pair
// (i, j), i < j, belongs to one wave: lane l adds the partials of the blocks l, l + 64, ... in index
// order (coalesced: the partials are slot-major) and a butterfly adds the 64 lanes, as k_clip_finish
// and block_sum_f64 do -- a fixed order for a given (P, k).  A wave takes four pairs at a time and
// issues all their loads before any add.  A NaN sum becomes +inf, the value is mirrored, the
// diagonal is zero.  The matrix is left in sd ([k * k] of the caller's LDS, visible to the whole
// block on return) and stored to dist.
constexpr int KRUM_FIN_THREADS = 1024;

__device__ __forceinline__ void pair_matrix(const double* partials, int nblocks, int nb, int k,
                                            double* sd, double* dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int WAVES = KRUM_FIN_THREADS / 64;
    // every load of a pair is issued before the first add (the grid's cap bounds them: 12 a lane)
    constexpr int NLD = 12;
    static_assert(krum_max_blocks(4) <= 64 * NLD && krum_max_blocks(64) <= 64 * NLD, "NLD");
    auto lane_sum = [&](int idx) -> double {
        const int i = idx / k, j = idx - i * k;
        double a = 0.0;
        if (idx < k * k && i < j) {
            const double* src = partials + (long)krum_slot(i, j, nb) * nblocks;
            double x[NLD];
#pragma unroll
            for (int u = 0; u < NLD; ++u) x[u] = lane + 64 * u < nblocks ? src[lane + 64 * u] : 0.0;
#pragma unroll
            for (int u = 0; u < NLD; ++u) a = lane + 64 * u < nblocks ? a + x[u] : a;
        }
        return a;
    };
    auto store = [&](int idx, double a) {
        const int i = idx / k, j = idx - i * k;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0 && idx < k * k && i <= j) {
            a = a != a ? (double)__builtin_inff() : a;
            sd[i * k + j] = a;                  // (the diagonal: no partial was added, 0)
            sd[j * k + i] = a;
        }
    };
    for (int base = wave; base < k * k; base += 4 * WAVES) {
        double a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = lane_sum(base + u * WAVES);
#pragma unroll
        for (int u = 0; u < 4; ++u) store(base + u * WAVES, a[u]);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < k * k; idx += KRUM_FIN_THREADS) dist[idx] = sd[idx];
}

// pair_matrix, then csrc/krum.h's score / selection code on the matrix in LDS
__global__ void __launch_bounds__(KRUM_FIN_THREADS)
k_krum_finish(const double* partials, int nblocks, int nb, int k, int f, int m, double* dist,
              double* score, int32_t* sel) {
    __shared__ double sd[RULE_MAX_ARR * RULE_MAX_ARR];
    __shared__ double ss[RULE_MAX_ARR];
    __shared__ int32_t sr[RULE_MAX_ARR];
    pair_matrix(partials, nblocks, nb, k, sd, dist);
    krum_score_select(sd, ss, sr, sel, k, f, m, (int)threadIdx.x, KRUM_FIN_THREADS,
                      [] { __syncthreads(); });
    if ((int)threadIdx.x < k) score[threadIdx.x] = ss[threadIdx.x];
}

// the doubles k_krum_dist writes for (P, k): one run of NPB * 16 a block
static long pair_partials(long P, int k) {
    const int kpad = krum_kpad(k);
    return krum_blocks(P, kpad) * krum_npb(kpad) * 16;
}

// The pairwise-distance stage on `stream`: k_krum_dist over the table -> partials (probe id
// kid_dist; algorithmic HBM bytes: the `arrays` distinct entries read once), then the consumer's
// finish launch, finish(probe slot, partials, nblocks, nb), which is to call pair_matrix (probe id
// kid_fin; bytes: the pairs' partials read, dist and a [k] result written, and fin_bytes of its own).
template <class F>
static int launch_pair_dist(const EntryTable& T, double* partials, long P, int k, int kid_dist,
                            int arrays, int kid_fin, double fin_bytes, hipStream_t stream,
                            F&& finish) {
    const int kpad = krum_kpad(k);
    const long nblocks = krum_blocks(P, kpad);
    KrumDistArgs D{};
    D.T = T;
    D.partials = partials;
    D.P = P;
    D.k = k;
    D.ntiles = (int)krum_tiles(P, kpad);
    {
        const ProbeSlot ps = probe_begin();
        const dim3 grid((unsigned)nblocks);
        with_kpad<4>(kpad, [&](auto kp) {
            constexpr int KPAD = decltype(kp)::value;
            hipExtLaunchKernelGGL((k_krum_dist<KPAD>), grid, dim3(KrumGeom<KPAD>::NT), 0, stream,
                                  ps.start, ps.stop, 0, D);
        });
        FLSIM_LAUNCH_CHECK();
        if (probe_end(ps, kid_dist, 4.0 * (double)P * arrays)) return 2;
    }
    const ProbeSlot ps = probe_begin();
    finish(ps, (const double*)partials, (int)nblocks, kpad / 4);
    FLSIM_LAUNCH_CHECK();
    if (probe_end(ps, kid_fin, 8.0 * (double)nblocks * (k * (k - 1) / 2) + 8.0 * k * (k + 1) +
                                   fin_bytes))
        return 2;
    return 0;
}

// the stage's host twin: every distance as the fp64 sum of the squared fp64 differences of the
// means in element order (one fma each; a pair is computed once and mirrored), NaN -> +inf, a zero
// diagonal
template <class M>
static void pair_dist_host(M&& mean, int k, long P, double* dist) {
    for (int i = 0; i < k; ++i) {
        dist[(long)i * k + i] = 0.0;
        for (int j = i + 1; j < k; ++j) {
            double a = 0.0;
            for (long e = 0; e < P; ++e) {
                const double d = (double)mean(i, e) - (double)mean(j, e);
                a = __builtin_fma(d, d, a);
            }
            a = a != a ? (double)__builtin_inff() : a;
            dist[(long)i * k + j] = a;
            dist[(long)j * k + i] = a;
        }
    }
}

struct KrumApplyArgs {
    EntryTable T;
    ApplyOut O;
    const int32_t* sel;                 // [m] the selection k_krum_finish wrote (device memory)
    int nsel;
    float fm;                           // (float)m: the divisor of the selected entries' sum
};
static_assert(sizeof(KrumApplyArgs) <= 4096, "kernel argument block");

// One thread owns one element, as k_robust.  The selection is read from device memory; it is
// launch-uniform (readfirstlane: the entry pointer, its count and the reciprocal come from the
// kernel arguments by scalar loads).  Only the m selected entries are loaded, eight loads in flight;
// g = (x_sel0 + x_sel1 + ...) / (float)m: the divisions, sequential fp32 adds in index order and
// one IEEE division, as the text.  Then the update of kind OK, or OK_GOUT as k_robust.
template <int OK>
__global__ void __launch_bounds__(256) k_krum_apply(KrumApplyArgs A) {
    ApplyElem<OK> el;
    if (!el.begin(A.O)) return;
    el.load_state(A.O);
    const long e = el.e;
    const bool live = el.live;
    float acc = 0.f;
    for (int t0 = 0; t0 < A.nsel; t0 += 8) {
        float x[8], c[8], rc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            x[u] = 0.f;
            c[u] = 1.f;
            rc[u] = 1.f;
            if (t0 + u < A.nsel) {
                const int j = __builtin_amdgcn_readfirstlane(A.sel[t0 + u]) & (RULE_MAX_ARR - 1);
                const float* src = A.T.ent[j];
                c[u] = A.T.cnt[j];
                rc[u] = A.T.rcnt[j];
                if (src && live) x[u] = __builtin_nontemporal_load(src + e);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (t0 + u < A.nsel) {
                const float y = div_const(x[u], c[u], rc[u]);
                acc = (t0 + u == 0) ? y : acc + y;
            }
        }
    }
    el.finish(A.O, __fdiv_rn(acc, A.fm));
}

// flsim_krum's hyper-parameters; before any pointer check, like check_optim
static int check_krum(const flsim_krum* r) {
    FLSIM_REQUIRE(r, "null Krum rule");
    FLSIM_REQUIRE(r->k >= 3 && r->k <= RULE_MAX_ARR, "Krum over k = %d entries (3 .. %d)", r->k,
                  RULE_MAX_ARR);
    FLSIM_REQUIRE(r->f >= 0 && r->f <= RULE_MAX_ARR && r->k >= 2 * r->f + 3,
                  "Invalid f = %d for k = %d entries: f >= 0 and k >= 2 * f + 3", r->f, r->k);
    FLSIM_REQUIRE(r->m >= 1 && r->m <= r->k - r->f,
                  "Invalid m = %d for k = %d entries and f = %d: 1 <= m <= k - f", r->m, r->k,
                  r->f);
    return check_counts(r->count, r->k);
}

// ================================================================================================
// Bulyan: Krum's distance launch, the repeated selection, the window around the median over the
// selected entries (include/flsim.h: flsim_bulyan; csrc/bulyan.h: the selection and the window /
// sum code shared with the host)
// ================================================================================================
// pair_matrix (the pairwise-distance stage, Krum's matrix), then csrc/bulyan.h's selection on the
// matrix in LDS; order, the winning scores and the ascending selection go out at the end
__global__ void __launch_bounds__(KRUM_FIN_THREADS)
k_bulyan_finish(const double* partials, int nblocks, int nb, int k, int f, double* dist,
                double* score, int32_t* order, int32_t* sel) {
    __shared__ double sd[RULE_MAX_ARR * RULE_MAX_ARR];
    __shared__ double ss[RULE_MAX_ARR], sw[RULE_MAX_ARR];
    __shared__ int32_t so[RULE_MAX_ARR], sl[RULE_MAX_ARR];
    __shared__ uint8_t sn[RULE_MAX_ARR * RULE_MAX_ARR];
    pair_matrix(partials, nblocks, nb, k, sd, dist);
    bulyan_order(sd, sn, ss, sw, so, sl, k, f, (int)threadIdx.x, KRUM_FIN_THREADS,
                 [] { __syncthreads(); });
    __syncthreads();
    if ((int)threadIdx.x < k - 2 * f) {
        score[threadIdx.x] = sw[threadIdx.x];
        order[threadIdx.x] = so[threadIdx.x];
        sel[threadIdx.x] = sl[threadIdx.x];
    }
}

struct BulyanApplyArgs {
    EntryTable T;
    ApplyOut O;
    const int32_t* sel;                 // [theta] the selection k_bulyan_finish wrote (device memory)
    int theta, beta;
    float fbeta;                        // (float)beta: the divisor of the window's sum
};
static_assert(sizeof(BulyanApplyArgs) <= 4096, "kernel argument block");

// One thread owns one element, as k_robust.  The selection is read from device memory; it is
// launch-uniform (readfirstlane: the entry pointer, its count and the reciprocal come from the
// kernel arguments by scalar loads), as k_krum_apply reads it.  Only the theta selected entries are
// loaded, non-temporally, all of them before any arithmetic; then p / m / v; then the divisions,
// the keys, the network over KPAD = the padded theta, csrc/bulyan.h's window and sum, one IEEE
// division by (float)beta and the update of kind OK, or OK_GOUT as k_robust.
template <int KPAD, int OK>
__global__ void __launch_bounds__(256) k_bulyan_apply(BulyanApplyArgs A) {
    ApplyElem<OK> el;
    if (!el.begin(A.O)) return;
    const long e = el.e;
    float x[KPAD];
#pragma unroll
    for (int t = 0; t < KPAD; ++t) {
        x[t] = 0.f;
        if (t < A.theta) {
            const int j = __builtin_amdgcn_readfirstlane(A.sel[t]) & (RULE_MAX_ARR - 1);
            const float* src = A.T.ent[j];
            if (src && el.live) x[t] = __builtin_nontemporal_load(src + e);
        }
    }
    el.load_state(A.O);
    uint32_t key[KPAD];
#pragma unroll
    for (int t = 0; t < KPAD; ++t) {
        key[t] = ROBUST_PAD;
        if (t < A.theta) {
            const int j = __builtin_amdgcn_readfirstlane(A.sel[t]) & (RULE_MAX_ARR - 1);
            key[t] = robust_key(div_const(x[t], A.T.cnt[j], A.T.rcnt[j]));
        }
    }
    const float g = bulyan_window_sum<KPAD>(key, A.theta, A.beta);
    el.finish(A.O, __fdiv_rn(g, A.fbeta));
}

// flsim_bulyan's hyper-parameters; before any pointer check, like check_optim
static int check_bulyan(const flsim_bulyan* r) {
    FLSIM_REQUIRE(r, "null Bulyan rule");
    FLSIM_REQUIRE(r->k >= 3 && r->k <= RULE_MAX_ARR, "Bulyan over k = %d entries (3 .. %d)", r->k,
                  RULE_MAX_ARR);
    FLSIM_REQUIRE(r->f >= 0 && r->f <= RULE_MAX_ARR && r->k >= 4 * r->f + 3,
                  "Invalid f = %d for k = %d entries: f >= 0 and k >= 4 * f + 3", r->f, r->k);
    return check_counts(r->count, r->k);
}

// the host twin's elements: the same divisions, keys, network, window and sum as k_bulyan_apply
template <int KPAD>
static void bulyan_eval_host(const flsim_bulyan* r, const int32_t* sel, long P, float* g_out) {
    const int theta = r->k - 2 * r->f, beta = theta - 2 * r->f;
    for (long e = 0; e < P; ++e) {
        uint32_t key[KPAD];
        for (int t = 0; t < KPAD; ++t)
            key[t] = t < theta ? robust_key(bucket_mean(r->entries, r->count, sel[t], e))
                               : ROBUST_PAD;
        volatile float s = bulyan_window_sum<KPAD>(key, theta, beta), n = (float)beta;
        g_out[e] = s / n;
    }
}

// ================================================================================================
// Geometric median (RFA, smoothed Weiszfeld): distances to the iterate, the scalar step, apply
// (include/flsim.h: flsim_geomed; csrc/geomed.h: the geometry and the scalar code shared with the
// host)
// ================================================================================================
struct GeomedDistArgs {
    EntryTable T;                       // x_j = ent[j][e] / cnt[j], as k_robust forms it
    double w0[RULE_MAX_ARR];            // pair 0: w^(0) of "every entry alive" (the host's, fp64)
    const double* w;                    // later pairs: s->w, written by the finish launches
    const int32_t* state;               // later pairs: the dead flags [k], then the control words
    double* partials;                   // [k + 1][grid]
    long P;
    int k, ntiles, pair, iters;
};
static_assert(sizeof(GeomedDistArgs) <= 4096, "kernel argument block");

// Values an earlier launch wrote and this launch only reads, at launch-uniform addresses: through
// the constant address space they are scalar loads, like the kernel arguments (k_geomed_apply).
typedef const double __attribute__((address_space(4)))* GeomedConstF64;

// One streaming pass over the k entries for the iterate z of weights w: thread t of the block's
// 256 owns the elements u * 256 + t, u < U, of a tile (a wave's load is one coalesced 256-byte row;
// an entry need only be 4-byte aligned) and a block grid-strides over the tiles.  All k * U loads
// of a thread are issued before any arithmetic, non-temporally: each byte is read once.  Per
// element the bucket means x_j = ent / cnt (one fp32 division each, where it is loaded), then
// z = sum_j w_j * x_j: fp64, index order, one multiply and one add per term with contraction off,
// and ((double)x_j - z)^2 into the thread's k fp64 sums by one fma each.  z starts from +0.0 and
// a term of weight 0 (a dead entry: not loaded, x = 0) adds +-0: that differs from _wsum, which
// skips such a term and starts from the first one kept, in the sign of a zero z at most, which
// (x - z)^2 does not see.  The sums stay in registers over all the block's tiles; at the end each
// is added over the wave by a butterfly and over the four waves as (w0 + w1) + (w2 + w3), a fixed
// order, and written slot-major.
// The per-entry table (pointer, count, its reciprocal, weight: 384 words at KPAD = 64, more than
// the scalar registers hold) lives in LDS and is read by broadcast (all lanes one address), GRP
// entries at a time; a group wholly past k is skipped by a scalar branch, and inside a group
// nothing branches: an entry that is not loaded (NULL, dead, past k) reads the block's first loaded
// entry instead and an element past P reads element 0, and both are replaced by 0.
// PAIR0: the weights are the kernel arguments; every entry is loaded, and each thread notes in a
// 64-bit mask which entries held a NaN or an inf (OR-ed over the block into slot k): the finish
// launch finds the dead entries there.  (A second fp64 sum per entry for that would double the
// accumulators: 256 VGPRs at KPAD = 64.)
// Later pairs: iteration it = pair - redo; it == iters: one word is read and the block is out.  A
// dead entry is not loaded (its sum is ignored by the finish launch).
typedef const float __attribute__((address_space(1)))* GeomedGlobalF32;

// The distance kernels' table in LDS (k_geomed_dist, k_cclip_dist), written by wave 0 (lane j is
// entry j) and followed by the block's barrier: the address loaded for entry j (its own, or for an
// entry that is not loaded the first loaded one's), its weight weight(j), count and reciprocal,
// and the mask of the loaded entries, which is returned.  Unless PAIR0 an entry with dead[j] set
// is not loaded.
template <int KPAD, bool PAIR0, class WF>
__device__ __forceinline__ uint64_t dist_table(const EntryTable& T, int k, const int32_t* dead,
                                               WF&& weight, unsigned long long* s_ent, double* s_w,
                                               float* s_cnt, float* s_rcnt,
                                               unsigned long long* s_mask) {
    const int j = threadIdx.x;
    if (j < 64) {
        const float* src = nullptr;
        double w = 0.0;
        float c = 1.f, rc = 1.f;
        if (j < k) {
            src = T.ent[j];
            c = T.cnt[j];
            rc = T.rcnt[j];
            w = weight(j);
            if constexpr (!PAIR0) {
                if (dead[j]) src = nullptr;
            }
        }
        const unsigned long long ml = __ballot(src != nullptr);
        const int first = ml ? __builtin_ctzll(ml) : 0;
        const unsigned long long any = __shfl((unsigned long long)(uintptr_t)src, first, 64);
        if (j < KPAD) {
            s_ent[j] = src ? (unsigned long long)(uintptr_t)src : any;
            s_w[j] = w;
            s_cnt[j] = c;
            s_rcnt[j] = rc;
        }
        if (j == 0) *s_mask = ml;
    }
    __syncthreads();
    // launch-uniform: a scalar register pair, tested by scalar bit compares
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(*s_mask >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)*s_mask);
}

// The distance kernels' end: each of the thread's k sums is added over the wave by a butterfly
// and over the four waves as (w0 + w1) + (w2 + w3), a fixed order, and written slot-major; PAIR0:
// the threads' "held a NaN or an inf" masks are OR-ed over the block into slot k.
template <int KPAD, bool PAIR0>
__device__ __forceinline__ void dist_reduce(const double (&acc)[KPAD], uint32_t bad_lo,
                                            uint32_t bad_hi, int k, double* partials) {
    __shared__ double red[4][KPAD + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < KPAD; ++j) {
        if (j < k) {
            double a = acc[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            if (lane == 0) red[wave][j] = a;
        }
    }
    if constexpr (PAIR0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            bad_lo |= (uint32_t)__shfl_xor((int)bad_lo, o, 64);
            bad_hi |= (uint32_t)__shfl_xor((int)bad_hi, o, 64);
        }
        if (lane == 0)
            red[wave][KPAD] = __builtin_bit_cast(double, ((uint64_t)bad_hi << 32) | bad_lo);
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < k)
        partials[(long)t * gridDim.x + blockIdx.x] =
            (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    if constexpr (PAIR0) {
        if (t == 64) {
            uint64_t mk = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) mk |= __builtin_bit_cast(uint64_t, red[w][KPAD]);
            reinterpret_cast<uint64_t*>(partials)[(long)k * gridDim.x + blockIdx.x] = mk;
        }
    }
}

template <int KPAD, bool PAIR0>
__global__ void __launch_bounds__(256) k_geomed_dist(GeomedDistArgs A) {
#pragma clang fp contract(off)
    constexpr int U = geomed_unroll(KPAD), E = geomed_tile_elems(KPAD);
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    __shared__ unsigned long long s_ent[KPAD];  // the address loaded for entry j
    __shared__ double s_w[KPAD];
    __shared__ float s_cnt[KPAD], s_rcnt[KPAD];
    __shared__ unsigned long long s_mask;       // bit j: entry j is loaded
    int it = 0;
    if constexpr (!PAIR0) {
        it = A.pair - A.state[A.k + GEOMED_ST_REDO];
        if (it >= A.iters) return;
    }
    const uint64_t ld_mask = dist_table<KPAD, PAIR0>(
        A.T, A.k, A.state,
        [&](int j) {
            if constexpr (PAIR0) return A.w0[j];
            else return A.w[(long)it * A.k + j];
        },
        s_ent, s_w, s_cnt, s_rcnt, &s_mask);
    double acc[KPAD];
#pragma unroll
    for (int j = 0; j < KPAD; ++j) acc[j] = 0.0;
    uint32_t bad_lo = 0, bad_hi = 0;
    for (int tl = blockIdx.x; tl < A.ntiles; tl += gridDim.x) {
        // the table is read, and the mask and k tested, again in every tile: hoisted out of the
        // loop they would take some 400 registers
        asm volatile("" ::: "memory");
        int m_lo = (int)ld_mask, m_hi = (int)(ld_mask >> 32), k = A.k;
        asm volatile("" : "+v"(m_lo), "+v"(m_hi), "+v"(k));
        k = __builtin_amdgcn_readfirstlane(k);
        const uint64_t ldm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(m_hi) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane(m_lo);
        const long e0 = (long)tl * E + threadIdx.x;
        bool inb[U];
        long off[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            inb[u] = e0 + u * 256 < A.P;
            off[u] = inb[u] ? e0 + u * 256 : 0;
        }
        float x[U][KPAD];
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k && ldm != 0) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j) {
                    const GeomedGlobalF32 src = (GeomedGlobalF32)s_ent[j];
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        x[u][j] = __builtin_nontemporal_load(src + off[u]);
                }
            } else {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j)
#pragma unroll
                    for (int u = 0; u < U; ++u) x[u][j] = 0.f;
            }
        }
        double z[U];
#pragma unroll
        for (int u = 0; u < U; ++u) z[u] = 0.0;
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j) {
                    const float c = s_cnt[j], rc = s_rcnt[j];
                    const double w = s_w[j];
                    const bool ld = (ldm >> j) & 1;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float y = div_const((ld && inb[u]) ? x[u][j] : 0.f, c, rc);
                        x[u][j] = y;
                        if constexpr (PAIR0) {
                            const uint32_t nf =
                                !(fabsf(y) < __builtin_inff()) ? 1u << (j & 31) : 0u;
                            if (j < 32) bad_lo |= nf;
                            else bad_hi |= nf;
                        }
                        const double t = (double)y * w;
                        z[u] = z[u] + t;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) z[u] = inb[u] ? z[u] : 0.0;    // (past P: the sums gain 0)
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j)
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double d = (double)x[u][j] - z[u];
                        acc[j] = __builtin_fma(d, d, acc[j]);
                    }
            }
        }
    }
    dist_reduce<KPAD, PAIR0>(acc, bad_lo, bad_hi, A.k, A.partials);
}

struct GeomedFinArgs {
    int32_t count[RULE_MAX_ARR];
    const double* partials;             // [k + 1][nblocks]
    double* w;                          // s->w
    double* d2;                         // s->d2
    double* obj;                        // s->obj
    int32_t* state;                     // s->state
    double nu;
    int nblocks, k, pair, iters, weighted;
};

// The distance-to-iterate stage's two reductions, for one block of GEOMED_FIN_THREADS = 16 waves
// (k_geomed_finish, k_cclip_finish).  Both take the kernel's own argument struct (its partials,
// nblocks and k) by reference: with the three passed by value the compiler loads the arguments
// earlier and both kernels need 4 - 6 more SGPRs (profiles/pair_stage/README.md).
constexpr int GEOMED_FIN_THREADS = 1024;

// A.partials [k + 1][nblocks] -> sd[j], j < k.  Entry j's sum belongs to one wave: lane l adds the
// partials of the blocks l, l + 64, ... in index order (coalesced: the partials are slot-major) and
// a butterfly adds the 64 lanes, as pair_matrix does -- a fixed order for a given (P, k).  No
// barrier: the caller's next one publishes sd.
template <class Args>
__device__ __forceinline__ void entry_sums(const Args& A, double* sd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < A.k; j += GEOMED_FIN_THREADS / 64) {
        const double* src = A.partials + (long)j * A.nblocks;
        double a = 0.0;
#pragma unroll 8
        for (int b = lane; b < A.nblocks; b += 64) a += src[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) sd[j] = a;
    }
}

// pair 0: the OR of the blocks' NaN masks (row k of the partials) through smask[16]; thread t < k
// returns entry t's dead bit (t >= k: 0).  One barrier inside.
template <class Args>
__device__ __forceinline__ int32_t dead_mask(const Args& A, unsigned long long* smask) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, k = A.k;
    const unsigned long long* src =
        reinterpret_cast<const unsigned long long*>(A.partials) + (long)k * A.nblocks;
    unsigned long long mk = 0;
    for (int b = t; b < A.nblocks; b += GEOMED_FIN_THREADS) mk |= src[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mk |= __shfl_xor(mk, o, 64);
    if (lane == 0) smask[wave] = mk;
    __syncthreads();
    int32_t dead = 0;
    if (t < k) {
        unsigned long long all = 0;
        for (int w = 0; w < GEOMED_FIN_THREADS / 64; ++w) all |= smask[w];
        dead = (int32_t)((all >> t) & 1);
    }
    return dead;
}

// entry_sums; pair 0 also takes dead_mask, writes the dead flags and the control words, and w^(0)
// over the live entries (the host's, bit for bit, when none is dead); with a dead entry its
// distances are worthless (z was a NaN) and it stops there: "redo".  Then csrc/geomed.h's scalar
// code of one iteration on the sums in LDS, and d2, obj and the next w.
__global__ void __launch_bounds__(GEOMED_FIN_THREADS) k_geomed_finish(GeomedFinArgs A) {
    __shared__ double sd[RULE_MAX_ARR], sa[RULE_MAX_ARR], sw[RULE_MAX_ARR], sterm[RULE_MAX_ARR];
    __shared__ double ssum[2];
    __shared__ int32_t sdead[RULE_MAX_ARR];
    __shared__ unsigned long long smask[GEOMED_FIN_THREADS / 64];
    __shared__ int32_t sgo;
    const int t = threadIdx.x, k = A.k;
    int it = 0;
    if (A.pair > 0) {
        it = A.pair - A.state[k + GEOMED_ST_REDO];
        if (it >= A.iters) return;
    }
    entry_sums(A, sd);
    if (A.pair == 0) {
        const int32_t dead = dead_mask(A, smask);
        if (t < k) {
            sdead[t] = dead;
            A.state[t] = dead;
            sa[t] = geomed_alpha(A.weighted, A.count[t], dead);
        }
        __syncthreads();
        if (t == 0) {
            int nd = 0;
            for (int j = 0; j < k; ++j) nd += sdead[j];
            A.state[k + GEOMED_ST_REDO] = nd > 0;
            A.state[k + GEOMED_ST_NDEAD] = nd;
            for (int c = 2; c < GEOMED_ST_WORDS; ++c) A.state[k + c] = 0;
            ssum[0] = geomed_seqsum(sa, k);
            sgo = nd == 0 && A.iters > 0;
        }
        __syncthreads();
        if (t < k) A.w[t] = sa[t] / ssum[0];
        if (!sgo) return;
        __syncthreads();                // (ssum is rewritten below)
    } else {
        if (t < k) {
            const int32_t dead = A.state[t];
            sdead[t] = dead;
            sa[t] = geomed_alpha(A.weighted, A.count[t], dead);
        }
        __syncthreads();
    }
    geomed_iterate(sd, sa, sdead, k, A.nu, sterm, ssum, sw, t, GEOMED_FIN_THREADS,
                   [] { __syncthreads(); });
    if (t < k) {
        A.d2[(long)it * k + t] = sd[t];
        A.w[(long)(it + 1) * k + t] = sw[t];
    }
    if (t == 0) A.obj[it] = ssum[0];
}

struct GeomedApplyArgs {
    EntryTable T;
    ApplyOut O;
    const double* w;                    // w^(iters) (device memory, written by a finish launch)
    int k;
};
static_assert(sizeof(GeomedApplyArgs) <= 4096, "kernel argument block");

// One thread owns one element, as k_krum_apply.  The weights are launch-uniform scalar loads;
// an entry of weight 0 (a dead one) is not loaded, eight loads in flight.  z as _wsum forms it
// (k_geomed_dist), g = (float)z: one fp64 -> fp32 rounding.  Then the update of kind OK, or
// OK_GOUT.
// This kernel keeps its own copy of two shared pieces, both measured (profiles/bucket_step/
// README.md).  The head and tail are ApplyElem's, text for text: with ApplyElem the OK_GOUT
// instantiation is 1 us (2 %) slower at k = 9.  The loop over the entries is k_cclip_apply's,
// text for text: as a shared __forceinline__ function it costs both kernels 8 VGPRs and 14
// branches (the table then reaches the loop through a reference to the kernel argument).
template <int OK>
__global__ void __launch_bounds__(256) k_geomed_apply(GeomedApplyArgs A) {
#pragma clang fp contract(off)
    constexpr bool HAS_M = opt_n_state(OK) >= 1, HAS_V = opt_n_state(OK) == 2;
    const ApplyOut& O = A.O;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = e < O.P;
    if constexpr (OK != OK_GOUT) {
        if (!live) return;
    }
    float p = 0.f, m = 0.f, v = 0.f;
    if constexpr (OK != OK_GOUT) p = __builtin_nontemporal_load(O.p + e);
    if constexpr (HAS_M) m = __builtin_nontemporal_load(O.m + e);
    if constexpr (HAS_V) v = __builtin_nontemporal_load(O.v + e);
    GeomedConstF64 wdev = (GeomedConstF64)(uintptr_t)A.w;
    double z = 0.0;
    bool have = false;
    for (int j0 = 0; j0 < A.k; j0 += 8) {
        float x[8], c[8], rc[8];
        double w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            x[u] = 0.f;
            c[u] = 1.f;
            rc[u] = 1.f;
            w[u] = 0.0;
            if (j0 + u < A.k) {
                const int j = j0 + u;
                const float* src = A.T.ent[j];
                w[u] = wdev[j];
                c[u] = A.T.cnt[j];
                rc[u] = A.T.rcnt[j];
                if (geomed_nonzero(w[u]) && src && live) x[u] = __builtin_nontemporal_load(src + e);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (j0 + u < A.k && geomed_nonzero(w[u])) {
                const double t = (double)div_const(x[u], c[u], rc[u]) * w[u];
                z = have ? z + t : t;
                have = true;
            }
        }
    }
    const float g = (float)z;
    if constexpr (OK == OK_GOUT) {
        if (live) {
            if (O.g_out) __builtin_nontemporal_store(g, O.g_out + e);
            if (O.G) __builtin_nontemporal_store(g, O.G + e);
        }
        if (O.partials) {
            __shared__ double red[4];
            const double s = block_sum_f64(live ? (double)g * (double)g : 0.0, red);
            if (threadIdx.x == 0) O.partials[blockIdx.x] = s;
        }
    } else {
        if (O.g_out) __builtin_nontemporal_store(g, O.g_out + e);
        opt_update<OK>(O.ac, O.oc, g, p, m, v);
        __builtin_nontemporal_store(p, O.p + e);
        if constexpr (HAS_M) __builtin_nontemporal_store(m, O.m + e);
        if constexpr (HAS_V) __builtin_nontemporal_store(v, O.v + e);
    }
}

// flsim_geomed's hyper-parameters; before any pointer check, like check_optim
static int check_geomed(const flsim_geomed* r) {
    FLSIM_REQUIRE(r, "null geometric-median rule");
    FLSIM_REQUIRE(r->k >= 1 && r->k <= RULE_MAX_ARR,
                  "geometric median over k = %d entries (1 .. %d)", r->k, RULE_MAX_ARR);
    FLSIM_REQUIRE(r->iters >= 0 && r->iters <= FLSIM_GEOMED_MAX_ITERS,
                  "Invalid iters = %d: 0 <= iters <= %d", r->iters, FLSIM_GEOMED_MAX_ITERS);
    FLSIM_REQUIRE(r->nu > 0.0 && r->nu < (double)__builtin_inff(),
                  "Invalid nu = %g: it must be finite and > 0", r->nu);
    FLSIM_REQUIRE(r->weighted == 0 || r->weighted == 1,
                  "Invalid weighted = %d: 0 (uniform) or 1 (count)", r->weighted);
    return check_counts(r->count, r->k);
}

// ---- the distance-to-iterate stage's host twin (geometric median, centered clipping) -------------
// z as _wsum forms it: the center's term first (center nullable: none), then the entries' in index
// order, one fp64 multiply and one add per term, zero weights skipped
template <class M>
static double wsum_host(M&& mean, const double* wt, int k, long e, const float* center = nullptr,
                        double uw = 0.0) {
    double z = 0.0;
    bool have = false;
    if (center && geomed_nonzero(uw)) {
        volatile double t = (double)center[e] * uw;
        z = t;
        have = true;
    }
    for (int j = 0; j < k; ++j) {
        if (!geomed_nonzero(wt[j])) continue;
        volatile double t = (double)mean(j, e) * wt[j];
        z = have ? z + t : (double)t;
        have = true;
    }
    return z;
}

// dead[j]: entry j holds a mean that is not finite
template <class M>
static void dead_scan_host(M&& mean, int k, long P, int32_t* dead) {
    for (int j = 0; j < k; ++j) {
        dead[j] = 0;
        for (long e = 0; e < P && !dead[j]; ++e) {
            const float y = mean(j, e);
            dead[j] = !(__builtin_fabsf(y) < __builtin_inff());
        }
    }
}

// d[j] = the fp64 sum of ((double)x_j - z(e))^2 over the live entries, in element order (one fma
// each, as the kernels')
template <class M, class Z>
static void d2_host(M&& mean, Z&& z_of, const int32_t* dead, int k, long P, double* d) {
    for (int j = 0; j < k; ++j) d[j] = 0.0;
    for (long e = 0; e < P; ++e) {
        const double z = z_of(e);
        for (int j = 0; j < k; ++j) {
            if (dead[j]) continue;
            const double df = (double)mean(j, e) - z;
            d[j] = __builtin_fma(df, df, d[j]);
        }
    }
}

// ================================================================================================
// Simulated Byzantine workers: IPM and ALIE mixed into the bucket sums (include/flsim.h:
// flsim_attack; csrc/attack.h: the geometry and the element code shared with the host)
// ================================================================================================
struct AttackArgs {
    float* ent[RULE_MAX_ARR];           // bucket sums, updated in place
    int32_t honest[RULE_MAX_ARR];       // > 0: the entry is read
    int32_t byz[RULE_MAX_ARR];          // > 0: the entry is written
    float* b_out;                       // nullable
    union {
        double strength;
        const double* coef;             // the optimised attacks' mix: gamma * strength, which
    };                                  // k_attack_opt_finish wrote (device memory)
    long P;
    int k, kh, ntiles;
};
static_assert(sizeof(AttackArgs) <= 4096, "kernel argument block");

// One streaming pass, the shape of k_geomed_dist: thread t of the block's 256 owns the elements
// u * 256 + t, u < U, of a tile (a wave's load or store is one coalesced 256-byte row) and a block
// grid-strides over the tiles.  All loads of the honest entries for a thread's elements are issued
// before any arithmetic; then attack_craft (csrc/attack.h) per element: y_j, mu, var and b in fp64
// registers, in the text's order, contraction off; b rounded to fp32 once, stored to b_out, and
// H_j + b * (float)byz[j] (attack_mix: a separate fp32 multiply and add) to the entries with
// byz[j] >= 1 alone.  Nothing is summed across elements: the bits do not depend on the geometry.
// The per-entry table (the addresses loaded and stored to, (double)honest, (float)byz: 448 words at
// KPAD = 64; kept in the kernel arguments the pointers alone spilled 217 scalar registers) is
// built in LDS by wave 0 and read by broadcast, eight entries at a time, as in k_geomed_dist; a
// group wholly past k is skipped by a scalar branch, and the honest / Byzantine masks are
// launch-uniform scalar pairs.  An entry that is not read (honest == 0, padding) loads the first
// honest entry's address instead, and an element past P loads element 0: both values are dropped,
// so every load is in bounds and no byte of a write-only entry is ever read.
typedef float __attribute__((address_space(1)))* AttackGlobalF32;

template <int KPAD, int KIND>
__global__ void __launch_bounds__(256) k_attack(AttackArgs A) {
#pragma clang fp contract(off)
    constexpr int U = attack_unroll(KPAD), E = attack_tile_elems(KPAD);
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    __shared__ unsigned long long s_ent[KPAD];  // the address loaded for entry j
    __shared__ unsigned long long s_dst[KPAD];  // entry j itself: the address stored to
    __shared__ double s_hon[KPAD];
    __shared__ float s_byz[KPAD];
    __shared__ unsigned long long s_mask[2];    // bit j: entry j is read / is written
    {
        const int j = threadIdx.x;
        if (j < 64) {                           // (wave 0: lane j is entry j)
            float* src = nullptr;
            int h = 0, b = 0;
            if (j < A.k) {
                src = A.ent[j];
                h = A.honest[j];
                b = A.byz[j];
            }
            const unsigned long long mh = __ballot(h > 0), mb = __ballot(b > 0);
            const int first = mh ? __builtin_ctzll(mh) : 0;
            const unsigned long long any = __shfl((unsigned long long)(uintptr_t)src, first, 64);
            if (j < KPAD) {
                s_ent[j] = h > 0 ? (unsigned long long)(uintptr_t)src : any;
                s_dst[j] = (unsigned long long)(uintptr_t)src;
                s_hon[j] = h > 0 ? (double)h : 1.0;
                s_byz[j] = (float)b;
            }
            if (j == 0) {
                s_mask[0] = mh;
                s_mask[1] = mb;
            }
        }
        __syncthreads();
    }
    const unsigned long long mh0 = s_mask[0], mb0 = s_mask[1];
    for (int tl = blockIdx.x; tl < A.ntiles; tl += gridDim.x) {
        // the table is read, and the masks and k made scalar, again in every tile: hoisted out of
        // the loop they would hold their registers over all of it (k_geomed_dist)
        asm volatile("" ::: "memory");
        int h_lo = (int)mh0, h_hi = (int)(mh0 >> 32), b_lo = (int)mb0, b_hi = (int)(mb0 >> 32);
        int k = A.k;
        asm volatile("" : "+v"(h_lo), "+v"(h_hi), "+v"(b_lo), "+v"(b_hi), "+v"(k));
        k = __builtin_amdgcn_readfirstlane(k);
        const uint64_t hm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(h_hi) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane(h_lo);
        const uint64_t bm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(b_hi) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane(b_lo);
        const long e0 = (long)tl * E + threadIdx.x;
        bool inb[U];
        long off[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            inb[u] = e0 + u * 256 < A.P;
            off[u] = inb[u] ? e0 + u * 256 : 0;
        }
        float x[U][KPAD];
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j) {
                    const GeomedGlobalF32 src = (GeomedGlobalF32)s_ent[j];
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        x[u][j] = __builtin_nontemporal_load(src + off[u]);
                }
            } else {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j)
#pragma unroll
                    for (int u = 0; u < U; ++u) x[u][j] = 0.f;
            }
        }
        float b[U];
        if constexpr (KIND >= ATTACK_CRAFT_OPT) {
            const double coef = A.coef[0];          // launch-uniform: one scalar load
#pragma unroll
            for (int u = 0; u < U; ++u)
                b[u] = attack_opt_craft<KPAD, KIND - ATTACK_CRAFT_OPT>(x[u], s_hon, hm, k,
                                                                       (double)A.kh, coef);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
                b[u] = attack_craft<KPAD, KIND>(x[u], s_hon, hm, k, (double)A.kh, A.strength);
        }
        if (A.b_out) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (inb[u]) A.b_out[off[u]] = b[u];
        }
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j) {
                    if ((bm >> j) & 1) {
                        const AttackGlobalF32 dst = (AttackGlobalF32)s_dst[j];
                        const float nb = s_byz[j];
                        const bool hh = (hm >> j) & 1;
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (inb[u]) dst[off[u]] = attack_mix(x[u][j], hh, b[u], nb);
                    }
                }
            }
        }
    }
}

template <int KPAD>
static void launch_attack(int kind, dim3 grid, hipStream_t stream, const ProbeSlot& ps,
                          const AttackArgs& A) {
    if (kind == FLSIM_ATTACK_IPM)
        hipExtLaunchKernelGGL((k_attack<KPAD, FLSIM_ATTACK_IPM>), grid, dim3(256), 0, stream,
                              ps.start, ps.stop, 0, A);
    else if (kind == FLSIM_ATTACK_ALIE)
        hipExtLaunchKernelGGL((k_attack<KPAD, FLSIM_ATTACK_ALIE>), grid, dim3(256), 0, stream,
                              ps.start, ps.stop, 0, A);
    else if (kind == ATTACK_CRAFT_OPT + FLSIM_ATTACK_DIR_UNIT)
        hipExtLaunchKernelGGL((k_attack<KPAD, ATTACK_CRAFT_OPT + FLSIM_ATTACK_DIR_UNIT>), grid,
                              dim3(256), 0, stream, ps.start, ps.stop, 0, A);
    else if (kind == ATTACK_CRAFT_OPT + FLSIM_ATTACK_DIR_STD)
        hipExtLaunchKernelGGL((k_attack<KPAD, ATTACK_CRAFT_OPT + FLSIM_ATTACK_DIR_STD>), grid,
                              dim3(256), 0, stream, ps.start, ps.stop, 0, A);
    else
        hipExtLaunchKernelGGL((k_attack<KPAD, ATTACK_CRAFT_OPT + FLSIM_ATTACK_DIR_SIGN>), grid,
                              dim3(256), 0, stream, ps.start, ps.stop, 0, A);
}

static int check_attack_counts(int k, double strength, const int32_t* honest, const int32_t* byz,
                               int* kh);

// flsim_attack's fields, before any pointer is looked at; *kh: the entries with honest >= 1
static int check_attack(const flsim_attack* a, int* kh) {
    FLSIM_REQUIRE(a, "null attack");
    FLSIM_REQUIRE(a->kind == FLSIM_ATTACK_IPM || a->kind == FLSIM_ATTACK_ALIE,
                  "Invalid attack kind %d (0: ipm, 1: alie)", a->kind);
    return check_attack_counts(a->k, a->strength, a->honest, a->byz, kh);
}

// ... what flsim_attack and flsim_attack_opt share after the kind: k, the strength, the counts
static int check_attack_counts(int k, double strength, const int32_t* honest, const int32_t* byz,
                               int* kh) {
    FLSIM_REQUIRE(k >= 1 && k <= RULE_MAX_ARR, "attack over k = %d entries (1 .. %d)", k,
                  RULE_MAX_ARR);
    FLSIM_REQUIRE(strength >= 0.0 && strength < (double)__builtin_inff(),
                  "Invalid attack strength = %g: it must be finite and >= 0", strength);
    int nh = 0, nb = 0;
    for (int j = 0; j < k; ++j) {
        FLSIM_REQUIRE(honest[j] >= 0, "Invalid honest count %d of entry %d: it must be >= 0",
                      honest[j], j);
        FLSIM_REQUIRE(byz[j] >= 0, "Invalid Byzantine count %d of entry %d: it must be >= 0",
                      byz[j], j);
        FLSIM_REQUIRE(honest[j] > 0 || byz[j] > 0, "entry %d holds no worker: honest + byz "
                      "must be >= 1", j);
        nh += honest[j] > 0;
        nb += byz[j] > 0;
    }
    FLSIM_REQUIRE(nh >= 1, "ValueError: no entry holds an honest worker: the attacker has nothing "
                  "to observe");
    FLSIM_REQUIRE(nb >= 1, "no entry holds a Byzantine worker: nothing to attack");
    *kh = nh;
    return 0;
}

// ... and the pointers: every entry is read or written
static int check_attack_pointers(float* const* entries, int k, const float* b_out, long P) {
    for (int j = 0; j < k; ++j) {
        FLSIM_REQUIRE(entries[j], "null entry %d", j);
        FLSIM_REQUIRE(((uintptr_t)entries[j] & 15) == 0, "entry %d must be 16-byte aligned", j);
    }
    FLSIM_REQUIRE(((uintptr_t)b_out & 15) == 0, "b_out must be 16-byte aligned");
    FLSIM_REQUIRE(P > 0 && P < (1L << 31), "P = %ld out of range", P);
    for (int j = 0; j < k; ++j) {
        for (int q = 0; q < j; ++q)
            FLSIM_REQUIRE(!overlaps(entries[q], entries[j], P), "entries %d and %d overlap", q, j);
        FLSIM_REQUIRE(!overlaps(entries[j], b_out, P), "entry %d overlaps b_out", j);
    }
    return 0;
}

template <int KIND>
static void attack_eval_host(const flsim_attack* a, int kh, float* b_out, long P) {
    uint64_t hm = 0;
    double hon[RULE_MAX_ARR];
    for (int j = 0; j < RULE_MAX_ARR; ++j) {
        hon[j] = 1.0;
        if (j < a->k && a->honest[j] > 0) {
            hm |= 1ull << j;
            hon[j] = (double)a->honest[j];
        }
    }
    for (long e = 0; e < P; ++e) {
        float x[RULE_MAX_ARR];
        for (int j = 0; j < RULE_MAX_ARR; ++j) x[j] = ((hm >> j) & 1) ? a->entries[j][e] : 0.f;
        const float b = attack_craft<RULE_MAX_ARR, KIND>(x, hon, hm, a->k, (double)kh,
                                                         a->strength);
        if (b_out) b_out[e] = b;
        for (int j = 0; j < a->k; ++j)
            if (a->byz[j] > 0)
                a->entries[j][e] = attack_mix(x[j], (hm >> j) & 1, b, (float)a->byz[j]);
    }
}

// ================================================================================================
// The optimised attacks Min-Max and Min-Sum: the stats launch, the pairwise-distance stage over the
// honest entries, the finish (the matrix, the sums, gamma), then k_attack's mix (include/flsim.h:
// flsim_attack_opt; csrc/attack_opt.h: the geometry, the element code and the scalar solve shared
// with the host)
// ================================================================================================
struct AttackOptStatsArgs {
    const float* ent[RULE_MAX_ARR];     // the kh honest entries, compacted in index order
    int32_t honest[RULE_MAX_ARR];
    double* partials;                   // [2 * kh + 1][blocks], slot-major
    long P;
    int kh, ntiles;
};
static_assert(sizeof(AttackOptStatsArgs) <= 4096, "kernel argument block");

// One streaming pass, the shape of k_attack and k_geomed_dist: thread t of the block's 256 owns
// the elements u * 256 + t, u < U, of a tile and a block grid-strides over the tiles; the table
// (the address loaded, (double)honest) is built in LDS by wave 0 and read by broadcast; all loads
// of a thread's elements are issued before any arithmetic; a padding entry loads entry 0 and an
// element past P loads element 0, and both are dropped.  Per element attack_opt_stats_elem
// (csrc/attack_opt.h) forms y_j, mu, p and the 2 * kh + 1 products and adds them to the thread's
// sums: tiles in the block's order, u ascending.  Then every sum is added over the wave by a
// butterfly and over the four waves as (w0 + w1) + (w2 + w3), as dist_reduce does, and thread s
// stores slot s.
template <int KPAD, int DIR>
__global__ void __launch_bounds__(256) k_attack_opt_stats(AttackOptStatsArgs A) {
#pragma clang fp contract(off)
    constexpr int U = attack_opt_unroll(KPAD), E = attack_opt_tile_elems(KPAD);
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    __shared__ unsigned long long s_ent[KPAD];
    __shared__ double s_hon[KPAD];
    __shared__ double red[4][2 * KPAD + 1];
    {
        const int j = threadIdx.x;
        if (j < KPAD) {
            const bool in = j < A.kh;
            s_ent[j] = (unsigned long long)(uintptr_t)(in ? A.ent[j] : A.ent[0]);
            s_hon[j] = in ? (double)A.honest[j] : 1.0;
        }
        __syncthreads();
    }
    double a[KPAD], c[KPAD], q = 0.0;
#pragma unroll
    for (int j = 0; j < KPAD; ++j) a[j] = c[j] = 0.0;
    for (int tl = blockIdx.x; tl < A.ntiles; tl += gridDim.x) {
        // the table is read, and k made scalar, again in every tile (k_attack)
        asm volatile("" ::: "memory");
        int k = A.kh;
        asm volatile("" : "+v"(k));
        k = __builtin_amdgcn_readfirstlane(k);
        const long e0 = (long)tl * E + threadIdx.x;
        bool inb[U];
        long off[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            inb[u] = e0 + u * 256 < A.P;
            off[u] = inb[u] ? e0 + u * 256 : 0;
        }
        float x[U][KPAD];
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j) {
                    const GeomedGlobalF32 src = (GeomedGlobalF32)s_ent[j];
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        x[u][j] = __builtin_nontemporal_load(src + off[u]);
                }
            } else {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j)
#pragma unroll
                    for (int u = 0; u < U; ++u) x[u][j] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            attack_opt_stats_elem<KPAD, DIR>(x[u], s_hon, k, (double)A.kh, inb[u], a, c, q);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto wave_sum = [&](double v, int slot) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][slot] = v;
    };
#pragma unroll
    for (int j = 0; j < KPAD; ++j) {
        if (j < A.kh) {
            wave_sum(a[j], j);
            wave_sum(c[j], KPAD + j);
        }
    }
    wave_sum(q, 2 * KPAD);
    __syncthreads();
    const int t = threadIdx.x, kh = A.kh;
    if (t < 2 * kh + 1) {
        const int slot = t < kh ? t : t < 2 * kh ? KPAD + (t - kh) : 2 * KPAD;
        A.partials[(long)t * gridDim.x + blockIdx.x] =
            (red[0][slot] + red[1][slot]) + (red[2][slot] + red[3][slot]);
    }
}

struct AttackOptFinArgs {               // (entry_sums reads partials, nblocks and k)
    const double* partials;             // the stats launch's, [k = 2 * kh + 1][nblocks]
    int nblocks, k;
};

// One block of KRUM_FIN_THREADS: pair_matrix (the pairwise-distance stage, Krum's matrix), then
// the stats partials by entry_sums (the distance-to-iterate stage's fixed order), then
// attack_opt_gamma (csrc/attack_opt.h) on the matrix and the sums in LDS: thread i takes row i,
// thread 0 the scalar code.  coef = gamma * strength goes to the last word of the partials: the
// mix launch reads it from there (k_attack's argument block has no room for a second scalar).
__global__ void __launch_bounds__(KRUM_FIN_THREADS)
k_attack_opt_finish(const double* partials, int nblocks, int nb, int kh, AttackOptFinArgs S,
                    int kind, double strength, double* dist, double* stats, double* gamma,
                    double* coef) {
    static_assert(KRUM_FIN_THREADS == GEOMED_FIN_THREADS, "entry_sums' block");
    __shared__ double sd[RULE_MAX_ARR * RULE_MAX_ARR];
    __shared__ double ss[2 * RULE_MAX_ARR + 1];
    __shared__ double rmax[RULE_MAX_ARR], rsum[RULE_MAX_ARR];
    pair_matrix(partials, nblocks, nb, kh, sd, dist);
    entry_sums(S, ss);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kh) {
        stats[t] = ss[t];
        stats[RULE_MAX_ARR + t] = ss[kh + t];
    }
    if (t == 0) stats[2 * RULE_MAX_ARR] = ss[2 * kh];
    const double g = attack_opt_gamma(kind, ss, ss + kh, ss[2 * kh], sd, kh, rmax, rsum, t,
                                      KRUM_FIN_THREADS, [] { __syncthreads(); });
    if (t == 0) {
        gamma[0] = g;
        coef[0] = g * strength;         // the mix's scalar: one multiply, here
    }
}

// flsim_attack_opt's fields, before any pointer is looked at; *kh: the entries with honest >= 1
static int check_attack_opt(const flsim_attack_opt* a, int* kh) {
    FLSIM_REQUIRE(a, "null attack");
    FLSIM_REQUIRE(a->kind == FLSIM_ATTACK_MINMAX || a->kind == FLSIM_ATTACK_MINSUM,
                  "Invalid attack kind %d (2: minmax, 3: minsum)", a->kind);
    FLSIM_REQUIRE(a->dir == FLSIM_ATTACK_DIR_UNIT || a->dir == FLSIM_ATTACK_DIR_STD ||
                  a->dir == FLSIM_ATTACK_DIR_SIGN,
                  "Invalid attack direction %d (0: unit, 1: std, 2: sign)", a->dir);
    return check_attack_counts(a->k, a->strength, a->honest, a->byz, kh);
}

// with_dir: FLSIM_ATTACK_DIR_* as a constant
template <class F>
static void with_dir(int dir, F&& f) {
    if (dir == FLSIM_ATTACK_DIR_UNIT) f(IntC<FLSIM_ATTACK_DIR_UNIT>{});
    else if (dir == FLSIM_ATTACK_DIR_STD) f(IntC<FLSIM_ATTACK_DIR_STD>{});
    else f(IntC<FLSIM_ATTACK_DIR_SIGN>{});
}

// host (testing): given the distances (the pairwise stage's host twin over the honest entries'
// fp32 means), the sums by csrc/attack_opt.h's element code in element order, gamma by its
// scalar code, then the mix over host pointers
template <int DIR>
static void attack_opt_eval_host(const flsim_attack_opt* a, int kh, double* stats, double* gamma,
                                 const double* dist, float* b_out, long P) {
    constexpr int K = RULE_MAX_ARR;
    const float* hent[K];
    double hcd[K], hon[K];
    uint64_t hm = 0;
    for (int j = 0, i = 0; j < K; ++j) {
        hon[j] = hcd[j] = 1.0;
        if (j < a->k && a->honest[j] > 0) {
            hm |= 1ull << j;
            hon[j] = (double)a->honest[j];
            hent[i] = a->entries[j];
            hcd[i++] = (double)a->honest[j];
        }
    }
    double sa[K], sc[K], q = 0.0, rmax[K], rsum[K];
    for (int j = 0; j < K; ++j) sa[j] = sc[j] = 0.0;
    for (long e = 0; e < P; ++e) {
        float x[K];
        for (int i = 0; i < K; ++i) x[i] = i < kh ? hent[i][e] : 0.f;
        attack_opt_stats_elem<K, DIR>(x, hcd, kh, (double)kh, true, sa, sc, q);
    }
    for (int i = 0; i < FLSIM_ATTACK_OPT_STATS; ++i) stats[i] = 0.0;
    for (int i = 0; i < kh; ++i) {
        stats[i] = sa[i];
        stats[K + i] = sc[i];
    }
    stats[2 * K] = q;
    gamma[0] = attack_opt_gamma((int)a->kind, sa, sc, q, dist, kh, rmax, rsum, 0, 1, [] {});
    const double coef = gamma[0] * a->strength;
    for (long e = 0; e < P; ++e) {
        float x[K];
        for (int j = 0; j < K; ++j) x[j] = ((hm >> j) & 1) ? a->entries[j][e] : 0.f;
        const float b = attack_opt_craft<K, DIR>(x, hon, hm, a->k, (double)kh, coef);
        if (b_out) b_out[e] = b;
        for (int j = 0; j < a->k; ++j)
            if (a->byz[j] > 0)
                a->entries[j][e] = attack_mix(x[j], (hm >> j) & 1, b, (float)a->byz[j]);
    }
}

// ================================================================================================
// Nearest-neighbour mixing of the entries before any rule: Krum's distance launch, finish + the
// neighbour selection, the mix in place (include/flsim.h: flsim_nnm; csrc/nnm.h: the geometry of
// the mix, the selection and the element code shared with the host)
// ================================================================================================
// One block of KRUM_FIN_THREADS: pair_matrix (the pairwise-distance stage, Krum's matrix), then
// csrc/nnm.h's selection on the matrix in LDS: thread i takes row i.
__global__ void __launch_bounds__(KRUM_FIN_THREADS)
k_nnm_finish(const double* partials, int nblocks, int nb, int k, int f, double* dist,
             uint64_t* nbr) {
    __shared__ double sd[RULE_MAX_ARR * RULE_MAX_ARR];
    pair_matrix(partials, nblocks, nb, k, sd, dist);
    nnm_select(sd, nbr, k, f, (int)threadIdx.x, KRUM_FIN_THREADS);
}

struct NnmMixArgs {
    float* ent[RULE_MAX_ARR];           // in: bucket sums; out: the mixed means, in place
    float cnt[RULE_MAX_ARR];            // (float)count[j] and RN(1 / that), as the EntryTable's
    float rcnt[RULE_MAX_ARR];
    const uint64_t* nbr;                // [k] the masks k_nnm_finish wrote (device memory)
    long P;
    int k, ntiles;
    float fn;                           // (float)(k - f): the divisor of every neighbour sum
};
static_assert(sizeof(NnmMixArgs) <= 4096, "kernel argument block");

// One streaming pass, the shape of k_attack: thread t of the block's 256 owns the elements
// u * 256 + t, u < U, of a tile (a wave's load or store is one coalesced 256-byte row) and a block
// grid-strides over the tiles.  All loads of all k entries for a thread's elements are issued
// before any arithmetic or store; then the bucket means x_j = ent[j][e] / cnt[j] by div_const as
// k_robust forms them, and for every i < k the mixed value y_i = nnm_mix_elem (csrc/nnm.h): the
// neighbours of i added in ascending j, fp32, contraction off, one IEEE division -- stored to
// ent[i].  In place is safe without any ordering between blocks or threads: every element of
// every entry is read and written by one thread only, and that thread has all k values of the
// element in registers before its first store.  The per-entry table (addresses, counts, the
// neighbour masks: loaded from device memory once, by wave 0) is built in LDS and read by
// broadcast, as in k_attack; the mask of row i and k are made scalar (readfirstlane), so every
// test of a mask bit is a wave-uniform scalar branch.  x is indexed by the unrolled j alone and the
// loop over i indexes only LDS: no register array is indexed at run time (scratch stays 0).  A
// padding entry loads entry 0's address and an element past P loads element 0: both values are
// dropped, so every load is in bounds, and nothing is stored past P.
template <int KPAD>
__global__ void __launch_bounds__(256) k_nnm_mix(NnmMixArgs A) {
#pragma clang fp contract(off)
    constexpr int U = nnm_unroll(KPAD), E = nnm_tile_elems(KPAD);
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    __shared__ unsigned long long s_ent[KPAD];  // the address loaded for entry j
    __shared__ unsigned long long s_nbr[KPAD];  // the neighbours of entry j
    __shared__ float s_cnt[KPAD], s_rcnt[KPAD];
    {
        const int j = threadIdx.x;
        if (j < KPAD) {
            const bool in = j < A.k;
            s_ent[j] = (unsigned long long)(uintptr_t)(in ? A.ent[j] : A.ent[0]);
            s_nbr[j] = in ? (unsigned long long)A.nbr[j] : 0ull;
            s_cnt[j] = in ? A.cnt[j] : 1.f;
            s_rcnt[j] = in ? A.rcnt[j] : 1.f;
        }
        __syncthreads();
    }
    for (int tl = blockIdx.x; tl < A.ntiles; tl += gridDim.x) {
        // k is made scalar again in every tile, as k_attack does
        asm volatile("" ::: "memory");
        int k = A.k;
        asm volatile("" : "+v"(k));
        k = __builtin_amdgcn_readfirstlane(k);
        const long e0 = (long)tl * E + threadIdx.x;
        bool inb[U];
        long off[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            inb[u] = e0 + u * 256 < A.P;
            off[u] = inb[u] ? e0 + u * 256 : 0;
        }
        float x[U][KPAD];
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j) {
                    const GeomedGlobalF32 src = (GeomedGlobalF32)s_ent[j];
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        x[u][j] = __builtin_nontemporal_load(src + off[u]);
                }
            } else {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j)
#pragma unroll
                    for (int u = 0; u < U; ++u) x[u][j] = 0.f;
            }
        }
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j) {
                    const float c = s_cnt[j], rc = s_rcnt[j];
#pragma unroll
                    for (int u = 0; u < U; ++u) x[u][j] = div_const(x[u][j], c, rc);
                }
            }
        }
        for (int i = 0; i < k; ++i) {
            const unsigned long long mi = s_nbr[i];
            const uint64_t m =
                ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(mi >> 32)) << 32) |
                (uint32_t)__builtin_amdgcn_readfirstlane((int)mi);
            const AttackGlobalF32 dst = (AttackGlobalF32)s_ent[i];
            float y[U];
            nnm_mix_elem<KPAD, U>(x, m, k, A.fn, y);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (inb[u]) dst[off[u]] = y[u];
        }
    }
}

// flsim_nnm's fields, before any pointer is looked at
static int check_nnm(const flsim_nnm* a) {
    FLSIM_REQUIRE(a, "null NNM");
    FLSIM_REQUIRE(a->k >= 1 && a->k <= RULE_MAX_ARR, "NNM over k = %d entries (1 .. %d)", a->k,
                  RULE_MAX_ARR);
    FLSIM_REQUIRE(a->f >= 0 && 2 * (long)a->f < a->k,
                  "Invalid NNM f = %d for k = %d entries: f >= 0 and 2 * f < k", a->f, a->k);
    return check_counts(a->count, a->k);
}

// ================================================================================================
// Centered clipping with a carried center (CClip): distances to the iterate, the scalar step, apply
// (include/flsim.h: flsim_cclip; csrc/cclip.h: the scalar code shared with the host; the geometry
// is csrc/geomed.h's)
// ================================================================================================
struct CclipDistArgs {
    EntryTable T;                       // x_j = ent[j][e] / cnt[j], as k_robust forms it
    const float* center;               // [P]; not read by a FRESH launch
    const double* u;                    // later pairs: s->u, written by the finish launches
    const double* w;                    // later pairs: s->w
    const int32_t* state;               // later pairs: the dead flags [k]
    double* partials;                   // [k + 1][grid]
    long P;
    int k, ntiles, pair;
};
static_assert(sizeof(CclipDistArgs) <= 4096, "kernel argument block");

// One streaming pass over the k entries and the center for the iterate z = u * c + sum_j w_j * x_j:
// the geometry, the LDS table, the load pattern and the reduction of k_geomed_dist (its comment),
// plus the center as one more operand of z: the center's term first, then the entries in index
// order, one multiply and one add per term with contraction off.  z starts from c * u (+0.0 with
// no center term) and a term of weight 0 adds +-0: as in k_geomed_dist that differs from _wsum in
// the sign of a zero z at most, which (x - z)^2 does not see.  No distance is taken for the center.
// PAIR0: w = 0 by construction, so z = c (+0.0 when FRESH) and no entry enters z: a NaN or an inf
// in an entry cannot reach another entry's distance, and there is no redo pass.  Every entry is
// loaded for its distance and for the "held a NaN or an inf" mask in slot k; an entry's value is
// used as soon as it arrives, so only the sums stay in registers over a tile.
// Later pairs: u and w are read from s->u and s->w; a dead entry is not loaded; the center is not
// loaded while u is +-0 (_wsum's skip-zero rule), nor by a FRESH launch at all.
template <int KPAD, bool PAIR0, bool FRESH>
__global__ void __launch_bounds__(256) k_cclip_dist(CclipDistArgs A) {
#pragma clang fp contract(off)
    constexpr int U = geomed_unroll(KPAD), E = geomed_tile_elems(KPAD);
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    __shared__ unsigned long long s_ent[KPAD];  // the address loaded for entry j
    __shared__ double s_w[KPAD];
    __shared__ float s_cnt[KPAD], s_rcnt[KPAD];
    __shared__ unsigned long long s_mask;       // bit j: entry j is loaded
    __shared__ double s_u;
    if (threadIdx.x == 0) {                     // (before dist_table's barrier)
        double u = 1.0;
        if constexpr (!PAIR0) u = A.u[A.pair];
        s_u = u;
    }
    const uint64_t ld_mask = dist_table<KPAD, PAIR0>(
        A.T, A.k, A.state,
        [&](int j) {
            if constexpr (PAIR0) return 0.0;
            else return A.w[(long)A.pair * A.k + j];
        },
        s_ent, s_w, s_cnt, s_rcnt, &s_mask);
    const GeomedGlobalF32 cen = (GeomedGlobalF32)(uintptr_t)A.center;
    double acc[KPAD];
#pragma unroll
    for (int j = 0; j < KPAD; ++j) acc[j] = 0.0;
    uint32_t bad_lo = 0, bad_hi = 0;
    for (int tl = blockIdx.x; tl < A.ntiles; tl += gridDim.x) {
        // the table is read, and the mask and k tested, again in every tile (k_geomed_dist)
        asm volatile("" ::: "memory");
        int m_lo = (int)ld_mask, m_hi = (int)(ld_mask >> 32), k = A.k;
        asm volatile("" : "+v"(m_lo), "+v"(m_hi), "+v"(k));
        k = __builtin_amdgcn_readfirstlane(k);
        const uint64_t ldm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(m_hi) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane(m_lo);
        const long e0 = (long)tl * E + threadIdx.x;
        bool inb[U];
        long off[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            inb[u] = e0 + u * 256 < A.P;
            off[u] = inb[u] ? e0 + u * 256 : 0;
        }
        // the center's term: launch-uniform whether it is loaded
        double z[U];
#pragma unroll
        for (int u = 0; u < U; ++u) z[u] = 0.0;
        if constexpr (!FRESH) {
            const double uw = s_u;
            const uint64_t ub = __builtin_bit_cast(uint64_t, uw) << 1;
            const bool ldc = (__builtin_amdgcn_readfirstlane((int)(ub >> 32)) |
                              __builtin_amdgcn_readfirstlane((int)ub)) != 0;
            if (PAIR0 || ldc) {
                float c[U];
#pragma unroll
                for (int u = 0; u < U; ++u) c[u] = __builtin_nontemporal_load(cen + off[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if constexpr (PAIR0) z[u] = (double)c[u];
                    else z[u] = (double)c[u] * uw;
                }
            }
        }
        if constexpr (PAIR0) {
#pragma unroll
            for (int u = 0; u < U; ++u) z[u] = inb[u] ? z[u] : 0.0;    // (past P: the sums gain 0)
#pragma unroll
            for (int j0 = 0; j0 < KPAD; j0 += GRP) {
                if (j0 < k) {
                    float x[U][GRP];
                    if (ldm != 0) {
#pragma unroll
                        for (int j = 0; j < GRP; ++j) {
                            const GeomedGlobalF32 src = (GeomedGlobalF32)s_ent[j0 + j];
#pragma unroll
                            for (int u = 0; u < U; ++u)
                                x[u][j] = __builtin_nontemporal_load(src + off[u]);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < GRP; ++j)
#pragma unroll
                            for (int u = 0; u < U; ++u) x[u][j] = 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < GRP; ++j) {
                        const float c = s_cnt[j0 + j], rc = s_rcnt[j0 + j];
                        const bool ld = (ldm >> (j0 + j)) & 1;
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float y = div_const((ld && inb[u]) ? x[u][j] : 0.f, c, rc);
                            const uint32_t nf =
                                !(fabsf(y) < __builtin_inff()) ? 1u << ((j0 + j) & 31) : 0u;
                            if (j0 + j < 32) bad_lo |= nf;
                            else bad_hi |= nf;
                            const double d = (double)y - z[u];
                            acc[j0 + j] = __builtin_fma(d, d, acc[j0 + j]);
                        }
                    }
                }
            }
        } else {
            float x[U][KPAD];
#pragma unroll
            for (int j0 = 0; j0 < KPAD; j0 += GRP) {
                if (j0 < k && ldm != 0) {
#pragma unroll
                    for (int j = j0; j < j0 + GRP; ++j) {
                        const GeomedGlobalF32 src = (GeomedGlobalF32)s_ent[j];
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            x[u][j] = __builtin_nontemporal_load(src + off[u]);
                    }
                } else {
#pragma unroll
                    for (int j = j0; j < j0 + GRP; ++j)
#pragma unroll
                        for (int u = 0; u < U; ++u) x[u][j] = 0.f;
                }
            }
#pragma unroll
            for (int j0 = 0; j0 < KPAD; j0 += GRP) {
                if (j0 < k) {
#pragma unroll
                    for (int j = j0; j < j0 + GRP; ++j) {
                        const float c = s_cnt[j], rc = s_rcnt[j];
                        const double w = s_w[j];
                        const bool ld = (ldm >> j) & 1;
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float y = div_const((ld && inb[u]) ? x[u][j] : 0.f, c, rc);
                            x[u][j] = y;
                            const double t = (double)y * w;
                            z[u] = z[u] + t;
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) z[u] = inb[u] ? z[u] : 0.0;    // (past P: the sums gain 0)
#pragma unroll
            for (int j0 = 0; j0 < KPAD; j0 += GRP) {
                if (j0 < k) {
#pragma unroll
                    for (int j = j0; j < j0 + GRP; ++j)
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const double d = (double)x[u][j] - z[u];
                            acc[j] = __builtin_fma(d, d, acc[j]);
                        }
                }
            }
        }
    }
    dist_reduce<KPAD, PAIR0>(acc, bad_lo, bad_hi, A.k, A.partials);
}

struct CclipFinArgs {
    int32_t count[RULE_MAX_ARR];
    const double* partials;             // [k + 1][nblocks]
    double* u;                          // s->u
    double* w;                          // s->w
    double* d2;                         // s->d2
    double* s;                          // s->s
    int32_t* state;                     // s->state
    double tau;
    int nblocks, k, pair, weighted;
};

// One block of 16 waves: entry_sums; pair 0 also takes dead_mask, writes the dead flags and the
// control words, and u[0] = 1, w[0] = 0.  Then csrc/cclip.h's scalar code of one iteration on the
// sums in LDS, and d2[r], s[r], u[r + 1] and w[r + 1].
__global__ void __launch_bounds__(GEOMED_FIN_THREADS) k_cclip_finish(CclipFinArgs A) {
    __shared__ double sd[RULE_MAX_ARR], sa[RULE_MAX_ARR], sw[RULE_MAX_ARR], ss[RULE_MAX_ARR];
    __shared__ double sterm[RULE_MAX_ARR], swn[RULE_MAX_ARR];
    __shared__ double ssum[CCLIP_SUM_WORDS];
    __shared__ int32_t sdead[RULE_MAX_ARR];
    __shared__ unsigned long long smask[GEOMED_FIN_THREADS / 64];
    const int t = threadIdx.x, k = A.k, r = A.pair;
    entry_sums(A, sd);
    double u = 1.0;
    if (r == 0) {
        const int32_t dead = dead_mask(A, smask);
        if (t < k) {
            sdead[t] = dead;
            A.state[t] = dead;
            sa[t] = geomed_alpha(A.weighted, A.count[t], dead);
            sw[t] = 0.0;
            A.w[t] = 0.0;
        }
        __syncthreads();
        if (t == 0) {
            int nd = 0;
            for (int j = 0; j < k; ++j) nd += sdead[j];
            A.state[k + CCLIP_ST_NDEAD] = nd;
            for (int c = 1; c < CCLIP_ST_WORDS; ++c) A.state[k + c] = 0;
            A.u[0] = 1.0;
        }
    } else {
        u = A.u[r];
        if (t < k) {
            const int32_t dead = A.state[t];
            sdead[t] = dead;
            sa[t] = geomed_alpha(A.weighted, A.count[t], dead);
            sw[t] = A.w[(long)r * k + t];
        }
    }
    __syncthreads();
    cclip_iterate(sd, sa, sdead, k, A.tau, u, sw, ss, sterm, ssum, swn, t, GEOMED_FIN_THREADS,
                  [] { __syncthreads(); });
    if (t < k) {
        A.d2[(long)r * k + t] = sd[t];
        A.s[(long)r * k + t] = ss[t];
        A.w[(long)(r + 1) * k + t] = swn[t];
    }
    if (t == 0) A.u[r + 1] = ssum[CCLIP_SUM_U];
}

struct CclipApplyArgs {
    EntryTable T;
    ApplyOut O;
    const double* u;                    // &u[iters] (device memory, written by a finish launch)
    const double* w;                    // w[iters]
    float* center;                      // read (unless fresh or u = +-0), then g
    int k, fresh;
};
static_assert(sizeof(CclipApplyArgs) <= 4096, "kernel argument block");

// One thread owns one element, as k_geomed_apply: z as _wsum forms it over the center (first; not
// loaded when fresh or while its weight is +-0) and the entries of non-zero weight, g = (float)z,
// center[e] = g (the unclipped g; the element's only reader is this thread, before the store),
// then the update of kind OK, or OK_GOUT.  Like k_geomed_apply it keeps its own copy of the head and
// tail and of the loop over the entries, for the same measured reasons (its comment).
template <int OK>
__global__ void __launch_bounds__(256) k_cclip_apply(CclipApplyArgs A) {
#pragma clang fp contract(off)
    constexpr bool HAS_M = opt_n_state(OK) >= 1, HAS_V = opt_n_state(OK) == 2;
    const ApplyOut& O = A.O;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = e < O.P;
    if constexpr (OK != OK_GOUT) {
        if (!live) return;
    }
    float p = 0.f, m = 0.f, v = 0.f;
    if constexpr (OK != OK_GOUT) p = __builtin_nontemporal_load(O.p + e);
    if constexpr (HAS_M) m = __builtin_nontemporal_load(O.m + e);
    if constexpr (HAS_V) v = __builtin_nontemporal_load(O.v + e);
    GeomedConstF64 wdev = (GeomedConstF64)(uintptr_t)A.w;
    GeomedConstF64 udev = (GeomedConstF64)(uintptr_t)A.u;
    double z = 0.0;
    bool have = false;
    if (!A.fresh) {
        const double uw = udev[0];
        if (geomed_nonzero(uw)) {
            const float c = live ? __builtin_nontemporal_load(A.center + e) : 0.f;
            z = (double)c * uw;
            have = true;
        }
    }
    for (int j0 = 0; j0 < A.k; j0 += 8) {
        float x[8], c[8], rc[8];
        double w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            x[u] = 0.f;
            c[u] = 1.f;
            rc[u] = 1.f;
            w[u] = 0.0;
            if (j0 + u < A.k) {
                const int j = j0 + u;
                const float* src = A.T.ent[j];
                w[u] = wdev[j];
                c[u] = A.T.cnt[j];
                rc[u] = A.T.rcnt[j];
                if (geomed_nonzero(w[u]) && src && live) x[u] = __builtin_nontemporal_load(src + e);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (j0 + u < A.k && geomed_nonzero(w[u])) {
                const double t = (double)div_const(x[u], c[u], rc[u]) * w[u];
                z = have ? z + t : t;
                have = true;
            }
        }
    }
    const float g = (float)z;
    if constexpr (OK == OK_GOUT) {
        if (live) {
            __builtin_nontemporal_store(g, A.center + e);
            if (O.g_out) __builtin_nontemporal_store(g, O.g_out + e);
            if (O.G) __builtin_nontemporal_store(g, O.G + e);
        }
        if (O.partials) {
            __shared__ double red[4];
            const double s = block_sum_f64(live ? (double)g * (double)g : 0.0, red);
            if (threadIdx.x == 0) O.partials[blockIdx.x] = s;
        }
    } else {
        __builtin_nontemporal_store(g, A.center + e);
        if (O.g_out) __builtin_nontemporal_store(g, O.g_out + e);
        opt_update<OK>(O.ac, O.oc, g, p, m, v);
        __builtin_nontemporal_store(p, O.p + e);
        if constexpr (HAS_M) __builtin_nontemporal_store(m, O.m + e);
        if constexpr (HAS_V) __builtin_nontemporal_store(v, O.v + e);
    }
}

template <int KPAD>
static void launch_cclip_dist(bool pair0, bool fresh, dim3 grid, hipStream_t stream,
                              const ProbeSlot& ps, const CclipDistArgs& A) {
#define FLSIM_CCLIP_DIST(P0, FR)                                                                  \
    hipExtLaunchKernelGGL((k_cclip_dist<KPAD, P0, FR>), grid, dim3(256), 0, stream, ps.start,     \
                          ps.stop, 0, A)
    if (pair0 && fresh) FLSIM_CCLIP_DIST(true, true);
    else if (pair0) FLSIM_CCLIP_DIST(true, false);
    else if (fresh) FLSIM_CCLIP_DIST(false, true);
    else FLSIM_CCLIP_DIST(false, false);
#undef FLSIM_CCLIP_DIST
}

// flsim_cclip's hyper-parameters; before any pointer check, like check_optim
static int check_cclip(const flsim_cclip* r) {
    FLSIM_REQUIRE(r, "null centered-clipping rule");
    FLSIM_REQUIRE(r->k >= 1 && r->k <= RULE_MAX_ARR,
                  "centered clipping over k = %d entries (1 .. %d)", r->k, RULE_MAX_ARR);
    FLSIM_REQUIRE(r->iters >= 1 && r->iters <= FLSIM_CCLIP_MAX_ITERS,
                  "Invalid iters = %d: 1 <= iters <= %d", r->iters, FLSIM_CCLIP_MAX_ITERS);
    FLSIM_REQUIRE(r->tau > 0.0 && r->tau < (double)__builtin_inff(),
                  "Invalid tau = %g: it must be finite and > 0", r->tau);
    FLSIM_REQUIRE(r->weighted == 0 || r->weighted == 1,
                  "Invalid weighted = %d: 0 (uniform) or 1 (count)", r->weighted);
    FLSIM_REQUIRE(r->fresh == 0 || r->fresh == 1,
                  "Invalid fresh = %d: 0 (the center is read) or 1 (it counts as all zero)",
                  r->fresh);
    return check_counts(r->count, r->k);
}

}  // namespace flsim

using namespace flsim;

extern "C" {

// ---- rule() + Adam from S_t in a buffer ---------------------------------------------------------
// tensor_sizes: numel of each parameter tensor in named_parameters order (the cascade's column
// rule is per tensor)
int flsim_aggregate_adam_rule(const float* S, const flsim_rule* rule, float* p, float* m, float* v,
                              long P, const long* tensor_sizes, int n_tensors, long step, double lr,
                              double beta1, double beta2, double eps, hipStream_t stream) {
    return flsim_aggregate_adam_rule_push(S, nullptr, rule, p, m, v, P, tensor_sizes, n_tensors,
                                          step, lr, beta1, beta2, eps, stream);
}

// the same, also writing S_t to S_out (the slow worker's FIFO slot at a tick, main.py:156,161)
// in the same pass: world > 1 after the all-reduce
int flsim_aggregate_adam_rule_push(const float* S, float* S_out, const flsim_rule* rule, float* p,
                                   float* m, float* v, long P, const long* tensor_sizes,
                                   int n_tensors, long step, double lr, double beta1, double beta2,
                                   double eps, hipStream_t stream) {
    const flsim_optim o = adam_optim(lr, beta1, beta2, eps);
    return flsim_aggregate_optim_rule_push(S, S_out, rule, p, m, v, P, tensor_sizes, n_tensors,
                                           step, &o, stream);
}

// rule() + the update rule of `optim` (include/flsim.h); m / v may be null where the kind does
// not own them
int flsim_aggregate_optim_rule_push(const float* S, float* S_out, const flsim_rule* rule, float* p,
                                    float* m, float* v, long P, const long* tensor_sizes,
                                    int n_tensors, long step, const flsim_optim* optim,
                                    hipStream_t stream) {
    return flsim_aggregate_optim_wrule_push(S, S_out, rule, nullptr, p, m, v, P, tensor_sizes,
                                            n_tensors, step, optim, stream);
}

// the same with a staleness-weighted rule: sum_j w_j * entry_j / divisor, w = 1 for the S_t
// entries and wts->w[q] for arrays[q]; wts == NULL: the plain mean above
int flsim_aggregate_optim_wrule_push(const float* S, float* S_out, const flsim_rule* rule,
                                     const flsim_rule_weights* wts, float* p, float* m, float* v,
                                     long P, const long* tensor_sizes, int n_tensors, long step,
                                     const flsim_optim* optim, hipStream_t stream) {
    return flsim_aggregate_optim_crule_push(S, S_out, nullptr, rule, wts, nullptr, p, m, v, P,
                                            tensor_sizes, n_tensors, step, optim, stream);
}

// the same with delay compensation (include/flsim.h): comp->theta_src[q] (nullable) is the
// snapshot of arrays[q]; theta_out (nullable) receives the pre-update p in the same pass.  Either
// one selects the C kernels, which run in the weighted form (wts == NULL: weights 1.0, divisor k)
int flsim_aggregate_optim_crule_push(const float* S, float* S_out, float* theta_out,
                                     const flsim_rule* rule, const flsim_rule_weights* wts,
                                     const flsim_rule_comp* comp, float* p, float* m, float* v,
                                     long P, const long* tensor_sizes, int n_tensors, long step,
                                     const flsim_optim* optim, hipStream_t stream) {
    return flsim_aggregate_optim_clip_push(S, S_out, theta_out, rule, wts, comp, nullptr, p, m, v,
                                           P, tensor_sizes, n_tensors, step, optim, stream);
}

// the doubles a clipped step over P elements writes, for any layout of at most 4096 tensors: a
// launch covers at most MAX_TAILS tensor tails, so at most 513 launches; a launch over n
// elements has at most n / 1024 + 2 streaming blocks, and each streaming block that is an edge
// block adds 4 * G <= 8 edge pieces.  The robust step (flsim_robust_optim_step) is one launch
// without edge pieces, one partial per block of 256 elements: ceil(P / 256) <= 4 * (P / 1024) + 4
// of them, inside this bound
long flsim_clip_partials(long P) {
    if (P < 0) return 0;
    return 9 * (P / 1024 + 2 * (4096 / MAX_TAILS + 1));
}

// the same with global-norm clipping between rule() and the update (include/flsim.h): the stream
// runs as OK_GOUT (g -> clip->G, one fp64 sum of squares per block -> clip->partials), then
// k_clip_finish and k_clip_apply of the optimizer's kind; clip == NULL: the entry point above
int flsim_aggregate_optim_clip_push(const float* S, float* S_out, float* theta_out,
                                    const flsim_rule* rule, const flsim_rule_weights* wts,
                                    const flsim_rule_comp* comp, const flsim_clip* clip, float* p,
                                    float* m, float* v, long P, const long* tensor_sizes,
                                    int n_tensors, long step, const flsim_optim* optim,
                                    hipStream_t stream) {
    RC(check_optim(optim));
    RC(check_weights(wts));
    RC(check_comp(comp, rule));
    RC(check_clip(clip));
    const bool cform = comp != nullptr || theta_out != nullptr;
    const int nstate = optim_n_state(optim);
    FLSIM_REQUIRE(S && p && (m || nstate < 1) && (v || nstate < 2) && tensor_sizes && rule,
                  "null pointer");
    if (nstate < 2) v = nullptr;
    if (nstate < 1) m = nullptr;
    FLSIM_REQUIRE(P > 0 && P < (1L << 31), "P = %ld out of range", P);
    const uintptr_t al = (uintptr_t)S | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v |
                         (uintptr_t)S_out;
    FLSIM_REQUIRE((al & 15) == 0, "S/S_out/p/m/v must be 16-byte aligned");
    AggArgs A{};
    RC(make_rule(rule, &A.R));
    for (int q = 0; q < A.R.narr; ++q)
        FLSIM_REQUIRE(((uintptr_t)A.R.arr[q] & 15) == 0, "entry arrays must be 16-byte aligned");
    OptLaunch ol;
    RC(make_opt_launch(optim, wts ? wts->divisor : (double)rule->k, step, &ol));
    A.ac = ol.ac;
    A.oc = ol.oc;
    if (wts) RC(make_weights(rule, wts, S, S_out, A.w, RULE_MAX_ARR));
    else if (cform) unit_weights(A.R.narr, A.w);
    int nsnap = 0;
    if (cform) {
        CompLaunch cl;
        RC(make_comp(rule, comp, S, S_out, theta_out, p, RULE_MAX_ARR, &cl));
        A.ac.lam = cl.lam;
        A.theta_out = cl.theta_out;
        for (int q = 0; q < A.R.narr; ++q) A.snap[q] = cl.snap[q];
        nsnap = cl.nsnap;
    }
    // the register-array stream for the reference order with <= 2 entry arrays: 2 float4 groups
    // per thread without a stale array, 1 with (tools/agg_bench.py, profiles/r03a/agg_bench.txt:
    // 28.2 vs 28.4 us for k = 512; 32.0 vs 33.1 us for k = 513 with the stale S_{t-d});
    // FLSIM_AGG_G = 1 / 2 forces a form, 0 the LDS-staged k_agg_stream (measurement only)
    int agg_g = A.R.narr == 0 ? 2 : 1;
    if (const char* e = lab_env("FLSIM_AGG_G")) agg_g = atoi(e);
    if (agg_g < 0 || agg_g > AGG_GMAX) agg_g = 1;
    const bool reg = A.R.prog == nullptr && A.R.narr <= 2 && agg_g > 0;
    const int G = reg ? agg_g : 1;
    A.S = S;
    A.S_out = S_out;
    A.p = p;
    A.m = m;
    A.v = v;
    long off = 0;
    for (int t = 0; t < n_tensors; ++t) {
        FLSIM_REQUIRE(tensor_sizes[t] > 0, "tensor %d has size %ld", t, tensor_sizes[t]);
        off += tensor_sizes[t];
    }
    FLSIM_REQUIRE(off == P, "tensor sizes sum to %ld, P = %ld", off, P);
    if (clip) {
        FLSIM_REQUIRE(clip->G && clip->partials && clip->out, "null clip buffer");
        FLSIM_REQUIRE((((uintptr_t)clip->G | (uintptr_t)clip->partials | (uintptr_t)clip->out) &
                       15) == 0, "clip G/partials/out must be 16-byte aligned");
        const float* others[] = {S, S_out, theta_out, p, m, v};
        for (const float* o : others)
            FLSIM_REQUIRE(!overlaps(clip->G, o, P), "clip G overlaps S/S_out/theta_out/p/m/v");
        for (int q = 0; q < A.R.narr; ++q)
            FLSIM_REQUIRE(!overlaps(clip->G, A.R.arr[q], P) && !overlaps(clip->G, A.snap[q], P),
                          "clip G overlaps entry array %d or its snapshot", q);
        A.G = clip->G;
        A.partials = clip->partials;
    }
    // one launch per <= MAX_TAILS tensor tails (the last numel % 32 elements of each tensor);
    // a clipped step first walks the launches without launching, for the partials it will write
    const int ok_launch = clip ? (int)OK_GOUT : ol.ok;
    long n_part = 0;                // blocks launched so far (a clipped step: partials written)
    auto walk = [&](bool dry) -> int {
    n_part = 0;
    off = 0;
    long lo = 0;
    int t = 0;
    while (lo < P) {
        A.ntail = 0;
        long hi = lo;
        while (t < n_tensors) {
            const long n = tensor_sizes[t];
            const long body = rule_body((int)n, wts != nullptr || cform);
            const bool tail = body != n;
            if (tail && A.ntail == MAX_TAILS) break;
            if (tail) {
                A.tail_lo[A.ntail] = (int)(off + body);
                A.tail_hi[A.ntail] = (int)(off + n);
                A.ntail++;
            }
            off += n;
            hi = off;
            ++t;
        }
        A.lo = lo;
        A.hi = hi;
        A.g0 = lo / 4;
        const long groups = (hi + 3) / 4 - A.g0;
        const long gpb = 256L * G;                  // float4 groups per streaming block
        const long nblk = (groups + gpb - 1) / gpb;
        // edge pieces: the first and last block when they cross the launch range, and every
        // block holding a tail range (host copy of block_touch)
        A.nedge = 0;
        auto add_block = [&](long b) {
            const long blo = 4 * (A.g0 + b * gpb);
            for (int j = 0; j < A.nedge; j += 4 * G)
                if (A.edge_lo[j] == blo) return;
            for (int j = 0; j < 4 * G; ++j) A.edge_lo[A.nedge++] = blo + 256 * j;
        };
        for (long b : {0L, nblk - 1}) {
            const long blo = 4 * (A.g0 + b * gpb);
            if (blo < A.lo || blo + 4 * gpb > A.hi) add_block(b);
        }
        for (int j = 0; j < A.ntail; ++j) {
            const long b0 = (A.tail_lo[j] / 4 - A.g0) / gpb;
            const long b1 = ((A.tail_hi[j] - 1) / 4 - A.g0) / gpb;
            for (long b = b0; b <= b1; ++b) add_block(b);
        }
        // algorithmic HBM bytes: read S_t + the distinct entry arrays + p and the kind's state
        // arrays (m, v: 2, 1 or 0 of them); write p and the state arrays [+ S_out]
        // (a clipped step's first launch: S_t + the entry arrays [+ p: C form] read, G written)
        const double bytes = clip
            ? 4.0 * (double)(hi - lo) * (2 + (cform ? 1 : 0) + A.R.distinct + (S_out ? 1 : 0) +
                                         nsnap + (theta_out ? 1 : 0))
            : 4.0 * (double)(hi - lo) * (3 + 2 * nstate + A.R.distinct + (S_out ? 1 : 0) + nsnap +
                                         (theta_out ? 1 : 0));
        A.part0 = n_part;
        n_part += nblk + A.nedge;
        lo = hi;
        if (dry) continue;
        const ProbeSlot ps = probe_begin();
        const dim3 grid((unsigned)(nblk + A.nedge));
        if (!reg && A.R.prog != nullptr) RC(stage_program(A.R, stream));
        if (cform) launch_agg_kind<true, true>(ok_launch, reg, G, grid, stream, ps, A);
        else if (wts) launch_agg_kind<true>(ok_launch, reg, G, grid, stream, ps, A);
        else launch_agg_kind<false>(ok_launch, reg, G, grid, stream, ps, A);
        FLSIM_LAUNCH_CHECK();
        if (probe_end(ps, clip ? K_AGG_GOUT : (A.R.prog == nullptr ? K_AGG : K_AGG_SEQ), bytes))
            return 2;
    }
    return 0;
    };
    if (!clip) return walk(false);
    RC(walk(true));
    FLSIM_REQUIRE(clip->n_partials >= n_part, "clip n_partials = %ld, this step writes %ld",
                  clip->n_partials, n_part);
    RC(walk(false));
    return clip_finish_apply(clip, n_part, ol, p, m, v, P, stream);
}

// reference order: weight_ups = [S] * c + stale[0 .. n_stale) (main.py:161-172)
int flsim_aggregate_adam(const float* S, int c, const float* const* stale, int n_stale,
                         float* p, float* m, float* v, long P, const long* tensor_sizes,
                         int n_tensors, long step, double lr, double beta1, double beta2,
                         double eps, hipStream_t stream) {
    FLSIM_REQUIRE(c >= 0 && n_stale >= 0 && n_stale <= 8, "bad entry counts c=%d ns=%d", c,
                  n_stale);
    FLSIM_REQUIRE(c + n_stale > 0, "empty weight_ups (reference: IndexError in rule, main.py:25)");
    flsim_rule r{};
    r.k = c + n_stale;
    r.c = c;
    r.n_arrays = n_stale;
    for (int q = 0; q < n_stale; ++q) r.arrays[q] = stale ? stale[q] : nullptr;
    return flsim_aggregate_adam_rule(S, &r, p, m, v, P, tensor_sizes, n_tensors, step, lr, beta1,
                                     beta2, eps, stream);
}

// independent-entry semantics: S already holds the sum of the k distinct entries
int flsim_aggregate_adam_sum(const float* S, int k, float* p, float* m, float* v, long P,
                             const long* tensor_sizes, int n_tensors, long step, double lr,
                             double beta1, double beta2, double eps, hipStream_t stream) {
    FLSIM_REQUIRE(k > 0, "empty weight_ups (reference: IndexError in rule, main.py:25)");
    flsim_rule r{};
    r.k = k;
    r.c = 1;
    return flsim_aggregate_adam_rule(S, &r, p, m, v, P, tensor_sizes, n_tensors, step, lr, beta1,
                                     beta2, eps, stream);
}

// host: rule()'s summation program for k entries with the non-S entries at pos[] (increasing)
// holding array arr[], in the device's macro-word form (cascade.h): prog[cap] int32 = pairs (lo,
// hi) + one fetch-pad pair; info[4] = {pairs, pair index of the row_sum part, need, lp}.
int flsim_cascade_program(int k, const int32_t* pos, const int32_t* arr, int n_events,
                          int32_t* prog, int cap, int32_t* info) {
    FLSIM_REQUIRE(prog && info && (n_events == 0 || (pos && arr)), "null pointer");
    FLSIM_REQUIRE(n_events >= 0 && n_events <= CASC_MAX_K, "n_events = %d", n_events);
    const int ocap = 72 + 40 * (n_events + 8);
    int32_t* ops = new int32_t[ocap];
    CascInfo ci{};
    int len = build_cascade_program(k, pos, arr, n_events, ops, ocap, &ci);
    CascInfo mi{};
    if (len > 0) len = build_macro_program(ops, ci, reinterpret_cast<uint32_t*>(prog), cap / 2, &mi);
    delete[] ops;
    FLSIM_REQUIRE(len != -3, "k = %d entries: supported 1 .. %d", k, CASC_MAX_K);
    FLSIM_REQUIRE(len != -1, "events must have increasing positions in [0, k) and arrays >= 0");
    FLSIM_REQUIRE(len > 0, "program longer than %d words (or an array index past 63)", cap);
    info[0] = mi.len;
    info[1] = mi.tail_off;
    info[2] = mi.need;
    info[3] = mi.lp;
    return 0;
}

// host interpreter of a macro program (testing): out[e] = the cascade sum of element e, x = S[e],
// entry arrays ys[q][e]; tail[e] != 0 selects the row_sum program.  wf (nullable): entry array q
// enters as ys[q][e] * wf[q]; fdiv != 0: out[e] = sum / fdiv.
// theta_now / theta_src / lam (nullable): the C kernels' compensation in front of the weight.
static void eval_host(const int32_t* prog, const int32_t* info, const float* S,
                      const float* const* ys, const float* wf, int n_arrays, float fdiv,
                      const uint8_t* tail, long n, float* out, const float* theta_now = nullptr,
                      const float* const* theta_src = nullptr, float lam = 0.f) {
    struct HostPairs {
        const int32_t* w;
        uint32_t lo(int i) const { return (uint32_t)w[2 * i]; }
        uint32_t hi(int i) const { return (uint32_t)w[2 * i + 1]; }
    } hp{prog};
    for (long e = 0; e < n; ++e) {
        const CascVals<float> cv = casc_values(S[e], info[2], info[3]);
        auto yf = [&](int q) -> float {
            if (!(q < n_arrays && ys[q])) return 0.f;
            float y = ys[q][e];
            if (theta_src && theta_src[q]) y = compensate(y, theta_now[e], theta_src[q][e], lam);
            return wf ? y * wf[q] : y;
        };
        const float s = casc_run_macro(hp, (tail && tail[e]) ? info[1] : 0, cv, yf);
        out[e] = fdiv != 0.f ? s / fdiv : s;
    }
}

int flsim_cascade_eval_host(const int32_t* prog, const int32_t* info, const float* S,
                            const float* const* ys, int n_arrays, const uint8_t* tail, long n,
                            float* out) {
    FLSIM_REQUIRE(prog && info && S && out, "null pointer");
    eval_host(prog, info, S, ys, nullptr, n_arrays, 0.f, tail, n, out);
    return 0;
}

// the weighted twin of the W kernels (testing): entry array q enters as ys[q][e] * (float)w[q]
// (one fp32 multiply where the value is loaded) and out[e] = sum / (float)divisor (the IEEE
// division); weights and divisor are refused as the entry points refuse them
int flsim_cascade_eval_host_w(const int32_t* prog, const int32_t* info, const float* S,
                              const float* const* ys, const double* w, int n_arrays,
                              double divisor, const uint8_t* tail, long n, float* out) {
    FLSIM_REQUIRE(n_arrays >= 0 && n_arrays <= RULE_MAX_ARR, "n_arrays = %d", n_arrays);
    FLSIM_REQUIRE(w || n_arrays == 0, "null pointer");
    flsim_rule_weights rw{};
    rw.n = n_arrays;
    for (int q = 0; q < n_arrays; ++q) rw.w[q] = w[q];
    rw.divisor = divisor;
    RC(check_weights(&rw));
    FLSIM_REQUIRE(prog && info && S && out && (ys || n_arrays == 0), "null pointer");
    AdamConst ac;
    RC(make_divisor(divisor, &ac));
    float wf[RULE_MAX_ARR];
    for (int q = 0; q < n_arrays; ++q) wf[q] = (float)w[q];
    eval_host(prog, info, S, ys, wf, n_arrays, ac.fk, tail, n, out);
    return 0;
}

// the compensated twin of the C kernels (testing): flsim_cascade_eval_host_w with
// compensate(ys[q][e], theta_now[e], theta_src[q][e], (float)lambda) in front of the weight for
// every array with a snapshot; w == NULL: weights 1.0.  lambda is refused as the entry points
// refuse it.
int flsim_cascade_eval_host_c(const int32_t* prog, const int32_t* info, const float* S,
                              const float* const* ys, const double* w, int n_arrays,
                              double divisor, const float* theta_now,
                              const float* const* theta_src, double lambda, const uint8_t* tail,
                              long n, float* out) {
    FLSIM_REQUIRE(n_arrays >= 0 && n_arrays <= RULE_MAX_ARR, "n_arrays = %d", n_arrays);
    flsim_rule_weights rw{};
    rw.n = n_arrays;
    for (int q = 0; q < n_arrays; ++q) rw.w[q] = w ? w[q] : 1.0;
    rw.divisor = divisor;
    RC(check_weights(&rw));
    FLSIM_REQUIRE(lambda >= 0.0 && lambda <= 3.0e38, "Invalid delay compensation lambda %g",
                  lambda);
    FLSIM_REQUIRE(prog && info && S && out && (ys || n_arrays == 0) && (theta_now || !theta_src),
                  "null pointer");
    AdamConst ac;
    RC(make_divisor(divisor, &ac));
    float wf[RULE_MAX_ARR];
    for (int q = 0; q < n_arrays; ++q) wf[q] = (float)rw.w[q];
    eval_host(prog, info, S, ys, wf, n_arrays, ac.fk, tail, n, out, theta_now, theta_src,
              (float)lambda);
    return 0;
}

// the clipped step's twin (testing): g as the twins above give it (w == NULL and theta_src ==
// NULL: the plain mean), then total_norm = (float)sqrt(sum of the fp64 squares, in element
// order), coef = min(RN(1 / (total_norm + f32(1e-6))) * f32(max_norm), 1) with a NaN kept, and
// g_out = g * coef.  max_norm is refused as the entry point refuses it.
int flsim_cascade_eval_host_clip(const int32_t* prog, const int32_t* info, const float* S,
                                 const float* const* ys, const double* w, int n_arrays,
                                 double divisor, const float* theta_now,
                                 const float* const* theta_src, double lambda, const uint8_t* tail,
                                 long n, double max_norm, float* g_out, float* norm_coef) {
    flsim_clip c{};
    c.max_norm = (float)max_norm;
    RC(check_clip(&c));
    FLSIM_REQUIRE(g_out && norm_coef, "null pointer");
    if (w || theta_src) {
        RC(flsim_cascade_eval_host_c(prog, info, S, ys, w, n_arrays, divisor, theta_now,
                                     theta_src, lambda, tail, n, g_out));
    } else {
        FLSIM_REQUIRE(n_arrays >= 0 && n_arrays <= RULE_MAX_ARR, "n_arrays = %d", n_arrays);
        FLSIM_REQUIRE(prog && info && S && (ys || n_arrays == 0), "null pointer");
        AdamConst ac;
        RC(make_divisor(divisor, &ac));
        eval_host(prog, info, S, ys, nullptr, n_arrays, ac.fk, tail, n, g_out);
    }
    double tot = 0.0;
    for (long e = 0; e < n; ++e) tot += (double)g_out[e] * (double)g_out[e];
    volatile float t = (float)sqrt(tot), one = 1.f, eps = 1e-6f;
    volatile float den = t + eps;
    volatile float rcp = one / den;
    float coef = rcp * c.max_norm;
    coef = coef > 1.0f ? 1.0f : coef;
    for (long e = 0; e < n; ++e) g_out[e] = g_out[e] * coef;
    norm_coef[0] = t;
    norm_coef[1] = coef;
    return 0;
}

// ---- robust rules: median / trimmed mean over bucket means + the update (include/flsim.h) --------
// One launch of k_robust in the optimizer's kind; optim == NULL: OK_GOUT writing g_out alone; clip:
// OK_GOUT writing clip->G and the per-block partials, then k_clip_finish and k_clip_apply as the
// clipped entry point above runs them.
int flsim_robust_optim_step(const flsim_robust* r, const flsim_clip* clip, float* g_out, float* p,
                            float* m, float* v, long P, long step, const flsim_optim* optim,
                            hipStream_t stream) {
    RC(check_robust(r));
    BucketStep B;
    RC(step_begin(optim, clip, g_out, p, m, v, P, step, &B));
    RC(check_clip_buffers(B, nullptr));
    RobustArgs A{};
    int distinct = 0;
    RC(fill_entries(B, r->entries, r->count, r->k, "", nullptr, 0, nullptr, &A.T, &distinct));
    const int kpad = robust_kpad(r->k);
    A.k = r->k;
    A.kind = r->kind;
    A.trim = r->trim;
    A.fn = (float)(r->k - 2 * r->trim);
    // the rule's own arrays: each distinct entry read once
    return launch_apply(B, A, K_ROBUST, distinct, stream,
                        [&](auto ok, dim3 grid, const ProbeSlot& ps) {
                            with_kpad<2>(kpad, [&](auto kp) {
                                hipExtLaunchKernelGGL(
                                    (k_robust<decltype(kp)::value, decltype(ok)::value>), grid,
                                    dim3(256), 0, stream, ps.start, ps.stop, 0, A);
                            });
                        });
}

// host (testing): g of the rule text for host pointers, through robust.h's network and select / sum
int flsim_robust_eval_host(const flsim_robust* r, long P, float* g_out) {
    RC(check_robust(r));
    FLSIM_REQUIRE(g_out, "null pointer");
    FLSIM_REQUIRE(P > 0, "P = %ld out of range", P);
    with_kpad<2>(robust_kpad(r->k), [&](auto kp) {
        robust_eval_host<decltype(kp)::value>(r, P, g_out);
    });
    return 0;
}

// ---- Krum / Multi-Krum over bucket means + the update (include/flsim.h) --------------------------
long flsim_krum_partials(long P, int k) {
    if (k < 1 || k > RULE_MAX_ARR || P < 1 || P >= (1L << 31)) return 0;
    return pair_partials(P, k);
}

long flsim_krum_tile_elems(int k) {
    if (k < 1 || k > RULE_MAX_ARR) return 0;
    return krum_tile_elems(krum_kpad(k));
}

// Three launches: k_krum_dist -> s->partials; k_krum_finish -> s->dist, s->score, s->sel;
// k_krum_apply in the optimizer's kind (optim == NULL: OK_GOUT writing g_out alone; clip: OK_GOUT
// writing clip->G and the per-block partials, then k_clip_finish and k_clip_apply).
int flsim_krum_optim_step(const flsim_krum* r, const flsim_krum_scratch* s, const flsim_clip* clip,
                          float* g_out, float* p, float* m, float* v, long P, long step,
                          const flsim_optim* optim, hipStream_t stream) {
    RC(check_krum(r));
    BucketStep B;
    RC(step_begin(optim, clip, g_out, p, m, v, P, step, &B));
    static const char name[] = "Krum";
    const flsim_krum_scratch none{};
    if (!s) s = &none;
    const long n_dist = pair_partials(P, r->k);
    constexpr int NS = 4;
    const Span sc[NS] = {{s->partials, 8 * n_dist},
                         {s->dist, 8L * r->k * r->k},
                         {s->score, 8L * r->k},
                         {s->sel, 4L * r->m}};
    RC(check_scratch_pointers(name, sc, NS, s->n_partials, n_dist));
    RC(check_scratch(B, name, sc, NS, nullptr));
    RC(check_clip_buffers(B, nullptr));
    KrumApplyArgs A{};
    int distinct = 0;
    RC(fill_entries(B, r->entries, r->count, r->k, name, sc, NS, nullptr, &A.T, &distinct));
    // the finish launch's own bytes: sel written
    RC(launch_pair_dist(A.T, s->partials, P, r->k, K_KRUM_DIST, distinct, K_KRUM_FIN, 4.0 * r->m,
                        stream, [&](const ProbeSlot& ps, const double* part, int nblocks, int nb) {
                            hipExtLaunchKernelGGL(k_krum_finish, dim3(1), dim3(KRUM_FIN_THREADS), 0,
                                                  stream, ps.start, ps.stop, 0, part, nblocks, nb,
                                                  (int)r->k, (int)r->f, (int)r->m, s->dist,
                                                  s->score, s->sel);
                        }));
    A.sel = s->sel;
    A.nsel = r->m;
    A.fm = (float)r->m;
    // the rule's own arrays: the m selected entries read
    return launch_apply(B, A, K_KRUM_APPLY, r->m, stream,
                        [&](auto ok, dim3 grid, const ProbeSlot& ps) {
                            hipExtLaunchKernelGGL((k_krum_apply<decltype(ok)::value>), grid,
                                                  dim3(256), 0, stream, ps.start, ps.stop, 0, A);
                        });
}

// host (testing): the text for host pointers.  The bucket means by one fp32 division each, every
// distance as the fp64 sum of the squared fp64 differences in element order (a pair is computed
// once and mirrored), NaN -> +inf, then csrc/krum.h's score / selection code and g as the text
// forms it.
int flsim_krum_eval_host(const flsim_krum* r, long P, double* dist, double* score, int32_t* sel,
                         float* g_out) {
    RC(check_krum(r));
    FLSIM_REQUIRE(dist && score && sel, "null pointer");
    FLSIM_REQUIRE(P > 0, "P = %ld out of range", P);
    const int k = r->k;
    auto mean = [&](int j, long e) { return bucket_mean(r->entries, r->count, j, e); };
    pair_dist_host(mean, k, P, dist);
    int32_t rank[RULE_MAX_ARR];
    krum_score_select(dist, score, rank, sel, k, (int)r->f, (int)r->m, 0, 1, [] {});
    if (!g_out) return 0;
    for (long e = 0; e < P; ++e) {
        volatile float acc = mean(sel[0], e);
        for (int t = 1; t < r->m; ++t) acc = acc + mean(sel[t], e);
        volatile float fm = (float)r->m;
        g_out[e] = acc / fm;
    }
    return 0;
}

// ---- Bulyan over bucket means + the update (include/flsim.h) -------------------------------------
long flsim_bulyan_partials(long P, int k) { return flsim_krum_partials(P, k); }   // (pair_partials)

// Three launches: k_krum_dist -> s->partials (Krum's launch and geometry); k_bulyan_finish ->
// s->dist, s->score, s->order, s->sel; k_bulyan_apply in the optimizer's kind (optim == NULL:
// OK_GOUT writing g_out alone; clip: OK_GOUT writing clip->G and the per-block partials, then
// k_clip_finish and k_clip_apply).
int flsim_bulyan_optim_step(const flsim_bulyan* r, const flsim_bulyan_scratch* s,
                            const flsim_clip* clip, float* g_out, float* p, float* m, float* v,
                            long P, long step, const flsim_optim* optim, hipStream_t stream) {
    RC(check_bulyan(r));
    BucketStep B;
    RC(step_begin(optim, clip, g_out, p, m, v, P, step, &B));
    static const char name[] = "Bulyan";
    const flsim_bulyan_scratch none{};
    if (!s) s = &none;
    const int theta = r->k - 2 * r->f, beta = theta - 2 * r->f;
    const long n_dist = pair_partials(P, r->k);
    constexpr int NS = 5;
    const Span sc[NS] = {{s->partials, 8 * n_dist},
                         {s->dist, 8L * r->k * r->k},
                         {s->score, 8L * theta},
                         {s->order, 4L * theta},
                         {s->sel, 4L * theta}};
    RC(check_scratch_pointers(name, sc, NS, s->n_partials, n_dist));
    RC(check_scratch(B, name, sc, NS, nullptr));
    RC(check_clip_buffers(B, nullptr));
    BulyanApplyArgs A{};
    int distinct = 0;
    RC(fill_entries(B, r->entries, r->count, r->k, name, sc, NS, nullptr, &A.T, &distinct));
    // the finish launch's own bytes: order and sel written
    RC(launch_pair_dist(A.T, s->partials, P, r->k, K_BULYAN_DIST, distinct, K_BULYAN_FIN,
                        8.0 * theta, stream,
                        [&](const ProbeSlot& ps, const double* part, int nblocks, int nb) {
                            hipExtLaunchKernelGGL(k_bulyan_finish, dim3(1), dim3(KRUM_FIN_THREADS),
                                                  0, stream, ps.start, ps.stop, 0, part, nblocks,
                                                  nb, (int)r->k, (int)r->f, s->dist, s->score,
                                                  s->order, s->sel);
                        }));
    A.sel = s->sel;
    A.theta = theta;
    A.beta = beta;
    A.fbeta = (float)beta;
    const int kpad = robust_kpad(theta);
    // the rule's own arrays: the theta selected entries read
    return launch_apply(B, A, K_BULYAN_APPLY, theta, stream,
                        [&](auto ok, dim3 grid, const ProbeSlot& ps) {
                            with_kpad<4>(kpad, [&](auto kp) {
                                hipExtLaunchKernelGGL(
                                    (k_bulyan_apply<decltype(kp)::value, decltype(ok)::value>),
                                    grid, dim3(256), 0, stream, ps.start, ps.stop, 0, A);
                            });
                        });
}

// host (testing): the text for host pointers.  The distances as flsim_krum_eval_host forms them,
// then csrc/bulyan.h's selection and, per element, its window and sum over the selected means.
int flsim_bulyan_eval_host(const flsim_bulyan* r, long P, double* dist, double* score,
                           int32_t* order, int32_t* sel, float* g_out) {
    RC(check_bulyan(r));
    FLSIM_REQUIRE(dist && score && order && sel, "null pointer");
    FLSIM_REQUIRE(P > 0, "P = %ld out of range", P);
    const int k = r->k, theta = k - 2 * r->f;
    auto mean = [&](int j, long e) { return bucket_mean(r->entries, r->count, j, e); };
    pair_dist_host(mean, k, P, dist);
    uint8_t nbr[RULE_MAX_ARR * RULE_MAX_ARR];
    double work[RULE_MAX_ARR];
    bulyan_order(dist, nbr, work, score, order, sel, k, (int)r->f, 0, 1, [] {});
    if (!g_out) return 0;
    with_kpad<4>(robust_kpad(theta), [&](auto kp) {
        bulyan_eval_host<decltype(kp)::value>(r, sel, P, g_out);
    });
    return 0;
}

// ---- geometric median (RFA) over bucket means + the update (include/flsim.h) ---------------------
long flsim_geomed_partials(long P, int k) {
    if (k < 1 || k > RULE_MAX_ARR || P < 1 || P >= (1L << 31)) return 0;
    return geomed_blocks(P, geomed_kpad(k)) * (k + 1);
}

long flsim_geomed_tile_elems(int k) {
    if (k < 1 || k > RULE_MAX_ARR) return 0;
    return geomed_tile_elems(geomed_kpad(k));
}

// iters + 1 pairs (k_geomed_dist -> s->partials; k_geomed_finish -> s->d2, s->obj, s->w,
// s->state), then k_geomed_apply in the optimizer's kind (optim == NULL: OK_GOUT writing g_out
// alone; clip: OK_GOUT writing clip->G and the per-block partials, then k_clip_finish and
// k_clip_apply).
int flsim_geomed_optim_step(const flsim_geomed* r, const flsim_geomed_scratch* s,
                            const flsim_clip* clip, float* g_out, float* p, float* m, float* v,
                            long P, long step, const flsim_optim* optim, hipStream_t stream) {
    RC(check_geomed(r));
    BucketStep B;
    RC(step_begin(optim, clip, g_out, p, m, v, P, step, &B));
    static const char name[] = "geometric-median";
    const flsim_geomed_scratch none{};
    if (!s) s = &none;
    const int k = r->k, iters = r->iters;
    const int kpad = geomed_kpad(k);
    const long nblocks = geomed_blocks(P, kpad);
    const long n_dist = nblocks * (k + 1);
    // (a buffer of no bytes -- d2 and obj at iters = 0 -- overlaps nothing)
    constexpr int NS = 5;
    const Span sc[NS] = {{s->partials, 8 * n_dist},
                         {s->w, 8L * (iters + 1) * k},
                         {s->d2, 8L * iters * k},
                         {s->obj, 8L * iters},
                         {s->state, 4L * (k + GEOMED_ST_WORDS)}};
    RC(check_scratch_pointers(name, sc, NS, s->n_partials, n_dist));
    RC(check_scratch(B, name, sc, NS, nullptr));
    RC(check_clip_buffers(B, nullptr));
    GeomedDistArgs D{};
    GeomedFinArgs F{};
    GeomedApplyArgs A{};
    int distinct = 0;
    RC(fill_entries(B, r->entries, r->count, k, name, sc, NS, nullptr, &D.T, &distinct));
    A.T = D.T;
    double alpha[RULE_MAX_ARR];
    for (int j = 0; j < k; ++j) {
        F.count[j] = r->count[j];
        alpha[j] = geomed_alpha(r->weighted, r->count[j], 0);
    }
    geomed_w0(alpha, k, D.w0);
    D.w = s->w;
    D.state = s->state;
    D.partials = s->partials;
    D.P = P;
    D.k = k;
    D.ntiles = (int)geomed_tiles(P, kpad);
    D.iters = iters;
    F.partials = s->partials;
    F.w = s->w;
    F.d2 = s->d2;
    F.obj = s->obj;
    F.state = s->state;
    F.nu = r->nu;
    F.nblocks = (int)nblocks;
    F.k = k;
    F.iters = iters;
    F.weighted = r->weighted;
    for (int pair = 0; pair <= iters; ++pair) {
        D.pair = F.pair = pair;
        {
            const ProbeSlot ps = probe_begin();
            const dim3 grid((unsigned)nblocks);
            with_kpad<4>(kpad, [&](auto kp) {
                constexpr int KPAD = decltype(kp)::value;
                if (pair == 0)
                    hipExtLaunchKernelGGL((k_geomed_dist<KPAD, true>), grid, dim3(256), 0, stream,
                                          ps.start, ps.stop, 0, D);
                else
                    hipExtLaunchKernelGGL((k_geomed_dist<KPAD, false>), grid, dim3(256), 0, stream,
                                          ps.start, ps.stop, 0, D);
            });
            FLSIM_LAUNCH_CHECK();
            // algorithmic HBM bytes: each distinct entry read once
            if (probe_end(ps, K_GEOMED_DIST, 4.0 * (double)P * distinct)) return 2;
        }
        const ProbeSlot ps = probe_begin();
        hipExtLaunchKernelGGL(k_geomed_finish, dim3(1), dim3(GEOMED_FIN_THREADS), 0, stream,
                              ps.start, ps.stop, 0, F);
        FLSIM_LAUNCH_CHECK();
        if (probe_end(ps, K_GEOMED_FIN, 8.0 * (double)nblocks * (k + (pair == 0)) + 8.0 * (3 * k + 1)))
            return 2;
    }
    A.w = s->w + (long)iters * k;
    A.k = k;
    // the rule's own arrays: the distinct entries read
    return launch_apply(B, A, K_GEOMED_APPLY, distinct, stream,
                        [&](auto ok, dim3 grid, const ProbeSlot& ps) {
                            hipExtLaunchKernelGGL((k_geomed_apply<decltype(ok)::value>), grid,
                                                  dim3(256), 0, stream, ps.start, ps.stop, 0, A);
                        });
}

// host (testing): the text for host pointers.  The bucket means by one fp32 division each; z as
// _wsum forms it; every distance as the fp64 sum of ((double)x_j - z)^2 in element order (one fma
// each, as the kernel's); then csrc/geomed.h's scalar code, and g = (float)z at w^(iters).
int flsim_geomed_eval_host(const flsim_geomed* r, long P, double* w, double* d2, double* obj,
                           float* g_out) {
    RC(check_geomed(r));
    const int k = r->k, iters = r->iters;
    FLSIM_REQUIRE(w && (iters == 0 || (d2 && obj)), "null pointer");
    FLSIM_REQUIRE(P > 0, "P = %ld out of range", P);
    auto mean = [&](int j, long e) { return bucket_mean(r->entries, r->count, j, e); };
    auto wsum = [&](const double* wt, long e) { return wsum_host(mean, wt, k, e); };
    int32_t dead[RULE_MAX_ARR];
    double a[RULE_MAX_ARR], term[RULE_MAX_ARR], sums[2];
    dead_scan_host(mean, k, P, dead);
    for (int j = 0; j < k; ++j) a[j] = geomed_alpha(r->weighted, r->count[j], dead[j]);
    geomed_w0(a, k, w);
    for (int it = 0; it < iters; ++it) {
        double* d = d2 + (long)it * k;
        d2_host(mean, [&](long e) { return wsum(w + (long)it * k, e); }, dead, k, P, d);
        geomed_iterate(d, a, dead, k, r->nu, term, sums, w + (long)(it + 1) * k, 0, 1, [] {});
        obj[it] = sums[0];
    }
    if (!g_out) return 0;
    for (long e = 0; e < P; ++e) g_out[e] = (float)wsum(w + (long)iters * k, e);
    return 0;
}

// ---- simulated Byzantine workers: IPM / ALIE mixed into the bucket sums (include/flsim.h) --------
long flsim_attack_tile_elems(int k) {
    if (k < 1 || k > RULE_MAX_ARR) return 0;
    return attack_tile_elems(attack_kpad(k));
}

// one launch of k_attack on `stream`
int flsim_attack_entries(const flsim_attack* a, float* b_out, long P, hipStream_t stream) {
    int kh = 0;
    RC(check_attack(a, &kh));
    RC(check_attack_pointers(a->entries, a->k, b_out, P));
    AttackArgs A{};
    int nread = 0, nwritten = 0;
    for (int j = 0; j < a->k; ++j) {
        A.ent[j] = a->entries[j];
        A.honest[j] = a->honest[j];
        A.byz[j] = a->byz[j];
        nread += a->honest[j] > 0;
        nwritten += a->byz[j] > 0;
    }
    A.b_out = b_out;
    A.strength = a->strength;
    A.P = P;
    A.k = a->k;
    A.kh = kh;
    const int kpad = attack_kpad(a->k);
    A.ntiles = (int)attack_tiles(P, kpad);
    const dim3 grid((unsigned)attack_blocks(P, kpad));
    const ProbeSlot ps = probe_begin();
    with_kpad<4>(kpad, [&](auto kp) {
        launch_attack<decltype(kp)::value>(a->kind, grid, stream, ps, A);
    });
    FLSIM_LAUNCH_CHECK();
    // algorithmic HBM bytes: the honest entries read, the Byzantine-holding ones and b_out written
    if (probe_end(ps, K_ATTACK, 4.0 * (double)P * (nread + nwritten + (b_out ? 1 : 0)))) return 2;
    return 0;
}

// host (testing): the same checks, then csrc/attack.h's element code over host pointers
int flsim_attack_eval_host(const flsim_attack* a, float* b_out, long P) {
    int kh = 0;
    RC(check_attack(a, &kh));
    RC(check_attack_pointers(a->entries, a->k, b_out, P));
    if (a->kind == FLSIM_ATTACK_IPM)
        attack_eval_host<FLSIM_ATTACK_IPM>(a, kh, b_out, P);
    else
        attack_eval_host<FLSIM_ATTACK_ALIE>(a, kh, b_out, P);
    return 0;
}

// ---- the optimised attacks Min-Max / Min-Sum mixed into the bucket sums (include/flsim.h) ---------
long flsim_attack_opt_partials(long P, int k) {
    if (k < 1 || k > RULE_MAX_ARR || P < 1 || P >= (1L << 31)) return 0;
    long n = 0;
    for (int kh = 1; kh <= k; ++kh) {
        const long m = pair_partials(P, kh) + attack_opt_stats_partials(P, kh) + 1;
        n = m > n ? m : n;
    }
    return n;
}

long flsim_attack_opt_tile_elems(int kh) {
    if (kh < 1 || kh > RULE_MAX_ARR) return 0;
    return attack_opt_tile_elems(attack_opt_kpad(kh));
}

// Four launches on `stream`: k_attack_opt_stats -> the second part of s->partials; k_krum_dist
// over the honest entries -> the first part (Krum's launch and geometry); k_attack_opt_finish ->
// s->dist, s->stats, s->gamma and gamma * strength in the last word of the partials; k_attack's
// mix, which reads that word.  (The stats launch goes first:
// the pairwise stage issues its finish right after its distance launch, and the two streaming
// launches do not depend on each other.)
int flsim_attack_opt_entries(const flsim_attack_opt* a, const flsim_attack_opt_scratch* s,
                             float* b_out, long P, hipStream_t stream) {
    int kh = 0;
    RC(check_attack_opt(a, &kh));
    RC(check_attack_pointers(a->entries, a->k, b_out, P));
    static const char name[] = "attack";
    const flsim_attack_opt_scratch none{};
    if (!s) s = &none;
    const int k = a->k;
    const long n_pair = pair_partials(P, kh), n_stats = attack_opt_stats_partials(P, kh);
    constexpr int NS = 4;
    const Span sc[NS] = {{s->partials, 8 * (n_pair + n_stats + 1)},
                         {s->dist, 8L * kh * kh},
                         {s->stats, 8L * FLSIM_ATTACK_OPT_STATS},
                         {s->gamma, 8}};
    RC(check_scratch_pointers(name, sc, NS, s->n_partials, n_pair + n_stats + 1));
    // the entries (read or written) and b_out against the scratch, then the scratch against itself
    StepBuffers B{};
    B.P = P;
    for (int c = 0; c < NS; ++c)
        FLSIM_REQUIRE(!overlaps(sc[c].ptr, sc[c].bytes, b_out, 4 * P),
                      "b_out overlaps the %s scratch", name);
    EntryTable all{}, T{};
    int distinct = 0;
    int32_t ones[RULE_MAX_ARR], hcnt[RULE_MAX_ARR];
    const float* hent[RULE_MAX_ARR];
    for (int j = 0, i = 0; j < k; ++j) {
        ones[j] = 1;
        if (a->honest[j] > 0) {
            hent[i] = a->entries[j];
            hcnt[i++] = a->honest[j];
        }
    }
    RC(fill_entries(B, a->entries, ones, k, name, sc, NS, nullptr, &all, &distinct));
    RC(check_scratch(B, name, sc, NS, nullptr));
    RC(fill_entries(B, hent, hcnt, kh, name, nullptr, 0, nullptr, &T, &distinct));
    double* const stats_part = s->partials + n_pair;
    const int spad = attack_opt_kpad(kh);
    const long sblocks = attack_opt_blocks(P, spad);
    {
        AttackOptStatsArgs S{};
        for (int i = 0; i < kh; ++i) {
            S.ent[i] = hent[i];
            S.honest[i] = hcnt[i];
        }
        S.partials = stats_part;
        S.P = P;
        S.kh = kh;
        S.ntiles = (int)attack_opt_tiles(P, spad);
        const ProbeSlot ps = probe_begin();
        const dim3 grid((unsigned)sblocks);
        with_kpad<4>(spad, [&](auto kp) {
            with_dir(a->dir, [&](auto d) {
                hipExtLaunchKernelGGL(
                    (k_attack_opt_stats<decltype(kp)::value, decltype(d)::value>), grid, dim3(256),
                    0, stream, ps.start, ps.stop, 0, S);
            });
        });
        FLSIM_LAUNCH_CHECK();
        // algorithmic HBM bytes: the honest entries read once
        if (probe_end(ps, K_ATTACK, 4.0 * (double)P * kh)) return 2;
    }
    const AttackOptFinArgs F{stats_part, (int)sblocks, 2 * kh + 1};
    RC(launch_pair_dist(T, s->partials, P, kh, K_ATTACK, distinct, K_ATTACK,
                        8.0 * (double)sblocks * (2 * kh + 1) + 8.0 * (2 * kh + 2), stream,
                        [&](const ProbeSlot& ps, const double* part, int nblocks, int nb) {
                            hipExtLaunchKernelGGL(k_attack_opt_finish, dim3(1),
                                                  dim3(KRUM_FIN_THREADS), 0, stream, ps.start,
                                                  ps.stop, 0, part, nblocks, nb, kh, F,
                                                  (int)a->kind, a->strength, s->dist, s->stats,
                                                  s->gamma, stats_part + n_stats);
                        }));
    AttackArgs A{};
    int nwritten = 0;
    for (int j = 0; j < k; ++j) {
        A.ent[j] = a->entries[j];
        A.honest[j] = a->honest[j];
        A.byz[j] = a->byz[j];
        nwritten += a->byz[j] > 0;
    }
    A.b_out = b_out;
    A.coef = stats_part + n_stats;
    A.P = P;
    A.k = k;
    A.kh = kh;
    const int kpad = attack_kpad(k);
    A.ntiles = (int)attack_tiles(P, kpad);
    const dim3 grid((unsigned)attack_blocks(P, kpad));
    const ProbeSlot ps = probe_begin();
    with_kpad<4>(kpad, [&](auto kp) {
        launch_attack<decltype(kp)::value>(ATTACK_CRAFT_OPT + a->dir, grid, stream, ps, A);
    });
    FLSIM_LAUNCH_CHECK();
    if (probe_end(ps, K_ATTACK, 4.0 * (double)P * (kh + nwritten + (b_out ? 1 : 0)))) return 2;
    return 0;
}

// host (testing): the same checks about a, the entries, b_out and P, then attack_opt_eval_host
int flsim_attack_opt_eval_host(const flsim_attack_opt* a, double* dist, double* stats,
                               double* gamma, float* b_out, long P) {
    int kh = 0;
    RC(check_attack_opt(a, &kh));
    RC(check_attack_pointers(a->entries, a->k, b_out, P));
    FLSIM_REQUIRE(dist && stats && gamma, "null pointer");
    const float* hent[RULE_MAX_ARR];
    int32_t hcnt[RULE_MAX_ARR];
    for (int j = 0, i = 0; j < a->k; ++j)
        if (a->honest[j] > 0) {
            hent[i] = a->entries[j];
            hcnt[i++] = a->honest[j];
        }
    pair_dist_host([&](int j, long e) { return bucket_mean(hent, hcnt, j, e); }, kh, P, dist);
    with_dir(a->dir, [&](auto d) {
        attack_opt_eval_host<decltype(d)::value>(a, kh, stats, gamma, dist, b_out, P);
    });
    return 0;
}

// ---- nearest-neighbour mixing of the entries, in place (include/flsim.h) --------------------------
long flsim_nnm_partials(long P, int k) { return flsim_krum_partials(P, k); }   // (pair_partials)

long flsim_nnm_tile_elems(int k) {
    if (k < 1 || k > RULE_MAX_ARR) return 0;
    return nnm_tile_elems(nnm_kpad(k));
}

// Three launches on `stream`: k_krum_dist -> s->partials (Krum's launch and geometry; it pads to
// KPAD >= 4 with zero rows, so k = 1 and 2 take it too); k_nnm_finish -> s->dist, s->nbr;
// k_nnm_mix over the entries in place.
int flsim_nnm_entries(const flsim_nnm* a, const flsim_nnm_scratch* s, long P, hipStream_t stream) {
    RC(check_nnm(a));
    const int k = a->k;
    for (int j = 0; j < k; ++j) {
        FLSIM_REQUIRE(a->entries[j], "null entry %d", j);
        FLSIM_REQUIRE(((uintptr_t)a->entries[j] & 15) == 0, "entry %d must be 16-byte aligned", j);
    }
    FLSIM_REQUIRE(P > 0 && P < (1L << 31), "P = %ld out of range", P);
    static const char name[] = "NNM";
    const flsim_nnm_scratch none{};
    if (!s) s = &none;
    const long n_dist = pair_partials(P, k);
    constexpr int NS = 3;
    const Span sc[NS] = {{s->partials, 8 * n_dist}, {s->dist, 8L * k * k}, {s->nbr, 8L * k}};
    RC(check_scratch_pointers(name, sc, NS, s->n_partials, n_dist));
    for (int j = 0; j < k; ++j)
        for (int q = 0; q < j; ++q)
            FLSIM_REQUIRE(!overlaps(a->entries[q], a->entries[j], P), "entries %d and %d overlap",
                          q, j);
    // no p / m / v / clip here: the entries against the scratch, then the scratch against itself
    StepBuffers B{};
    B.P = P;
    EntryTable T{};
    NnmMixArgs M{};
    int distinct = 0;                   // k: no entry is null, none overlaps another
    RC(fill_entries(B, a->entries, a->count, k, name, sc, NS, nullptr, &T, &distinct));
    RC(check_scratch(B, name, sc, NS, nullptr));
    for (int j = 0; j < k; ++j) {
        M.ent[j] = a->entries[j];
        M.cnt[j] = T.cnt[j];
        M.rcnt[j] = T.rcnt[j];
    }
    RC(launch_pair_dist(T, s->partials, P, k, K_NNM_DIST, distinct, K_NNM_FIN, 0.0, stream,
                        [&](const ProbeSlot& ps, const double* part, int nblocks, int nb) {
                            hipExtLaunchKernelGGL(k_nnm_finish, dim3(1), dim3(KRUM_FIN_THREADS), 0,
                                                  stream, ps.start, ps.stop, 0, part, nblocks, nb,
                                                  k, (int)a->f, s->dist, s->nbr);
                        }));
    M.nbr = s->nbr;
    M.P = P;
    M.k = k;
    M.fn = (float)(k - a->f);
    const int mpad = nnm_kpad(k);
    M.ntiles = (int)nnm_tiles(P, mpad);
    {
        const ProbeSlot ps = probe_begin();
        const dim3 grid((unsigned)nnm_blocks(P, mpad));
        with_kpad<4>(mpad, [&](auto kp) {
            hipExtLaunchKernelGGL((k_nnm_mix<decltype(kp)::value>), grid, dim3(256), 0, stream,
                                  ps.start, ps.stop, 0, M);
        });
        FLSIM_LAUNCH_CHECK();
        // algorithmic HBM bytes: every entry read once and written once
        if (probe_end(ps, K_NNM_MIX, 8.0 * (double)P * k)) return 2;
    }
    return 0;
}

// host (testing): the text for host pointers.  The bucket means by one fp32 division each, every
// distance as the fp64 sum of the squared fp64 differences in element order (a pair is computed
// once and mirrored), NaN -> +inf, a zero diagonal; then csrc/nnm.h's selection and element code.
// a->entries are read only; out (nullable) is [k * P], row-major.
int flsim_nnm_eval_host(const flsim_nnm* a, long P, double* dist, uint64_t* nbr, float* out) {
    RC(check_nnm(a));
    const int k = a->k;
    for (int j = 0; j < k; ++j) FLSIM_REQUIRE(a->entries[j], "null entry %d", j);
    FLSIM_REQUIRE(dist && nbr, "null pointer");
    FLSIM_REQUIRE(P > 0, "P = %ld out of range", P);
    auto mean = [&](int j, long e) { return bucket_mean(a->entries, a->count, j, e); };
    pair_dist_host(mean, k, P, dist);
    nnm_select(dist, nbr, k, (int)a->f, 0, 1);
    if (!out) return 0;
    const float fn = (float)(k - a->f);
    for (long e = 0; e < P; ++e) {
        float x[1][RULE_MAX_ARR], y[1];
        for (int j = 0; j < RULE_MAX_ARR; ++j) x[0][j] = j < k ? mean(j, e) : 0.f;
        for (int i = 0; i < k; ++i) {
            nnm_mix_elem<RULE_MAX_ARR, 1>(x, nbr[i], k, fn, y);
            out[(long)i * P + e] = y[0];
        }
    }
    return 0;
}

// ---- centered clipping (CClip) over bucket means + the update (include/flsim.h) -------------------
long flsim_cclip_partials(long P, int k) {
    if (k < 1 || k > RULE_MAX_ARR || P < 1 || P >= (1L << 31)) return 0;
    return geomed_blocks(P, geomed_kpad(k)) * (k + 1);
}

long flsim_cclip_tile_elems(int k) {
    if (k < 1 || k > RULE_MAX_ARR) return 0;
    return geomed_tile_elems(geomed_kpad(k));
}

// iters pairs (k_cclip_dist -> s->partials; k_cclip_finish -> s->d2, s->s, s->u, s->w, s->state),
// then k_cclip_apply in the optimizer's kind, which also stores g to r->center (optim == NULL:
// OK_GOUT writing g_out alone; clip: OK_GOUT writing clip->G and the per-block partials, then
// k_clip_finish and k_clip_apply).
int flsim_cclip_optim_step(const flsim_cclip* r, const flsim_cclip_scratch* s,
                           const flsim_clip* clip, float* g_out, float* p, float* m, float* v,
                           long P, long step, const flsim_optim* optim, hipStream_t stream) {
    RC(check_cclip(r));
    BucketStep B;
    RC(step_begin(optim, clip, g_out, p, m, v, P, step, &B));
    static const char name[] = "centered-clipping";
    float* const center = r->center;
    FLSIM_REQUIRE(center, "null centered-clipping center");
    FLSIM_REQUIRE(((uintptr_t)center & 15) == 0, "centered-clipping center must be 16-byte aligned");
    for (const float* o : B.outs)
        FLSIM_REQUIRE(!overlaps(center, o, P), "centered-clipping center overlaps p/m/v/g_out");
    const flsim_cclip_scratch none{};
    if (!s) s = &none;
    const int k = r->k, iters = r->iters;
    const int kpad = geomed_kpad(k);
    const long nblocks = geomed_blocks(P, kpad);
    const long n_dist = nblocks * (k + 1);
    constexpr int NS = 6;
    const Span sc[NS] = {{s->partials, 8 * n_dist},      {s->u, 8L * (iters + 1)},
                         {s->w, 8L * (iters + 1) * k},   {s->d2, 8L * iters * k},
                         {s->s, 8L * iters * k},         {s->state, 4L * (k + CCLIP_ST_WORDS)}};
    RC(check_scratch_pointers(name, sc, NS, s->n_partials, n_dist));
    RC(check_scratch(B, name, sc, NS, center));
    RC(check_clip_buffers(B, center));
    CclipDistArgs D{};
    CclipFinArgs F{};
    CclipApplyArgs A{};
    int distinct = 0;
    RC(fill_entries(B, r->entries, r->count, k, name, sc, NS, center, &D.T, &distinct));
    A.T = D.T;
    for (int j = 0; j < k; ++j) F.count[j] = r->count[j];
    const bool fresh = r->fresh != 0;
    D.center = center;
    D.u = s->u;
    D.w = s->w;
    D.state = s->state;
    D.partials = s->partials;
    D.P = P;
    D.k = k;
    D.ntiles = (int)geomed_tiles(P, kpad);
    F.partials = s->partials;
    F.u = s->u;
    F.w = s->w;
    F.d2 = s->d2;
    F.s = s->s;
    F.state = s->state;
    F.tau = r->tau;
    F.nblocks = (int)nblocks;
    F.k = k;
    F.weighted = r->weighted;
    for (int pair = 0; pair < iters; ++pair) {
        D.pair = F.pair = pair;
        {
            const ProbeSlot ps = probe_begin();
            const dim3 grid((unsigned)nblocks);
            with_kpad<4>(kpad, [&](auto kp) {
                launch_cclip_dist<decltype(kp)::value>(pair == 0, fresh, grid, stream, ps, D);
            });
            FLSIM_LAUNCH_CHECK();
            // algorithmic HBM bytes: each distinct entry and (unless fresh) the center read once
            if (probe_end(ps, K_CCLIP_DIST, 4.0 * (double)P * (distinct + (fresh ? 0 : 1))))
                return 2;
        }
        const ProbeSlot ps = probe_begin();
        hipExtLaunchKernelGGL(k_cclip_finish, dim3(1), dim3(GEOMED_FIN_THREADS), 0, stream,
                              ps.start, ps.stop, 0, F);
        FLSIM_LAUNCH_CHECK();
        if (probe_end(ps, K_CCLIP_FIN, 8.0 * (double)nblocks * (k + (pair == 0)) + 8.0 * (4 * k + 2)))
            return 2;
    }
    A.u = s->u + iters;
    A.w = s->w + (long)iters * k;
    A.center = center;
    A.k = k;
    A.fresh = fresh;
    // the rule's own arrays: the distinct entries and (unless fresh) the center read, the center
    // written
    return launch_apply(B, A, K_CCLIP_APPLY, distinct + (fresh ? 1 : 2), stream,
                        [&](auto ok, dim3 grid, const ProbeSlot& ps) {
                            hipExtLaunchKernelGGL((k_cclip_apply<decltype(ok)::value>), grid,
                                                  dim3(256), 0, stream, ps.start, ps.stop, 0, A);
                        });
}

// host (testing): the text for host pointers.  The bucket means by one fp32 division each; z as
// _wsum forms it, the center's term first; every distance as the fp64 sum of ((double)x_j - z)^2
// in element order (one fma each, as the kernel's); then csrc/cclip.h's scalar code, and
// g = (float)z at (u[iters], w[iters]).
int flsim_cclip_eval_host(const flsim_cclip* r, long P, double* u, double* w, double* d2, double* s,
                          float* g_out, float* center_out) {
    RC(check_cclip(r));
    const int k = r->k, iters = r->iters;
    const bool fresh = r->fresh != 0;
    FLSIM_REQUIRE(u && w && d2 && s, "null pointer");
    FLSIM_REQUIRE(fresh || r->center, "null centered-clipping center");
    FLSIM_REQUIRE(P > 0, "P = %ld out of range", P);
    auto mean = [&](int j, long e) { return bucket_mean(r->entries, r->count, j, e); };
    auto wsum = [&](double uw, const double* wt, long e) {
        return wsum_host(mean, wt, k, e, fresh ? nullptr : r->center, uw);
    };
    int32_t dead[RULE_MAX_ARR];
    double a[RULE_MAX_ARR], term[RULE_MAX_ARR], sums[CCLIP_SUM_WORDS];
    dead_scan_host(mean, k, P, dead);
    for (int j = 0; j < k; ++j) {
        a[j] = geomed_alpha(r->weighted, r->count[j], dead[j]);
        w[j] = 0.0;
    }
    u[0] = 1.0;
    for (int it = 0; it < iters; ++it) {
        double* d = d2 + (long)it * k;
        d2_host(mean, [&](long e) { return wsum(u[it], w + (long)it * k, e); }, dead, k, P, d);
        cclip_iterate(d, a, dead, k, r->tau, u[it], w + (long)it * k, s + (long)it * k, term, sums,
                      w + (long)(it + 1) * k, 0, 1, [] {});
        u[it + 1] = sums[CCLIP_SUM_U];
    }
    if (!g_out && !center_out) return 0;
    for (long e = 0; e < P; ++e) {
        const float g = (float)wsum(u[iters], w + (long)iters * k, e);
        if (g_out) g_out[e] = g;
        if (center_out) center_out[e] = g;
    }
    return 0;
}

}  // extern "C"
