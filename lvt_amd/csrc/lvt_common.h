// Shared helpers for the liblvt_hip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "lvt_hip.h"

void lvt_set_error(const char *fmt, ...);

#define LVT_REQUIRE(cond, ...)                                  \
    do {                                                        \
        if (!(cond)) {                                          \
            lvt_set_error(__VA_ARGS__);                         \
            return LVT_EINVAL;                                  \
        }                                                       \
    } while (0)

#define LVT_CHECK_LAUNCH(name)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            lvt_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));      \
            return LVT_ELAUNCH;                                                       \
        }                                                                             \
    } while (0)

static inline bool lvt_aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
// the activation / mask flags of an epilogue go together: LEAKY excludes the other activations, LEAKY_MASK qualifies MASK
static inline bool lvt_epi_flags_ok(int flags) {
    if ((flags & LVT_EPI_LEAKY) && (flags & (LVT_EPI_RELU | LVT_EPI_TANH | LVT_EPI_SIGMOID))) return false;
    return !(flags & LVT_EPI_LEAKY_MASK) || (flags & LVT_EPI_MASK);
}
#define LVT_REQUIRE_EPI(flags, name)                                                                                         \
    LVT_REQUIRE(lvt_epi_flags_ok(flags), "%s: LVT_EPI_LEAKY excludes RELU / TANH / SIGMOID, and LVT_EPI_LEAKY_MASK needs LVT_EPI_MASK", name)
static inline __host__ __device__ long long lvt_cdiv(long long a, long long b) { return (a + b - 1) / b; }

// 256 CUs x 8 XCDs on MI355X; used only to size grids / split-K, never for correctness.
#define LVT_NUM_CU 256


// ---- max |.| reporting of the kernels that produce engine operands (LVT_MATH_F16X2 scales, include/lvt_hip.h) -----------
// Non-negative floats order like their bit patterns, so the cross-workgroup step is an INTEGER atomic max: exact and
// order-independent (the library has no floating-point atomics).  One atomic per WORKGROUP, and only when the value would
// change what is already there (a racy read is fine: the atomic decides) -- same-address atomics serialise at ~6 ns each
// on this part, 8192 of them cost a stand-alone pass 50 us.  `scratch`: >= blockDim.x / 64 floats of LDS that every
// thread may overwrite; all threads of the workgroup must call.
#ifdef __HIPCC__
// |a| of a FINITE a, else 0: the max |.| of an operand is taken over its finite entries -- an inf / nan element poisons the
// products it takes part in through its own fp16 hi term (inf * s = inf), and must not collapse the scale of all the others
__device__ __forceinline__ float lvt_absf(float a) {
    const float b = fabsf(a);
    return b < __builtin_inff() ? b : 0.f;
}
// LVT_EPI_SIGMOID: 1 / (1 + 2^(-v log2 e)) on v_exp_f32 and v_rcp_f32 (1 ulp each), four instructions and no temporaries per
// element -- libm's expf and the IEEE quotient cost the 128 x 128 transposed-convolution tile kernel 24 registers and with them
// its second wave per SIMD.  The rounding of the exponent's argument is a relative error |v| 2^-23.5 of e^-v, which
// the quotient damps by e^-v / (1 + e^-v)^2: the absolute error stays below 2^-22 for every v.  2^x overflows to +inf below
// v = -88.7 and the reciprocal is then exactly 0; above v = 16.7 the sum rounds to 1.  No NaN for a finite v.
// `real`: the column is a channel of the layer, not one of the zero pads (LVT_EPI_PAD), which stay 0 instead of sigmoid(0).
__device__ __forceinline__ float lvt_sigmoidf(float v) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v * -1.44269504088896341f));
}
__device__ __forceinline__ float lvt_sigmoid_col(float v, bool real) { return real ? lvt_sigmoidf(v) : 0.f; }
// LVT_EPI_LEAKY: v > 0 ? v : 0.2 v as one multiply and one max (0.2 v > v exactly when v < 0; leaky(0) = 0, NaN stays NaN).
#define LVT_LEAKY_SLOPE 0.2f
__device__ __forceinline__ float lvt_leakyf(float v) { return fmaxf(v, LVT_LEAKY_SLOPE * v); }
// LVT_EPI_MASK (+ LVT_EPI_LEAKY_MASK): v where the saved output m is positive, else 0 (ReLU) or 0.2 v (leaky; an exact 0 of m takes
// the 0.2 branch, torch's leaky_relu_backward rule)
__device__ __forceinline__ float lvt_maskf(float v, float m, bool leaky) { return m > 0.f ? v : (leaky ? LVT_LEAKY_SLOPE * v : 0.f); }
__device__ __forceinline__ void lvt_block_amax_commit(float m, float *dst, float *scratch) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    const int nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) m = fmaxf(m, scratch[w]);
        const unsigned bits = __float_as_uint(m);
        if (bits > __hip_atomic_load(reinterpret_cast<unsigned *>(dst), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(reinterpret_cast<unsigned *>(dst), bits);
    }
}
// ---- operand scale of the f16x2 arithmetic (gemm_engine.hip describes the split) -- the ONE definition, restated in Python
// by tests/util_f16_scale.py.  `bits`: the bit pattern of a non-negative float >= max |a| (0 and subnormals included; 255 in
// the exponent: inf / nan propagate).  Returns s = 2^(se - 127) with max * s in [2^14, 2^15) wherever the clamp does not bind
// and adds -(se - 127) to `unscale`, the exponent that undoes it on the result.  Lower clamp 2: s stays a normal number for
// a max up to 2^127.  Upper clamp 243 = 254 - 11: the splits form v * (s * 2048) for the low term, and s * 2048 must stay
// finite (<= 2^127) -- with s = 2^125 (the clamp this replaced, 252) it was +inf for every operand with max |a| < 2^-102, and
// 0 * inf = NaN for an all-zero one.  An operand below 2^-102 therefore sits lower in the fp16 range (max * s = 2^14 for a
// max of 2^-102, 2^-10 for 2^-126) and has that many fewer spare binades below its max; a zero operand gives exact zeros.
__device__ __forceinline__ float lvt_f16_scale_bits(unsigned bits, int &unscale) {
    const int eb = (int)((bits >> 23) & 0xffu);                                      // biased exponent
    int se = 268 - eb;                                                               // 127 + 14 - (eb - 127)
    se = se < 2 ? 2 : (se > 243 ? 243 : se);
    unscale -= se - 127;
    return __uint_as_float((unsigned)se << 23);
}
// from the device scalar(s) that hold the max (any upper bound works, a loose one costs range); NULL: the operand is unscaled
__device__ __forceinline__ float lvt_f16_scale(const float *amax, int &unscale, const float *amax2 = nullptr) {
    if (!amax) return 1.f;
    unsigned bits = __float_as_uint(*amax);
    if (amax2) bits = max(bits, __float_as_uint(*amax2));                            // non-negative floats order like their bits
    return lvt_f16_scale_bits(bits, unscale);
}
#endif
