// 2x2 average pool and nearest 2x upsample on channels-last fp32 activations (include/lvt_hip.h, ABI 660): nn.AvgPool2d(2) and
// nn.Upsample(scale_factor=2) of the reference's ConvEncoder / ConvDecoder, and each other's backward (pool with scale 1 is the
// upsample's, upsample with scale 0.25 the pool's).  Streaming kernels: every element is read once and written once, 16 bytes per
// access along the channels, so a wave instruction covers 1 KB of consecutive addresses whenever 2 W Cp >= 256 floats.
//
// A thread owns one float4 of the SMALL tensor (the pool's output, the upsample's input) and with it the four float4 of the large
// one: four independent 16-byte loads (eight with a mask) are in flight per thread before the first store, 256 threads x 8 resident
// workgroups per CU keep >= 128 KB per CU outstanding -- above the ~64 KB a CU needs to cover HBM latency at its share of the
// bandwidth.  The grid is the work in 256-thread groups, capped at 8 per CU with a grid-stride loop behind it; a tensor below
// that cap (small N) simply runs one float4 group per thread.  The optional mask has the OUTPUT's shape and applies the
// (Leaky)ReLU backward of the layer in front, as the engine's epilogues do (lvt_maskf).  max |out| leaves through the library's
// integer max (lvt_block_amax_commit); there is no floating-point atomic and the summation order is fixed.
#include "lvt_common.h"

#define RS_THREADS 256

__device__ __forceinline__ float4 rs_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void rs_st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float rs_amax4(float m, float4 v) {
    return fmaxf(m, fmaxf(fmaxf(lvt_absf(v.x), lvt_absf(v.y)), fmaxf(lvt_absf(v.z), lvt_absf(v.w))));
}
__device__ __forceinline__ float4 rs_mask4(float4 v, float4 m, bool leaky) {
    return make_float4(lvt_maskf(v.x, m.x, leaky), lvt_maskf(v.y, m.y, leaky), lvt_maskf(v.z, m.z, leaky), lvt_maskf(v.w, m.w, leaky));
}

// x (rows2 * 2, W, Cp) -> out (rows2, W / 2, Cp), rows2 = N * H / 2 (H even: the row pairs never straddle two images).
// n4: float4 of the output; q = Cp / 4; Wo = W / 2.
template <bool MASK>
__global__ __launch_bounds__(RS_THREADS) void lvt_pool2x2_kernel(const float *__restrict__ x, long long n4, int q, int Wo, float scale,
                                                                 const float *__restrict__ mask, int leaky,
                                                                 float *__restrict__ out, float *__restrict__ out_amax) {
#pragma clang fp contract(off)
    __shared__ float scratch[RS_THREADS / 64];
    const long long rowf = 2LL * Wo * q * 4;          // floats per input row
    float am = 0.f;
    for (long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * RS_THREADS) {
        const long long pix = i / q;
        const int c4 = (int)(i - pix * q);
        const long long ro = pix / Wo;
        const int j = (int)(pix - ro * Wo);
        const float *p = x + 2 * ro * rowf + ((long long)2 * j * q + c4) * 4;
        const float4 a = rs_ld4(p), b = rs_ld4(p + 4 * q), c = rs_ld4(p + rowf), d = rs_ld4(p + rowf + 4 * q);
        float4 m4;
        if (MASK) m4 = rs_ld4(mask + i * 4);
        float4 v = make_float4(((a.x + b.x) + (c.x + d.x)) * scale, ((a.y + b.y) + (c.y + d.y)) * scale,
                               ((a.z + b.z) + (c.z + d.z)) * scale, ((a.w + b.w) + (c.w + d.w)) * scale);
        if (MASK) v = rs_mask4(v, m4, leaky);
        rs_st4(out + i * 4, v);
        am = rs_amax4(am, v);
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, scratch);
}

// x (rows, W, Cp) -> out (rows * 2, 2 W, Cp), rows = N * H.  n4: float4 of the input.
template <bool MASK>
__global__ __launch_bounds__(RS_THREADS) void lvt_upsample2x2_kernel(const float *__restrict__ x, long long n4, int q, int W, float scale,
                                                                     const float *__restrict__ mask, int leaky,
                                                                     float *__restrict__ out, float *__restrict__ out_amax) {
    __shared__ float scratch[RS_THREADS / 64];
    const long long rowf = 2LL * W * q * 4;           // floats per output row
    float am = 0.f;
    for (long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * RS_THREADS) {
        const long long pix = i / q;
        const int c4 = (int)(i - pix * q);
        const long long r = pix / W;
        const int j = (int)(pix - r * W);
        const long long o = 2 * r * rowf + ((long long)2 * j * q + c4) * 4;
        float4 v = rs_ld4(x + i * 4);
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        if (MASK) {
            const float4 ma = rs_ld4(mask + o), mb = rs_ld4(mask + o + 4 * q), mc = rs_ld4(mask + o + rowf), md = rs_ld4(mask + o + rowf + 4 * q);
            const float4 va = rs_mask4(v, ma, leaky), vb = rs_mask4(v, mb, leaky), vc = rs_mask4(v, mc, leaky), vd = rs_mask4(v, md, leaky);
            rs_st4(out + o, va); rs_st4(out + o + 4 * q, vb); rs_st4(out + o + rowf, vc); rs_st4(out + o + rowf + 4 * q, vd);
            am = rs_amax4(rs_amax4(rs_amax4(rs_amax4(am, va), vb), vc), vd);
        } else {
            rs_st4(out + o, v); rs_st4(out + o + 4 * q, v); rs_st4(out + o + rowf, v); rs_st4(out + o + rowf + 4 * q, v);
            am = rs_amax4(am, v);
        }
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, scratch);
}

static unsigned rs_grid(long long n4) {
    const long long b = lvt_cdiv(n4, RS_THREADS), cap = 8LL * LVT_NUM_CU;
    return (unsigned)(b < cap ? b : cap);
}

static int rs_check(const char *name, const float *x, int N, int H, int W, int Cp, const float *mask, int mask_flags, const float *out) {
    LVT_REQUIRE(x && out && N > 0 && H > 0 && W > 0 && Cp > 0 && Cp % 4 == 0, "%s: bad arguments", name);
    LVT_REQUIRE(lvt_aligned16(x) && lvt_aligned16(out) && lvt_aligned16(mask), "%s: operands must be 16-byte aligned", name);
    LVT_REQUIRE(mask ? (mask_flags == LVT_EPI_MASK || mask_flags == (LVT_EPI_MASK | LVT_EPI_LEAKY_MASK)) : mask_flags == 0,
                "%s: mask_flags must be LVT_EPI_MASK (| LVT_EPI_LEAKY_MASK) with a mask and 0 without", name);
    return LVT_OK;
}

extern "C" int lvt_pool2x2(const float *x, int N, int H, int W, int Cp, float scale, const float *mask, int mask_flags, float *out,
                           float *out_amax, void *stream) {
    int rc = rs_check("lvt_pool2x2", x, N, H, W, Cp, mask, mask_flags, out); if (rc) return rc;
    LVT_REQUIRE(H % 2 == 0 && W % 2 == 0, "lvt_pool2x2: H and W must be even (got %d x %d)", H, W);
    const int q = Cp / 4, Wo = W / 2, leaky = (mask_flags & LVT_EPI_LEAKY_MASK) != 0;
    const long long n4 = (long long)N * (H / 2) * Wo * q;
    if (mask)
        lvt_pool2x2_kernel<true><<<rs_grid(n4), RS_THREADS, 0, (hipStream_t)stream>>>(x, n4, q, Wo, scale, mask, leaky, out, out_amax);
    else
        lvt_pool2x2_kernel<false><<<rs_grid(n4), RS_THREADS, 0, (hipStream_t)stream>>>(x, n4, q, Wo, scale, mask, leaky, out, out_amax);
    LVT_CHECK_LAUNCH("lvt_pool2x2");
    return LVT_OK;
}

extern "C" int lvt_upsample2x2(const float *x, int N, int H, int W, int Cp, float scale, const float *mask, int mask_flags, float *out,
                               float *out_amax, void *stream) {
    int rc = rs_check("lvt_upsample2x2", x, N, H, W, Cp, mask, mask_flags, out); if (rc) return rc;
    const int q = Cp / 4, leaky = (mask_flags & LVT_EPI_LEAKY_MASK) != 0;
    const long long n4 = (long long)N * H * W * q;
    if (mask)
        lvt_upsample2x2_kernel<true><<<rs_grid(n4), RS_THREADS, 0, (hipStream_t)stream>>>(x, n4, q, W, scale, mask, leaky, out, out_amax);
    else
        lvt_upsample2x2_kernel<false><<<rs_grid(n4), RS_THREADS, 0, (hipStream_t)stream>>>(x, n4, q, W, scale, mask, leaky, out, out_amax);
    LVT_CHECK_LAUNCH("lvt_upsample2x2");
    return LVT_OK;
}
