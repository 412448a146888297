// Pixel shuffle by 2 with an activation, and its inverse, on channels-last fp32 activations (include/lvt_hip.h, ABI 670):
// nn.PixelShuffle(2) [+ ReLU | Tanh | Sigmoid] of the reference's ResShuffleDecoder (generator/resdecoder.py:105-109) and its
// backward.  Streaming kernels in the idiom of resample.hip: every element is read once and written once, 16 bytes per access on
// the coarse side, grid = the work in 256-thread groups capped at 8 per CU with a grid-stride loop behind it, max |out| through the
// library's integer max (lvt_block_amax_commit), no floating-point atomic: two runs give the same bits.
//
// Form: a thread owns ONE channel of one coarse pixel.  On the coarse side that is one float4 (the sub-pixels (0,0) (0,1) (1,0) (1,1)
// of channel c sit at channel offset 4c), on the fine side one scalar at each of the 2 x 2 pixels; consecutive lanes hold consecutive
// channels, so the coarse access is 16 bytes per lane and 1 KB per wave, each fine access 256 consecutive bytes per wave.  The other
// candidate -- a thread owns four channels, transposes 4 x 4 in its registers and moves 16 bytes per lane on both sides -- is kept
// in tools/ubench/shuffle_forms.hip, which times the two side by side: at the decoder's two shapes with 512 frames this form took
// 100 us against 109 us and 10.4 us against 12.1 us on one MI355X (DESIGN 3.10 has the table; why the other loses was not
// investigated further).  With C % 4 != 0
// (the image end: 12 -> 3 channels carried as 4) the threads of the fine side's pad channels load nothing and store exact zeros,
// whatever the activation -- the same kernel, no second path; the inverse simply has no thread for a pad channel.
#include "lvt_common.h"

#define SH_THREADS 256

__device__ __forceinline__ float4 sh_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void sh_st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float sh_amax4(float m, float4 v) {
    return fmaxf(m, fmaxf(fmaxf(lvt_absf(v.x), lvt_absf(v.y)), fmaxf(lvt_absf(v.z), lvt_absf(v.w))));
}
template <int ACT>
__device__ __forceinline__ float sh_act(float v) {
    if (ACT == LVT_EPI_RELU) return fmaxf(v, 0.f);
    if (ACT == LVT_EPI_TANH) return tanhf(v);
    if (ACT == LVT_EPI_SIGMOID) return lvt_sigmoidf(v);
    return v;
}
template <int ACT>
__device__ __forceinline__ float4 sh_act4(float4 v) {
    return make_float4(sh_act<ACT>(v.x), sh_act<ACT>(v.y), sh_act<ACT>(v.z), sh_act<ACT>(v.w));
}

// x (rows, W, 4 C) -> out (2 rows, 2 W, Cp), rows = N * H.  n: threads' worth of work = rows * W * Cp (the pad channels included).
template <int ACT>
__global__ __launch_bounds__(SH_THREADS) void lvt_pixel_shuffle2_kernel(const float *__restrict__ x, long long n, int Cp, int W, int C,
                                                                        float *__restrict__ out, float *__restrict__ out_amax) {
    __shared__ float scratch[SH_THREADS / 64];
    const long long rowf = 2LL * W * Cp;              // floats per output row
    float am = 0.f;
    for (long long i = (long long)blockIdx.x * SH_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SH_THREADS) {
        const long long pix = i / Cp;
        const int c = (int)(i - pix * Cp);
        const long long r = pix / W;
        const int j = (int)(pix - r * W);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) v = sh_act4<ACT>(sh_ld4(x + (pix * C + c) * 4));
        float *o = out + 2 * r * rowf + (long long)2 * j * Cp + c;
        o[0] = v.x; o[Cp] = v.y; o[rowf] = v.z; o[rowf + Cp] = v.w;
        am = sh_amax4(am, v);
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, scratch);
}

// g (2 rows, 2 W, Cp) -> out (rows, W, 4 C): the inverse.  n = rows * W * C: channels C.. of g have no thread and are never read.
__global__ __launch_bounds__(SH_THREADS) void lvt_pixel_unshuffle2_kernel(const float *__restrict__ g, long long n, int Cp, int W, int C,
                                                                          float *__restrict__ out, float *__restrict__ out_amax) {
    __shared__ float scratch[SH_THREADS / 64];
    const long long rowf = 2LL * W * Cp;              // floats per input row
    float am = 0.f;
    for (long long i = (long long)blockIdx.x * SH_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SH_THREADS) {
        const long long pix = i / C;
        const int c = (int)(i - pix * C);
        const long long r = pix / W;
        const int j = (int)(pix - r * W);
        const float *p = g + 2 * r * rowf + (long long)2 * j * Cp + c;
        const float4 v = make_float4(p[0], p[Cp], p[rowf], p[rowf + Cp]);
        sh_st4(out + i * 4, v);
        am = sh_amax4(am, v);
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, scratch);
}

static unsigned sh_grid(long long n) {
    const long long b = lvt_cdiv(n, SH_THREADS), cap = 8LL * LVT_NUM_CU;
    return (unsigned)(b < cap ? b : cap);
}

// C <= 2^27 keeps 4 C and pad4(C) ints.  Pixels and elements are indexed with long long and no row count is held in an int;
// four int extents can still overflow that, so the element count is bounded as well.
static int sh_check(const char *name, const float *a, int N, int H, int W, int C, const float *out) {
    LVT_REQUIRE(a && out, "%s: null operand", name);
    LVT_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "%s: N, H, W, C must be positive (got %d, %d, %d, %d)", name, N, H, W, C);
    LVT_REQUIRE(C <= (1 << 27), "%s: C = %d is out of range", name, C);
    LVT_REQUIRE((double)N * H * W * 4.0 * (C + 3) < 4e18, "%s: %d x %d x %d x %d elements overflow the index type", name, N, H, W, 4 * C);
    LVT_REQUIRE(lvt_aligned16(a) && lvt_aligned16(out), "%s: operands must be 16-byte aligned", name);
    return LVT_OK;
}

extern "C" int lvt_pixel_shuffle2(const float *x, int N, int H, int W, int C, int act, float *out, float *out_amax, void *stream) {
    int rc = sh_check("lvt_pixel_shuffle2", x, N, H, W, C, out); if (rc) return rc;
    LVT_REQUIRE(act == 0 || act == LVT_EPI_RELU || act == LVT_EPI_TANH || act == LVT_EPI_SIGMOID,
                "lvt_pixel_shuffle2: act must be 0, LVT_EPI_RELU, LVT_EPI_TANH or LVT_EPI_SIGMOID (got %d)", act);
    const int Cp = (C + 3) / 4 * 4;
    const long long n = (long long)N * H * W * Cp;
    const dim3 grid(sh_grid(n)), block(SH_THREADS);
    hipStream_t s = (hipStream_t)stream;
    switch (act) {
    case LVT_EPI_RELU: lvt_pixel_shuffle2_kernel<LVT_EPI_RELU><<<grid, block, 0, s>>>(x, n, Cp, W, C, out, out_amax); break;
    case LVT_EPI_TANH: lvt_pixel_shuffle2_kernel<LVT_EPI_TANH><<<grid, block, 0, s>>>(x, n, Cp, W, C, out, out_amax); break;
    case LVT_EPI_SIGMOID: lvt_pixel_shuffle2_kernel<LVT_EPI_SIGMOID><<<grid, block, 0, s>>>(x, n, Cp, W, C, out, out_amax); break;
    default: lvt_pixel_shuffle2_kernel<0><<<grid, block, 0, s>>>(x, n, Cp, W, C, out, out_amax); break;
    }
    LVT_CHECK_LAUNCH("lvt_pixel_shuffle2");
    return LVT_OK;
}

extern "C" int lvt_pixel_unshuffle2(const float *g, int N, int H, int W, int C, float *out, float *out_amax, void *stream) {
    int rc = sh_check("lvt_pixel_unshuffle2", g, N, H, W, C, out); if (rc) return rc;
    const int Cp = (C + 3) / 4 * 4;
    const long long n = (long long)N * H * W * C;
    lvt_pixel_unshuffle2_kernel<<<sh_grid(n), SH_THREADS, 0, (hipStream_t)stream>>>(g, n, Cp, W, C, out, out_amax);
    LVT_CHECK_LAUNCH("lvt_pixel_unshuffle2");
    return LVT_OK;
}
