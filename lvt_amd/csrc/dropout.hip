// Residual dropout of the video transformer: out = res + keep * (z * s), keep drawn from a counter-based
// Philox4x32-10 stream, so the backward pass regenerates the mask from (seed, site, rank, pass) and nothing mask-sized is
// ever stored.  The stream is stated once in plain Python (lvt_amd/hip/dropout.py); these kernels follow it bit for bit.
// Streaming: 16-byte loads and stores, one Philox call per thread per group of four consecutive elements, a grid-stride loop
// over a 64-bit group index; the data never passes through LDS (the 16 bytes below are the scratch of the max |out| record).
#include "lvt_common.h"

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

// ten rounds; each 32 x 32 -> 64 product is ONE v_mad_u64_u32 (high and low word together), two per round
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c0;
        const unsigned long long p1 = (unsigned long long)PHILOX_M1 * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the product is rounded on its own (no contraction into an FMA): a float32 numpy statement gives the same bits
__device__ __forceinline__ float drop1(float z, float r, bool keep, float s) {
#pragma clang fp contract(off)
    const float zs = z * s;
    return keep ? r + zs : r;
}

// RES: out = keep ? res + z s : res; else out = keep ? z s : +0.  z and out may be the same buffer (every thread reads its
// group before it writes it), hence no __restrict__ on them.
template <bool RES>
__global__ __launch_bounds__(256) void lvt_dropout_kernel(const float *z, const float *res, long long n, unsigned k0, unsigned k1,
                                                           unsigned site_rank, unsigned pass, unsigned T, float s, float *out,
                                                           float *out_amax) {
    __shared__ float amax_scratch[4];
    float am = 0.f;
    const long long groups = (n + 3) >> 2;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        unsigned w[4];
        philox4x32_10((unsigned)g, (unsigned)((unsigned long long)g >> 32), site_rank, pass, k0, k1, w);
        const long long i = g << 2;
        if (i + 4 <= n) {
            const float4 a = reinterpret_cast<const float4 *>(z)[g];
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            if (RES) r = reinterpret_cast<const float4 *>(res)[g];
            const float4 o = make_float4(drop1(a.x, r.x, w[0] >= T, s), drop1(a.y, r.y, w[1] >= T, s),
                                         drop1(a.z, r.z, w[2] >= T, s), drop1(a.w, r.w, w[3] >= T, s));
            reinterpret_cast<float4 *>(out)[g] = o;
            am = fmaxf(am, fmaxf(fmaxf(lvt_absf(o.x), lvt_absf(o.y)), fmaxf(lvt_absf(o.z), lvt_absf(o.w))));
        } else {
            // the last group of an n that is no multiple of four: its unused words are discarded
            for (int j = 0; j < 3 && i + j < n; ++j) {
                const float o = drop1(z[i + j], RES ? res[i + j] : 0.f, w[j] >= T, s);
                out[i + j] = o;
                am = fmaxf(am, lvt_absf(o));
            }
        }
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, amax_scratch);
}

static int dropout_launch(const char *name, const float *z, const float *res, long long n, unsigned long long seed,
                          unsigned site_rank, unsigned pass, unsigned T, float s, float *out, unsigned *out_amax, void *stream) {
    LVT_REQUIRE(n > 0, "%s: n = %lld, at least one element", name, n);
    LVT_REQUIRE(z && out, "%s: null pointer", name);
    LVT_REQUIRE(lvt_aligned16(z) && lvt_aligned16(res) && lvt_aligned16(out), "%s: pointers must be 16-byte aligned", name);
    LVT_REQUIRE((((uintptr_t)out_amax) & 3) == 0, "%s: out_amax must be 4-byte aligned", name);
    long long blocks = lvt_cdiv(lvt_cdiv(n, 4), 256);
    if (blocks > 2048) blocks = 2048;              // 8 workgroups per CU; the grid-stride loop takes the rest
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    float *am = reinterpret_cast<float *>(out_amax);
    if (res)
        hipLaunchKernelGGL(lvt_dropout_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, res, n, k0, k1,
                           site_rank, pass, T, s, out, am);
    else
        hipLaunchKernelGGL(lvt_dropout_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, res, n, k0, k1,
                           site_rank, pass, T, s, out, am);
    LVT_CHECK_LAUNCH("lvt_dropout_kernel");
    return LVT_OK;
}

extern "C" int lvt_dropout_add(const float *z, const float *res, long long n, unsigned long long seed, unsigned site_rank,
                               unsigned pass, unsigned T, float s, float *out, unsigned *out_amax, void *stream) {
    return dropout_launch("lvt_dropout_add", z, res, n, seed, site_rank, pass, T, s, out, out_amax, stream);
}

extern "C" int lvt_dropout_bwd(const float *g, long long n, unsigned long long seed, unsigned site_rank, unsigned pass, unsigned T,
                               float s, float *out, unsigned *out_amax, void *stream) {
    return dropout_launch("lvt_dropout_bwd", g, nullptr, n, seed, site_rank, pass, T, s, out, out_amax, stream);
}
