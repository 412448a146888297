// Cosine codebook lookup (MODEL.CODEBOOK.COSINE): l2-normalisation of the d-wide groups of channels-last rows and
// its backward.  The rule is stated once in plain torch (lvt_amd/modeling/vq/cosine.py); with ss the sum of squares of a group,
//   fwd: inv = 1 / max(sqrt(ss), eps),  y = x * inv                         (F.normalize(x, dim=-1, eps))
//   bwd: dx = inv * (g - y * (y . g))  where the norm was above eps,  dx = inv * g  where it was clamped (inv == 1 / eps)
// x is (rows, G * d) contiguous, so its rows * G groups are consecutive runs of d floats and the row structure plays no part.
// Streaming: 16-byte loads and stores, a group is owned by a segment of S lanes (S: the smallest power of two that covers the
// d / 4 float4s of a group, at most 64; lane j of the segment holds float4s j, j + 64, ... when d > 256: NV of them), a wave
// holds 64 / S groups at a time -- at the shipped 4 x 64 geometry one row: 4 groups x 16 lanes -- and walks the groups in a
// grid-stride loop.  The sum of squares (the dot product) is added up inside a lane in element order and across the segment by
// an xor butterfly, whose two sides form the same sum a + b = b + a: every lane of the segment ends with the same bits, and
// two runs give the same bits.  No LDS and no atomics take part in it (the 16 bytes below are the scratch of the max |.|
// record, one integer atomic max per workgroup: lvt_common.h).
// Contract: groups whose sum of squares is finite in fp32 (encoder outputs are O(1); elements above 1.8e19 overflow it).
#include "lvt_common.h"

#define L2N_THREADS 256
#define L2N_GROUP_FLOATS_MAX 1024
#define L2N_ROW_FLOATS_MAX 4096

template <int S>
__device__ __forceinline__ float l2n_segment_sum(float v) {
#pragma unroll
    for (int o = S >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float l2n_amax4(float am, const float4 &o) {
    return fmaxf(am, fmaxf(fmaxf(lvt_absf(o.x), lvt_absf(o.y)), fmaxf(lvt_absf(o.z), lvt_absf(o.w))));
}

// x and y may be the same buffer (a lane reads its float4s before it writes them): no __restrict__ on them
template <int S, int NV>
__global__ __launch_bounds__(L2N_THREADS) void lvt_l2norm_fwd_kernel(const float *x, long long ngroups, int nq, float eps, float *y,
                                                                      float *inv, float *out_amax) {
    __shared__ float amax_scratch[L2N_THREADS / 64];
    constexpr int GPW = 64 / S;                                    // groups a wave holds at a time
    const int lane = threadIdx.x & 63, seg = lane / S, sl = lane % S;
    const long long wave = (long long)blockIdx.x * (L2N_THREADS / 64) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (L2N_THREADS / 64) * GPW;
    float am = 0.f;
    for (long long base = wave * GPW; base < ngroups; base += stride) {          // (wave-uniform trip count: the exchanges below
        const long long gi = base + seg;                                         //  run with every lane active)
        const bool live = gi < ngroups;
        const float4 *src = reinterpret_cast<const float4 *>(x) + gi * nq;
        float4 v[NV];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = sl + j * S;
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && q < nq) v[j] = src[q];
            ss += v[j].x * v[j].x;
            ss += v[j].y * v[j].y;
            ss += v[j].z * v[j].z;
            ss += v[j].w * v[j].w;
        }
        ss = l2n_segment_sum<S>(ss);
        const float r = 1.f / fmaxf(sqrtf(ss), eps);
        float4 *dst = reinterpret_cast<float4 *>(y) + gi * nq;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = sl + j * S;
            if (live && q < nq) {
                const float4 o = make_float4(v[j].x * r, v[j].y * r, v[j].z * r, v[j].w * r);
                dst[q] = o;
                am = l2n_amax4(am, o);
            }
        }
        if (inv && live && sl == 0) inv[gi] = r;
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, amax_scratch);
}

template <int S, int NV>
__global__ __launch_bounds__(L2N_THREADS) void lvt_l2norm_bwd_kernel(const float *g, const float *y, const float *inv,
                                                                      long long ngroups, int nq, float eps, float *dx,
                                                                      float *out_amax) {
    __shared__ float amax_scratch[L2N_THREADS / 64];
    constexpr int GPW = 64 / S;
    const int lane = threadIdx.x & 63, seg = lane / S, sl = lane % S;
    const long long wave = (long long)blockIdx.x * (L2N_THREADS / 64) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (L2N_THREADS / 64) * GPW;
    const float r_clamped = 1.f / eps;                   // what the forward wrote for a clamped group: the same quotient
    float am = 0.f;
    for (long long base = wave * GPW; base < ngroups; base += stride) {
        const long long gi = base + seg;
        const bool live = gi < ngroups;
        const float4 *gs = reinterpret_cast<const float4 *>(g) + gi * nq;
        const float4 *ys = reinterpret_cast<const float4 *>(y) + gi * nq;
        const float r = live ? inv[gi] : 0.f;
        float4 a[NV], u[NV];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = sl + j * S;
            a[j] = u[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && q < nq) {
                a[j] = gs[q];
                u[j] = ys[q];
            }
            dot += u[j].x * a[j].x;
            dot += u[j].y * a[j].y;
            dot += u[j].z * a[j].z;
            dot += u[j].w * a[j].w;
        }
        dot = l2n_segment_sum<S>(dot);
        if (r == r_clamped) dot = 0.f;                   // the norm was clamped to eps: y = x / eps, dx = g / eps
        float4 *dst = reinterpret_cast<float4 *>(dx) + gi * nq;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = sl + j * S;
            if (live && q < nq) {
                const float4 o = make_float4(r * (a[j].x - u[j].x * dot), r * (a[j].y - u[j].y * dot),
                                             r * (a[j].z - u[j].z * dot), r * (a[j].w - u[j].w * dot));
                dst[q] = o;
                am = l2n_amax4(am, o);
            }
        }
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, amax_scratch);
}

static int l2n_check(const char *name, long long rows, int G, int d, float eps) {
    LVT_REQUIRE(rows > 0 && G >= 1, "%s: rows = %lld, G = %d: at least one row and one group", name, rows, G);
    LVT_REQUIRE(d >= 16 && d <= L2N_GROUP_FLOATS_MAX && d % 16 == 0, "%s: group width d = %d, a multiple of 16 from 16 to %d", name,
                d, L2N_GROUP_FLOATS_MAX);
    LVT_REQUIRE((long long)G * d <= L2N_ROW_FLOATS_MAX, "%s: G * d = %lld floats per row, at most %d", name, (long long)G * d,
                L2N_ROW_FLOATS_MAX);
    LVT_REQUIRE(eps > 0.f && eps < __builtin_inff(), "%s: eps must be positive and finite", name);
    return LVT_OK;
}

// a function of `rows` only: 16 rows per workgroup pass, at most 8 workgroups per CU; the grid-stride loop takes the rest
static unsigned l2n_blocks(long long rows) {
    const long long b = lvt_cdiv(rows, 16);
    return (unsigned)(b > 8 * LVT_NUM_CU ? 8 * LVT_NUM_CU : b);
}

#define L2N_DISPATCH(KERNEL, ...)                                                                                            \
    do {                                                                                                                     \
        const dim3 grid(l2n_blocks(rows)), block(L2N_THREADS);                                                               \
        hipStream_t s_ = (hipStream_t)stream;                                                                                \
        if (nq <= 4) hipLaunchKernelGGL((KERNEL<4, 1>), grid, block, 0, s_, __VA_ARGS__);                                    \
        else if (nq <= 8) hipLaunchKernelGGL((KERNEL<8, 1>), grid, block, 0, s_, __VA_ARGS__);                               \
        else if (nq <= 16) hipLaunchKernelGGL((KERNEL<16, 1>), grid, block, 0, s_, __VA_ARGS__);                             \
        else if (nq <= 32) hipLaunchKernelGGL((KERNEL<32, 1>), grid, block, 0, s_, __VA_ARGS__);                             \
        else if (nq <= 64) hipLaunchKernelGGL((KERNEL<64, 1>), grid, block, 0, s_, __VA_ARGS__);                             \
        else hipLaunchKernelGGL((KERNEL<64, 4>), grid, block, 0, s_, __VA_ARGS__);                                           \
    } while (0)

extern "C" int lvt_l2norm_groups_fwd(const float *x, long long rows, int G, int d, float eps, float *y, float *inv,
                                     unsigned *out_amax, void *stream) {
    if (int rc = l2n_check("lvt_l2norm_groups_fwd", rows, G, d, eps)) return rc;
    LVT_REQUIRE(x && y, "lvt_l2norm_groups_fwd: null pointer");
    LVT_REQUIRE(lvt_aligned16(x) && lvt_aligned16(y), "lvt_l2norm_groups_fwd: x and y must be 16-byte aligned");
    LVT_REQUIRE((((uintptr_t)inv) & 3) == 0 && (((uintptr_t)out_amax) & 3) == 0,
                "lvt_l2norm_groups_fwd: inv and out_amax must be 4-byte aligned");
    const long long ngroups = rows * G;
    const int nq = d / 4;
    L2N_DISPATCH(lvt_l2norm_fwd_kernel, x, ngroups, nq, eps, y, inv, reinterpret_cast<float *>(out_amax));
    LVT_CHECK_LAUNCH("lvt_l2norm_fwd_kernel");
    return LVT_OK;
}

extern "C" int lvt_l2norm_groups_bwd(const float *g, const float *y, const float *inv, long long rows, int G, int d, float eps,
                                     float *dx, unsigned *out_amax, void *stream) {
    if (int rc = l2n_check("lvt_l2norm_groups_bwd", rows, G, d, eps)) return rc;
    LVT_REQUIRE(g && y && inv && dx, "lvt_l2norm_groups_bwd: null pointer");
    LVT_REQUIRE(lvt_aligned16(g) && lvt_aligned16(y) && lvt_aligned16(dx), "lvt_l2norm_groups_bwd: g, y and dx must be 16-byte aligned");
    LVT_REQUIRE((((uintptr_t)inv) & 3) == 0 && (((uintptr_t)out_amax) & 3) == 0,
                "lvt_l2norm_groups_bwd: inv and out_amax must be 4-byte aligned");
    const long long ngroups = rows * G;
    const int nq = d / 4;
    L2N_DISPATCH(lvt_l2norm_bwd_kernel, g, y, inv, ngroups, nq, eps, dx, reinterpret_cast<float *>(out_amax));
    LVT_CHECK_LAUNCH("lvt_l2norm_bwd_kernel");
    return LVT_OK;
}
