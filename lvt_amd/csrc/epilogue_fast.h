// The plain GEMM epilogue, straightened (round 6).
//
// lvt_epilogue_vec (gemm_engine.hip) turns a wave's 64 x 64 accumulator sub-tile through LDS so that a lane owns 4 consecutive
// columns, and then runs, for each of its 16 float4, the whole menu of the engine: run-time flag tests (a branch around every
// bias / residual / mask load), a 64-bit row * ldc product, the ConvTranspose row decode, the bf16 plane forms -- ~1500 vector
// and ~650 scalar instructions with 156 branches per workgroup tile, between four workgroup barriers.  Phase stamps inside
// lvt_gemm_p2_kernel (profiles/r06_gemm_fixed_cost.txt): 4.85 us of the 8.2 us a 256 x 128 tile costs beside its main loop, and
// removing its global stores changes 0.7 us -- the epilogue is bound by its own instruction stream, not by memory.  The K = 512
// products of a transformer layer are one such tile per CU and launch: a third of their time.
//
// Here, for the plain forms (row-major C or the pixel permutation of the frame-resident convolutions, flags in {BIAS, RESIDUAL,
// RELU, MASK, LEAKY, LEAKY_MASK}, or the split-K partial store):
//   * the flag set is a template parameter (the kernels switch over the six combinations the models use; anything else takes
//     the run-time form of the same body);
//   * a lane's column is fixed (bias loaded once), its rows step by 4;
//   * the residual / mask values of a 32-row round are requested before its first store;
//   * the LDS turn-table of a wave is private to the wave and LDS executes a wave's instructions in order, so there is NO
//     workgroup barrier inside: waves drain independently;
//   * the current max |C| scalar is read at the START of the epilogue (its latency hides behind the stores) instead of after
//     the reduction (lvt_block_amax_commit pays a global round trip on the critical path of every workgroup).
// Arithmetic and its order are those of lvt_epilogue_vec: results are bit-identical.
//
// Round 8: a wave whose sub-tile lies inside C, in a launch with alpha == 1 and one leading dimension for C / residual / mask
// (every launch of the two models), takes lvt_epi_lean_wave below -- the same steps without the alpha multiply, the row / column
// predicates and the 64-bit vector address arithmetic, 307-610 instructions per wave and tile instead of 589-1437.
#pragma once
#include "lvt_common.h"

typedef float lvt_f32x16 __attribute__((ext_vector_type(16)));

// acc <- (acc + 2^-11 acx) 2^unscale for a wave's accumulator pair (the end of every f16x2 main loop).  ldexpf(fmaf(..)) is two
// full-rate-or-worse instructions per element (v_fma_f32 + v_ldexp_f32, 2.8 issue units); with s = 2^unscale a float, acc s and
// acx (2^-11 s) are exact products and fma(acx, 2^-11 s, acc s) rounds the same exact sum once -- the packed forms (v_pk_mul_f32,
// v_pk_fma_f32) do two elements each.  Same bits unless the result is subnormal (the two-step form rounds such a value twice).
template <int TM, int TN>
__device__ __forceinline__ void lvt_f16x2_finish(lvt_f32x16 (&acc)[TM][TN], lvt_f32x16 (&acx)[TM][TN], int unscale) {
    if (unscale >= -100 && unscale <= 120) {
        const float s = __uint_as_float((unsigned)(unscale + 127) << 23), sx = __uint_as_float((unsigned)(unscale + 116) << 23);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = acx[i][j] * sx + acc[i][j] * s;
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = ldexpf(fmaf(acx[i][j][r], 1.f / 2048.f, acc[i][j][r]), unscale);
    }
}

struct LvtEpi {
    int M, N;
    float *C; long long ldc;            // C + coff already applied by the caller? no: coff is added here (res / mask share it)
    long long coff;
    float alpha; int flags;
    const float *bias; const float *res; long long ldr; const float *mask; long long ldm;
};

// tile row -> row of C: identity for the GEMMs; the frame-resident convolutions permute the pixels of a frame (gemm_engine.hip).
// Every map is affine inside an aligned group of 4 tile rows: rm(a + r) = rm(a) + LANE_STEP r for a % 4 == 0, 0 <= r < 4 -- what
// lets lvt_epi_lean_wave address a row as a wave-uniform row (scalar) plus a lane term that never changes.
struct LvtRowIdentity {
    static constexpr int LANE_STEP = 1;
    __device__ __forceinline__ long long operator()(int row) const { return row; }
};

// F >= 0: compile-time flag set; F < 0: the flags of `e` at run time.  Returns the wave's max |stored value|.
// wave_tile: 32 x 64 floats of LDS private to the wave.  (m_w, n_w): first row / column of the wave's 64 x 64 sub-tile.
template <int F, int TM, int TN, class RM = LvtRowIdentity>
__device__ __forceinline__ float lvt_epi_fast_wave(const LvtEpi &e, lvt_f32x16 (&acc)[TM][TN], float *wave_tile, int m_w, int n_w,
                                                   int lane, const RM rm = RM()) {
    // no fused multiply-add across the epilogue steps: alpha acc, + bias, + res are rounded one by one, as in lvt_epilogue_vec and
    // the scalar lvt_epilogue (a contraction the compiler makes in one form only breaks their bit identity for alpha != 1)
#pragma clang fp contract(off)
    static_assert(TM == 2 && TN == 2, "64 x 64 sub-tiles");
    constexpr int SW = TN * 32;
    const int flags = F >= 0 ? F : e.flags;
    const bool f_bias = flags & LVT_EPI_BIAS, f_res = flags & LVT_EPI_RESIDUAL, f_relu = flags & LVT_EPI_RELU, f_mask = flags & LVT_EPI_MASK;
    const bool f_leaky = flags & LVT_EPI_LEAKY, f_lkm = flags & LVT_EPI_LEAKY_MASK;      // (clear in every compile-time set but the two below)
    const int l31 = lane & 31, half = lane >> 5;
    const int c4 = lane & 15, r0 = lane >> 4;
    const int col = n_w + 4 * c4;
    const bool colok = col < e.N;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f_bias && colok) bias4 = *reinterpret_cast<const float4 *>(e.bias + col);
    float am = 0.f;
    // residual / mask rows of BOTH 32-row rounds are requested up front: requested per round (round 6, first form) a cold operand --
    // the saved hidden activation that masks the FFN data gradient comes from HBM -- exposed its latency once per round (the
    // 16384 x 512 x 512 product with a mask 51 us against 37 without).
    long long orow_all[TM][8];
    float4 rv_all[TM][8], mv_all[TM][8];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row0 = m_w + i * 32 + r0;
#pragma unroll
        for (int u = 0; u < 8; ++u) orow_all[i][u] = rm(row0 + 4 * u);
    }
    auto request = [&](int i) {
        const int row0 = m_w + i * 32 + r0;
        if (f_res) {
            const float *rp = e.res + e.coff + col;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                rv_all[i][u] = (colok && row0 + 4 * u < e.M) ? *reinterpret_cast<const float4 *>(rp + orow_all[i][u] * e.ldr) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (f_mask) {
            const float *mp = e.mask + e.coff + col;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                mv_all[i][u] = (colok && row0 + 4 * u < e.M) ? *reinterpret_cast<const float4 *>(mp + orow_all[i][u] * e.ldm) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
#pragma unroll
    for (int i = 0; i < TM; ++i) request(i);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) wave_tile[((r & 3) + 8 * (r >> 2) + 4 * half) * SW + 32 * j + l31] = acc[i][j][r];
        const int row0 = m_w + i * 32 + r0;                                  // rows row0 + 4 u, u = 0 .. 7
        const long long (&orow)[8] = orow_all[i];
        const float4 (&rv)[8] = rv_all[i];
        const float4 (&mv)[8] = mv_all[i];
        float *cp = e.C + e.coff + col;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float4 v = *reinterpret_cast<const float4 *>(&wave_tile[(r0 + 4 * u) * SW + 4 * c4]);
            v.x *= e.alpha; v.y *= e.alpha; v.z *= e.alpha; v.w *= e.alpha;
            if (f_bias) { v.x += bias4.x; v.y += bias4.y; v.z += bias4.z; v.w += bias4.w; }
            if (f_res) { v.x += rv[u].x; v.y += rv[u].y; v.z += rv[u].z; v.w += rv[u].w; }
            if (f_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            if (f_leaky) { v.x = lvt_leakyf(v.x); v.y = lvt_leakyf(v.y); v.z = lvt_leakyf(v.z); v.w = lvt_leakyf(v.w); }
            if (f_mask) { v.x = lvt_maskf(v.x, mv[u].x, f_lkm); v.y = lvt_maskf(v.y, mv[u].y, f_lkm); v.z = lvt_maskf(v.z, mv[u].z, f_lkm); v.w = lvt_maskf(v.w, mv[u].w, f_lkm); }
            if (colok && row0 + 4 * u < e.M) {
                am = fmaxf(am, fmaxf(fmaxf(lvt_absf(v.x), lvt_absf(v.y)), fmaxf(lvt_absf(v.z), lvt_absf(v.w))));
                *reinterpret_cast<float4 *>(cp + orow[u] * e.ldc) = v;
            }
        }
    }
    return am;
}

// The same epilogue for the launches of the models, with what their results do not need taken out (round 8,
// profiles/r08_epilogue_lean.txt).  Preconditions, all wave-uniform (lvt_epi_lean_ok + the sub-tile test of lvt_epi_fast_pick;
// anything else takes lvt_epi_fast_wave above, in the same kernel):
//   * alpha == 1: x * 1.0f is x bit for bit, the 64 multiplies per lane go;
//   * the wave's 64 x 64 sub-tile lies inside C: no row / column predicate around the loads, the max and the stores;
//   * 0 <= ldc < 2^20, and the residual / mask share it (ldr == ldc, ldm == ldc): a row's address is a scalar 64-bit pointer
//     (C + coff + n_w + rm(first row) ldc, then + d ldc with d = rm(row) - rm(first row) in [0, 1024) for the three row maps: one
//     32-bit scalar product per row) plus ONE 32-bit byte offset per lane that never changes (LANE_STEP r0 ldc + 4 c4 floats)
//     and that C, residual and mask share: no vector address arithmetic at all, global_load / global_store take the scalar base;
//   * a compile-time flag set.
// max |C| of the finite values, as lvt_absf defines it: t(v) = (bits(v) << 1) + 2^24 (mod 2^32) drops the sign, wraps inf / NaN
// (exponent 255) below 2^24 and keeps the order of the finite |v| at or above it, so an UNSIGNED max over t that starts at 2^24
// (= t(0)) is the max over the finite |v| -- one v_lshl_add_u32 per element and one v_max3_u32 per two, against a class test, a
// select and a max each.  Exact: non-negative floats order like their bit patterns (lvt_common.h).
// Arithmetic per element and its order are those of lvt_epi_fast_wave: bit-identical.
// (pins a uniform global pointer in scalar registers: keeps the row pointer apart from the lane offset in the address of a load /
// store, which then takes it as its scalar base)
typedef __attribute__((address_space(1))) char lvt_gchar;
typedef float lvt_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) lvt_f32x4 lvt_gf32x4;
__device__ __forceinline__ lvt_gchar *lvt_sgpr_ptr(lvt_gchar *p) { asm("" : "+s"(p)); return p; }
template <int F, int TM, int TN, class RM>
__device__ __forceinline__ float lvt_epi_lean_wave(const LvtEpi &e, lvt_f32x16 (&acc)[TM][TN], float *wave_tile, int m_w, int n_w, int lane,
                                                   const RM rm) {
#pragma clang fp contract(off)
    static_assert(F >= 0 && TM == 2 && TN == 2, "compile-time flags, 64 x 64 sub-tiles");
    constexpr int SW = TN * 32;
    constexpr bool f_bias = F & LVT_EPI_BIAS, f_res = F & LVT_EPI_RESIDUAL, f_relu = F & LVT_EPI_RELU, f_mask = F & LVT_EPI_MASK;
    constexpr bool f_leaky = F & LVT_EPI_LEAKY, f_lkm = F & LVT_EPI_LEAKY_MASK;
    const int l31 = lane & 31, half = lane >> 5;
    const int c4 = lane & 15, r0 = lane >> 4;
    const unsigned loff = (unsigned)(RM::LANE_STEP * r0) * (unsigned)e.ldc * 4u + 16u * c4;      // bytes
    const unsigned ld4 = (unsigned)e.ldc * 4u;                                                    // < 2^22
    const long long first = (e.coff + n_w + rm(m_w) * e.ldc) * 4;                                 // uniform, bytes
    lvt_f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (f_bias) bias4 = *(const lvt_gf32x4 *)((lvt_gchar *)(e.bias + n_w) + 16u * c4);
    unsigned rowb[TM][8];                                          // uniform: bytes from the first row to row m_w + 32 i + 4 u
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int u = 0; u < 8; ++u) rowb[i][u] = (unsigned)(rm(m_w + 32 * i + 4 * u) - rm(m_w)) * ld4;
    lvt_gchar *Cb = (lvt_gchar *)e.C + first;
    lvt_gchar *Rb = f_res ? (lvt_gchar *)e.res + first : nullptr;
    lvt_gchar *Mb = f_mask ? (lvt_gchar *)e.mask + first : nullptr;
    lvt_f32x4 rv[TM][8], mv[TM][8];
#pragma unroll
    for (int i = 0; i < TM; ++i) {                                            // both rounds up front, as in lvt_epi_fast_wave
        if (f_res) {
#pragma unroll
            for (int u = 0; u < 8; ++u) rv[i][u] = *(const lvt_gf32x4 *)(lvt_sgpr_ptr(Rb + rowb[i][u]) + loff);
        }
        if (f_mask) {
#pragma unroll
            for (int u = 0; u < 8; ++u) mv[i][u] = *(const lvt_gf32x4 *)(lvt_sgpr_ptr(Mb + rowb[i][u]) + loff);
        }
    }
    auto key = [](float x) { return (__float_as_uint(x) << 1) + (1u << 24); };
    unsigned am = 1u << 24;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) wave_tile[((r & 3) + 8 * (r >> 2) + 4 * half) * SW + 32 * j + l31] = acc[i][j][r];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            lvt_f32x4 v = *reinterpret_cast<const lvt_f32x4 *>(&wave_tile[(r0 + 4 * u) * SW + 4 * c4]);
            if (f_bias) v += bias4;                      // (vector adds: two v_pk_add_f32, each element rounded as the scalar add)
            if (f_res) v += rv[i][u];
            if (f_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            if (f_leaky) { v.x = lvt_leakyf(v.x); v.y = lvt_leakyf(v.y); v.z = lvt_leakyf(v.z); v.w = lvt_leakyf(v.w); }
            if (f_mask) { v.x = lvt_maskf(v.x, mv[i][u].x, f_lkm); v.y = lvt_maskf(v.y, mv[i][u].y, f_lkm); v.z = lvt_maskf(v.z, mv[i][u].z, f_lkm); v.w = lvt_maskf(v.w, mv[i][u].w, f_lkm); }
            am = max(max(am, key(v.x)), key(v.y));
            am = max(max(am, key(v.z)), key(v.w));
            *(lvt_gf32x4 *)(lvt_sgpr_ptr(Cb + rowb[i][u]) + loff) = v;
        }
    }
    return __uint_as_float((am - (1u << 24)) >> 1);
}

// what a launch must meet for lvt_epi_lean_wave (decided once per workgroup: kernel arguments only)
__device__ __forceinline__ bool lvt_epi_lean_ok(const LvtEpi &e) {
    return e.alpha == 1.f && (unsigned long long)e.ldc < (1ull << 20) && (!(e.flags & LVT_EPI_RESIDUAL) || e.ldr == e.ldc) &&
           (!(e.flags & LVT_EPI_MASK) || e.ldm == e.ldc);
}
// one flag set: the lean form where the launch allows it and the wave's sub-tile is whole, else today's
template <int F, int TM, int TN, class RM = LvtRowIdentity>
__device__ __forceinline__ float lvt_epi_fast_pick(const LvtEpi &e, lvt_f32x16 (&acc)[TM][TN], float *wave_tile, int m_w, int n_w, int lane,
                                                   const RM rm = RM()) {
    if constexpr (F >= 0) {
        const int m_u = __builtin_amdgcn_readfirstlane(m_w), n_u = __builtin_amdgcn_readfirstlane(n_w);   // (uniform already: into SGPRs)
        if (lvt_epi_lean_ok(e) && m_u + TM * 32 <= e.M && n_u + TN * 32 <= e.N)
            return lvt_epi_lean_wave<F, TM, TN, RM>(e, acc, wave_tile, m_u, n_u, lane, rm);
    }
    return lvt_epi_fast_wave<F, TM, TN, RM>(e, acc, wave_tile, m_w, n_w, lane, rm);
}

// the switch over the flag sets of the models' launches
template <int TM, int TN, class RM = LvtRowIdentity>
__device__ __forceinline__ float lvt_epi_fast_dispatch(const LvtEpi &e, lvt_f32x16 (&acc)[TM][TN], float *wave_tile, int m_w, int n_w, int lane,
                                                       const RM rm = RM()) {
#define LVT_EPI_CASE(F) case (F): return lvt_epi_fast_pick<(F), TM, TN, RM>(e, acc, wave_tile, m_w, n_w, lane, rm)
    switch (e.flags & (LVT_EPI_BIAS | LVT_EPI_RESIDUAL | LVT_EPI_RELU | LVT_EPI_MASK | LVT_EPI_LEAKY | LVT_EPI_LEAKY_MASK)) {
    LVT_EPI_CASE(0);
    LVT_EPI_CASE(LVT_EPI_BIAS);
    LVT_EPI_CASE(LVT_EPI_BIAS | LVT_EPI_RELU);
    LVT_EPI_CASE(LVT_EPI_BIAS | LVT_EPI_RESIDUAL);
    LVT_EPI_CASE(LVT_EPI_BIAS | LVT_EPI_RESIDUAL | LVT_EPI_RELU);
    LVT_EPI_CASE(LVT_EPI_RESIDUAL);
    LVT_EPI_CASE(LVT_EPI_MASK);
    LVT_EPI_CASE(LVT_EPI_RESIDUAL | LVT_EPI_MASK);
    LVT_EPI_CASE(LVT_EPI_BIAS | LVT_EPI_LEAKY);                    // the conv + LeakyReLU layers of ConvEncoder / ConvDecoder
    LVT_EPI_CASE(LVT_EPI_MASK | LVT_EPI_LEAKY_MASK);               // and their data gradients
    default: return lvt_epi_fast_wave<-1, TM, TN, RM>(e, acc, wave_tile, m_w, n_w, lane, rm);
    }
#undef LVT_EPI_CASE
}

// max |C| of the workgroup into the device scalar: `seen` is the scalar's value read by thread 0 at the start of the epilogue (a
// stale value only costs an atomic that changes nothing).  scratch: >= blockDim.x / 64 floats of LDS no wave is still using --
// callers pass a region outside the turn-tables.  All threads call; one barrier.
__device__ __forceinline__ unsigned lvt_amax_peek(const float *dst) {
    return (dst && threadIdx.x == 0) ? __hip_atomic_load(reinterpret_cast<const unsigned *>(dst), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
}
__device__ __forceinline__ void lvt_block_amax_commit_seen(float m, float *dst, float *scratch, unsigned seen) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    const int nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) m = fmaxf(m, scratch[w]);
        const unsigned bits = __float_as_uint(m);
        if (bits > seen) atomicMax(reinterpret_cast<unsigned *>(dst), bits);
    }
}
