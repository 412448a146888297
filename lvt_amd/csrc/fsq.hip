// Finite scalar quantisation (MODEL.CODEBOOK.FSQ.LEVELS): the bound-and-round of the projected rows, its
// straight-through backward and the decode from code indices.  The rule is stated once in plain torch
// (lvt_amd/modeling/vq/fsq.py); per entry i of a d-wide group, with the constants of level L_i formed on the host in float64,
//   fwd:    b = tanh(z_p + shift) * half_l - offset,  q = rint(b),  digit = q + w,  z_q = q / w,  idx = sum digit_i prod_{j<i} L_j
//   bwd:    dz_p = g * (half_l / w) * (1 - tanh^2(z_p + shift))
//   decode: digits of idx by successive division, z_q = (digit - w) / w           (the same quotient: the same bits as fwd)
// Rows of num * d floats with a row stride ld >= num * d, ld a multiple of 4; the pad columns [num * d, ld) are written as 0.
// Streaming: one thread owns a row and walks it in 16-byte loads and stores -- the column index, and with it the entry of the
// level table, is the same in every lane, so the table is read from the launch arguments with scalar loads and nothing is
// indexed per lane; the lanes of a wave hold consecutive rows, whose float4s share cache lines across the walk, and the int64
// codes of a group are consecutive in (rows / P, num, P).  Every output element is a function of its own input element(s): no
// reductions, no LDS traffic (the 16 bytes below are the scratch of the max |.| record, one integer atomic max per workgroup:
// lvt_common.h), no float atomics, the same bits run to run.
#include <math.h>
#include "lvt_common.h"

#define FSQ_THREADS 256
#define FSQ_LD_MAX 4096
#define FSQ_CODES_MAX (1ll << 30)

struct fsq_table {
    int d;
    int L[LVT_FSQ_MAX_LEVELS], w[LVT_FSQ_MAX_LEVELS];
    float half_l[LVT_FSQ_MAX_LEVELS], shift[LVT_FSQ_MAX_LEVELS], offset[LVT_FSQ_MAX_LEVELS], wf[LVT_FSQ_MAX_LEVELS],
        slope[LVT_FSQ_MAX_LEVELS];
};

__device__ __forceinline__ float fsq_amax4(float am, const float4 &o) {
    return fmaxf(am, fmaxf(fmaxf(lvt_absf(o.x), lvt_absf(o.y)), fmaxf(lvt_absf(o.z), lvt_absf(o.w))));
}

// position of (row r, group 0) in the (rows / P, num, P) code tensor; group g sits g * P further
__device__ __forceinline__ long long fsq_code_base(long long r, int num, int P) { return (r / P) * num * P + r % P; }

template <bool ZQ, bool IDX>
__global__ __launch_bounds__(FSQ_THREADS) void lvt_fsq_fwd_kernel(const float *__restrict__ zp, long long rows, int num, int nq,
                                                                   fsq_table t, int P, float *__restrict__ zq,
                                                                   long long *__restrict__ idx, float *out_amax) {
    __shared__ float amax_scratch[FSQ_THREADS / 64];
    const int nd = num * t.d;
    float am = 0.f;
    for (long long r = (long long)blockIdx.x * FSQ_THREADS + threadIdx.x; r < rows; r += (long long)gridDim.x * FSQ_THREADS) {
        const float4 *src = reinterpret_cast<const float4 *>(zp) + r * nq;
        float4 *dst = reinterpret_cast<float4 *>(zq) + r * nq;
        long long *ip = IDX ? idx + fsq_code_base(r, num, P) : nullptr;
        int i = 0;                                   // entry of the group: the same in every lane
        unsigned code = 0, mult = 1;
        for (int q = 0; q < nq; ++q) {
            const float4 v4 = src[q];
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = 0.f;
                if (4 * q + j < nd) {
                    const int w = t.w[i];
                    const float b = tanhf(v[j] + t.shift[i]) * t.half_l[i] - t.offset[i];
                    // (the rule's range [-w, L - 1 - w] holds for every finite input; the clamp keeps a NaN row's code a code)
                    const float qv = fmaxf(fminf(rintf(b), (float)(t.L[i] - 1 - w)), (float)-w);
                    const int digit = (int)qv + w;
                    o[j] = (float)(digit - w) / t.wf[i];      // (from the integer, as decode forms it: rint(-0.3) = -0 is stored as +0)
                    code += (unsigned)digit * mult;
                    mult *= (unsigned)t.L[i];
                    if (++i == t.d) {
                        if (IDX) {
                            *ip = (long long)code;
                            ip += P;
                        }
                        i = 0, code = 0, mult = 1;
                    }
                }
            }
            if (ZQ) {
                const float4 o4 = make_float4(o[0], o[1], o[2], o[3]);
                dst[q] = o4;
                am = fsq_amax4(am, o4);
            }
        }
    }
    if (ZQ && out_amax) lvt_block_amax_commit(am, out_amax, amax_scratch);
}

__global__ __launch_bounds__(FSQ_THREADS) void lvt_fsq_bwd_kernel(const float *__restrict__ g, const float *__restrict__ zp,
                                                                   long long rows, int num, int nq, fsq_table t,
                                                                   float *__restrict__ dzp, float *out_amax) {
    __shared__ float amax_scratch[FSQ_THREADS / 64];
    const int nd = num * t.d;
    float am = 0.f;
    for (long long r = (long long)blockIdx.x * FSQ_THREADS + threadIdx.x; r < rows; r += (long long)gridDim.x * FSQ_THREADS) {
        const float4 *gs = reinterpret_cast<const float4 *>(g) + r * nq;
        const float4 *zs = reinterpret_cast<const float4 *>(zp) + r * nq;
        float4 *dst = reinterpret_cast<float4 *>(dzp) + r * nq;
        int i = 0;
        for (int q = 0; q < nq; ++q) {
            const float4 g4 = gs[q], z4 = zs[q];
            const float a[4] = {g4.x, g4.y, g4.z, g4.w}, v[4] = {z4.x, z4.y, z4.z, z4.w};
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = 0.f;
                if (4 * q + j < nd) {
                    const float th = tanhf(v[j] + t.shift[i]);
                    o[j] = a[j] * (t.slope[i] * (1.f - th * th));
                    if (++i == t.d) i = 0;
                }
            }
            const float4 o4 = make_float4(o[0], o[1], o[2], o[3]);
            dst[q] = o4;
            am = fsq_amax4(am, o4);
        }
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, amax_scratch);
}

__global__ __launch_bounds__(FSQ_THREADS) void lvt_fsq_decode_kernel(const long long *__restrict__ idx, long long rows, int num,
                                                                      int nq, fsq_table t, int P, float *__restrict__ zq,
                                                                      float *out_amax) {
    __shared__ float amax_scratch[FSQ_THREADS / 64];
    const int nd = num * t.d;
    float am = 0.f;
    for (long long r = (long long)blockIdx.x * FSQ_THREADS + threadIdx.x; r < rows; r += (long long)gridDim.x * FSQ_THREADS) {
        const long long *ip = idx + fsq_code_base(r, num, P);
        float4 *dst = reinterpret_cast<float4 *>(zq) + r * nq;
        int i = 0;
        unsigned rest = 0;
        for (int q = 0; q < nq; ++q) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = 0.f;
                if (4 * q + j < nd) {
                    if (i == 0) {
                        rest = (unsigned)*ip;            // (a code is below prod(levels) <= 2^30; whatever else arrives decodes
                        ip += P;                         //  to in-range digits of its low 32 bits)
                    }
                    const unsigned L = (unsigned)t.L[i];
                    const int digit = (int)(rest % L);
                    rest /= L;
                    o[j] = (float)(digit - t.w[i]) / t.wf[i];
                    if (++i == t.d) i = 0;
                }
            }
            const float4 o4 = make_float4(o[0], o[1], o[2], o[3]);
            dst[q] = o4;
            am = fsq_amax4(am, o4);
        }
    }
    if (out_amax) lvt_block_amax_commit(am, out_amax, amax_scratch);
}

// the constants of fsq.py step 2, formed in float64 and handed over as floats
static int fsq_make_table(const char *name, long long rows, int num, int ld, const lvt_fsq_levels &lv, fsq_table &t) {
    LVT_REQUIRE(rows > 0 && num >= 1, "%s: rows = %lld, num = %d: at least one row and one group", name, rows, num);
    LVT_REQUIRE(lv.d >= 1 && lv.d <= LVT_FSQ_MAX_LEVELS, "%s: %d levels, from 1 to %d", name, lv.d, LVT_FSQ_MAX_LEVELS);
    long long codes = 1;
    for (int i = 0; i < LVT_FSQ_MAX_LEVELS; ++i) {
        const int L = i < lv.d ? lv.levels[i] : 2;
        LVT_REQUIRE(L >= 2 && L <= 64, "%s: level %d is %d, from 2 to 64", name, i, L);
        if (i < lv.d) codes *= L;
        LVT_REQUIRE(codes <= FSQ_CODES_MAX, "%s: prod(levels) above 2^30", name);
        const double half_l = (L - 1.0) * (1.0 + 1e-3) / 2.0, offset = L % 2 == 0 ? 0.5 : 0.0;
        t.L[i] = L;
        t.w[i] = L / 2;
        t.wf[i] = (float)(L / 2);
        t.half_l[i] = (float)half_l;
        t.offset[i] = (float)offset;
        t.shift[i] = (float)atanh(offset / half_l);
        t.slope[i] = (float)(half_l / (L / 2));
    }
    t.d = lv.d;
    LVT_REQUIRE(ld % 4 == 0 && ld <= FSQ_LD_MAX && (long long)num * lv.d <= ld,
                "%s: row stride ld = %d, a multiple of 4 from num * d = %lld to %d", name, ld, (long long)num * lv.d, FSQ_LD_MAX);
    return LVT_OK;
}

static int fsq_check_codes(const char *name, const void *idx, long long rows, int P) {
    LVT_REQUIRE(P >= 1 && rows % P == 0, "%s: P = %d positions per sample must divide rows = %lld", name, P, rows);
    LVT_REQUIRE((((uintptr_t)idx) & 7) == 0, "%s: idx must be 8-byte aligned", name);
    return LVT_OK;
}

// a function of `rows` only: one row per thread, at most 8 workgroups per CU; the grid-stride loop takes the rest
static unsigned fsq_blocks(long long rows) {
    const long long b = lvt_cdiv(rows, FSQ_THREADS);
    return (unsigned)(b > 8 * LVT_NUM_CU ? 8 * LVT_NUM_CU : b);
}

extern "C" int lvt_fsq_fwd(const float *z_p, long long rows, int num, int ld, lvt_fsq_levels levels, int P, float *z_q,
                           long long *idx, unsigned *out_amax, void *stream) {
    fsq_table t;
    if (int rc = fsq_make_table("lvt_fsq_fwd", rows, num, ld, levels, t)) return rc;
    LVT_REQUIRE(z_p && (z_q || idx), "lvt_fsq_fwd: null z_p, or neither z_q nor idx");
    LVT_REQUIRE(lvt_aligned16(z_p) && lvt_aligned16(z_q), "lvt_fsq_fwd: z_p and z_q must be 16-byte aligned");
    LVT_REQUIRE((((uintptr_t)out_amax) & 3) == 0, "lvt_fsq_fwd: out_amax must be 4-byte aligned");
    if (idx)
        if (int rc = fsq_check_codes("lvt_fsq_fwd", idx, rows, P)) return rc;
    const dim3 grid(fsq_blocks(rows)), block(FSQ_THREADS);
    hipStream_t s = (hipStream_t)stream;
    float *am = reinterpret_cast<float *>(out_amax);
    const int nq = ld / 4;
    if (z_q && idx) hipLaunchKernelGGL((lvt_fsq_fwd_kernel<true, true>), grid, block, 0, s, z_p, rows, num, nq, t, P, z_q, idx, am);
    else if (z_q) hipLaunchKernelGGL((lvt_fsq_fwd_kernel<true, false>), grid, block, 0, s, z_p, rows, num, nq, t, 1, z_q, idx, am);
    else hipLaunchKernelGGL((lvt_fsq_fwd_kernel<false, true>), grid, block, 0, s, z_p, rows, num, nq, t, P, z_q, idx, am);
    LVT_CHECK_LAUNCH("lvt_fsq_fwd_kernel");
    return LVT_OK;
}

extern "C" int lvt_fsq_bwd(const float *g, const float *z_p, long long rows, int num, int ld, lvt_fsq_levels levels, float *dz_p,
                           unsigned *out_amax, void *stream) {
    fsq_table t;
    if (int rc = fsq_make_table("lvt_fsq_bwd", rows, num, ld, levels, t)) return rc;
    LVT_REQUIRE(g && z_p && dz_p, "lvt_fsq_bwd: null pointer");
    LVT_REQUIRE(lvt_aligned16(g) && lvt_aligned16(z_p) && lvt_aligned16(dz_p), "lvt_fsq_bwd: g, z_p and dz_p must be 16-byte aligned");
    LVT_REQUIRE((((uintptr_t)out_amax) & 3) == 0, "lvt_fsq_bwd: out_amax must be 4-byte aligned");
    hipLaunchKernelGGL(lvt_fsq_bwd_kernel, dim3(fsq_blocks(rows)), dim3(FSQ_THREADS), 0, (hipStream_t)stream, g, z_p, rows, num,
                       ld / 4, t, dz_p, reinterpret_cast<float *>(out_amax));
    LVT_CHECK_LAUNCH("lvt_fsq_bwd_kernel");
    return LVT_OK;
}

extern "C" int lvt_fsq_decode(const long long *idx, long long rows, int num, int ld, lvt_fsq_levels levels, int P, float *z_q,
                              unsigned *out_amax, void *stream) {
    fsq_table t;
    if (int rc = fsq_make_table("lvt_fsq_decode", rows, num, ld, levels, t)) return rc;
    LVT_REQUIRE(idx && z_q, "lvt_fsq_decode: null pointer");
    LVT_REQUIRE(lvt_aligned16(z_q), "lvt_fsq_decode: z_q must be 16-byte aligned");
    LVT_REQUIRE((((uintptr_t)out_amax) & 3) == 0, "lvt_fsq_decode: out_amax must be 4-byte aligned");
    if (int rc = fsq_check_codes("lvt_fsq_decode", idx, rows, P)) return rc;
    hipLaunchKernelGGL(lvt_fsq_decode_kernel, dim3(fsq_blocks(rows)), dim3(FSQ_THREADS), 0, (hipStream_t)stream, idx, rows, num,
                       ld / 4, t, P, z_q, reinterpret_cast<float *>(out_amax));
    LVT_CHECK_LAUNCH("lvt_fsq_decode_kernel");
    return LVT_OK;
}
