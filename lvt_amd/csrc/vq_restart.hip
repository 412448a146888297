// Codebook restart (MODEL.CODEBOOK.RESTART): re-seed codes that no row selects from encoder outputs of the
// current pass, and record codebook health.  Two launches around the all-reduce of the EMA statistics:
//   lvt_vq_restart_candidates    cand[g][k][:] = sub-vector g of the global row r(seed, pass, g, k) if this rank owns the row,
//                                else zeros -- for ALL codes, because which ones are dead is known only after the all-reduce.
//                                `cand` lies behind `stats` in ONE buffer, so the SUM over ranks that completes the statistics
//                                also gathers the candidates exactly (every rank but the owner adds zeros).
//   lvt_vq_ema_finalize_restart  the arithmetic of lvt_vq_ema_finalize (csrc/vq.hip), then: a code whose global count of
//                                this pass is 0 and whose updated running_size is below the threshold takes its candidate
//                                (weight = c, running_sum = c * threshold, running_size = threshold); health record,
//                                cumulative restart counter, pass counter.
// No atomics, fixed summation order, plain vector stores.  One workgroup per codebook group owns everything it writes; the
// pass counter is written by workgroup 0 alone and read by nobody in that launch.
#include "lvt_common.h"

#define RST_THREADS 512

// splitmix64's finaliser: the counter-based hash of the draw (restated in Python: lvt_amd/hip/vq.py restart_row)
__host__ __device__ static inline unsigned long long rst_mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// global row that code k of codebook i draws in pass `pass`: uniform in its own stratum [k R / K, (k + 1) R / K) of the R rows
// (an empty stratum, R < K: its lower end, which is < R).  k R < 2^11 R: no overflow below 2^52 rows.
__host__ __device__ static inline long long rst_row(unsigned long long seed, unsigned long long pass, int i, int k, long long R,
                                                    int KC) {
    const unsigned long long h = rst_mix64(seed ^ (pass * 0x9E3779B97F4A7C15ULL) ^ (((unsigned long long)(unsigned)i << 32) | (unsigned)k));
    const long long lo = (long long)k * R / KC, hi = (long long)(k + 1) * R / KC;
    return lo + (hi > lo ? (long long)(h % (unsigned long long)(hi - lo)) : 0);
}

// one thread per 16 bytes of cand: consecutive lanes copy consecutive float4 of one row (D / 4 lanes per code)
__global__ __launch_bounds__(256) void lvt_vq_restart_candidates_kernel(const float *__restrict__ z, long long rows_local, int ldz,
                                                                       int D, int KC, long long row0, long long R,
                                                                       unsigned long long seed,
                                                                       const long long *__restrict__ pass, int shared_index,
                                                                       float *__restrict__ cand) {
    const int g = blockIdx.y, q = D >> 2;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= KC * q) return;
    const int k = item / q, c = item - k * q;
    const long long r = rst_row(seed, (unsigned long long)*pass, shared_index ? 0 : g, k, R, KC) - row0;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r >= 0 && r < rows_local) v = *reinterpret_cast<const float4 *>(z + r * ldz + (long long)g * D + 4 * c);
    *reinterpret_cast<float4 *>(cand + ((long long)g * KC + k) * D + 4 * c) = v;
}

// sum over the workgroup in the fixed order of a binary tree; every thread gets the result
template <class T>
__device__ __forceinline__ T rst_block_sum(T v, T *red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = RST_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// one workgroup of RST_THREADS per codebook group.  The update is lvt_vq_ema_finalize_kernel's, operation for operation (the
// same expressions, the same tree over the same 512 partial sums for n): a code that is not restarted comes out bit for bit
// as it does there.
template <int DT>
__global__ __launch_bounds__(RST_THREADS) void lvt_vq_ema_finalize_restart_kernel(
    const float *__restrict__ stats, const float *__restrict__ cand, int KC, int d_arg, float decay, float one_minus_decay,
    float eps, float threshold, float *__restrict__ running_size, float *__restrict__ running_sum, float *__restrict__ weight,
    float *__restrict__ health, long long *__restrict__ total, long long *__restrict__ pass) {
    const int D = DT ? DT : d_arg;
    __shared__ float red[RST_THREADS];
    __shared__ double redd[RST_THREADS];
    __shared__ int redi[RST_THREADS];
    __shared__ unsigned char dead[2048];            // 1: restarted in this pass
    __shared__ float ntot;
    const int g = blockIdx.x, tid = threadIdx.x;
    float *rs = running_size + (long long)g * KC;
    float *rsum = running_sum + (long long)g * KC * D;
    float *w = weight + (long long)g * KC * D;
    const float *st = stats + (long long)g * KC * (D + 1);
    const float *cd = cand + (long long)g * KC * D;
    float part = 0.f;
    double cnt = 0.0;
    int ndead = 0, nrest = 0;
    for (int k = tid; k < KC; k += blockDim.x) {
        const float count = st[k * (D + 1) + D];
        const float v = rs[k] * decay + one_minus_decay * count;
        rs[k] = v;
        part += v;
        cnt += (double)count;
        const bool below = v < threshold, restart = below && count == 0.f;
        dead[k] = restart;
        ndead += below;
        nrest += restart;
    }
    red[tid] = part;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) ntot = red[0];
    __syncthreads();
    const float n = ntot;               // (taken before any restart)
    // health: perplexity exp(-sum p ln p) of this pass's global counts in fp64, rounded once
    const double all = rst_block_sum(cnt, redd);
    double ent = 0.0;
    for (int k = tid; k < KC; k += blockDim.x) {
        const float count = st[k * (D + 1) + D];
        if (count > 0.f) {
            const double p = (double)count / all;
            ent += p * log(p);
        }
    }
    ent = rst_block_sum(ent, redd);
    ndead = rst_block_sum(ndead, redi);
    nrest = rst_block_sum(nrest, redi);
    constexpr int FB = 8;
    const int tot = KC * D;
    for (int i0 = tid; i0 < tot; i0 += blockDim.x * FB) {
        float a[FB], b[FB], c[FB], e[FB];
        bool re[FB];
#pragma unroll
        for (int u = 0; u < FB; ++u) {
            const int i = i0 + u * blockDim.x;
            const bool ok = i < tot;
            const int k = ok ? i / D : 0, d = DT || ok ? i % D : 0;
            a[u] = ok ? rsum[i] : 0.f; b[u] = st[k * (D + 1) + d]; c[u] = rs[k];
            re[u] = dead[k] != 0;
            e[u] = ok && re[u] ? cd[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < FB; ++u) {
            const int i = i0 + u * blockDim.x;
            if (i < tot) {
                const float s = a[u] * decay + one_minus_decay * b[u];
                const float size_ = (c[u] + eps) / (n + KC * eps) * n;
                rsum[i] = re[u] ? e[u] * threshold : s;
                w[i] = re[u] ? e[u] : s / size_;
            }
        }
    }
    __syncthreads();                    // every read of rs[] above is done
    for (int k = tid; k < KC; k += blockDim.x)
        if (dead[k]) rs[k] = threshold;
    if (tid == 0) {
        health[3 * g + 0] = all > 0.0 ? (float)exp(-ent) : 0.f;
        health[3 * g + 1] = (float)ndead;
        health[3 * g + 2] = (float)nrest;
        total[g] += nrest;
        if (g == 0) *pass += 1;
    }
}

static bool rst_geometry_ok(int D, int KC) { return D % 16 == 0 && D >= 16 && D <= 256 && KC % 64 == 0 && KC >= 64 && KC <= 2048; }

extern "C" int lvt_vq_restart_candidates(const float *z, long long rows_local, int ldz, int num, int D, int KC, int P, int rank,
                                         int world, unsigned long long seed, const long long *pass, int shared_index,
                                         float *cand, void *stream) {
    LVT_REQUIRE(z && pass && cand, "vq_restart_candidates: null pointer");
    LVT_REQUIRE(rst_geometry_ok(D, KC),
                "vq_restart_candidates: unsupported geometry D=%d KC=%d (D: multiple of 16 in 16..256; KC: multiple of 64 in 64..2048)",
                D, KC);
    LVT_REQUIRE(rows_local > 0 && num > 0 && P > 0 && rows_local % P == 0, "vq_restart_candidates: bad rows/P");
    LVT_REQUIRE(world > 0 && rank >= 0 && rank < world, "vq_restart_candidates: rank %d of world %d", rank, world);
    LVT_REQUIRE(rows_local <= (1LL << 40) / world, "vq_restart_candidates: too many rows");
    LVT_REQUIRE(ldz % 4 == 0 && ldz >= num * D && lvt_aligned16(z) && lvt_aligned16(cand), "vq_restart_candidates: alignment / ldz");
    const dim3 grid((unsigned)lvt_cdiv((long long)KC * (D / 4), 256), num);
    hipLaunchKernelGGL(lvt_vq_restart_candidates_kernel, grid, dim3(256), 0, (hipStream_t)stream, z, rows_local, ldz, D, KC,
                       (long long)rank * rows_local, (long long)world * rows_local, seed, pass, shared_index, cand);
    LVT_CHECK_LAUNCH("lvt_vq_restart_candidates_kernel");
    return LVT_OK;
}

extern "C" int lvt_vq_ema_finalize_restart(const float *stats, const float *cand, int num, int D, int KC, float decay, float eps,
                                           float threshold, float *running_size, float *running_sum, float *weight,
                                           float *health, long long *restarts_total, long long *pass, void *stream) {
    LVT_REQUIRE(stats && cand && running_size && running_sum && weight && health && restarts_total && pass && num > 0,
                "vq_ema_finalize_restart: bad args");
    LVT_REQUIRE(rst_geometry_ok(D, KC),
                "vq_ema_finalize_restart: unsupported geometry D=%d KC=%d (D: multiple of 16 in 16..256; KC: multiple of 64 in 64..2048)",
                D, KC);
    LVT_REQUIRE(threshold >= 0.f && threshold < __builtin_inff(), "vq_ema_finalize_restart: threshold must be finite and >= 0");
    // (1 - decay) as lvt_vq_ema_finalize takes it
    const float omd = (float)(1.0 - (double)decay);
    hipLaunchKernelGGL(D == 64 ? lvt_vq_ema_finalize_restart_kernel<64> : lvt_vq_ema_finalize_restart_kernel<0>, dim3(num),
                       dim3(RST_THREADS), 0, (hipStream_t)stream, stats, cand, KC, D, decay, omd, eps, threshold, running_size,
                       running_sum, weight, health, restarts_total, pass);
    LVT_CHECK_LAUNCH("lvt_vq_ema_finalize_restart_kernel");
    return LVT_OK;
}
