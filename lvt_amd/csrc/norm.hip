// Batch normalisation of the conv stacks (nn.BatchNorm2d / NaiveSyncBatchNorm / FrozenBatchNorm2d of the reference's
// vidgen/layers/batch_norm.py) on channels-last activations: y is (M = N*H*W, Cp) fp32, Cp = C rounded up to 4, and the
// pad channels C..Cp-1 are zero on entry and on exit.
//
// Every reduction is deterministic: a workgroup owns one (row block, column chunk) tile and writes its partial with plain
// stores; a second launch combines the partials of a channel in a fixed order (in fp64).  The statistics partials are
// (mean, M2) pairs: each thread sums its column slice SHIFTED by the first value it reads (exact by Sterbenz for data
// whose |mean| / std is large, so the fp32 sums see only the spread); the shift is the tile's first row, common to its
// threads, which then merge their shifted (mean, M2) with Chan's pairwise rule.  The shift travels with the partial and is
// added back in fp64, so the mean is rounded to fp32 once.  No float atomics anywhere; the only atomic is the integer max
// of the max |.| reports.
#include "lvt_common.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_TARGET_BLOCKS = 2048;

// Tiling shared by the two column reductions: `tpr` threads per row read 4 channels each (16-byte loads), `rpar` rows are in
// flight per workgroup, a workgroup reduces `rpb` rows of a 4*tpr-channel chunk.  A function of (M, Cp) only, so the
// combine order -- and with it every bit of the result -- does not depend on the device or on the run.
struct BnTile {
    int tpr, rpar, chunks, P;
    long long rpb;
};

BnTile bn_tile(long long M, int Cp) {
    BnTile t;
    t.tpr = 1;
    while (t.tpr * 2 <= 16 && t.tpr * 2 * 4 <= Cp) t.tpr *= 2;
    t.rpar = BN_THREADS / t.tpr;
    t.chunks = (int)lvt_cdiv(Cp, 4 * t.tpr);
    long long target = BN_TARGET_BLOCKS / t.chunks;
    if (target < 1) target = 1;
    long long rpb = lvt_cdiv(M, target);
    if (rpb < 4LL * t.rpar) rpb = 4LL * t.rpar;
    rpb = lvt_cdiv(rpb, t.rpar) * t.rpar;
    t.rpb = rpb;
    t.P = (int)lvt_cdiv(M, rpb);
    return t;
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float el(const float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// (count, mean, M2) merge of b into a (Chan et al.); n == 0 on either side is the identity.
__device__ __forceinline__ void chan_merge(float &ma, float &qa, int &na, float mb, float qb, int nb) {
    if (nb == 0) return;
    if (na == 0) {
        ma = mb; qa = qb; na = nb;
        return;
    }
    const int n = na + nb;
    const float d = mb - ma;
    const float fb = (float)nb / (float)n;
    ma += d * fb;
    qa += qb + d * d * ((float)na * fb);
    na = n;
}

// Per (row block, chunk) partial of every channel of y: mean = pshift + pmean, M2 = pm2 -> [P][Cp] each.
__global__ __launch_bounds__(BN_THREADS) void lvt_bn_stats_partial_kernel(const float *__restrict__ y, long long M, int Cp,
                                                                           int tpr, int rpar, long long rpb,
                                                                           float *__restrict__ pmean, float *__restrict__ pm2,
                                                                           float *__restrict__ pshift) {
    __shared__ float s_mean[BN_THREADS * 4];
    __shared__ float s_m2[BN_THREADS * 4];
    __shared__ int s_n[BN_THREADS];
    const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr;
    const int c = (blockIdx.x * tpr + tx) * 4;
    const long long r0 = (long long)blockIdx.y * rpb;
    const long long r1 = r0 + rpb < M ? r0 + rpb : M;
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 0;
    const float4 s = c < Cp ? ld4(y + r0 * Cp + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < Cp && r0 + ty < r1) {
        float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
        for (long long r = r0 + ty; r < r1; r += rpar, ++n) {
            const float4 v = ld4(y + r * Cp + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = el(v, j) - el(s, j);
                a1[j] += d;
                a2[j] = fmaf(d, d, a2[j]);
            }
        }
        const float inv = 1.f / (float)n;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m = a1[j] * inv;
            mean[j] = m;
            m2[j] = fmaxf(a2[j] - a1[j] * m, 0.f);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s_mean[threadIdx.x * 4 + j] = mean[j];
        s_m2[threadIdx.x * 4 + j] = m2[j];
    }
    s_n[threadIdx.x] = n;
    __syncthreads();
    for (int half = rpar >> 1; half > 0; half >>= 1) {          // fixed pairwise tree over the rows in flight
        if (ty < half) {
            const int a = threadIdx.x, b = threadIdx.x + half * tpr;
            int na = s_n[a];
            const int nb = s_n[b];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int nj = na;
                float ma = s_mean[a * 4 + j], qa = s_m2[a * 4 + j];
                chan_merge(ma, qa, nj, s_mean[b * 4 + j], s_m2[b * 4 + j], nb);
                s_mean[a * 4 + j] = ma;
                s_m2[a * 4 + j] = qa;
            }
            s_n[a] = na + nb;
        }
        __syncthreads();
    }
    if (ty == 0 && c < Cp) {
        const long long o = (long long)blockIdx.y * Cp + c;
        st4(pmean + o, make_float4(s_mean[tx * 4], s_mean[tx * 4 + 1], s_mean[tx * 4 + 2], s_mean[tx * 4 + 3]));
        st4(pm2 + o, make_float4(s_m2[tx * 4], s_m2[tx * 4 + 1], s_m2[tx * 4 + 2], s_m2[tx * 4 + 3]));
        st4(pshift + o, s);
    }
}

// The combines: a workgroup owns CB_CH channels; its CB_LANES lanes per channel take the partials p = lane, lane + CB_LANES, ...
// and a fixed tree adds the lanes (fp64 throughout), so the order is fixed.  The partials (P x Cp, just written, L2-resident)
// are few, so what bounds the combine is how many loads are in flight: one workgroup per channel, 256 lanes, P / 256 loads
// each (at 16 channels per workgroup the 8 - 16 workgroups of a C = 128 - 256 layer walked 64 partials per lane: 22 - 35 us).
constexpr int CB_CH = 1, CB_LANES = BN_THREADS / CB_CH;

__device__ __forceinline__ double lane_sum(double v, double *s, int tx, int ty) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int half = CB_LANES >> 1; half > 0; half >>= 1) {
        if (ty < half) s[threadIdx.x] += s[threadIdx.x + half * CB_CH];
        __syncthreads();
    }
    const double r = s[tx];
    __syncthreads();
    return r;
}

// Partials (mean = pshift + pmean, M2, rows) -> stats[c] = mean, stats[Cp + c] = biased variance; two passes: the mean, then
// sum M2_p + n_p (mean_p - mean)^2.
__global__ __launch_bounds__(BN_THREADS) void lvt_bn_stats_combine_kernel(const float *__restrict__ pmean,
                                                                          const float *__restrict__ pm2,
                                                                          const float *__restrict__ pshift, int P, long long M,
                                                                          long long rpb, int Cp, float *__restrict__ stats) {
    __shared__ double s[BN_THREADS];
    const int tx = threadIdx.x % CB_CH, ty = threadIdx.x / CB_CH;
    const int c = blockIdx.x * CB_CH + tx;
    double a = 0.0;
    if (c < Cp)
        for (int p = ty; p < P; p += CB_LANES) {
            const long long r0 = (long long)p * rpb, o = (long long)p * Cp + c;
            const double nb = (double)((r0 + rpb < M ? r0 + rpb : M) - r0);
            a += nb * ((double)pshift[o] + (double)pmean[o]);
        }
    const double mean = lane_sum(a, s, tx, ty) / (double)M;
    double q = 0.0;
    if (c < Cp)
        for (int p = ty; p < P; p += CB_LANES) {
            const long long r0 = (long long)p * rpb, o = (long long)p * Cp + c;
            const double nb = (double)((r0 + rpb < M ? r0 + rpb : M) - r0);
            const double d = ((double)pshift[o] + (double)pmean[o]) - mean;
            q += (double)pm2[o] + nb * d * d;
        }
    const double m2 = lane_sum(q, s, tx, ty);
    if (ty == 0 && c < Cp) {
        stats[c] = (float)mean;
        stats[Cp + c] = (float)(m2 / (double)M);
    }
}

// scale / shift from batch (or running) statistics, plus the running-statistics update.
__global__ void lvt_bn_finalize_kernel(const float *__restrict__ stats, int nranks, long long count, int C, int Cp,
                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                       float *__restrict__ running_mean, float *__restrict__ running_var,
                                       long long *__restrict__ num_batches_tracked, float momentum, float eps, int flags,
                                       float *__restrict__ scale, float *__restrict__ shift, float *__restrict__ saved) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && (flags & LVT_BN_COUNT) && !(flags & LVT_BN_RUNNING)) num_batches_tracked[0] += 1;
    if (c >= Cp) return;
    if (c >= C) {
        scale[c] = 0.f;
        shift[c] = 0.f;
        saved[c] = 0.f;
        saved[Cp + c] = 0.f;
        return;
    }
    double mean, var;
    if (flags & LVT_BN_RUNNING) {
        mean = running_mean[c];
        var = running_var[c];
    } else {
        // equal-weight merge of the ranks (NaiveSyncBatchNorm, stats_mode ""): mean of the means, and the mean of the
        // variances plus the spread of the means == E[x^2] - mean^2 over the union, without the cancellation
        double s = 0.0;
        for (int r = 0; r < nranks; ++r) s += stats[(long long)r * 2 * Cp + c];
        mean = s / nranks;
        double v = 0.0;
        for (int r = 0; r < nranks; ++r) {
            const double d = stats[(long long)r * 2 * Cp + c] - mean;
            v += stats[(long long)r * 2 * Cp + Cp + c] + d * d;
        }
        var = v / nranks;
    }
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double sc = (double)gamma[c] * rstd;
    scale[c] = (float)sc;
    shift[c] = (float)((double)beta[c] - mean * sc);
    saved[c] = (float)mean;
    saved[Cp + c] = (float)rstd;
    if ((flags & LVT_BN_UPDATE) && !(flags & LVT_BN_RUNNING)) {
        const double n = (double)count * nranks;
        const double vr = (flags & LVT_BN_UNBIASED) ? (n > 1.0 ? var * n / (n - 1.0) : var) : var;
        running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
        running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * vr);
    }
}

// real: the channel is not one of the zero pads (only the sigmoid, whose value at 0 is not 0, needs to know)
__device__ __forceinline__ float bn_act(float v, int flags, bool real) {
    if (flags & LVT_EPI_RELU) return fmaxf(v, 0.f);
    if (flags & LVT_EPI_LEAKY) return lvt_leakyf(v);
    if (flags & LVT_EPI_TANH) return tanhf(v);
    if (flags & LVT_EPI_SIGMOID) return lvt_sigmoid_col(v, real);
    return v;
}

// out = act(y * scale[c] + shift[c] (+ res)), 4 channels per thread, grid-stride; max |out| -> *out_amax.
__global__ __launch_bounds__(BN_THREADS) void lvt_bn_apply_kernel(const float *__restrict__ y, const float *__restrict__ res,
                                                                  long long n4, int Cp, const float *__restrict__ scale,
                                                                  const float *__restrict__ shift, int flags,
                                                                  float *__restrict__ out, float *__restrict__ out_amax) {
    __shared__ float scratch[BN_THREADS / 64];
    const int q = Cp >> 2;
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % q) * 4;
        const float4 v = ld4(y + i * 4), a = ld4(scale + c), b = ld4(shift + c);
        float4 r = make_float4(fmaf(v.x, a.x, b.x), fmaf(v.y, a.y, b.y), fmaf(v.z, a.z, b.z), fmaf(v.w, a.w, b.w));
        if (res) {
            const float4 e = ld4(res + i * 4);
            r.x += e.x; r.y += e.y; r.z += e.z; r.w += e.w;
        }
        const int nr = Cp - LVT_EPI_PAD_OF(flags) - c;
        r.x = bn_act(r.x, flags, nr > 0); r.y = bn_act(r.y, flags, nr > 1); r.z = bn_act(r.z, flags, nr > 2); r.w = bn_act(r.w, flags, nr > 3);
        st4(out + i * 4, r);
        m = fmaxf(m, fmaxf(fmaxf(lvt_absf(r.x), lvt_absf(r.y)), fmaxf(lvt_absf(r.z), lvt_absf(r.w))));
    }
    if (out_amax) lvt_block_amax_commit(m, out_amax, scratch);
}

// Per (row block, chunk) partial sums of g and g * (y - mean[c]) -> part [P][2][Cp].
__global__ __launch_bounds__(BN_THREADS) void lvt_bn_bwd_partial_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                                        const float *__restrict__ saved, long long M, int Cp,
                                                                        int tpr, int rpar, long long rpb, float *__restrict__ part) {
    __shared__ float s_a[BN_THREADS * 4];
    __shared__ float s_b[BN_THREADS * 4];
    const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr;
    const int c = (blockIdx.x * tpr + tx) * 4;
    const long long r0 = (long long)blockIdx.y * rpb;
    const long long r1 = r0 + rpb < M ? r0 + rpb : M;
    float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < Cp) {
        const float4 mu = ld4(saved + c);
        for (long long r = r0 + ty; r < r1; r += rpar) {
            const float4 gv = ld4(g + r * Cp + c), yv = ld4(y + r * Cp + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sa[j] += el(gv, j);
                sb[j] = fmaf(el(gv, j), el(yv, j) - el(mu, j), sb[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s_a[threadIdx.x * 4 + j] = sa[j];
        s_b[threadIdx.x * 4 + j] = sb[j];
    }
    __syncthreads();
    for (int half = rpar >> 1; half > 0; half >>= 1) {
        if (ty < half) {
            const int a = threadIdx.x * 4, b = (threadIdx.x + half * tpr) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s_a[a + j] += s_a[b + j];
                s_b[a + j] += s_b[b + j];
            }
        }
        __syncthreads();
    }
    if (ty == 0 && c < Cp) {
        const long long o = (long long)blockIdx.y * 2 * Cp + c;
        st4(part + o, make_float4(s_a[tx * 4], s_a[tx * 4 + 1], s_a[tx * 4 + 2], s_a[tx * 4 + 3]));
        st4(part + o + Cp, make_float4(s_b[tx * 4], s_b[tx * 4 + 1], s_b[tx * 4 + 2], s_b[tx * 4 + 3]));
    }
}

// sums[c] = sum g, sums[Cp + c] = sum g * xhat = rstd * sum g (y - mean), partials in the fixed lane order (fp64).
__global__ __launch_bounds__(BN_THREADS) void lvt_bn_bwd_combine_kernel(const float *__restrict__ part, int P, int Cp,
                                                                        const float *__restrict__ saved, float *__restrict__ sums) {
    __shared__ double s[BN_THREADS];
    const int tx = threadIdx.x % CB_CH, ty = threadIdx.x / CB_CH;
    const int c = blockIdx.x * CB_CH + tx;
    double a = 0.0, b = 0.0;
    if (c < Cp)
        for (int p = ty; p < P; p += CB_LANES) {
            a += part[(long long)p * 2 * Cp + c];
            b += part[(long long)p * 2 * Cp + Cp + c];
        }
    a = lane_sum(a, s, tx, ty);
    b = lane_sum(b, s, tx, ty);
    if (ty == 0 && c < Cp) {
        sums[c] = (float)a;
        sums[Cp + c] = (float)(b * (double)saved[Cp + c]);
    }
}

// dy = scale (g - sum g / n - xhat sum g xhat / n)  (LVT_BN_TRAIN), else scale g; max |dy| -> *dy_amax.
__global__ __launch_bounds__(BN_THREADS) void lvt_bn_bwd_apply_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                                      long long n4, int Cp, const float *__restrict__ scale,
                                                                      const float *__restrict__ saved, const float *__restrict__ sums,
                                                                      float inv_n, int train, float *__restrict__ dy,
                                                                      float *__restrict__ dy_amax) {
    __shared__ float scratch[BN_THREADS / 64];
    const int q = Cp >> 2;
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % q) * 4;
        const float4 gv = ld4(g + i * 4), a = ld4(scale + c);
        float4 r;
        if (train) {
            const float4 yv = ld4(y + i * 4), mu = ld4(saved + c), rs = ld4(saved + Cp + c);
            const float4 sg = ld4(sums + c), sgx = ld4(sums + Cp + c);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (el(yv, j) - el(mu, j)) * el(rs, j);
                o[j] = el(a, j) * (el(gv, j) - el(sg, j) * inv_n - xh * (el(sgx, j) * inv_n));
            }
            r = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            r = make_float4(a.x * gv.x, a.y * gv.y, a.z * gv.z, a.w * gv.w);
        }
        st4(dy + i * 4, r);
        m = fmaxf(m, fmaxf(fmaxf(lvt_absf(r.x), lvt_absf(r.y)), fmaxf(lvt_absf(r.z), lvt_absf(r.w))));
    }
    if (dy_amax) lvt_block_amax_commit(m, dy_amax, scratch);
}

// Eval fold of up to FOLD_MAX layers per launch (blockIdx.y = layer): scale = gamma rstd from the running statistics,
// exactly as lvt_bn_finalize forms it, into LDS; w_out[o][co][k] = w[o][co][k] scale[co]; bias_out = beta - mean scale
// (pad channels 0); max |w_out| -> *w_amax.
constexpr int FOLD_MAX = 16, FOLD_CO_MAX = 1024;
struct FoldTable { lvt_bn_fold_entry e[FOLD_MAX]; };

__global__ __launch_bounds__(BN_THREADS) void lvt_bn_fold_kernel(const FoldTable t) {
    __shared__ float s_scale[FOLD_CO_MAX];
    __shared__ float scratch[BN_THREADS / 64];
    const lvt_bn_fold_entry &e = t.e[blockIdx.y];
    for (int c = threadIdx.x; c < e.Co; c += blockDim.x) {
        const double rstd = 1.0 / sqrt((double)e.running_var[c] + (double)e.eps);
        const double sc = (double)e.gamma[c] * rstd;
        s_scale[c] = (float)sc;
        if (blockIdx.x == 0) e.bias_out[c] = (float)((double)e.beta[c] - (double)e.running_mean[c] * sc);
    }
    if (blockIdx.x == 0)
        for (int c = e.Co + threadIdx.x; c < e.Cp; c += blockDim.x) e.bias_out[c] = 0.f;
    __syncthreads();
    const long long n = (long long)e.outer * e.Co * e.inner;
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = e.w[i] * s_scale[(i / e.inner) % e.Co];
        e.w_out[i] = v;
        m = fmaxf(m, lvt_absf(v));
    }
    if (e.w_amax) lvt_block_amax_commit(m, e.w_amax, scratch);
}

int grid_for(long long work) {
    long long b = lvt_cdiv(work, BN_THREADS);
    if (b > 8LL * LVT_NUM_CU) b = 8LL * LVT_NUM_CU;
    return (int)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" size_t lvt_bn_workspace_bytes(long long M, int Cp) {
    if (M <= 0 || Cp <= 0) return 0;
    const BnTile t = bn_tile(M, Cp);
    return (size_t)t.P * 3 * Cp * sizeof(float);
}

extern "C" int lvt_bn_stats(const float *y, long long M, int Cp, float *stats, void *workspace, size_t workspace_bytes,
                            void *stream) {
    LVT_REQUIRE(y && stats && workspace && M > 0 && Cp > 0 && Cp % 4 == 0, "lvt_bn_stats: bad arguments (M=%lld Cp=%d)", M, Cp);
    LVT_REQUIRE(lvt_aligned16(y) && lvt_aligned16(workspace), "lvt_bn_stats: y / workspace must be 16-byte aligned");
    const BnTile t = bn_tile(M, Cp);
    if (workspace_bytes < (size_t)t.P * 3 * Cp * sizeof(float)) {
        lvt_set_error("lvt_bn_stats: workspace too small");
        return LVT_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    float *pmean = (float *)workspace, *pm2 = pmean + (size_t)t.P * Cp, *pshift = pm2 + (size_t)t.P * Cp;
    lvt_bn_stats_partial_kernel<<<dim3(t.chunks, t.P), BN_THREADS, 0, s>>>(y, M, Cp, t.tpr, t.rpar, t.rpb, pmean, pm2, pshift);
    LVT_CHECK_LAUNCH("lvt_bn_stats_partial");
    lvt_bn_stats_combine_kernel<<<(int)lvt_cdiv(Cp, CB_CH), BN_THREADS, 0, s>>>(pmean, pm2, pshift, t.P, M, t.rpb, Cp,
                                                                                      stats);
    LVT_CHECK_LAUNCH("lvt_bn_stats_combine");
    return LVT_OK;
}

extern "C" int lvt_bn_finalize(const float *stats, int nranks, long long count, int C, int Cp, const float *gamma,
                               const float *beta, float *running_mean, float *running_var, long long *num_batches_tracked,
                               float momentum, float eps, int flags, float *scale, float *shift, float *saved, void *stream) {
    LVT_REQUIRE(gamma && beta && scale && shift && saved && C > 0 && Cp >= C && Cp % 4 == 0,
                "lvt_bn_finalize: bad arguments (C=%d Cp=%d)", C, Cp);
    LVT_REQUIRE((flags & LVT_BN_RUNNING) ? (running_mean && running_var) : (stats && nranks > 0 && count > 0),
                "lvt_bn_finalize: missing statistics");
    LVT_REQUIRE(!(flags & LVT_BN_UPDATE) || (running_mean && running_var), "lvt_bn_finalize: LVT_BN_UPDATE needs the running buffers");
    LVT_REQUIRE(!(flags & LVT_BN_COUNT) || num_batches_tracked, "lvt_bn_finalize: LVT_BN_COUNT needs num_batches_tracked");
    lvt_bn_finalize_kernel<<<(int)lvt_cdiv(Cp, BN_THREADS), BN_THREADS, 0, (hipStream_t)stream>>>(
        stats, nranks, count, C, Cp, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, flags, scale,
        shift, saved);
    LVT_CHECK_LAUNCH("lvt_bn_finalize");
    return LVT_OK;
}

extern "C" int lvt_bn_apply(const float *y, const float *res, long long M, int Cp, const float *scale, const float *shift,
                            int flags, float *out, float *out_amax, void *stream) {
    LVT_REQUIRE(y && scale && shift && out && M > 0 && Cp > 0 && Cp % 4 == 0, "lvt_bn_apply: bad arguments");
    LVT_REQUIRE(!(flags & LVT_EPI_LEAKY) || !(flags & (LVT_EPI_RELU | LVT_EPI_TANH | LVT_EPI_SIGMOID)),
                "lvt_bn_apply: LVT_EPI_LEAKY excludes RELU / TANH / SIGMOID");
    LVT_REQUIRE(lvt_aligned16(y) && lvt_aligned16(out) && lvt_aligned16(scale) && lvt_aligned16(shift) && (!res || lvt_aligned16(res)),
                "lvt_bn_apply: operands must be 16-byte aligned");
    const long long n4 = M * Cp / 4;
    lvt_bn_apply_kernel<<<grid_for(n4), BN_THREADS, 0, (hipStream_t)stream>>>(y, res, n4, Cp, scale, shift, flags, out, out_amax);
    LVT_CHECK_LAUNCH("lvt_bn_apply");
    return LVT_OK;
}

extern "C" int lvt_bn_bwd_reduce(const float *g, const float *y, long long M, int Cp, const float *saved, float *sums,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    LVT_REQUIRE(g && y && saved && sums && workspace && M > 0 && Cp > 0 && Cp % 4 == 0, "lvt_bn_bwd_reduce: bad arguments");
    LVT_REQUIRE(lvt_aligned16(g) && lvt_aligned16(y) && lvt_aligned16(saved) && lvt_aligned16(workspace),
                "lvt_bn_bwd_reduce: operands must be 16-byte aligned");
    const BnTile t = bn_tile(M, Cp);
    if (workspace_bytes < (size_t)t.P * 2 * Cp * sizeof(float)) {
        lvt_set_error("lvt_bn_bwd_reduce: workspace too small");
        return LVT_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    float *part = (float *)workspace;
    lvt_bn_bwd_partial_kernel<<<dim3(t.chunks, t.P), BN_THREADS, 0, s>>>(g, y, saved, M, Cp, t.tpr, t.rpar, t.rpb, part);
    LVT_CHECK_LAUNCH("lvt_bn_bwd_partial");
    lvt_bn_bwd_combine_kernel<<<(int)lvt_cdiv(Cp, CB_CH), BN_THREADS, 0, s>>>(part, t.P, Cp, saved, sums);
    LVT_CHECK_LAUNCH("lvt_bn_bwd_combine");
    return LVT_OK;
}

extern "C" int lvt_bn_bwd_apply(const float *g, const float *y, long long M, int Cp, const float *scale, const float *saved,
                                const float *sums, long long n, int flags, float *dy, float *dy_amax, void *stream) {
    const int train = (flags & LVT_BN_TRAIN) != 0;
    LVT_REQUIRE(g && scale && dy && M > 0 && Cp > 0 && Cp % 4 == 0, "lvt_bn_bwd_apply: bad arguments");
    LVT_REQUIRE(!train || (y && saved && sums && n > 0), "lvt_bn_bwd_apply: LVT_BN_TRAIN needs y, saved, sums and n");
    LVT_REQUIRE(lvt_aligned16(g) && lvt_aligned16(dy) && lvt_aligned16(scale) && (!train || (lvt_aligned16(y) &&
                lvt_aligned16(saved) && lvt_aligned16(sums))), "lvt_bn_bwd_apply: operands must be 16-byte aligned");
    const long long n4 = M * Cp / 4;
    lvt_bn_bwd_apply_kernel<<<grid_for(n4), BN_THREADS, 0, (hipStream_t)stream>>>(g, y, n4, Cp, scale, saved, sums,
                                                                                  train ? (float)(1.0 / (double)n) : 0.f, train,
                                                                                  dy, dy_amax);
    LVT_CHECK_LAUNCH("lvt_bn_bwd_apply");
    return LVT_OK;
}

extern "C" int lvt_bn_fold(const lvt_bn_fold_entry *entries, int n, void *stream) {
    LVT_REQUIRE(entries && n > 0, "lvt_bn_fold: bad arguments");
    for (int base = 0; base < n; base += FOLD_MAX) {
        const int cnt = n - base < FOLD_MAX ? n - base : FOLD_MAX;
        FoldTable t;
        long long biggest = 0;
        for (int i = 0; i < cnt; ++i) {
            const lvt_bn_fold_entry &e = entries[base + i];
            LVT_REQUIRE(e.w && e.w_out && e.gamma && e.beta && e.running_mean && e.running_var && e.bias_out && e.outer > 0 &&
                        e.Co > 0 && e.Co <= FOLD_CO_MAX && e.Cp >= e.Co && e.inner > 0,
                        "lvt_bn_fold: bad entry %d (Co <= %d)", base + i, FOLD_CO_MAX);
            t.e[i] = e;
            const long long ne = (long long)e.outer * e.Co * e.inner;
            if (ne > biggest) biggest = ne;
        }
        lvt_bn_fold_kernel<<<dim3(grid_for(biggest) / 8 + 1, cnt), BN_THREADS, 0, (hipStream_t)stream>>>(t);
        LVT_CHECK_LAUNCH("lvt_bn_fold");
    }
    return LVT_OK;
}
