// Per-frame PSNR and SSIM of channels-first fp32 frames (FrameQualityEvaluator; the rule in plain Python:
// lvt_amd/evaluation/quality.py frame_quality_reference).  SSIM is Wang et al. 2004: 11x11 Gaussian window, sigma 1.5, no
// padding, weighted biased variances, C1 = (0.01 L)^2, C2 = (0.03 L)^2; the SSIM of a frame is the mean of the map over its
// channels and positions.  Two launches:
//   lvt_frame_quality         one workgroup per (plane, FQ_TH x FQ_TW tile of the map): the (FQ_TH + 10) x (FQ_TW + 10) input tile
//                             of both planes goes to LDS once, minus a per-tile pivot (the tile's first pixel of each plane); the
//                             horizontal 11-tap pass leaves the five windowed quantities (x, y, x^2, y^2, xy) in LDS, the vertical
//                             pass and the SSIM ratio stay in registers.  The second moments are taken about the pivot: variance and
//                             covariance do not move with a shift, and E[x^2] - mu^2 of the unshifted values loses 3e-4 of the
//                             SSIM of a bright flat frame in fp32.  -> two fp64 partials per workgroup (sum of the SSIM map over
//                             the tile, sum of squared differences over the input pixels the tile OWNS), plain stores.
//   lvt_frame_quality_finish  one workgroup: per frame the partials of its channels and tiles added in a fixed order -> frames[f] =
//                             {psnr, ssim}, and the caller's accumulator {sum psnr, sum ssim, frames with mse != 0, frames}.
// lvt_frame_quality_vs is the first launch with frame f of `a` compared against frame f % Fb of `b` (S sampled videos against
// one target, PredictionQualityEvaluator): the same kernel, whose workgroups look up their plane of b.
//   lvt_prediction_select     one workgroup over the (S, T) table `finish` wrote: the best sample per metric by the mean over the
//                             predicted steps, and the clip's contribution to the per-step curves (the rule in plain Python:
//                             prediction_quality_reference).
// No atomics, fixed summation orders: the same inputs give the same bits.
#include <math.h>
#include "lvt_common.h"

#define FQ_WIN 11
#define FQ_HALO (FQ_WIN - 1)
#define FQ_TH 16                        // map rows per tile
#define FQ_TW 32                        // map columns per tile: one half-wave reads one row of the intermediate (conflict-free)
#define FQ_IH (FQ_TH + FQ_HALO)         // 26 input rows
#define FQ_IW (FQ_TW + FQ_HALO)         // 42 input columns
#define FQ_THREADS 256
// LDS per workgroup: 2 x 26 x 42 x 4 (input tiles) + 5 x 26 x 32 x 4 (horizontal pass) + 32 = 25408 bytes: six workgroups per CU
static_assert(2 * FQ_IH * FQ_IW * 4 + 5 * FQ_IH * FQ_TW * 4 + 32 <= 80 * 1024, "two workgroups per CU must fit the 160 KiB LDS");

struct FqWindow { float w[FQ_WIN]; };   // the normalised Gaussian, rounded from fp64 once on the host

// sum of the workgroup's 256 fp64 values in a fixed tree (xor butterfly inside each wave, the four wave sums in wave order);
// every thread gets the result.  `scratch`: 4 doubles, reusable after the next barrier.
__device__ __forceinline__ double fq_block_sum(double v, double *scratch) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

__global__ __launch_bounds__(FQ_THREADS) void lvt_frame_quality_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                                       int C, int Fb, int H, int W, int tiles_x, int tiles,
                                                                       const FqWindow win, double c1, double c2,
                                                                       double *__restrict__ partials) {
    __shared__ float sa[FQ_IH][FQ_IW], sb[FQ_IH][FQ_IW];
    __shared__ float mid[5][FQ_IH][FQ_TW];
    __shared__ double scratch[4];
    const int tid = threadIdx.x;
    const long long plane = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(plane * tiles);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * FQ_TH, x0 = tx * FQ_TW;
    const int OH = H - FQ_HALO, OW = W - FQ_HALO;
    const int th = min(FQ_TH, OH - y0), tw = min(FQ_TW, OW - x0);          // map positions of this tile (>= 1)
    // the input pixels whose squared difference this tile counts: its own FQ_TH x FQ_TW block, and the last tile of a row /
    // column also takes the 10 rows / columns behind its map positions -- every pixel of the plane belongs to exactly one tile
    const int own_h = y0 + FQ_TH >= OH ? H - y0 : FQ_TH, own_w = x0 + FQ_TW >= OW ? W - x0 : FQ_TW;
    // frame f of a against frame f % Fb of b (Fb == F: plane against plane)
    const long long fa = plane / C;
    const long long plane_b = (fa % Fb) * C + (plane - fa * C);
    const float *pa = a + plane * H * W, *pb = b + plane_b * H * W;
    const float piv_a = pa[(long long)y0 * W + x0], piv_b = pb[(long long)y0 * W + x0];

    double se = 0.0;
    for (int i = tid; i < FQ_IH * FQ_IW; i += FQ_THREADS) {
        const int r = i / FQ_IW, c = i - r * FQ_IW;
        const int gy = y0 + r, gx = x0 + c;
        float va = piv_a, vb = piv_b;                                      // outside the plane: 0 after the shift, never used
        if (gy < H && gx < W) {
            va = pa[(long long)gy * W + gx];
            vb = pb[(long long)gy * W + gx];
            if (r < own_h && c < own_w) {
                const double d = (double)va - (double)vb;
                se += d * d;
            }
        }
        sa[r][c] = va - piv_a;
        sb[r][c] = vb - piv_b;
    }
    __syncthreads();

    // horizontal pass: a half-wave takes the 32 columns of one row, lane j reads columns j .. j + 10.  The three second moments are
    // formed by the same operations, so that equal planes give equal bits (and an SSIM of exactly 1).
    for (int i = tid; i < FQ_IH * FQ_TW; i += FQ_THREADS) {
        const int r = i / FQ_TW, j = i - r * FQ_TW;
        float hx = 0.f, hy = 0.f, hxx = 0.f, hyy = 0.f, hxy = 0.f;
#pragma unroll
        for (int k = 0; k < FQ_WIN; ++k) {
            const float x = sa[r][j + k], y = sb[r][j + k];
            const float wx = __fmul_rn(win.w[k], x), wy = __fmul_rn(win.w[k], y);
            hx = __fadd_rn(hx, wx);
            hy = __fadd_rn(hy, wy);
            hxx = __fmaf_rn(wx, x, hxx);
            hyy = __fmaf_rn(wy, y, hyy);
            hxy = __fmaf_rn(wx, y, hxy);
        }
        mid[0][r][j] = hx; mid[1][r][j] = hy; mid[2][r][j] = hxx; mid[3][r][j] = hyy; mid[4][r][j] = hxy;
    }
    __syncthreads();

    // vertical pass and the ratio.  From here on fp64: the products of two fp32 values are exact there, so the expressions below
    // do not depend on whether the compiler contracts them.
    double ss = 0.0;
    for (int i = tid; i < FQ_TH * FQ_TW; i += FQ_THREADS) {
        const int r = i / FQ_TW, j = i - r * FQ_TW;
        if (r < th && j < tw) {
            float v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < FQ_WIN; ++k) s = __fmaf_rn(win.w[k], mid[q][r + k][j], s);
                v[q] = s;
            }
            const double mx = v[0], my = v[1];
            const double sxx = (double)v[2] - mx * mx, syy = (double)v[3] - my * my, sxy = (double)v[4] - mx * my;
            const double ux = (double)piv_a + mx, uy = (double)piv_b + my;
            const double num = (2.0 * (ux * uy) + c1) * (2.0 * sxy + c2);
            const double den = (ux * ux + uy * uy + c1) * (sxx + syy + c2);
            ss += num / den;
        }
    }
    ss = fq_block_sum(ss, scratch);
    se = fq_block_sum(se, scratch);
    if (tid == 0) *reinterpret_cast<double2 *>(partials + 2 * (long long)blockIdx.x) = make_double2(ss, se);
}

// frames[f] = {psnr, ssim}; acc += {sum of finite psnr, sum ssim, frames with mse != 0, frames}.  Wave w takes frames w, w + 4, ..;
// its lanes add the frame's partials strided by 64, then the butterfly.  The accumulator sums go over the frames in a fixed
// order too (thread t: frames t, t + 256, ..; then the tree).
__global__ __launch_bounds__(FQ_THREADS) void lvt_frame_quality_finish_kernel(const double *__restrict__ partials, int F,
                                                                              long long per_frame, double n_map, double n_pix,
                                                                              double range2, double *__restrict__ frames,
                                                                              double *__restrict__ acc) {
    __shared__ double scratch[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int f = wave; f < F; f += FQ_THREADS / 64) {
        const double *p = partials + 2 * per_frame * f;
        double ss = 0.0, se = 0.0;
        for (long long i = lane; i < per_frame; i += 64) {
            const double2 v = *reinterpret_cast<const double2 *>(p + 2 * i);
            ss += v.x;
            se += v.y;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            ss += __shfl_xor(ss, d, 64);
            se += __shfl_xor(se, d, 64);
        }
        if (lane == 0) {
            const double mse = se / n_pix;
            frames[2 * f] = mse == 0.0 ? (double)__builtin_inff() : 10.0 * log10(range2 / mse);
            frames[2 * f + 1] = ss / n_map;
        }
    }
    __syncthreads();                        // frames[] of this workgroup's own stores
    double ps = 0.0, sm = 0.0, fin = 0.0;
    for (int f = threadIdx.x; f < F; f += FQ_THREADS) {
        const double psnr = frames[2 * f];
        if (psnr != (double)__builtin_inff()) {
            ps += psnr;
            fin += 1.0;
        }
        sm += frames[2 * f + 1];
    }
    ps = fq_block_sum(ps, scratch);
    sm = fq_block_sum(sm, scratch);
    fin = fq_block_sum(fin, scratch);
    if (threadIdx.x == 0) {
        acc[0] += ps;
        acc[1] += sm;
        acc[2] += fin;
        acc[3] += (double)F;
    }
}

static inline bool fq_range_ok(double r) { return r > 0.0 && r < (double)__builtin_inff(); }        // (false for NaN)

extern "C" long long lvt_frame_quality_partials(int C, int H, int W) {
    if (C <= 0 || H < FQ_WIN || W < FQ_WIN) return -1;
    return (long long)C * lvt_cdiv(H - FQ_HALO, FQ_TH) * lvt_cdiv(W - FQ_HALO, FQ_TW);
}

static int fq_launch(const char *who, const float *a, const float *b, int F, int Fb, int C, int H, int W, double data_range,
                     double *partials, long long n_partials, void *stream) {
    LVT_REQUIRE(a && b && partials, "%s: null pointer", who);
    LVT_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3) == 0 && lvt_aligned16(partials), "%s: misaligned pointer", who);
    LVT_REQUIRE(F > 0 && C > 0, "%s: F=%d frames of C=%d channels", who, F, C);
    LVT_REQUIRE(Fb > 0 && F % Fb == 0, "%s: F=%d frames against Fb=%d, F must be a multiple of Fb >= 1", who, F, Fb);
    LVT_REQUIRE(H >= FQ_WIN && W >= FQ_WIN, "%s: H=%d W=%d, the 11x11 window needs H and W >= 11", who, H, W);
    LVT_REQUIRE(fq_range_ok(data_range), "%s: data_range must be positive and finite", who);
    const long long need = lvt_frame_quality_partials(C, H, W);
    LVT_REQUIRE(need == n_partials, "%s: %lld partials per frame for a shape that needs %lld", who, n_partials, need);
    LVT_REQUIRE((long long)F * need < (1ll << 31), "%s: too many tiles in one launch", who);
    // the window: exp(-(k - 5)^2 / (2 sigma^2)), sigma 1.5, normalised in fp64, rounded once
    FqWindow win;
    double g[FQ_WIN], sum = 0.0;
    for (int k = 0; k < FQ_WIN; ++k) sum += g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < FQ_WIN; ++k) win.w[k] = (float)(g[k] / sum);
    const int tiles_x = (int)lvt_cdiv(W - FQ_HALO, FQ_TW), tiles = tiles_x * (int)lvt_cdiv(H - FQ_HALO, FQ_TH);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    hipLaunchKernelGGL(lvt_frame_quality_kernel, dim3((unsigned)(F * need)), dim3(FQ_THREADS), 0, (hipStream_t)stream, a, b, C, Fb,
                       H, W, tiles_x, tiles, win, c1, c2, partials);
    LVT_CHECK_LAUNCH("lvt_frame_quality_kernel");
    return LVT_OK;
}

extern "C" int lvt_frame_quality(const float *a, const float *b, int F, int C, int H, int W, double data_range, double *partials,
                                 long long n_partials, void *stream) {
    return fq_launch("frame_quality", a, b, F, F, C, H, W, data_range, partials, n_partials, stream);
}

extern "C" int lvt_frame_quality_vs(const float *a, const float *b, int F, int Fb, int C, int H, int W, double data_range,
                                    double *partials, long long n_partials, void *stream) {
    return fq_launch("frame_quality_vs", a, b, F, Fb, C, H, W, data_range, partials, n_partials, stream);
}

extern "C" int lvt_frame_quality_finish(const double *partials, int F, int C, int H, int W, double data_range,
                                        long long n_partials, double *frames, double *acc, void *stream) {
    LVT_REQUIRE(partials && frames && acc, "frame_quality_finish: null pointer");
    LVT_REQUIRE(lvt_aligned16(partials) && (((uintptr_t)frames | (uintptr_t)acc) & 7) == 0,
                "frame_quality_finish: misaligned pointer");
    LVT_REQUIRE(F > 0 && C > 0, "frame_quality_finish: F=%d frames of C=%d channels", F, C);
    LVT_REQUIRE(H >= FQ_WIN && W >= FQ_WIN, "frame_quality_finish: H=%d W=%d, the 11x11 window needs H and W >= 11", H, W);
    LVT_REQUIRE(fq_range_ok(data_range), "frame_quality_finish: data_range must be positive and finite");
    const long long need = lvt_frame_quality_partials(C, H, W);
    LVT_REQUIRE(need == n_partials, "frame_quality_finish: %lld partials per frame for a shape that needs %lld", n_partials, need);
    hipLaunchKernelGGL(lvt_frame_quality_finish_kernel, dim3(1), dim3(FQ_THREADS), 0, (hipStream_t)stream, partials, F, need,
                       (double)C * (H - FQ_HALO) * (W - FQ_HALO), (double)C * H * W, data_range * data_range, frames, acc);
    LVT_CHECK_LAUNCH("lvt_frame_quality_finish_kernel");
    return LVT_OK;
}

// ---- best-of-N selection over the (S, T) table of {psnr, ssim} pairs (PredictionQualityEvaluator) -------------------
// A candidate for the best sample: its score and its index.  `a` goes before `b` when its score is larger, when b's score is NaN
// and a's is not, or when neither decides and a has the lower index: a total order, so the reduction below finds the same sample in
// whatever order it meets them -- the largest score, the lowest index among equals, and sample 0 when every score is NaN.
struct FqCand { double v; int s; };

__device__ __forceinline__ bool fq_before(const FqCand &a, const FqCand &b) {
    if (a.v > b.v) return true;
    if (b.v > a.v) return false;
    const bool na = a.v != a.v, nb = b.v != b.v;
    if (na != nb) return nb;
    return a.s < b.s;
}

// the first of the workgroup's 256 candidates in that order; every thread gets it.  `slots`: 4 candidates.
__device__ __forceinline__ FqCand fq_block_best(FqCand c, FqCand *slots) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        FqCand o;
        o.v = __shfl_xor(c.v, d, 64);
        o.s = __shfl_xor(c.s, d, 64);
        if (fq_before(o, c)) c = o;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = c;
    __syncthreads();
    FqCand r = slots[0];
#pragma unroll
    for (int w = 1; w < FQ_THREADS / 64; ++w)
        if (fq_before(slots[w], r)) r = slots[w];
    return r;
}

__device__ __forceinline__ bool fq_finite(double v) { return v - v == 0.0; }         // (false for +-inf and NaN)

// Thread i scores samples i, i + 256, ..: the plain fp64 sum of the sample's values over t = n_prime .. T-1 in ascending t, divided
// by T - n_prime (a +inf psnr takes part).  After the two reductions thread j takes the steps n_prime + j, n_prime + j + 256, ..
// and adds that step's row of eight values to `curves`, with the sums over the samples in ascending s.
__global__ __launch_bounds__(FQ_THREADS) void lvt_prediction_select_kernel(const double *__restrict__ frames, int S, int T,
                                                                           int n_prime, double *__restrict__ curves,
                                                                           int *__restrict__ best) {
    __shared__ FqCand slots[4];
    const double steps = (double)(T - n_prime);
    FqCand bp, bs;
    bp.v = bs.v = (double)__builtin_nanf("");
    bp.s = bs.s = 0x7fffffff;                               // a thread without a sample: behind every real candidate
    for (int s = threadIdx.x; s < S; s += FQ_THREADS) {
        const double *row = frames + 2 * (long long)s * T;
        double p = 0.0, q = 0.0;
        for (int t = n_prime; t < T; ++t) {
            p += row[2 * t];
            q += row[2 * t + 1];
        }
        FqCand cp, cs;
        cp.v = p / steps; cp.s = s;
        cs.v = q / steps; cs.s = s;
        if (fq_before(cp, bp)) bp = cp;
        if (fq_before(cs, bs)) bs = cs;
    }
    bp = fq_block_best(bp, slots);
    bs = fq_block_best(bs, slots);
    if (threadIdx.x == 0) {
        best[0] = bp.s;
        best[1] = bs.s;
    }
    for (int t = n_prime + threadIdx.x; t < T; t += FQ_THREADS) {
        double ps = 0.0, pn = 0.0, sm = 0.0;
        for (int s = 0; s < S; ++s) {
            const double *v = frames + 2 * ((long long)s * T + t);
            if (fq_finite(v[0])) {
                ps += v[0];
                pn += 1.0;
            }
            sm += v[1];
        }
        const double pb = frames[2 * ((long long)bp.s * T + t)];
        double *c = curves + 8 * (long long)t;
        if (fq_finite(pb)) {
            c[0] += pb;
            c[1] += 1.0;
        }
        c[2] += frames[2 * ((long long)bs.s * T + t) + 1];
        c[3] += ps;
        c[4] += pn;
        c[5] += sm;
        c[6] += 1.0;
        c[7] += (double)S;
    }
}

extern "C" int lvt_prediction_select(const double *frames, int S, int T, int n_prime, double *curves, int *best, void *stream) {
    LVT_REQUIRE(frames && curves && best, "prediction_select: null pointer");
    LVT_REQUIRE((((uintptr_t)frames | (uintptr_t)curves) & 7) == 0 && ((uintptr_t)best & 3) == 0,
                "prediction_select: misaligned pointer");
    LVT_REQUIRE(S >= 1 && T >= 1, "prediction_select: S=%d sampled videos of T=%d frames", S, T);
    LVT_REQUIRE(n_prime >= 0 && n_prime < T, "prediction_select: n_prime=%d outside [0, T=%d)", n_prime, T);
    hipLaunchKernelGGL(lvt_prediction_select_kernel, dim3(1), dim3(FQ_THREADS), 0, (hipStream_t)stream, frames, S, T, n_prime,
                       curves, best);
    LVT_CHECK_LAUNCH("lvt_prediction_select_kernel");
    return LVT_OK;
}
