// SSIM term of the reconstruction loss (LOSS.SSIM.LAMBDA; the rule in plain torch:
// lvt_amd/evaluation/quality.py ssim_loss_reference):
//     loss = lam * (1 - mean over frames, real channels and map positions of SSIM(u(xt), u(x))),   u = v * std[c] + mean[c]
// on the channels-last activations (N, 1, H, W, Cp) of the conv stacks, and its gradient w.r.t. xt.  SSIM is the rule of
// quality.hip (11x11 Gaussian window of sigma 1.5, no padding, biased weighted moments).  Two launches:
//   lvt_ssim_loss_fwd     one workgroup per (frame, channel quad, SL_T x SL_T tile of PIXELS).  The tile's map positions are those
//                         with the same coordinates as its pixels; the gradient of a pixel p collects the map positions p - 10 .. p,
//                         so with a gradient buffer the workgroup evaluates the map on the tile plus a 10-position halo before it
//                         (SL_M = 26 per side) from an input tile of SL_I = 36 per side, and recomputes what its neighbours compute
//                         too: nothing is exchanged through global memory.  Both planes are denormalised and staged in LDS minus a
//                         per-tile pivot of their own (the tile's first pixel; quality.hip says why), one plane of floats per
//                         channel of the quad.  Per channel: horizontal 11-tap pass of (x, y, x^2, y^2, xy) -> LDS, vertical pass ->
//                         registers, SSIM and the three coefficient maps in fp64, then the two transposed 11-tap passes in fp32.
//                         Without a gradient buffer only the tile's own map positions are evaluated (same operations on them: same
//                         loss bits).  -> one fp64 partial per workgroup (sum of the SSIM map over the tile), a plain store.
//   lvt_ssim_loss_finish  one workgroup adds the partials in a fixed order -> out[0] = lam * (1 - sum / n) in fp32.
// The gradient.  With x' = u(xt) - piv_x, y' = u(x) - piv_y, the windowed means mx', my' of those, ux = piv_x + mx', uy = piv_y + my',
//   A1 = 2 ux uy + C1, B1 = ux^2 + uy^2 + C1, A2 = 2 sxy + C2, B2 = sxx + syy + C2, lum = A1 / B1, con = A2 / B2, S = lum con
//   dm    = dS/dmx          = 2 con (uy - ux lum) / B1
//   gamma = dS/dsxy         = 2 lum / B2
//   bsum  = 2 dS/dsxx + gamma = 2 lum (1 - con) / B2
//   a     = dm - bsum mx' - gamma (my' - mx')
//   dS_total/du_x(p) = (W^T a)(p) + x'(p) (W^T bsum)(p) + (y'(p) - x'(p)) (W^T gamma)(p)
// which is the closed form of the rule regrouped about the pivots and about x = y: for equal planes lum = con = 1 and a, bsum and
// the difference are exact zeros (SSIM exactly 1, loss and gradient exactly 0), and for nearly equal ones nothing large cancels.
// No atomics, fixed summation orders: the same inputs give the same bits.
#include <math.h>
#include "lvt_common.h"

#define SL_WIN 11
#define SL_HALO (SL_WIN - 1)
#define SL_T 16                         // pixels per tile side
#define SL_M (SL_T + SL_HALO)           // 26 map positions per side: local m <-> global map coordinate p0 - 10 + m
#define SL_I (SL_M + SL_HALO)           // 36 input pixels per side:  local i <-> global pixel coordinate p0 - 10 + i
#define SL_THREADS 256
#define SL_MID (5 * SL_I * SL_M)        // floats of the horizontal pass; the coefficient maps (3 x 26 x 26) and the transposed
#define SL_COEF (3 * SL_M * SL_M)       // vertical pass (3 x 16 x 26) live in the same floats once the vertical pass has read them
#define SL_PER_THREAD ((SL_M * SL_M + SL_THREADS - 1) / SL_THREADS)        // 3 map positions per thread
// LDS per workgroup: 2 x 4 x 36 x 36 x 4 (input tiles) + 5 x 36 x 26 x 4 (passes) + 32 = 60224 bytes: two workgroups per CU
static_assert(SL_COEF + 3 * SL_T * SL_M <= SL_MID, "coefficient maps and transposed pass fit the horizontal pass's floats");
static_assert(2 * 4 * SL_I * SL_I * 4 + SL_MID * 4 + 32 <= 64 * 1024, "static LDS of one workgroup, two per CU in 160 KiB");
static_assert(SL_T * SL_T == SL_THREADS, "one thread per pixel of the tile");

struct SlWindow { float w[SL_WIN]; };   // the normalised Gaussian, rounded from fp64 once on the host

__device__ __forceinline__ double sl_block_sum(double v, double *scratch) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

template <int BWD>
__global__ __launch_bounds__(SL_THREADS) void lvt_ssim_loss_kernel(const float *__restrict__ xt, const float *__restrict__ x, int H,
                                                                   int W, int Cp, int C, const float *__restrict__ mean,
                                                                   const float *__restrict__ stdv, int tiles_x, int tiles,
                                                                   const SlWindow win, double c1, double c2, double gscale,
                                                                   double *__restrict__ partials, float *__restrict__ G) {
    __shared__ float sa[4][SL_I][SL_I], sb[4][SL_I][SL_I];
    __shared__ float work[SL_MID];
    __shared__ double scratch[4];
    float (*mid)[SL_I][SL_M] = reinterpret_cast<float (*)[SL_I][SL_M]>(work);
    float (*coef)[SL_M][SL_M] = reinterpret_cast<float (*)[SL_M][SL_M]>(work);
    float (*tv)[SL_T][SL_M] = reinterpret_cast<float (*)[SL_T][SL_M]>(work + SL_COEF);
    const int tid = threadIdx.x;
    const int quads = Cp >> 2;
    const int tile = blockIdx.x % tiles;
    const int fq = blockIdx.x / tiles;
    const int quad = fq % quads;
    const long long f = fq / quads;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int py0 = ty * SL_T, px0 = tx * SL_T;                            // the tile's first pixel (inside the plane)
    const int OH = H - SL_HALO, OW = W - SL_HALO;
    const int lo = BWD ? 0 : SL_HALO;                                      // first local map / input index that is needed
    const float *pa = xt + f * H * W * Cp + 4 * quad, *pb = x + f * H * W * Cp + 4 * quad;

    float m4[4], s4[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const int c = 4 * quad + ch;
        m4[ch] = c < C ? mean[c] : 0.f;
        s4[ch] = c < C ? stdv[c] : 0.f;
    }
    float piv_a[4], piv_b[4];
    {
        const long long o = ((long long)py0 * W + px0) * Cp;
        const float4 va = *reinterpret_cast<const float4 *>(pa + o), vb = *reinterpret_cast<const float4 *>(pb + o);
        piv_a[0] = __fmaf_rn(va.x, s4[0], m4[0]); piv_a[1] = __fmaf_rn(va.y, s4[1], m4[1]);
        piv_a[2] = __fmaf_rn(va.z, s4[2], m4[2]); piv_a[3] = __fmaf_rn(va.w, s4[3], m4[3]);
        piv_b[0] = __fmaf_rn(vb.x, s4[0], m4[0]); piv_b[1] = __fmaf_rn(vb.y, s4[1], m4[1]);
        piv_b[2] = __fmaf_rn(vb.z, s4[2], m4[2]); piv_b[3] = __fmaf_rn(vb.w, s4[3], m4[3]);
    }
    // stage: 16-byte pixel loads, one LDS plane per channel.  Outside the plane: 0 after the shift, read only by map positions
    // that do not exist.
    const int side = SL_I - lo;
    for (int i = tid; i < side * side; i += SL_THREADS) {
        const int r = lo + i / side, c = lo + i % side;
        const int gy = py0 - SL_HALO + r, gx = px0 - SL_HALO + c;
        float4 ua = make_float4(0.f, 0.f, 0.f, 0.f), ub = ua;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long long o = ((long long)gy * W + gx) * Cp;
            const float4 va = *reinterpret_cast<const float4 *>(pa + o), vb = *reinterpret_cast<const float4 *>(pb + o);
            ua.x = __fsub_rn(__fmaf_rn(va.x, s4[0], m4[0]), piv_a[0]); ub.x = __fsub_rn(__fmaf_rn(vb.x, s4[0], m4[0]), piv_b[0]);
            ua.y = __fsub_rn(__fmaf_rn(va.y, s4[1], m4[1]), piv_a[1]); ub.y = __fsub_rn(__fmaf_rn(vb.y, s4[1], m4[1]), piv_b[1]);
            ua.z = __fsub_rn(__fmaf_rn(va.z, s4[2], m4[2]), piv_a[2]); ub.z = __fsub_rn(__fmaf_rn(vb.z, s4[2], m4[2]), piv_b[2]);
            ua.w = __fsub_rn(__fmaf_rn(va.w, s4[3], m4[3]), piv_a[3]); ub.w = __fsub_rn(__fmaf_rn(vb.w, s4[3], m4[3]), piv_b[3]);
        }
        sa[0][r][c] = ua.x; sa[1][r][c] = ua.y; sa[2][r][c] = ua.z; sa[3][r][c] = ua.w;
        sb[0][r][c] = ub.x; sb[1][r][c] = ub.y; sb[2][r][c] = ub.z; sb[3][r][c] = ub.w;
    }
    __syncthreads();

    double ss = 0.0;
    float gout[4] = {0.f, 0.f, 0.f, 0.f};
    const int mside = SL_M - lo;
    for (int ch = 0; ch < 4; ++ch) {
        if (4 * quad + ch >= C) break;                                     // pad channels: no SSIM, gradient exactly 0 (uniform branch)
        // horizontal pass.  The three second moments are formed by the same operations: equal planes give equal bits.
        for (int i = tid; i < side * mside; i += SL_THREADS) {
            const int r = lo + i / mside, j = lo + i % mside;
            float hx = 0.f, hy = 0.f, hxx = 0.f, hyy = 0.f, hxy = 0.f;
#pragma unroll
            for (int k = 0; k < SL_WIN; ++k) {
                const float a = sa[ch][r][j + k], b = sb[ch][r][j + k];
                const float wa = __fmul_rn(win.w[k], a), wb = __fmul_rn(win.w[k], b);
                hx = __fadd_rn(hx, wa);
                hy = __fadd_rn(hy, wb);
                hxx = __fmaf_rn(wa, a, hxx);
                hyy = __fmaf_rn(wb, b, hyy);
                hxy = __fmaf_rn(wa, b, hxy);
            }
            mid[0][r][j] = hx; mid[1][r][j] = hy; mid[2][r][j] = hxx; mid[3][r][j] = hyy; mid[4][r][j] = hxy;
        }
        __syncthreads();

        // vertical pass, the ratio and the coefficient maps (fp64: products of two fp32 values are exact there)
        float ca[SL_PER_THREAD], cb[SL_PER_THREAD], cg[SL_PER_THREAD];
#pragma unroll
        for (int t = 0; t < SL_PER_THREAD; ++t) {
            ca[t] = cb[t] = cg[t] = 0.f;
            const int i = tid + t * SL_THREADS;
            if (i < mside * mside) {
                const int r = lo + i / mside, j = lo + i % mside;
                const int qy = py0 - SL_HALO + r, qx = px0 - SL_HALO + j; // global map position
                if (qy >= 0 && qy < OH && qx >= 0 && qx < OW) {
                    float v[5];
#pragma unroll
                    for (int q = 0; q < 5; ++q) {
                        float s = 0.f;
#pragma unroll
                        for (int k = 0; k < SL_WIN; ++k) s = __fmaf_rn(win.w[k], mid[q][r + k][j], s);
                        v[q] = s;
                    }
                    const double mx = v[0], my = v[1];
                    const double sxx = (double)v[2] - mx * mx, syy = (double)v[3] - my * my, sxy = (double)v[4] - mx * my;
                    const double ux = (double)piv_a[ch] + mx, uy = (double)piv_b[ch] + my;
                    const double a1 = 2.0 * (ux * uy) + c1, b1 = ux * ux + uy * uy + c1;
                    const double a2 = 2.0 * sxy + c2, b2 = sxx + syy + c2;
                    const double lum = a1 / b1, con = a2 / b2;
                    if (r >= SL_HALO && j >= SL_HALO) ss += lum * con;    // the tile's own map positions
                    if (BWD) {
                        const double dm = 2.0 * con * (uy - ux * lum) / b1;
                        const double gamma = 2.0 * lum / b2;
                        const double bsum = gamma * (1.0 - con);
                        ca[t] = (float)(dm - bsum * mx - gamma * (my - mx));
                        cb[t] = (float)bsum;
                        cg[t] = (float)gamma;
                    }
                }
            }
        }
        if (BWD) {
            __syncthreads();                                               // every read of the horizontal pass is done
#pragma unroll
            for (int t = 0; t < SL_PER_THREAD; ++t) {
                const int i = tid + t * SL_THREADS;
                if (i < SL_M * SL_M) {
                    const int r = i / SL_M, j = i % SL_M;
                    coef[0][r][j] = ca[t]; coef[1][r][j] = cb[t]; coef[2][r][j] = cg[t];
                }
            }
            __syncthreads();
            // transposed vertical pass: pixel row t of the tile collects map rows t + 10 - k (local), k = 0 .. 10
            for (int i = tid; i < SL_T * SL_M; i += SL_THREADS) {
                const int t = i / SL_M, j = i % SL_M;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int k = 0; k < SL_WIN; ++k) {
                    s0 = __fmaf_rn(win.w[k], coef[0][t + SL_HALO - k][j], s0);
                    s1 = __fmaf_rn(win.w[k], coef[1][t + SL_HALO - k][j], s1);
                    s2 = __fmaf_rn(win.w[k], coef[2][t + SL_HALO - k][j], s2);
                }
                tv[0][t][j] = s0; tv[1][t][j] = s1; tv[2][t][j] = s2;
            }
            __syncthreads();
            // transposed horizontal pass and the pixel's own values: one thread per pixel of the tile
            {
                const int t = tid / SL_T, j = tid % SL_T;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int k = 0; k < SL_WIN; ++k) {
                    s0 = __fmaf_rn(win.w[k], tv[0][t][j + SL_HALO - k], s0);
                    s1 = __fmaf_rn(win.w[k], tv[1][t][j + SL_HALO - k], s1);
                    s2 = __fmaf_rn(win.w[k], tv[2][t][j + SL_HALO - k], s2);
                }
                const float a = sa[ch][t + SL_HALO][j + SL_HALO], b = sb[ch][t + SL_HALO][j + SL_HALO];
                const float g = __fmaf_rn(__fsub_rn(b, a), s2, __fmaf_rn(a, s1, s0));
                gout[ch] = g * (float)(gscale * (double)s4[ch]);
            }
        }
        __syncthreads();                                                   // before the next channel's horizontal pass
    }
    if (BWD) {
        const int gy = py0 + tid / SL_T, gx = px0 + tid % SL_T;
        if (gy < H && gx < W)
            *reinterpret_cast<float4 *>(G + f * H * W * Cp + ((long long)gy * W + gx) * Cp + 4 * quad) =
                make_float4(gout[0], gout[1], gout[2], gout[3]);
    }
    ss = sl_block_sum(ss, scratch);
    if (tid == 0) partials[blockIdx.x] = ss;
}

// out[0] = lam * (1 - sum / n): thread t adds partials t, t + 256, .., then the fixed tree
__global__ __launch_bounds__(SL_THREADS) void lvt_ssim_loss_finish_kernel(const double *__restrict__ partials, long long count,
                                                                          double n, double lam, float *__restrict__ out) {
    __shared__ double scratch[4];
    double s = 0.0;
    for (long long i = threadIdx.x; i < count; i += SL_THREADS) s += partials[i];
    s = sl_block_sum(s, scratch);
    if (threadIdx.x == 0) out[0] = (float)(lam * (1.0 - s / n));
}

static inline bool sl_finite_pos(double r) { return r > 0.0 && r < (double)__builtin_inff(); }        // (false for NaN)

extern "C" long long lvt_ssim_loss_partials(int N, int H, int W, int Cp) {
    if (N <= 0 || H < SL_WIN || W < SL_WIN || Cp <= 0 || (Cp & 3)) return -1;
    return (long long)N * (Cp >> 2) * lvt_cdiv(H, SL_T) * lvt_cdiv(W, SL_T);
}

extern "C" int lvt_ssim_loss_fwd(const float *xt, const float *x, int N, int H, int W, int Cp, int C, const float *mean,
                                 const float *stdv, double data_range, double lam, double *partials, long long n_partials,
                                 float *G, void *stream) {
    LVT_REQUIRE(xt && x && mean && stdv && partials, "ssim_loss_fwd: null pointer");
    LVT_REQUIRE(lvt_aligned16(xt) && lvt_aligned16(x) && (!G || lvt_aligned16(G)) && (((uintptr_t)partials) & 7) == 0,
                "ssim_loss_fwd: misaligned pointer");
    LVT_REQUIRE(N > 0 && C > 0 && Cp == (C + 3) / 4 * 4, "ssim_loss_fwd: N=%d frames of C=%d channels padded to Cp=%d", N, C, Cp);
    LVT_REQUIRE(H >= SL_WIN && W >= SL_WIN, "ssim_loss_fwd: H=%d W=%d, the 11x11 window needs H and W >= 11", H, W);
    LVT_REQUIRE(sl_finite_pos(data_range), "ssim_loss_fwd: data_range must be positive and finite");
    LVT_REQUIRE(lam >= 0.0 && lam < (double)__builtin_inff(), "ssim_loss_fwd: lam must be non-negative and finite");
    const long long need = lvt_ssim_loss_partials(N, H, W, Cp);
    LVT_REQUIRE(need == n_partials, "ssim_loss_fwd: %lld partials for a shape that needs %lld", n_partials, need);
    LVT_REQUIRE(need < (1ll << 31), "ssim_loss_fwd: too many tiles in one launch");
    SlWindow win;
    double g[SL_WIN], sum = 0.0;
    for (int k = 0; k < SL_WIN; ++k) sum += g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < SL_WIN; ++k) win.w[k] = (float)(g[k] / sum);
    const int tiles_x = (int)lvt_cdiv(W, SL_T), tiles = tiles_x * (int)lvt_cdiv(H, SL_T);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    const double n = (double)N * C * (H - SL_HALO) * (W - SL_HALO);
    if (G)
        hipLaunchKernelGGL(lvt_ssim_loss_kernel<1>, dim3((unsigned)need), dim3(SL_THREADS), 0, (hipStream_t)stream, xt, x, H, W, Cp, C,
                           mean, stdv, tiles_x, tiles, win, c1, c2, -lam / n, partials, G);
    else
        hipLaunchKernelGGL(lvt_ssim_loss_kernel<0>, dim3((unsigned)need), dim3(SL_THREADS), 0, (hipStream_t)stream, xt, x, H, W, Cp, C,
                           mean, stdv, tiles_x, tiles, win, c1, c2, 0.0, partials, (float *)nullptr);
    LVT_CHECK_LAUNCH("lvt_ssim_loss_kernel");
    return LVT_OK;
}

extern "C" int lvt_ssim_loss_finish(const double *partials, long long n_partials, int N, int H, int W, int C, double lam, float *out,
                                    void *stream) {
    LVT_REQUIRE(partials && out, "ssim_loss_finish: null pointer");
    LVT_REQUIRE((((uintptr_t)partials) & 7) == 0 && (((uintptr_t)out) & 3) == 0, "ssim_loss_finish: misaligned pointer");
    LVT_REQUIRE(N > 0 && C > 0 && H >= SL_WIN && W >= SL_WIN, "ssim_loss_finish: N=%d C=%d H=%d W=%d", N, C, H, W);
    LVT_REQUIRE(lam >= 0.0 && lam < (double)__builtin_inff(), "ssim_loss_finish: lam must be non-negative and finite");
    LVT_REQUIRE(n_partials == lvt_ssim_loss_partials(N, H, W, (C + 3) / 4 * 4), "ssim_loss_finish: %lld partials for another shape",
                n_partials);
    hipLaunchKernelGGL(lvt_ssim_loss_finish_kernel, dim3(1), dim3(SL_THREADS), 0, (hipStream_t)stream, partials, n_partials,
                       (double)N * C * (H - SL_HALO) * (W - SL_HALO), lam, out);
    LVT_CHECK_LAUNCH("lvt_ssim_loss_finish_kernel");
    return LVT_OK;
}
