// Multi-tensor optimizer step: a handful of launches update every parameter of a sub-network.
// The reference builds one torch.optim param group per parameter (vidgen/solver/build.py:12-43), which
// turns an optimizer step into hundreds of tiny launches (394 tensors x ~6 kernels for DSFVT).  Here up to
// 64 tensors travel BY VALUE in the kernel arguments (no table upload, no host sync) and each workgroup
// updates one 16K-element chunk.  Math follows torch.optim.Adam / torch.optim.RMSprop (non-amsgrad,
// non-centered) operation by operation.  The *_scaled entries (ABI 680) run the same update on a clipped gradient; the global
// norm behind the clip coefficient comes from lvt_grad_sqnorm / lvt_grad_clip_coef below.
#include "lvt_common.h"
#include <math.h>
#include <type_traits>

typedef lvt_opt_entry LvtOptEntry;   // declared in lvt_hip.h; mirrored by ctypes in lvt_amd/hip/binding.py
#define OPT_CHUNK 16384
#define OPT_MAXT 64

struct OptArgs {
    int n;
    int chunk_prefix[OPT_MAXT + 1];
    LvtOptEntry e[OPT_MAXT];
};

__device__ __forceinline__ int find_tensor(const OptArgs &a, int blk) {
    int t = 0;
    while (t + 1 < a.n && a.chunk_prefix[t + 1] <= blk) ++t;
    return t;
}

// What a workgroup works on: tensor t of the launch's table, its entry e, and elements [lo, hi) of it (one chunk).
struct OptChunk {
    int t;
    LvtOptEntry e;
    long long lo, hi;
    __device__ __forceinline__ explicit OptChunk(const OptArgs &a) {
        t = find_tensor(a, blockIdx.x);
        e = a.e[t];
        lo = (long long)(blockIdx.x - a.chunk_prefix[t]) * OPT_CHUNK;
        hi = min(e.n, lo + OPT_CHUNK);
    }
};

// float4 lanes when the chunk of every stream of the tensor is 16-byte aligned and the tensor length is a multiple of 4
__device__ __forceinline__ bool opt_vec_ok(const LvtOptEntry &e, long long lo) {
    const uintptr_t a = (uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.s0 | (uintptr_t)(e.s1 ? e.s1 : e.s0);
    return (a & 15) == 0 && (e.n & 3) == 0 && (lo & 3) == 0;
}

// The gradient an update sees under clipping (ABI 680): g * coef, then the clamp.  The product is rounded on its own, as a
// gradient clipped in place is -- contracting it into the weight-decay sum behind it would round once instead of twice and
// break bit equality with the unscaled kernel at coef == 1.  The comparisons keep a NaN a NaN, as torch.clamp does.
__device__ __forceinline__ float clipped_grad(float g, float coef, float clamp) {
#pragma clang fp contract(off)
    g = g * coef;
    if (clamp > 0.f) g = g < -clamp ? -clamp : (g > clamp ? clamp : g);
    return g;
}

// Polyak averaging inside the step (lvt_*_step_ema): the table of a launch plus the shadow of every tensor, by value like the
// table itself.  The kernel-argument segment holds 4 KB; the widest EMA kernel adds nine 4- or 8-byte scalars behind this.
struct EmaArgs {
    OptArgs a;
    float *ema[OPT_MAXT];
};
static_assert(sizeof(EmaArgs) + 64 <= 4096, "EmaArgs and the scalars of the EMA kernels must fit the 4 KB of kernel arguments: "
                                            "carry fewer tensors per launch");

// e + w (p - e): the lerp_ form of torch.optim.swa_utils.get_ema_multi_avg_fn, w = 1 - decay
__device__ __forceinline__ float ema_follow(float e, float p, float w) { return e + w * (p - e); }
// Four elements of a shadow behind a float4 of new parameter values.  Which loop a tensor takes is decided by p, g, s0 and s1
// alone, as without averaging: the scalar and the float4 loop of a step do not round alike (the compiler contracts their
// multiply-adds differently), so a shadow that picked the loop would change the trajectory of p.  A shadow that is not
// 16-byte aligned (`vec` false) is read and written 4 bytes at a time instead.
__device__ __forceinline__ void ema_follow4(float *sh, const float4 &p, float w, bool vec) {
    if (vec) {
        float4 e = *reinterpret_cast<const float4 *>(sh);
        e.x = ema_follow(e.x, p.x, w); e.y = ema_follow(e.y, p.y, w);
        e.z = ema_follow(e.z, p.z, w); e.w = ema_follow(e.w, p.w, w);
        *reinterpret_cast<float4 *>(sh) = e;
        return;
    }
    const float e0 = sh[0], e1 = sh[1], e2 = sh[2], e3 = sh[3];
    sh[0] = ema_follow(e0, p.x, w); sh[1] = ema_follow(e1, p.y, w);
    sh[2] = ema_follow(e2, p.z, w); sh[3] = ema_follow(e3, p.w, w);
}

// The shadow behind the SCALAR loop of a step (tensors that are short, ragged or misaligned): a second sweep in which every
// thread revisits the elements it has just written.  The scalar loop itself stays free of the shadow so that it compiles to
// the instructions it has in the plain step -- with the shadow's arithmetic in its block the compiler contracts `upd`
// differently, and p would no longer come out bit for bit as without averaging.
__device__ __forceinline__ void ema_follow_scalar(float *sh, const float *p, long long lo, long long hi, float w) {
    for (long long i = lo + threadIdx.x; i < hi; i += 256) sh[i] = ema_follow(sh[i], p[i], w);
}

// SCALED = false is the body of lvt_adam_step as it always was (gscale and clamp are dead); SCALED = true: lvt_adam_step_scaled.
// EMA = true (lvt_adam_step_ema): the shadow ema[t] of every tensor follows the new parameter value while it is still in a
// register; EMA = false leaves `ema` and `w` dead, and the two instantiations without it are what they were.
template <bool SCALED, bool EMA>
__device__ __forceinline__ void adam_body(const OptArgs &a, float beta1, float beta2, float eps, float bc1, float bc2_sqrt,
                                          const lvt_clip_record *gscale, float clamp, float *const *ema, float w) {
    float coef = 1.f;
    if (SCALED && gscale) {
        if (gscale->skip) return;           // non-finite gradient norm: no store, p / s0 / s1 keep their bits
        coef = gscale->coef;
    }
    const OptChunk c(a);
    const LvtOptEntry &e = c.e;
    const float step = e.lr / bc1;
    auto upd = [&](float g, float p, float &m, float &v) -> float {
        if (SCALED) g = clipped_grad(g, coef, clamp);
        if (e.wd != 0.f) g += e.wd * p;
        m = m + (1.f - beta1) * (g - m);                                   // exp_avg.lerp_(grad, 1 - beta1)
        v = beta2 * v + (1.f - beta2) * g * g;                             // mul_(beta2).addcmul_(g, g, 1 - beta2)
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        return p - step * (m / denom);
    };
    float *const sh = EMA ? ema[c.t] : nullptr;
    const bool sh_vec = EMA && ((uintptr_t)sh & 15) == 0;
    if (opt_vec_ok(e, c.lo)) {              // 16-byte lanes: a wave instruction moves 1 KB instead of 256 B
        for (long long i = c.lo + 4 * threadIdx.x; i < c.hi; i += 1024) {
            const float4 g4 = *reinterpret_cast<const float4 *>(e.g + i), p4 = *reinterpret_cast<const float4 *>(e.p + i);
            float4 m4 = *reinterpret_cast<const float4 *>(e.s0 + i), v4 = *reinterpret_cast<const float4 *>(e.s1 + i), o;
            o.x = upd(g4.x, p4.x, m4.x, v4.x); o.y = upd(g4.y, p4.y, m4.y, v4.y);
            o.z = upd(g4.z, p4.z, m4.z, v4.z); o.w = upd(g4.w, p4.w, m4.w, v4.w);
            *reinterpret_cast<float4 *>(e.s0 + i) = m4; *reinterpret_cast<float4 *>(e.s1 + i) = v4;
            *reinterpret_cast<float4 *>(e.p + i) = o;
            if (EMA) ema_follow4(sh + i, o, w, sh_vec);
        }
        return;
    }
    for (long long i = c.lo + threadIdx.x; i < c.hi; i += 256) {
        float m = e.s0[i], v = e.s1[i];
        const float o = upd(e.g[i], e.p[i], m, v);
        e.p[i] = o;
        e.s0[i] = m; e.s1[i] = v;
    }
    if (EMA) ema_follow_scalar(sh, e.p, c.lo, c.hi, w);
}

__global__ __launch_bounds__(256) void lvt_adam_kernel(const OptArgs a, float beta1, float beta2, float eps,
                                                       float bc1, float bc2_sqrt) {
    adam_body<false, false>(a, beta1, beta2, eps, bc1, bc2_sqrt, nullptr, 0.f, nullptr, 0.f);
}

__global__ __launch_bounds__(256) void lvt_adam_scaled_kernel(const OptArgs a, float beta1, float beta2, float eps,
                                                              float bc1, float bc2_sqrt, const lvt_clip_record *gscale,
                                                              float clamp) {
    adam_body<true, false>(a, beta1, beta2, eps, bc1, bc2_sqrt, gscale, clamp, nullptr, 0.f);
}

// The EMA variants carry the table and the shadows in one by-value struct.  gscale == NULL and clamp == 0 launch the unscaled body.
template <bool SCALED>
__global__ __launch_bounds__(256) void lvt_adam_ema_kernel(const EmaArgs a, float beta1, float beta2, float eps, float bc1,
                                                           float bc2_sqrt, const lvt_clip_record *gscale, float clamp, float w) {
    adam_body<SCALED, true>(a.a, beta1, beta2, eps, bc1, bc2_sqrt, gscale, clamp, a.ema, w);
}

template <bool SCALED, bool EMA>
__device__ __forceinline__ void rmsprop_body(const OptArgs &a, float alpha, float eps, float momentum,
                                             const lvt_clip_record *gscale, float clamp, float *const *ema, float w) {
    float coef = 1.f;
    if (SCALED && gscale) {
        if (gscale->skip) return;
        coef = gscale->coef;
    }
    const OptChunk c(a);
    const LvtOptEntry &e = c.e;
    auto upd = [&](float g, float p, float &sq, float &buf) -> float {
        if (SCALED) g = clipped_grad(g, coef, clamp);
        if (e.wd != 0.f) g += e.wd * p;
        sq = alpha * sq + (1.f - alpha) * g * g;
        const float avg = sqrtf(sq) + eps;
        if (momentum > 0.f) { buf = momentum * buf + g / avg; return p - e.lr * buf; }
        return p - e.lr * (g / avg);
    };
    const bool mom = momentum > 0.f;
    float *const sh = EMA ? ema[c.t] : nullptr;
    const bool sh_vec = EMA && ((uintptr_t)sh & 15) == 0;
    if (opt_vec_ok(e, c.lo)) {
        for (long long i = c.lo + 4 * threadIdx.x; i < c.hi; i += 1024) {
            const float4 g4 = *reinterpret_cast<const float4 *>(e.g + i), p4 = *reinterpret_cast<const float4 *>(e.p + i);
            float4 s4 = *reinterpret_cast<const float4 *>(e.s0 + i), o;
            float4 b4 = mom ? *reinterpret_cast<const float4 *>(e.s1 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            o.x = upd(g4.x, p4.x, s4.x, b4.x); o.y = upd(g4.y, p4.y, s4.y, b4.y);
            o.z = upd(g4.z, p4.z, s4.z, b4.z); o.w = upd(g4.w, p4.w, s4.w, b4.w);
            *reinterpret_cast<float4 *>(e.s0 + i) = s4;
            if (mom) *reinterpret_cast<float4 *>(e.s1 + i) = b4;
            *reinterpret_cast<float4 *>(e.p + i) = o;
            if (EMA) ema_follow4(sh + i, o, w, sh_vec);
        }
        return;
    }
    for (long long i = c.lo + threadIdx.x; i < c.hi; i += 256) {
        float sq = e.s0[i], buf = mom ? e.s1[i] : 0.f;
        const float o = upd(e.g[i], e.p[i], sq, buf);
        e.p[i] = o;
        e.s0[i] = sq;
        if (mom) e.s1[i] = buf;
    }
    if (EMA) ema_follow_scalar(sh, e.p, c.lo, c.hi, w);
}

__global__ __launch_bounds__(256) void lvt_rmsprop_kernel(const OptArgs a, float alpha, float eps, float momentum) {
    rmsprop_body<false, false>(a, alpha, eps, momentum, nullptr, 0.f, nullptr, 0.f);
}

__global__ __launch_bounds__(256) void lvt_rmsprop_scaled_kernel(const OptArgs a, float alpha, float eps, float momentum,
                                                                 const lvt_clip_record *gscale, float clamp) {
    rmsprop_body<true, false>(a, alpha, eps, momentum, gscale, clamp, nullptr, 0.f);
}

template <bool SCALED>
__global__ __launch_bounds__(256) void lvt_rmsprop_ema_kernel(const EmaArgs a, float alpha, float eps, float momentum,
                                                              const lvt_clip_record *gscale, float clamp, float w) {
    rmsprop_body<SCALED, true>(a.a, alpha, eps, momentum, gscale, clamp, a.ema, w);
}

// Exchange of the contents of e.p and e.s0 (lvt_ema_swap): the chunking of the steps, float4 lanes when both sides allow.
__global__ __launch_bounds__(256) void lvt_ema_swap_kernel(const OptArgs a) {
    const OptChunk c(a);
    const LvtOptEntry &e = c.e;
    if ((((uintptr_t)e.p | (uintptr_t)e.s0) & 15) == 0 && (e.n & 3) == 0) {
        for (long long i = c.lo + 4 * threadIdx.x; i < c.hi; i += 1024) {
            const float4 x = *reinterpret_cast<const float4 *>(e.p + i), y = *reinterpret_cast<const float4 *>(e.s0 + i);
            *reinterpret_cast<float4 *>(e.p + i) = y;
            *reinterpret_cast<float4 *>(e.s0 + i) = x;
        }
        return;
    }
    for (long long i = c.lo + threadIdx.x; i < c.hi; i += 256) {
        const float x = e.p[i], y = e.s0[i];
        e.p[i] = y;
        e.s0[i] = x;
    }
}

// ---- global gradient norm (ABI 680) ------------------------------------------------------------------------------------------
// Sum of 256 per-thread fp64 values of a workgroup in a fixed tree: xor butterfly inside each wave, the four wave sums added in
// wave order by thread 0 (whose return value is the sum).  A NaN or inf anywhere comes out as NaN or inf.
__device__ __forceinline__ double block_sum_f64(double v, double *scratch) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

// one workgroup per 16384-element chunk, like the steps; only e.g and e.n of the table are set
__global__ __launch_bounds__(256) void lvt_grad_sqnorm_kernel(const OptArgs a, double *partials) {
    __shared__ double scratch[4];
    const OptChunk c(a);
    const LvtOptEntry &e = c.e;
    double acc = 0.0;
    auto sq = [&](float g) { const double d = (double)g; acc += d * d; };
    if (opt_vec_ok(e, c.lo)) {
        for (long long i = c.lo + 4 * threadIdx.x; i < c.hi; i += 1024) {
            const float4 g4 = *reinterpret_cast<const float4 *>(e.g + i);
            sq(g4.x); sq(g4.y); sq(g4.z); sq(g4.w);
        }
    } else {
        for (long long i = c.lo + threadIdx.x; i < c.hi; i += 256) sq(e.g[i]);
    }
    const double total = block_sum_f64(acc, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void lvt_grad_clip_coef_kernel(const double *partials, long long n, float max_norm,
                                                                 lvt_clip_record *record, long long *skipped) {
    __shared__ double scratch[4];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) acc += partials[i];
    const double total = block_sum_f64(acc, scratch);
    if (threadIdx.x == 0) {
        const bool finite = fabs(total) < __builtin_inf();            // false for NaN and for +inf
        const double norm = sqrt(total);
        lvt_clip_record r;
        r.norm = (float)norm;
        r.coef = finite ? (float)fmin(1.0, (double)max_norm / (norm + 1e-6)) : 0.f;
        r.skip = finite ? 0 : 1;
        r.reserved = 0;
        *record = r;
        if (!finite && skipped) *skipped += 1;
    }
}

// ---- host: a list of n tensors becomes launches of up to OPT_MAXT tensors each ------------------------------------------------
static OptArgs &opt_table(OptArgs &a) { return a; }
static OptArgs &opt_table(EmaArgs &a) { return a.a; }

// The one place where that happens, for every entry point of this file (`who`, named in the messages).  Args: OptArgs or EmaArgs.
// fill(args, i, src) -> LVT_OK or an error: validates entry `src` of the caller's list and writes it to slot i of the table
// (p, g, s0, s1, n, lr, wd as the kernel needs them, and the shadow slot of an EmaArgs); chunk_prefix is filled here.
// launch(args, blocks, done): `done` chunks went out with the slices before this one.
// The whole list is validated before the first launch: a refused call has launched nothing.
template <typename Args, typename Fill, typename Launch>
static int launch_slices(const char *who, int n, Fill fill, Launch launch) {
    for (int pass = 0; pass < 2; ++pass) {                    // 0: validate every slice, 1: build them again and launch
        long long done = 0;
        for (int base = 0; base < n; base += OPT_MAXT) {
            Args args = {};
            OptArgs &a = opt_table(args);
            a.n = (n - base) < OPT_MAXT ? (n - base) : OPT_MAXT;
            long long blocks = 0;
            for (int i = 0; i < a.n; ++i) {
                const int rc = fill(args, i, base + i);
                if (rc != LVT_OK) return rc;
                a.chunk_prefix[i] = (int)blocks;
                blocks += lvt_cdiv(a.e[i].n, OPT_CHUNK);
                LVT_REQUIRE(blocks < (1ll << 31), "%s: too many chunks in one launch", who);
            }
            a.chunk_prefix[a.n] = (int)blocks;
            if (pass == 0) continue;
            launch(args, (unsigned)blocks, done);
            LVT_CHECK_LAUNCH(who);
            done += blocks;
        }
    }
    return LVT_OK;
}

// The slices of a step: entry `src` of the host table, and its shadow when the launch carries shadows (Args = EmaArgs).
template <typename Args, typename Launch>
static int step_slices(const char *who, const LvtOptEntry *host, float *const *ema, int n, Launch launch) {
    return launch_slices<Args>(
        who, n,
        [&](Args &args, int i, int src) -> int {
            const LvtOptEntry &e = opt_table(args).e[i] = host[src];
            LVT_REQUIRE(e.p && e.g && e.s0 && e.n > 0, "%s: bad entry %d (null p, g or s0, or no elements)", who, src);
            if constexpr (std::is_same<Args, EmaArgs>::value) {
                float *sh = args.ema[i] = ema[src];
                LVT_REQUIRE(sh && (((uintptr_t)sh) & 3) == 0 && sh != e.p,
                            "%s: bad shadow %d (null, misaligned, or the parameter itself)", who, src);
            }
            return LVT_OK;
        },
        launch);
}

// One launcher per optimizer behind its three entry points: `ema` (nullable) selects the kernels that carry shadows, a clip
// (`gscale`, `clamp` or both) the scaled body.  p, exp_avg (s0), exp_avg_sq (s1) updated in place; `step` is the 1-based step
// count of these tensors.
static int adam_launch(const char *who, const LvtOptEntry *host, float *const *ema, int n, float beta1, float beta2, float eps,
                       int step, const lvt_clip_record *gscale, float clamp, float w, void *stream) {
    LVT_REQUIRE(host && n > 0 && step > 0, "%s: bad args", who);
    hipStream_t s = (hipStream_t)stream;
    const double bc1d = 1.0 - pow((double)beta1, step), bc2d = 1.0 - pow((double)beta2, step);
    const float bc1 = (float)bc1d, bc2_sqrt = (float)sqrt(bc2d);
    const bool scaled = gscale || clamp > 0.f;
    if (ema)
        return step_slices<EmaArgs>(who, host, ema, n, [&](const EmaArgs &a, unsigned blocks, long long) {
            auto kernel = scaled ? lvt_adam_ema_kernel<true> : lvt_adam_ema_kernel<false>;
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, a, beta1, beta2, eps, bc1, bc2_sqrt, gscale, clamp, w);
        });
    return step_slices<OptArgs>(who, host, nullptr, n, [&](const OptArgs &a, unsigned blocks, long long) {
        if (scaled)
            hipLaunchKernelGGL(lvt_adam_scaled_kernel, dim3(blocks), dim3(256), 0, s, a, beta1, beta2, eps, bc1, bc2_sqrt, gscale, clamp);
        else
            hipLaunchKernelGGL(lvt_adam_kernel, dim3(blocks), dim3(256), 0, s, a, beta1, beta2, eps, bc1, bc2_sqrt);
    });
}

// p, square_avg (s0), momentum_buffer (s1, may be NULL when momentum == 0) updated in place.
static int rmsprop_launch(const char *who, const LvtOptEntry *host, float *const *ema, int n, float alpha, float eps,
                          float momentum, const lvt_clip_record *gscale, float clamp, float w, void *stream) {
    LVT_REQUIRE(host && n > 0, "%s: bad args", who);
    hipStream_t s = (hipStream_t)stream;
    const bool scaled = gscale || clamp > 0.f;
    if (ema)
        return step_slices<EmaArgs>(who, host, ema, n, [&](const EmaArgs &a, unsigned blocks, long long) {
            auto kernel = scaled ? lvt_rmsprop_ema_kernel<true> : lvt_rmsprop_ema_kernel<false>;
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, a, alpha, eps, momentum, gscale, clamp, w);
        });
    return step_slices<OptArgs>(who, host, nullptr, n, [&](const OptArgs &a, unsigned blocks, long long) {
        if (scaled)
            hipLaunchKernelGGL(lvt_rmsprop_scaled_kernel, dim3(blocks), dim3(256), 0, s, a, alpha, eps, momentum, gscale, clamp);
        else
            hipLaunchKernelGGL(lvt_rmsprop_kernel, dim3(blocks), dim3(256), 0, s, a, alpha, eps, momentum);
    });
}

// The clip of a step: a 16-byte aligned record, a finite clamp > 0, or both.  The *_scaled entries refuse a call with neither
// (the plain entries are for that); the *_ema entries take it (`optional`) and then launch the unscaled body.
#define REQUIRE_CLIP_ARGS(name, optional)                                                                                    \
    LVT_REQUIRE(clamp >= 0.f && clamp < __builtin_inff() && (((uintptr_t)gscale) & 15) == 0 &&                               \
                    ((optional) || gscale || clamp > 0.f),                                                                   \
                name ": gscale must be 16-byte aligned and clamp finite and >= 0%s", (optional) ? "" : ", one of them given")
#define REQUIRE_EMA_ARGS(name)                                                                                               \
    LVT_REQUIRE(ema, name ": null shadow table");                                                                            \
    LVT_REQUIRE(w >= 0.f && w <= 1.f, name ": w = 1 - decay must lie in [0, 1]");                                            \
    REQUIRE_CLIP_ARGS(name, true)

extern "C" int lvt_adam_step(const LvtOptEntry *host, int n, float beta1, float beta2, float eps, int step,
                             void *stream) {
    return adam_launch("adam_step", host, nullptr, n, beta1, beta2, eps, step, nullptr, 0.f, 0.f, stream);
}

extern "C" int lvt_rmsprop_step(const LvtOptEntry *host, int n, float alpha, float eps, float momentum,
                                void *stream) {
    return rmsprop_launch("rmsprop_step", host, nullptr, n, alpha, eps, momentum, nullptr, 0.f, 0.f, stream);
}

extern "C" int lvt_adam_step_scaled(const LvtOptEntry *host, int n, float beta1, float beta2, float eps, int step,
                                    const lvt_clip_record *gscale, float clamp, void *stream) {
    REQUIRE_CLIP_ARGS("adam_step_scaled", false);
    return adam_launch("adam_step_scaled", host, nullptr, n, beta1, beta2, eps, step, gscale, clamp, 0.f, stream);
}

extern "C" int lvt_rmsprop_step_scaled(const LvtOptEntry *host, int n, float alpha, float eps, float momentum,
                                       const lvt_clip_record *gscale, float clamp, void *stream) {
    REQUIRE_CLIP_ARGS("rmsprop_step_scaled", false);
    return rmsprop_launch("rmsprop_step_scaled", host, nullptr, n, alpha, eps, momentum, gscale, clamp, 0.f, stream);
}

// ---- Polyak-averaged weights inside the steps ---------------------------------------------------------------------------------
extern "C" int lvt_adam_step_ema(const LvtOptEntry *host, float *const *ema, int n, float beta1, float beta2, float eps,
                                 int step, float w, const lvt_clip_record *gscale, float clamp, void *stream) {
    REQUIRE_EMA_ARGS("adam_step_ema");
    return adam_launch("adam_step_ema", host, ema, n, beta1, beta2, eps, step, gscale, clamp, w, stream);
}

extern "C" int lvt_rmsprop_step_ema(const LvtOptEntry *host, float *const *ema, int n, float alpha, float eps, float momentum,
                                    float w, const lvt_clip_record *gscale, float clamp, void *stream) {
    REQUIRE_EMA_ARGS("rmsprop_step_ema");
    return rmsprop_launch("rmsprop_step_ema", host, ema, n, alpha, eps, momentum, gscale, clamp, w, stream);
}

extern "C" int lvt_ema_swap(float *const *pa, float *const *pb, const long long *counts, int n, void *stream) {
    LVT_REQUIRE(pa && pb && counts && n > 0, "ema_swap: bad args");
    hipStream_t s = (hipStream_t)stream;
    return launch_slices<OptArgs>(
        "ema_swap", n,
        [&](OptArgs &a, int i, int src) -> int {
            float *x = pa[src], *y = pb[src];
            const long long cnt = counts[src];
            LVT_REQUIRE(x && y && x != y && cnt > 0 && ((((uintptr_t)x) | ((uintptr_t)y)) & 3) == 0,
                        "ema_swap: bad entry %d (null, misaligned or identical pointers, or no elements)", src);
            LVT_REQUIRE((x + cnt <= y) || (y + cnt <= x), "ema_swap: entry %d overlaps itself", src);
            a.e[i].p = x;
            a.e[i].s0 = y;
            a.e[i].n = cnt;
            return LVT_OK;
        },
        [&](const OptArgs &a, unsigned blocks, long long) {
            hipLaunchKernelGGL(lvt_ema_swap_kernel, dim3(blocks), dim3(256), 0, s, a);
        });
}

extern "C" long long lvt_grad_sqnorm_partials(const lvt_grad_entry *host, int n) {
    if (!host || n <= 0) return -1;
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (!host[i].g || host[i].n <= 0 || (((uintptr_t)host[i].g) & 3)) return -1;
        chunks += lvt_cdiv(host[i].n, OPT_CHUNK);
    }
    return chunks;
}

extern "C" int lvt_grad_sqnorm(const lvt_grad_entry *host, int n, double *partials, long long n_partials, void *stream) {
    LVT_REQUIRE(host && n > 0 && partials && (((uintptr_t)partials) & 7) == 0, "grad_sqnorm: bad args");
    const long long need = lvt_grad_sqnorm_partials(host, n);             // validates every entry
    LVT_REQUIRE(need > 0, "grad_sqnorm: bad entry (null or misaligned gradient, or no elements)");
    LVT_REQUIRE(need == n_partials, "grad_sqnorm: %lld partials for entries that need %lld", n_partials, need);
    hipStream_t s = (hipStream_t)stream;
    return launch_slices<OptArgs>(
        "grad_sqnorm", n,
        [&](OptArgs &a, int i, int src) -> int {
            a.e[i].g = host[src].g;
            a.e[i].n = host[src].n;
            return LVT_OK;
        },
        [&](const OptArgs &a, unsigned blocks, long long done) {
            hipLaunchKernelGGL(lvt_grad_sqnorm_kernel, dim3(blocks), dim3(256), 0, s, a, partials + done);
        });
}

extern "C" int lvt_grad_clip_coef(const double *partials, long long n_partials, float max_norm, lvt_clip_record *record,
                                  long long *skipped, void *stream) {
    LVT_REQUIRE(partials && n_partials > 0 && record && (((uintptr_t)record) & 15) == 0 && (((uintptr_t)skipped) & 7) == 0,
                "grad_clip_coef: bad args");
    LVT_REQUIRE(max_norm > 0.f && max_norm < __builtin_inff(), "grad_clip_coef: max_norm must be positive and finite");
    hipLaunchKernelGGL(lvt_grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, max_norm,
                       record, skipped);
    LVT_CHECK_LAUNCH("grad_clip_coef kernel");
    return LVT_OK;
}
