"""Typed wrappers over the HBM-bound helper kernels (csrc/elementwise.hip)."""
import ctypes as C

import torch

from . import binding as L


def _f32(*shape, like):
    return torch.empty(*shape, dtype=torch.float32, device=like.device)


def to_channels_last(x_bcr, ldo, mode=0, a=None, s=None):
    """(B, C, R) -> (B, R, ldo) with zero-padded channels; mode 1 applies (x - a[c]) / s[c]."""
    L.require(x_bcr, a, s)
    B, Cc, R = x_bcr.shape
    out = _f32(B, R, ldo, like=x_bcr)
    L.check(L.lib().lvt_to_channels_last(L.ptr(x_bcr), B, Cc, R, ldo, mode, L.ptr(a), L.ptr(s), L.ptr(out),
                                         L.out_amax(out), L.stream_ptr()), "lvt_to_channels_last")
    return out


def to_channels_first(x_brc, Cc, mode=0, a=None, s=None, lo=0.0, hi=0.0):
    """(B, R, ldi) -> (B, C, R); mode 2 applies clamp(x * s[c] + a[c], lo, hi)."""
    L.require(x_brc, a, s)
    B, R, ldi = x_brc.shape
    out = _f32(B, Cc, R, like=x_brc)
    L.check(L.lib().lvt_to_channels_first(L.ptr(x_brc), B, Cc, R, ldi, mode, L.ptr(a), L.ptr(s), lo, hi,
                                          L.ptr(out), L.stream_ptr()), "lvt_to_channels_first")
    return out


def _red_ws(dev):
    n = L.lib().lvt_reduce_workspace_bytes()
    return L.workspace(n, dev, "reduce"), n


def mse_fwd(a, b, denom, scale=1.0, l1=False):
    L.require(a, b)
    out = _f32(1, like=a)
    ws, n = _red_ws(a.device)
    L.check((L.lib().lvt_l1_fwd if l1 else L.lib().lvt_mse_fwd)(L.ptr(a), L.ptr(b), a.numel(), float(denom), scale, L.ptr(out), L.ptr(ws), n,
                                L.stream_ptr()), "lvt_mse_fwd")
    return out.view(())


def frame_quality(a, b, data_range, acc=None, frames=None):
    """Per-frame PSNR and SSIM of (F, C, H, W) or (C, H, W) fp32 device frames (csrc/quality.hip; the rule:
    lvt_amd.evaluation.quality.frame_quality_reference) -> (frames, acc): frames (F, 2) float64 = [psnr, ssim] per frame, psnr
    +inf where the frame's mse is 0; acc (4,) float64 += [sum of the finite psnr, sum of ssim, frames with a finite psnr, frames]
    (a fresh zeroed one when none is passed).  `frames`: an (F, 2) float64 tensor to write into instead of a new one.  Nothing is
    read on the host, and a refused call launches nothing."""
    L.require(a, b, acc, frames)
    if tuple(a.shape) != tuple(b.shape):
        raise L.LvtError("frame_quality: shapes differ, %s against %s" % (tuple(a.shape), tuple(b.shape)))
    if a.dim() not in (3, 4) or a.numel() == 0:
        raise L.LvtError("frame_quality: frames are (F, C, H, W) or (C, H, W) and not empty, got %s" % (tuple(a.shape),))
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise L.LvtError("frame_quality: float32 frames only, got %s and %s" % (a.dtype, b.dtype))
    F = a.shape[0] if a.dim() == 4 else 1
    Cc, H, W = a.shape[-3:]
    if H < 11 or W < 11:
        raise L.LvtError("frame_quality: H=%d W=%d, the 11x11 window needs H and W >= 11" % (H, W))
    data_range = float(data_range)
    if not 0.0 < data_range < float("inf"):
        raise L.LvtError("frame_quality: data_range must be positive and finite, got %r" % (data_range,))
    if acc is None:
        acc = torch.zeros(4, dtype=torch.float64, device=a.device)
    elif acc.dtype != torch.float64 or acc.numel() != 4 or acc.device != a.device:
        raise L.LvtError("frame_quality: acc is 4 float64 values on the frames' device")
    n = L.lib().lvt_frame_quality_partials(Cc, H, W)
    ws = L.workspace(F * n * 16, a.device, "frame_quality")
    if frames is None:
        frames = torch.empty(F, 2, dtype=torch.float64, device=a.device)
    elif frames.dtype != torch.float64 or tuple(frames.shape) != (F, 2) or frames.device != a.device:
        raise L.LvtError("frame_quality: frames is (%d, 2) float64 on the frames' device" % F)
    L.check(L.lib().lvt_frame_quality(L.ptr(a), L.ptr(b), F, Cc, H, W, data_range, L.ptr(ws), n, L.stream_ptr()), "lvt_frame_quality")
    L.check(L.lib().lvt_frame_quality_finish(L.ptr(ws), F, Cc, H, W, data_range, n, L.ptr(frames), L.ptr(acc), L.stream_ptr()),
            "lvt_frame_quality_finish")
    return frames, acc


def prediction_quality(samples, target, n_prime, data_range, curves=None, chunk_frames=512):
    """Best-of-N quality of S sampled videos against one target (csrc/quality.hip; the rule:
    lvt_amd.evaluation.quality.prediction_quality_reference).  samples (S, T, C, H, W), target (T, C, H, W): fp32 device frames in
    [0, data_range]; the first `n_prime` frames are left out of the scores and the curves.  -> (frames, best, curves): frames
    (S * T, 2) float64 = [psnr, ssim] of frame t of sample s against frame t of the target, sample-major; best (2,) int32 = the
    sample with the largest mean psnr / ssim over the predicted steps; curves (T, 8) float64 += this clip's row per step (columns:
    include/lvt_hip.h lvt_prediction_select; a fresh zeroed one when none is passed).  The compare runs over whole samples, at most
    `chunk_frames` frames (and at least one sample) per lvt_frame_quality_vs / lvt_frame_quality_finish pair, each pair writing
    its slice of the one table; the target is never copied.  One lvt_prediction_select follows.  Nothing is read on the host, and
    a refused call launches nothing."""
    if not torch.is_tensor(samples) or not torch.is_tensor(target):
        raise L.LvtError("prediction_quality: tensors expected")
    L.require(samples, target, curves)
    if samples.dim() != 5 or target.dim() != 4 or samples.numel() == 0 or tuple(samples.shape[1:]) != tuple(target.shape):
        raise L.LvtError("prediction_quality: shapes differ or are empty, samples (S, T, C, H, W) %s against target (T, C, H, W) %s"
                         % (tuple(samples.shape), tuple(target.shape)))
    if samples.dtype != torch.float32 or target.dtype != torch.float32:
        raise L.LvtError("prediction_quality: float32 frames only, got %s and %s" % (samples.dtype, target.dtype))
    if samples.device != target.device:
        raise L.LvtError("prediction_quality: samples on %s, target on %s" % (samples.device, target.device))
    S, T, Cc, H, W = samples.shape
    if H < 11 or W < 11:
        raise L.LvtError("prediction_quality: H=%d W=%d, the 11x11 window needs H and W >= 11" % (H, W))
    data_range, n_prime, chunk_frames = float(data_range), int(n_prime), int(chunk_frames)
    if not 0.0 < data_range < float("inf"):
        raise L.LvtError("prediction_quality: data_range must be positive and finite, got %r" % (data_range,))
    if not 0 <= n_prime < T:
        raise L.LvtError("prediction_quality: n_prime=%d outside [0, T=%d)" % (n_prime, T))
    if chunk_frames < 1:
        raise L.LvtError("prediction_quality: chunk_frames=%d, at least 1" % chunk_frames)
    if curves is None:
        curves = torch.zeros(T, 8, dtype=torch.float64, device=samples.device)
    elif curves.dtype != torch.float64 or tuple(curves.shape) != (T, 8) or curves.device != samples.device:
        raise L.LvtError("prediction_quality: curves is (%d, 8) float64 on the frames' device" % T)
    per = max(1, chunk_frames // T)                          # whole samples per launch pair
    n = L.lib().lvt_frame_quality_partials(Cc, H, W)
    if min(per, S) * T * n >= 1 << 31:
        raise L.LvtError("prediction_quality: %d frames of %d tiles in one launch, lower chunk_frames" % (min(per, S) * T, n))
    ws = L.workspace(min(per, S) * T * n * 16, samples.device, "frame_quality")
    frames = torch.empty(S * T, 2, dtype=torch.float64, device=samples.device)
    acc = torch.zeros(4, dtype=torch.float64, device=samples.device)          # scratch: `finish` needs one, nobody reads it
    best = torch.empty(2, dtype=torch.int32, device=samples.device)
    for s0 in range(0, S, per):
        F = (min(s0 + per, S) - s0) * T
        L.check(L.lib().lvt_frame_quality_vs(L.ptr(samples[s0]), L.ptr(target), F, T, Cc, H, W, data_range, L.ptr(ws), n,
                                             L.stream_ptr()), "lvt_frame_quality_vs")
        L.check(L.lib().lvt_frame_quality_finish(L.ptr(ws), F, Cc, H, W, data_range, n, L.ptr(frames[s0 * T]), L.ptr(acc),
                                                 L.stream_ptr()), "lvt_frame_quality_finish")
    L.check(L.lib().lvt_prediction_select(L.ptr(frames), S, T, n_prime, L.ptr(curves), L.ptr(best), L.stream_ptr()),
            "lvt_prediction_select")
    return frames, best, curves


def ssim_loss_fwd(xt, x, mean, std, data_range, lam, want_grad=False):
    """The SSIM term of the reconstruction loss on channels-last activations (csrc/ssim_loss.hip; the rule:
    lvt_amd.evaluation.quality.ssim_loss_reference).  xt (the reconstruction), x (the target): (N, 1, H, W, Cp) fp32 device
    tensors, Cp = C rounded up to 4 with zero pad channels; mean, std: C float32 values each on the same device (tensors; a
    sequence is copied there), the de-normalisation u = v * std[c] + mean[c].  -> (loss, G): loss the fp32 device scalar
    lam * (1 - mean SSIM(u(xt), u(x))); G = d loss / d xt shaped like xt (pad channels exact 0) when `want_grad`, else None and
    the backward half of the kernel is skipped (same loss bits).  Nothing is read on the host, and a refused call launches
    nothing."""
    if not torch.is_tensor(xt) or not torch.is_tensor(x):
        raise L.LvtError("ssim_loss_fwd: tensors expected")
    if tuple(xt.shape) != tuple(x.shape):
        raise L.LvtError("ssim_loss_fwd: shapes differ, %s against %s" % (tuple(xt.shape), tuple(x.shape)))
    if xt.dim() != 5 or xt.shape[1] != 1 or xt.numel() == 0 or xt.shape[-1] % 4:
        raise L.LvtError("ssim_loss_fwd: frames are channels-last (N, 1, H, W, Cp) with Cp a multiple of 4, got %s" % (tuple(xt.shape),))
    if xt.dtype != torch.float32 or x.dtype != torch.float32:
        raise L.LvtError("ssim_loss_fwd: float32 frames only, got %s and %s" % (xt.dtype, x.dtype))
    N, _, H, W, Cp = xt.shape
    if H < 11 or W < 11:
        raise L.LvtError("ssim_loss_fwd: H=%d W=%d, the 11x11 window needs H and W >= 11" % (H, W))
    data_range, lam = float(data_range), float(lam)
    if not 0.0 < data_range < float("inf"):
        raise L.LvtError("ssim_loss_fwd: data_range must be positive and finite, got %r" % (data_range,))
    if not 0.0 <= lam < float("inf"):
        raise L.LvtError("ssim_loss_fwd: lam must be non-negative and finite, got %r" % (lam,))
    Cc = len(mean)
    if len(std) != Cc or Cc < 1 or (Cc + 3) // 4 * 4 != Cp:
        raise L.LvtError("ssim_loss_fwd: %d means and %d stds for frames of %d channels (C rounded up to 4)" % (Cc, len(std), Cp))
    L.require(xt, x)
    if not torch.is_tensor(mean):
        mean = torch.tensor([float(v) for v in mean], dtype=torch.float32, device=xt.device)
    if not torch.is_tensor(std):
        std = torch.tensor([float(v) for v in std], dtype=torch.float32, device=xt.device)
    L.require(mean, std)
    if mean.dtype != torch.float32 or std.dtype != torch.float32 or mean.dim() != 1 or std.dim() != 1:
        raise L.LvtError("ssim_loss_fwd: mean and std are 1-D float32")
    n = L.lib().lvt_ssim_loss_partials(N, H, W, Cp)
    ws = L.workspace(n * 8, xt.device, "ssim_loss")
    out = _f32(1, like=xt)
    G = torch.empty_like(xt) if want_grad else None
    L.check(L.lib().lvt_ssim_loss_fwd(L.ptr(xt), L.ptr(x), N, H, W, Cp, Cc, L.ptr(mean), L.ptr(std), data_range, lam, L.ptr(ws), n,
                                      L.ptr(G), L.stream_ptr()), "lvt_ssim_loss_fwd")
    L.check(L.lib().lvt_ssim_loss_finish(L.ptr(ws), n, N, H, W, Cc, lam, L.ptr(out), L.stream_ptr()), "lvt_ssim_loss_finish")
    return out.view(()), G


def mse_bwd(a, b, denom, scale=1.0, gout=None, add=None, tanh_of_a=False, l1=False, g_plus=None, plus=None):
    """`plus` (with `g_plus`): the gradient G of a second loss term w.r.t. `a` and the device scalar autograd hands back for that
    term; the launch writes gout c (a - b | sign) + g_plus G as ONE tensor and reports its max |.| (lvt_mse_bwd_plus /
    lvt_l1_bwd_plus)."""
    L.require(a, b, gout, add, g_plus, plus)
    if (plus is None) != (g_plus is None):
        raise L.LvtError("mse_bwd: plus and g_plus go together")
    if plus is not None:
        if add is not None or tanh_of_a:
            raise L.LvtError("mse_bwd: plus excludes add and tanh_of_a")
        if tuple(plus.shape) != tuple(a.shape) or plus.dtype != torch.float32 or g_plus.numel() != 1 or g_plus.dtype != torch.float32:
            raise L.LvtError("mse_bwd: plus is shaped like a, g_plus one float32 value")
        out = torch.empty_like(a)
        L.check((L.lib().lvt_l1_bwd_plus if l1 else L.lib().lvt_mse_bwd_plus)(
            L.ptr(a), L.ptr(b), a.numel(), float(denom), scale, L.ptr(gout), L.ptr(g_plus), L.ptr(plus), L.ptr(out), L.out_amax(out),
            L.stream_ptr()), "lvt_mse_bwd_plus")
        return out
    out = torch.empty_like(a)
    L.check((L.lib().lvt_l1_bwd if l1 else L.lib().lvt_mse_bwd)(L.ptr(a), L.ptr(b), a.numel(), float(denom), scale, L.ptr(gout), L.ptr(add),
                                1 if tanh_of_a else 0, L.ptr(out), L.out_amax(out), L.stream_ptr()), "lvt_mse_bwd")
    return out


def tanh_bwd(g, y):
    L.require(g, y)
    out = torch.empty_like(g)
    L.check(L.lib().lvt_tanh_bwd(L.ptr(g), L.ptr(y), g.numel(), L.ptr(out), L.out_amax(out), L.stream_ptr()), "lvt_tanh_bwd")
    return out


def sigmoid_bwd(g, y):
    """g * y * (1 - y) from the saved sigmoid output y.  Reports max |out| (f16x2 mode)."""
    L.require(g, y)
    out = torch.empty_like(g)
    L.check(L.lib().lvt_sigmoid_bwd(L.ptr(g), L.ptr(y), g.numel(), L.ptr(out), L.out_amax(out), L.stream_ptr()), "lvt_sigmoid_bwd")
    return out


def mask_flags(mask, leaky):
    """Epilogue flags of a (Leaky)ReLU-backward mask: 0 without one, EPI_MASK, or EPI_MASK | EPI_LEAKY_MASK."""
    if mask is None:
        return 0
    return L.EPI_MASK | (L.EPI_LEAKY_MASK if leaky else 0)


def _resample(fn, name, x, out_hw, scale, mask, leaky):
    L.require(x, mask)
    N, H, W, Cp = x.shape[0], x.shape[-3], x.shape[-2], x.shape[-1]
    if x.numel() != N * H * W * Cp:
        raise L.LvtError("%s: frames only (N, 1, H, W, C) or (N, H, W, C), got %s" % (name, tuple(x.shape)))
    out = torch.empty(tuple(x.shape[:-3]) + out_hw + (Cp,), dtype=torch.float32, device=x.device)
    if mask is not None and tuple(mask.shape) != tuple(out.shape):
        raise L.LvtError("%s: the mask must have the output's shape %s, got %s" % (name, tuple(out.shape), tuple(mask.shape)))
    L.check(fn(L.ptr(x), N, H, W, Cp, float(scale), L.ptr(mask), mask_flags(mask, leaky), L.ptr(out), L.out_amax(out),
               L.stream_ptr()), name)
    return out


def pool2x2(x, scale=0.25, mask=None, leaky=False):
    """(N[,1],H,W,Cp) -> (N[,1],H/2,W/2,Cp): scale * the sum of every 2x2 window.  0.25: AvgPool2d(2); 1: the backward of the
    nearest upsample.  mask (the output's shape): times (mask > 0), or (mask > 0 ? 1 : 0.2) with `leaky`.  H, W even."""
    return _resample(L.lib().lvt_pool2x2, "lvt_pool2x2", x, (x.shape[-3] // 2, x.shape[-2] // 2), scale, mask, leaky)


def upsample2x2(x, scale=1.0, mask=None, leaky=False):
    """(N[,1],H,W,Cp) -> (N[,1],2H,2W,Cp): every pixel repeated 2x2, times scale.  1: Upsample(scale_factor=2); 0.25: the backward
    of the average pool.  mask as for pool2x2."""
    return _resample(L.lib().lvt_upsample2x2, "lvt_upsample2x2", x, (2 * x.shape[-3], 2 * x.shape[-2]), scale, mask, leaky)


_SHUFFLE_ACTS = {"": 0, "relu": L.EPI_RELU, "tanh": L.EPI_TANH, "sigmoid": L.EPI_SIGMOID}


def _frames(name, x):
    if x.dim() in (4, 5):
        N, H, W, Cx = x.shape[0], x.shape[-3], x.shape[-2], x.shape[-1]
        if x.numel() == N * H * W * Cx:
            return N, H, W, Cx
    raise L.LvtError("%s: frames only (N, 1, H, W, C) or (N, H, W, C), got %s" % (name, tuple(x.shape)))


def pixel_shuffle2(x, C, act=""):
    """(N[,1],H,W,4C) -> (N[,1],2H,2W,pad4(C)): nn.PixelShuffle(2) followed by `act` ("" | "relu" | "tanh" | "sigmoid");
    out[n,2h+i,2w+j,c] = act(x[n,h,w,4c+2i+j]), the pad channels C.. exact zeros under every act.  `act` may also be the epilogue
    flags of convnet._act_flag: the pad count that rides on a sigmoid flag is dropped, the kernel knows its pads from C."""
    L.require(x)
    N, H, W, Cx = _frames("lvt_pixel_shuffle2", x)
    if C <= 0 or Cx != 4 * C:
        raise L.LvtError("lvt_pixel_shuffle2: %d channels in, 4 * C = %d expected" % (Cx, 4 * C))
    if isinstance(act, str):
        if act not in _SHUFFLE_ACTS:
            raise L.LvtError("lvt_pixel_shuffle2: act %r is none of %s" % (act, sorted(_SHUFFLE_ACTS)))
        flag = _SHUFFLE_ACTS[act]
    else:
        flag = act & ~L.epi_pad(3)
    out = torch.empty(tuple(x.shape[:-3]) + (2 * H, 2 * W, (C + 3) // 4 * 4), dtype=torch.float32, device=x.device)
    L.check(L.lib().lvt_pixel_shuffle2(L.ptr(x), N, H, W, C, flag, L.ptr(out), L.out_amax(out), L.stream_ptr()), "lvt_pixel_shuffle2")
    return out


def pixel_unshuffle2(g, C):
    """(N[,1],2H,2W,pad4(C)) -> (N[,1],H,W,4C): the inverse (and backward) of pixel_shuffle2; the pad channels of g are ignored."""
    L.require(g)
    N, H2, W2, Cp = _frames("lvt_pixel_unshuffle2", g)
    if C <= 0 or Cp != (C + 3) // 4 * 4 or H2 % 2 or W2 % 2:
        raise L.LvtError("lvt_pixel_unshuffle2: (.., %d, %d, %d) is not the shuffle of C = %d channels" % (H2, W2, Cp, C))
    out = torch.empty(tuple(g.shape[:-3]) + (H2 // 2, W2 // 2, 4 * C), dtype=torch.float32, device=g.device)
    L.check(L.lib().lvt_pixel_unshuffle2(L.ptr(g), N, H2 // 2, W2 // 2, C, L.ptr(out), L.out_amax(out), L.stream_ptr()),
            "lvt_pixel_unshuffle2")
    return out


def axpy(x, alpha=1.0, alpha_dev=None, add=None):
    L.require(x, alpha_dev, add)
    out = torch.empty_like(x)
    L.check(L.lib().lvt_axpy(L.ptr(x), L.ptr(add), x.numel(), L.ptr(alpha_dev), alpha, L.ptr(out), L.stream_ptr()),
            "lvt_axpy")
    return out


def add_periodic_(x, table, P):
    L.require(x, table)
    d = x.shape[-1]
    L.check(L.lib().lvt_add_periodic(L.ptr(x), L.ptr(table), x.numel() // d, P, d, L.stream_ptr()),
            "lvt_add_periodic")
    L.drop_amax(x)          # rewritten in place behind torch's back
    return x


def layernorm_fwd(x, w, b, eps=1e-5, save_stats=True):
    L.require(x, w, b)
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    mean = _f32(rows, like=x) if save_stats else None
    rstd = _f32(rows, like=x) if save_stats else None
    # f16x2: the output feeds engine launches; its max |.| is the a-priori bound (max |w| sqrt(d - 1) + max |b|) (1 + 2^-20) (one
    # store; the 2^-20 covers the kernel's own fp32 rounding: tests/test_gpu_row_kernels.py)
    f16 = L.f16x2()
    L.check(L.lib().lvt_layernorm_fwd(L.ptr(x), rows, d, eps, L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(mean),
                                      L.ptr(rstd), L.out_amax(y), L.ptr(L.amax_of(w)) if f16 else None,
                                      L.ptr(L.amax_of(b)) if f16 else None, L.stream_ptr()), "lvt_layernorm_fwd")
    return y, mean, rstd


def layernorm_fwd_p2(x, w, b, eps=1e-5):
    """layernorm_fwd that also writes the output as a P2 image (csrc/gemm_p2.hip) under the a-priori bound it stores as the
    output's max |.|: -> (y, image data (float32-typed, y's shape), mean, rstd).  f16x2 arithmetic only."""
    L.require(x, w, b)
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    yp = torch.empty_like(x)
    mean, rstd = _f32(rows, like=x), _f32(rows, like=x)
    L.check(L.lib().lvt_layernorm_fwd_p2(L.ptr(x), rows, d, eps, L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(yp), L.ptr(mean),
                                         L.ptr(rstd), L.out_amax(y), L.ptr(L.amax_of(w)), L.ptr(L.amax_of(b)),
                                         L.stream_ptr()), "lvt_layernorm_fwd_p2")
    return y, yp, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, w, add=None):
    L.require(dy, x, mean, rstd, w, add)
    d = x.shape[-1]
    rows = x.numel() // d
    dx = torch.empty_like(x)
    dw, db = _f32(d, like=x), _f32(d, like=x)
    n = L.lib().lvt_layernorm_bwd_workspace_bytes(d)
    ws = L.workspace(n, x.device, "ln")
    L.check(L.lib().lvt_layernorm_bwd(L.ptr(dy), L.ptr(x), L.ptr(mean), L.ptr(rstd), L.ptr(w), rows, d, L.ptr(add),
                                      L.ptr(dx), L.ptr(dw), L.ptr(db), L.out_amax(dx), L.ptr(ws), n, L.stream_ptr()),
            "lvt_layernorm_bwd")
    return dx, dw, db


def row_gather(x, perm, S):
    """x (b*S, d) token matrix -> rows regrouped per sample: out[b*S + i] = x[b*S + perm[i]]."""
    L.require(x, perm)
    d = x.shape[-1]
    out = torch.empty_like(x)
    L.check(L.lib().lvt_row_gather(L.ptr(x), L.ptr(perm), x.numel() // (S * d), S, d, L.ptr(out), L.stream_ptr()),
            "lvt_row_gather")
    if L.f16x2() and L._valid_amax(x) is not None:
        L.set_amax(out, L._valid_amax(x))        # a permutation of the rows: same max |.|
    return out
