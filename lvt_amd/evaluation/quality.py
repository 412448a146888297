"""Per-frame PSNR and SSIM, stated once in plain torch (any device, any float dtype).  `frame_quality_reference` is the CPU branch
of `FrameQualityEvaluator` and the rule the gfx950 kernel behind `lvt_amd.hip.ew.frame_quality` is tested against
(csrc/quality.hip).

SSIM follows Wang, Bovik, Sheikh, Simoncelli, "Image quality assessment: from error visibility to structural similarity" (IEEE
TIP 2004): an 11x11 Gaussian window of sigma 1.5 normalised to sum 1 and applied separably, no padding (the map of an H x W plane
is (H-10) x (W-10)), the weighted biased variances and covariance E_w[xy] - mu_x mu_y, C1 = (0.01 L)^2, C2 = (0.03 L)^2 with L
the data range; the SSIM of a frame is the mean of the map over all its channels and positions.  This is the definition of
`skimage.metrics.structural_similarity(gaussian_weights=True, use_sample_covariance=False)` and the default of `pytorch_msssim`
(neither is a dependency of this package, and neither was at hand to compare with).

PSNR of a frame is 10 log10(L^2 / mse) with the mse over all channels of the frame; a frame with mse == 0 has none (+inf).

`prediction_quality_reference` states the best-of-N rule of `PredictionQualityEvaluator` on top of the per-frame values (which
sample of S sampled videos is the best under each metric, and the eight per-step sums a clip contributes; csrc/quality.hip
lvt_prediction_select).

`ssim_loss_reference` states the SSIM term of the reconstruction loss (LOSS.SSIM.LAMBDA, csrc/ssim_loss.hip) with the
same windows and constants, and `ssim_loss_closed_form` its gradient without autograd."""
import math

import torch

WINDOW, SIGMA = 11, 1.5


def gaussian_window(dtype=torch.float64, device=None):
    """The 11 taps exp(-(k - 5)^2 / (2 sigma^2)) normalised to sum 1 (formed in fp64, then cast)."""
    k = torch.arange(WINDOW, dtype=torch.float64) - (WINDOW - 1) / 2
    g = torch.exp(-k * k / (2 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype=dtype, device=device)


def windowed(x, win):
    """Separable valid correlation of the last two axes of `x` with the 1-D window: (..., H, W) -> (..., H-10, W-10)."""
    n = win.numel()
    W = x.shape[-1] - n + 1
    h = sum(win[k] * x[..., :, k:k + W] for k in range(n))
    H = x.shape[-2] - n + 1
    return sum(win[k] * h[..., k:k + H, :] for k in range(n))


def check_frames(a, b, data_range):
    """The refusals shared by the reference and the device op: -> (a, b) as (F, C, H, W), or ValueError naming the cause."""
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("frame quality: shapes differ, %s against %s" % (tuple(a.shape), tuple(b.shape)))
    if a.dim() == 3:
        a, b = a[None], b[None]
    if a.dim() != 4:
        raise ValueError("frame quality: frames are (F, C, H, W) or (C, H, W), got %s" % (tuple(a.shape),))
    if a.shape[-2] < WINDOW or a.shape[-1] < WINDOW:
        raise ValueError("frame quality: H=%d W=%d, the 11x11 window needs H and W >= 11" % (a.shape[-2], a.shape[-1]))
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("frame quality: no frames or no channels in %s" % (tuple(a.shape),))
    data_range = float(data_range)
    if not (data_range > 0 and math.isfinite(data_range)):
        raise ValueError("frame quality: data_range must be positive and finite, got %r" % (data_range,))
    return a, b


def frame_quality_reference(a, b, data_range, dtype=torch.float64):
    """(F, C, H, W) frames a, b -> (psnr[F], ssim[F]) in `dtype`; psnr is +inf for a frame with mse == 0."""
    a, b = check_frames(a, b, data_range)
    x, y = a.to(dtype), b.to(dtype)
    L = float(data_range)
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    psnr = torch.where(mse == 0, torch.full_like(mse, float("inf")), 10 * torch.log10(L * L / mse))
    win = gaussian_window(dtype, x.device)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mx, my = windowed(x, win), windowed(y, win)
    sxx = windowed(x * x, win) - mx * mx
    syy = windowed(y * y, win) - my * my
    sxy = windowed(x * y, win) - mx * my
    ssim = ((2 * (mx * my) + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    return psnr, ssim.mean(dim=(1, 2, 3))


def best_sample(scores):
    """The index of the largest of the 1-D `scores`: equal scores resolve to the lowest index, a NaN loses against every other
    value, and index 0 is chosen when all are NaN."""
    best = 0
    for s in range(1, scores.numel()):
        a, b = float(scores[s]), float(scores[best])
        if a > b or (math.isnan(b) and not math.isnan(a)):
            best = s
    return best


def prediction_select_reference(psnr, ssim, n_prime):
    """The selection half of `prediction_quality_reference` on (S, T) tables of per-frame values -> (best (2,) int64, curves
    (T, 8)): what lvt_prediction_select computes (csrc/quality.hip), in the same fp64 operations and orders."""
    if psnr.dim() != 2 or tuple(psnr.shape) != tuple(ssim.shape) or psnr.shape[0] < 1 or psnr.shape[1] < 1:
        raise ValueError("prediction quality: psnr and ssim are (S, T) with S, T >= 1, got %s and %s"
                         % (tuple(psnr.shape), tuple(ssim.shape)))
    S, T = psnr.shape
    if not 0 <= n_prime < T:
        raise ValueError("prediction quality: n_prime=%d outside [0, T=%d)" % (n_prime, T))
    psnr, ssim = psnr.double(), ssim.double()
    score_p, score_s = torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
    for t in range(n_prime, T):                              # ascending t; inf + finite = inf
        score_p, score_s = score_p + psnr[:, t].cpu(), score_s + ssim[:, t].cpu()
    bp, bs = best_sample(score_p / (T - n_prime)), best_sample(score_s / (T - n_prime))
    curves = torch.zeros(T, 8, dtype=torch.float64)
    for t in range(n_prime, T):
        row = curves[t]
        p = float(psnr[bp, t])
        if math.isfinite(p):
            row[0], row[1] = p, 1.0
        row[2] = float(ssim[bs, t])
        for s in range(S):                                   # ascending s
            p = float(psnr[s, t])
            if math.isfinite(p):
                row[3] += p
                row[4] += 1.0
            row[5] += float(ssim[s, t])
        row[6], row[7] = 1.0, float(S)
    return torch.tensor([bp, bs], dtype=torch.int64), curves


def prediction_quality_reference(samples, target, n_prime, data_range, dtype=torch.float64):
    """Best-of-N quality of S sampled videos against one target, the rule of `PredictionQualityEvaluator` (its CPU branch, and what
    `lvt_amd.hip.ew.prediction_quality` is tested against).  samples (S, T, C, H, W), target (T, C, H, W): frames in
    pixel space [0, data_range]; the first `n_prime` frames prime the sampler and are left out everywhere.
    -> (psnr (S, T), ssim (S, T), best (2,) int64, curves (T, 8) float64).  psnr[s], ssim[s] are `frame_quality_reference(
    samples[s], target)`.  The score of a sample under a metric is the mean of its values over t = n_prime .. T-1, added in
    ascending t (a +inf psnr takes part); best = (the sample with the largest psnr score, the one with the largest ssim score),
    chosen independently by `best_sample`.  curves is the clip's contribution to the per-step sums: rows below n_prime 0, row t
      0: psnr[best[0], t] if finite, else 0    1: 1 if it is finite, else 0    2: ssim[best[1], t]
      3: sum over s of the finite psnr[s, t]   4: their number                 5: sum over s of ssim[s, t]
      6: 1 (clips)                             7: S (sampled videos)."""
    if samples.dim() != 5 or samples.shape[0] < 1:
        raise ValueError("prediction quality: samples are (S, T, C, H, W) with S >= 1, got %s" % (tuple(samples.shape),))
    if target.dim() != 4:
        raise ValueError("prediction quality: the target is (T, C, H, W), got %s" % (tuple(target.shape),))
    n_prime = int(n_prime)
    if not 0 <= n_prime < target.shape[0]:
        raise ValueError("prediction quality: n_prime=%d outside [0, T=%d)" % (n_prime, target.shape[0]))
    per_sample = [frame_quality_reference(samples[s], target, data_range, dtype) for s in range(samples.shape[0])]
    psnr, ssim = torch.stack([p for p, _ in per_sample]), torch.stack([q for _, q in per_sample])
    best, curves = prediction_select_reference(psnr, ssim, n_prime)
    return psnr, ssim, best, curves


def ssim_loss_reference(x, y, mean, std, data_range, lam):
    """The SSIM term of the reconstruction loss (LOSS.SSIM.LAMBDA): the rule the gfx950 kernel behind
    `lvt_amd.hip.ew.ssim_loss_fwd` is tested against (csrc/ssim_loss.hip).  x (the reconstruction, not clamped) and y (the target)
    are (F, C, H, W) frames in the network's normalised space, in any float dtype and on any device; `mean`, `std`: C values
    that take them back to pixel space, u = v * std[c] + mean[c] (SSIM's luminance term assumes non-negative intensities).
    -> the scalar lam * (1 - mean over frames, channels and map positions of SSIM(u(x), u(y))), differentiable in x (and y),
    with the SSIM of `frame_quality_reference`: its windows, moments and constants, evaluated in the dtype of x."""
    x, y = check_frames(x, y, data_range)
    C = x.shape[1]
    if len(mean) != C or len(std) != C:
        raise ValueError("ssim loss: %d channels, %d means and %d stds" % (C, len(mean), len(std)))
    dt, dev = x.dtype, x.device
    m = torch.as_tensor(mean, dtype=torch.float64).to(dtype=dt, device=dev).view(1, C, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float64).to(dtype=dt, device=dev).view(1, C, 1, 1)
    ux, uy = x * s + m, y.to(dt) * s + m
    L = float(data_range)
    win = gaussian_window(dt, dev)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mx, my = windowed(ux, win), windowed(uy, win)
    sxx = windowed(ux * ux, win) - mx * mx
    syy = windowed(uy * uy, win) - my * my
    sxy = windowed(ux * uy, win) - mx * my
    ssim = ((2 * (mx * my) + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    return lam * (1 - ssim.mean())


def ssim_loss_closed_form(x, y, mean, std, data_range, lam):
    """d ssim_loss_reference / d x in closed form, without autograd: with the windowed moments of u(x), u(y) and
    A1 = 2 mx my + C1, A2 = 2 sxy + C2, B1 = mx^2 + my^2 + C1, B2 = sxx + syy + C2, S = A1 A2 / (B1 B2),
        dA1 = A2 / (B1 B2), dA2 = A1 / (B1 B2), dB1 = -S / B1, dB2 = -S / B2
        alpha = 2 my (dA1 - dA2) + 2 mx (dB1 - dB2), beta = 2 dB2, gamma = 2 dA2
        dS_total / du_x = W^T alpha + u_x W^T beta + u_y W^T gamma
    (W^T: the transpose of `windowed`, a full 11-tap pass in each direction), times -lam / (F C (H-10) (W-10)) and std[c]."""
    x, y = check_frames(x, y, data_range)
    F_, C, H, W = x.shape
    dt, dev = x.dtype, x.device
    m = torch.as_tensor(mean, dtype=torch.float64).to(dtype=dt, device=dev).view(1, C, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float64).to(dtype=dt, device=dev).view(1, C, 1, 1)
    ux, uy = x * s + m, y.to(dt) * s + m
    L = float(data_range)
    win = gaussian_window(dt, dev)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mx, my = windowed(ux, win), windowed(uy, win)
    sxx = windowed(ux * ux, win) - mx * mx
    syy = windowed(uy * uy, win) - my * my
    sxy = windowed(ux * uy, win) - mx * my
    A1, A2, B1, B2 = 2 * mx * my + c1, 2 * sxy + c2, mx * mx + my * my + c1, sxx + syy + c2
    S = A1 * A2 / (B1 * B2)
    dA1, dA2, dB1, dB2 = A2 / (B1 * B2), A1 / (B1 * B2), -S / B1, -S / B2
    alpha = 2 * my * (dA1 - dA2) + 2 * mx * (dB1 - dB2)
    beta, gamma = 2 * dB2, 2 * dA2

    def transposed(z):
        n = win.numel()
        v = z.new_zeros(*z.shape[:-2], H, z.shape[-1])
        for k in range(n):
            v[..., k:k + H - n + 1, :] += win[k] * z
        h = z.new_zeros(*z.shape[:-2], H, W)
        for k in range(n):
            h[..., :, k:k + W - n + 1] += win[k] * v
        return h

    g = transposed(alpha) + ux * transposed(beta) + uy * transposed(gamma)
    return g * (-lam / (F_ * C * (H - WINDOW + 1) * (W - WINDOW + 1))) * s
