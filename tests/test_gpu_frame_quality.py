"""Per-frame PSNR / SSIM on the device (csrc/quality.hip through ew.frame_quality, FrameQualityEvaluator) against
`frame_quality_reference` in fp64 on the CPU.

Bounds (set before the kernel ran; measured figures: profiles/frame_quality.jsonl):
  SSIM  per frame |kernel - fp64| <= max(4 e, 128 * 2^-24).  e is the error, against the same fp64, of `ssim_fp32_pivoted` below: the
        textbook formula with the moments taken about a pivot (here: the plane's first pixel), evaluated in fp32 on the CPU.  The
        factor 4 covers the kernel's other summation order and its per-tile pivots; the floor is the worst-case rounding of a
        121-term fp32 sum.  The unpivoted fp32 formula is off by 5e-5 to 2e-4 on the one- and two-window frames of the bright flat
        class, e is below 1e-7 there.
  PSNR  per frame within 1e-4 dB: the squared differences are exact fp64 products of fp32 values summed in fp64.
Shapes: a single window, one extra column, a partial tile in both directions with an odd frame count, the shipped frame size, and
(4, 3, 75, 43), whose 65 x 33 map has full and partial 16 x 32 tiles along both axes (four frames: lvt_mse_fwd, which one test
compares the squared error with, takes element counts that are multiples of 4)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 11, 11), (2, 1, 11, 12), (5, 3, 17, 23), (3, 3, 64, 64), (4, 3, 75, 43)]
MULTI_TILE = (4, 3, 75, 43)
CLASSES = ("noise", "noised_copy", "bright_flat", "ramp_mirror")
RANGES = (1.0, 255.0)
SSIM_FLOOR = 128 * 2.0 ** -24
PSNR_TOL_DB = 1e-4


def make_pair(kind, shape, L, seed=0):
    """(a, b) float32 on the CPU with values in [0, L]; frame f of b is distorted with its own strength s_f = (f + 1) / F, so that a
    frame mix-up changes the per-frame values."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * CLASSES.index(kind) + shape[-1])
    F = shape[0]
    s = (torch.arange(1, F + 1, dtype=torch.float32) / F).view(-1, 1, 1, 1)
    u = torch.rand(shape, generator=g)
    if kind == "noise":                                    # independent uniform noise (fully independent in the last frame)
        a = L * u
        b = (1 - s) * a + s * L * torch.rand(shape, generator=g)
    elif kind == "noised_copy":                            # a frame against a lightly noised, clamped copy of itself
        a = L * u
        b = (a + 0.02 * L * s * torch.randn(shape, generator=g)).clamp(0, L)
    elif kind == "bright_flat":                            # 0.999 L against 0.999 L - 1e-3 L u (the last frame; the others 0.5 .. 1 of it)
        a = torch.full(shape, 0.999 * L)
        b = a - 1e-3 * L * u * (0.5 + 0.5 * s)
    elif kind == "ramp_mirror":                            # a horizontal ramp against its mirror image, blended in by s_f
        ramp = L * torch.arange(shape[-1], dtype=torch.float32) / (shape[-1] - 1)
        a = ramp.expand(shape).contiguous()
        b = (1 - s) * a + s * a.flip(-1)
    else:
        raise KeyError(kind)
    return a.float().contiguous(), b.float().contiguous()


def _windowed32(x, win):
    W = x.shape[-1] - 10
    h = sum(win[k] * x[..., :, k:k + W] for k in range(11))
    H = x.shape[-2] - 10
    return sum(win[k] * h[..., k:k + H, :] for k in range(11))


def ssim_fp32_pivoted(a, b, L):
    """Wang et al.'s formula with pivots subtracted, in fp32 throughout (the per-frame mean of the fp32 map is taken in fp64):
    x' = x - x[0, 0] and y' = y - y[0, 0] per plane; variances and covariance from x', y'; the pivots added back for the means."""
    a, b = a.float(), b.float()
    k = torch.arange(11, dtype=torch.float64) - 5
    win = torch.exp(-k * k / (2 * 1.5 * 1.5))
    win = (win / win.sum()).float()
    pa, pb = a[..., :1, :1], b[..., :1, :1]
    x, y = a - pa, b - pb
    mx, my = _windowed32(x, win), _windowed32(y, win)
    sxx = _windowed32(x * x, win) - mx * mx
    syy = _windowed32(y * y, win) - my * my
    sxy = _windowed32(x * y, win) - mx * my
    ux, uy = mx + pa, my + pb
    c1, c2 = torch.tensor((0.01 * L) ** 2, dtype=torch.float32), torch.tensor((0.03 * L) ** 2, dtype=torch.float32)
    ssim = ((2 * (ux * uy) + c1) * (2 * sxy + c2)) / ((ux * ux + uy * uy + c1) * (sxx + syy + c2))
    assert ssim.dtype == torch.float32
    return ssim.double().mean(dim=(1, 2, 3))


_cache = {}


def case(kind, shape, L):
    """(a, b, psnr64, ssim64, e) of a case, computed once and shared (read-only) among the tests."""
    key = (kind, shape, L)
    if key not in _cache:
        from lvt_amd.evaluation import frame_quality_reference
        a, b = make_pair(kind, shape, L)
        psnr, ssim = frame_quality_reference(a, b, L)
        e = (ssim_fp32_pivoted(a, b, L) - ssim).abs()
        _cache[key] = (a, b, psnr, ssim, e)
    return _cache[key]


def kernel_errors(kind, shape, L):
    """-> (max |ssim - fp64|, max e, max |psnr - fp64| in dB, whether every frame is inside its bounds) of one case."""
    from lvt_amd.hip import ew
    a, b, psnr, ssim, e = case(kind, shape, L)
    frames, _ = ew.frame_quality(a.cuda(), b.cuda(), L)
    frames = frames.cpu()
    d_ssim, d_psnr = (frames[:, 1] - ssim).abs(), (frames[:, 0] - psnr).abs()
    ok = bool((d_ssim <= torch.clamp(4 * e, min=SSIM_FLOOR)).all()) and bool((d_psnr <= PSNR_TOL_DB).all())
    return float(d_ssim.max()), float(e.max()), float(d_psnr.max()), ok


@pytest.mark.parametrize("L", RANGES)
@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_fp64(shape, kind, L):
    _, _, psnr, ssim, e = case(kind, shape, L)
    assert torch.isfinite(psnr).all() and len(set(ssim.tolist())) == shape[0]          # every frame has its own value
    d_ssim, e_max, d_psnr, ok = kernel_errors(kind, shape, L)
    print("frame_quality %s %s L=%g: |ssim - fp64| %.3g (e %.3g, bound %.3g)  |psnr - fp64| %.3g dB"
          % (kind, shape, L, d_ssim, e_max, max(4 * e_max, SSIM_FLOOR), d_psnr))
    assert ok, (d_ssim, e_max, d_psnr)


def test_the_bound_tells_a_pivoted_kernel_from_an_unpivoted_one():
    """What the SSIM bound is worth: the textbook formula in plain fp32 (no pivot) misses it on the bright flat class, on the frames
    of one or two windows, where no mean over thousands of map positions hides the cancellation."""
    from lvt_amd.evaluation import frame_quality_reference
    for L, shape in ((1.0, (1, 1, 11, 11)), (255.0, (1, 1, 11, 11)), (1.0, (2, 1, 11, 12)), (255.0, (2, 1, 11, 12))):
        a, b, _, ssim, e = case("bright_flat", shape, L)
        _, plain = frame_quality_reference(a, b, L, dtype=torch.float32)
        assert float((plain.double() - ssim).abs().max()) > max(4 * float(e.max()), SSIM_FLOOR)


@pytest.mark.parametrize("L", RANGES)
def test_squared_error_is_counted_once(L):
    from lvt_amd.hip import ew
    a, b, _, _, _ = case("noise", MULTI_TILE, L)
    ad, bd = a.cuda(), b.cuda()
    frames, _ = ew.frame_quality(ad, bd, L)
    per_frame = a[0].numel()
    total = float((L * L / 10 ** (frames[:, 0].cpu() / 10) * per_frame).sum())
    want = float(ew.mse_fwd(ad, bd, denom=1.0))
    assert abs(total - want) <= 1e-6 * want, (total, want)
    # and every frame on its own, against fp64
    sq = ((a.double() - b.double()) ** 2).sum(dim=(1, 2, 3))
    got = L * L / 10 ** (frames[:, 0].cpu() / 10) * per_frame
    assert torch.allclose(got, sq, rtol=1e-9, atol=0)


@pytest.mark.parametrize("shape", [MULTI_TILE, (3, 3, 64, 64), (1, 1, 11, 11)], ids=lambda s: "x".join(map(str, s)))
def test_identical_inputs(shape):
    from lvt_amd.hip import ew
    for L in RANGES:
        a = make_pair("noise", shape, L)[0].cuda()
        acc = torch.tensor([3.0, 2.0, 5.0, 7.0], dtype=torch.float64, device="cuda")
        frames, acc2 = ew.frame_quality(a, a.clone(), L, acc=acc)
        assert acc2 is acc
        frames, acc = frames.cpu(), acc.cpu()
        assert (frames[:, 1] == 1.0).all() and (frames[:, 0] == float("inf")).all()
        assert acc.tolist() == [3.0, 2.0 + shape[0], 5.0, 7.0 + shape[0]]      # finite count unchanged, frame count advanced


def test_deterministic_and_accumulating():
    from lvt_amd.hip import ew
    L = 1.0
    a, b, _, _, _ = case("noised_copy", MULTI_TILE, L)
    ad, bd = a.cuda(), b.cuda()
    f1, acc = ew.frame_quality(ad, bd, L)
    f2, _ = ew.frame_quality(ad, bd, L)
    assert torch.equal(f1.view(torch.int64), f2.view(torch.int64))                      # bit-identical
    c, d, _, _, _ = case("ramp_mirror", (5, 3, 17, 23), L)
    f3, acc = ew.frame_quality(c.cuda(), d.cuda(), L, acc=acc)
    f4, acc = ew.frame_quality(ad[0], bd[0], L, acc=acc)                                # (C, H, W): one frame
    assert tuple(f4.shape) == (1, 2) and torch.equal(f4[0], f1[0])                      # ... with the bits it has inside the clip
    allf = torch.cat([f1, f3, f4]).cpu()
    n = torch.tensor(float(allf.shape[0]), dtype=torch.float64)
    assert allf.shape[0] == MULTI_TILE[0] + 5 + 1 and torch.isfinite(allf).all()
    want = torch.stack([allf[:, 0].sum(), allf[:, 1].sum(), n, n])
    assert torch.allclose(acc.cpu(), want, rtol=1e-12, atol=0), (acc.cpu(), want)


def test_refusals_launch_nothing():
    from lvt_amd.hip import ew
    from lvt_amd.hip.binding import LvtError
    z = torch.rand(2, 3, 16, 16, device="cuda")
    for a, b, L, F, why in ((z[:, :, :10].contiguous(), z[:, :, :10].contiguous(), 1.0, 2, "H=10"),
                            (z[..., :10].contiguous(), z[..., :10].contiguous(), 1.0, 2, "W=10"),
                            (z, z[:, :2].contiguous(), 1.0, 2, "shapes differ"), (z, z[:1], 1.0, 2, "shapes differ"),
                            (z, z, 0.0, 2, "data_range"), (z, z, -2.0, 2, "data_range"), (z, z, float("nan"), 2, "data_range"),
                            (z, z, float("inf"), 2, "data_range")):
        frames = torch.full((F, 2), float("nan"), dtype=torch.float64, device="cuda")
        acc = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
        with pytest.raises(LvtError, match=why):
            ew.frame_quality(a, b, L, acc=acc, frames=frames)
        torch.cuda.synchronize()
        assert torch.isnan(frames).all() and torch.isnan(acc).all(), why
    with pytest.raises(LvtError):
        ew.frame_quality(z.cpu(), z.cpu(), 1.0)                   # no CPU fallback behind the device op
    with pytest.raises(LvtError):
        ew.frame_quality(z.double(), z.double(), 1.0)


def test_evaluator_end_to_end():
    """tools/train_net.py --eval-only with TEST.EVALUATORS "MSEEvaluator,FrameQualityEvaluator": the reported means are those of
    frame_quality_reference over the reconstructions the model returns, and the MSE is what MSEEvaluator alone reports."""
    import seeded
    from lvt_amd.evaluation import DatasetEvaluators, build_evaluator, frame_quality_reference, inference_on_dataset
    from util_models import vqvae_seeded
    model, _, _, _ = vqvae_seeded(11, scale=0.05)
    cfg = model.cfg
    clips = [seeded.seeded_input("fq%d" % i, (16, 3, 64, 64), 11) for i in range(3)]
    loader = [[{"image_sequence": clips[i].numpy(), "video_idx": i}] for i in range(3)]
    cfg.TEST.EVALUATORS = "MSEEvaluator,FrameQualityEvaluator"
    ev = build_evaluator(cfg, "bair_test_seq")
    assert isinstance(ev, DatasetEvaluators)
    res = inference_on_dataset(model, loader, ev)
    cfg.TEST.EVALUATORS = "MSEEvaluator"
    alone = inference_on_dataset(model, loader, build_evaluator(cfg, "bair_test_seq"))
    assert res["reconstruction"]["MSE"] == alone["reconstruction"]["MSE"]
    # second pass: the reconstructions themselves
    model.eval()
    with torch.no_grad():
        recs = torch.cat([model(batch)[0]["reconstruction"].cpu() for batch in loader])
    tgt = torch.cat(clips)
    assert tuple(recs.shape) == (48, 3, 64, 64)
    psnr, ssim = frame_quality_reference(recs, tgt, 1.0)
    e = (ssim_fp32_pivoted(recs, tgt, 1.0) - ssim).abs()
    fq = res["frame_quality"]
    print("frame_quality end to end:", fq, "reference PSNR %.6f SSIM %.8f" % (float(psnr.mean()), float(ssim.mean())))
    assert fq["frames"] == 48 and fq["identical_frames"] == 0 and torch.isfinite(psnr).all()
    assert abs(fq["PSNR"] - float(psnr.mean())) <= PSNR_TOL_DB
    assert abs(fq["SSIM"] - float(ssim.mean())) <= float(torch.clamp(4 * e, min=SSIM_FLOOR).mean())
    assert math.isfinite(fq["SSIM"]) and 0 < fq["SSIM"] < 1
