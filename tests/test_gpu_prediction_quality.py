"""Best-of-N quality of sampled videos on the device (csrc/quality.hip lvt_frame_quality_vs + lvt_prediction_select through
ew.prediction_quality, VQVAEModel.decode_pixels, PredictionQualityEvaluator) against `prediction_quality_reference` in fp64 on the
CPU.

Bounds (set before the kernels ran):
  per-frame table  the bounds of tests/test_gpu_frame_quality.py, imported from it: SSIM within max(4 e, SSIM_FLOOR) with e the
                   error of `ssim_fp32_pivoted`, PSNR within PSNR_TOL_DB -- the compare kernel is that file's kernel.
  best             equal to the reference's for every case, nothing exempted: the inputs give sample s the noise 0.02 (1 + order[s]) L,
                   and the reference's gap between the best and the second score (asserted first: >= 1 dB, >= 1e-3 SSIM) is three
                   orders above the per-frame bounds.
  curves           the rule recomputed in fp64 on the CPU from the kernel's OWN table, rtol 1e-12: the selection adds nothing but
                   fp64 sums in stated orders.
Shapes (S, T, C, H, W, n_prime): one window and one sample; two samples of two frames; partial tiles with an odd S; full and
partial 16 x 32 tiles along both axes; the shipped frame with the shipped priming length.  Each also with `chunk_frames` set so
that the samples split into several compare launches (where S > 1), which must not change a bit."""
import os

import pytest
import torch

from test_gpu_frame_quality import PSNR_TOL_DB, SSIM_FLOOR, make_pair, ssim_fp32_pivoted

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 11, 11, 0), (2, 2, 1, 11, 12, 1), (3, 4, 3, 17, 45, 1), (5, 3, 3, 75, 43, 0), (4, 16, 3, 64, 64, 14)]
RANGES = (1.0, 255.0)
_ids = lambda s: "x".join(map(str, s))


def make_clip(shape, L, seed=0):
    """(samples (S, T, C, H, W), target (T, C, H, W)) float32 on the CPU: target = L rand, sample s = clamp(target + sigma_s L randn, 0, L)
    with sigma_s = 0.02 (1 + order[s]); order[s] = (3 s + 1) % S, or S - 1 - s when 3 divides S: the best sample is not sample 0."""
    S, T, C, H, W, _ = shape
    g = torch.Generator().manual_seed(7000 + 100 * seed + 10 * S + W)
    target = L * torch.rand((T, C, H, W), generator=g)
    order = [(3 * s + 1) % S if S % 3 else S - 1 - s for s in range(S)]
    samples = torch.stack([(target + 0.02 * (1 + order[s]) * L * torch.randn(target.shape, generator=g)).clamp(0, L) for s in range(S)])
    return samples.float().contiguous(), target.float().contiguous(), order


_cache = {}


def case(shape, L):
    """(samples, target, order, psnr64, ssim64, best64, curves64, e) of a case, computed once and shared (read-only)."""
    key = (shape, L)
    if key not in _cache:
        from lvt_amd.evaluation import prediction_quality_reference
        samples, target, order = make_clip(shape, L)
        psnr, ssim, best, curves = prediction_quality_reference(samples, target, shape[5], L)
        S, T = shape[:2]
        e = (ssim_fp32_pivoted(samples.flatten(0, 1), target.repeat(S, 1, 1, 1), L).view(S, T) - ssim).abs()
        _cache[key] = (samples, target, order, psnr, ssim, best, curves, e)
    return _cache[key]


def _rule(frames, S, T, n_prime):
    """The selection rule in fp64 on the CPU from a device table (S * T, 2)."""
    from lvt_amd.evaluation.quality import prediction_select_reference
    t = frames.cpu().view(S, T, 2)
    return prediction_select_reference(t[..., 0], t[..., 1], n_prime)


def _bits(x):
    return x.contiguous().view(torch.int64)


@pytest.mark.parametrize("L", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_against_fp64(shape, L):
    from lvt_amd.hip import ew
    S, T, C, H, W, n_prime = shape
    samples, target, order, psnr, ssim, best, curves, e = case(shape, L)
    # the reference's own gaps first: what makes `best` a fair demand
    steps = T - n_prime
    for name, score, need in (("psnr", psnr[:, n_prime:].sum(1) / steps, 1.0), ("ssim", ssim[:, n_prime:].sum(1) / steps, 1e-3)):
        top = score.sort(descending=True).values
        if S > 1:
            print("prediction_quality %s L=%g: reference %s gap %.4g" % (shape, L, name, float(top[0] - top[1])))
            assert float(top[0] - top[1]) >= need, (name, top)
    assert best.tolist() == [order.index(0)] * 2 and (S == 1 or best[0] != 0)
    assert torch.isfinite(psnr).all()

    frames, got_best, got_curves = ew.prediction_quality(samples.cuda(), target.cuda(), n_prime, L)
    assert frames.dtype == torch.float64 and tuple(frames.shape) == (S * T, 2) and frames.is_cuda
    assert got_best.dtype == torch.int32 and tuple(got_best.shape) == (2,) and got_best.is_cuda
    assert got_curves.dtype == torch.float64 and tuple(got_curves.shape) == (T, 8) and got_curves.is_cuda
    table = frames.cpu().view(S, T, 2)
    d_psnr, d_ssim = (table[..., 0] - psnr).abs(), (table[..., 1] - ssim).abs()
    print("prediction_quality %s L=%g: |ssim - fp64| %.3g (e %.3g, bound %.3g)  |psnr - fp64| %.3g dB"
          % (shape, L, float(d_ssim.max()), float(e.max()), max(4 * float(e.max()), SSIM_FLOOR), float(d_psnr.max())))
    assert bool((d_ssim <= torch.clamp(4 * e, min=SSIM_FLOOR)).all()), (d_ssim, e)
    assert bool((d_psnr <= PSNR_TOL_DB).all()), d_psnr
    assert got_best.cpu().tolist() == best.tolist()
    rule_best, rule_curves = _rule(frames, S, T, n_prime)
    assert got_best.cpu().tolist() == rule_best.tolist()
    assert (got_curves[:n_prime] == 0).all()
    assert torch.allclose(got_curves.cpu(), rule_curves, rtol=1e-12, atol=0), (got_curves.cpu(), rule_curves)
    assert (got_curves[n_prime:, 6] == 1).all() and (got_curves[n_prime:, 7] == S).all()

    # several compare launches: whole samples per chunk, the same bits
    chunk = T * max(1, S // 2)
    f2, b2, c2 = ew.prediction_quality(samples.cuda(), target.cuda(), n_prime, L, chunk_frames=chunk)
    assert torch.equal(_bits(f2), _bits(frames)) and torch.equal(_bits(c2), _bits(got_curves)) and torch.equal(b2, got_best)
    f3, b3, c3 = ew.prediction_quality(samples.cuda(), target.cuda(), n_prime, L, chunk_frames=1)      # below T: one sample per chunk
    assert torch.equal(_bits(f3), _bits(frames)) and torch.equal(_bits(c3), _bits(got_curves)) and torch.equal(b3, got_best)


def _compare_vs(a, b, F, Fb, L):
    """lvt_frame_quality_vs + lvt_frame_quality_finish through the C ABI -> (frames (F, 2), a fresh acc (4,))."""
    from lvt_amd.hip import binding as B
    Cc, H, W = a.shape[-3:]
    n = B.lib().lvt_frame_quality_partials(Cc, H, W)
    ws = torch.empty(F * n * 2, dtype=torch.float64, device="cuda")
    frames = torch.empty(F, 2, dtype=torch.float64, device="cuda")
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    B.check(B.lib().lvt_frame_quality_vs(B.ptr(a), B.ptr(b), F, Fb, Cc, H, W, L, B.ptr(ws), n, B.stream_ptr()), "lvt_frame_quality_vs")
    B.check(B.lib().lvt_frame_quality_finish(B.ptr(ws), F, Cc, H, W, L, n, B.ptr(frames), B.ptr(acc), B.stream_ptr()), "finish")
    return frames, acc


@pytest.mark.parametrize("L", RANGES)
def test_bit_identity(L):
    from lvt_amd.hip import ew
    # Fb == F: the bits of lvt_frame_quality, on the multi-tile shape of the frame-quality tests
    a, b = (t.cuda() for t in make_pair("noised_copy", (4, 3, 75, 43), L))
    want_f, want_acc = ew.frame_quality(a, b, L)
    got_f, got_acc = _compare_vs(a, b, 4, 4, L)
    assert torch.equal(_bits(got_f), _bits(want_f)) and torch.equal(_bits(got_acc), _bits(want_acc))
    # the broadcast compare: the bits of lvt_frame_quality on S copies of the target
    for shape in ((3, 4, 3, 17, 45, 1), (5, 3, 3, 75, 43, 0)):
        S, T = shape[:2]
        samples, target = case(shape, L)[:2]
        sd, td = samples.cuda(), target.cuda()
        want_f, want_acc = ew.frame_quality(sd.flatten(0, 1), td.repeat(S, 1, 1, 1), L)
        got_f, got_acc = _compare_vs(sd, td, S * T, T, L)
        assert torch.equal(_bits(got_f), _bits(want_f)) and torch.equal(_bits(got_acc), _bits(want_acc))
        f1, b1, c1 = ew.prediction_quality(sd, td, shape[5], L)
        f2, b2, c2 = ew.prediction_quality(sd, td, shape[5], L)
        assert torch.equal(_bits(f1), _bits(want_f))
        assert torch.equal(_bits(f1), _bits(f2)) and torch.equal(b1, b2) and torch.equal(_bits(c1), _bits(c2))


def test_duplicate_sample_ties_to_the_lowest_index():
    from lvt_amd.hip import ew
    shape, L = (3, 4, 3, 17, 45, 1), 1.0
    samples, target, order = case(shape, L)[:3]
    assert order == [2, 1, 0]
    dup = samples.clone()
    dup[0] = samples[2]                              # the best sample now sits at 0 and, bit for bit, at 2
    frames, best, curves = ew.prediction_quality(dup.cuda(), target.cuda(), 1, L)
    table = frames.view(3, 4, 2)
    assert torch.equal(_bits(table[0]), _bits(table[2]))
    assert best.cpu().tolist() == [0, 0]
    rule_best, rule_curves = _rule(frames, 3, 4, 1)
    assert rule_best.tolist() == [0, 0] and torch.allclose(curves.cpu(), rule_curves, rtol=1e-12, atol=0)
    # and where the pair is not the best, the tie is not what decides
    dup = samples.clone()
    dup[1] = samples[0]                              # samples 0 and 1: the noisiest, twice; sample 2 stays the best
    _, best, _ = ew.prediction_quality(dup.cuda(), target.cuda(), 1, L)
    assert best.cpu().tolist() == [2, 2]


class _TableVQVAE:
    """`decode_pixels` as a lookup of a frame's first code in a table of device frames."""
    encoder = generator = codebook = None

    def __init__(self, table):
        self.table = table

    def set_generator_requires_grad(self, flag):
        pass

    def eval(self):
        return self

    def decode_pixels(self, codes):
        return self.table[codes.reshape(codes.shape[0], -1)[:, 0].to(self.table.device)]


def test_identical_best_frame():
    """The noisiest sample reproduces one predicted frame exactly: its PSNR score is +inf, it is the best PSNR sample, the frame
    is left out of columns 0 and 1, nothing is NaN; and the evaluator counts it as an identical best frame."""
    from lvt_amd.evaluation import PredictionQualityEvaluator, prediction_quality_reference
    from lvt_amd.hip import ew
    from util_models import ROOT, dsfvt_cfg
    shape, L = (3, 4, 3, 17, 45, 1), 1.0
    samples, target, order = case(shape, L)[:3]
    samples = samples.clone()
    samples[0, 2] = target[2]
    psnr, ssim, best, curves = prediction_quality_reference(samples, target, 1, L)
    assert best.tolist() == [0, 2] and psnr[0, 2] == float("inf")
    frames, got_best, got_curves = ew.prediction_quality(samples.cuda(), target.cuda(), 1, L)
    table = frames.cpu().view(3, 4, 2)
    assert got_best.cpu().tolist() == [0, 2]
    assert table[0, 2, 0] == float("inf") and table[0, 2, 1] == 1.0 and not torch.isnan(table).any()
    got_curves = got_curves.cpu()
    assert torch.isfinite(got_curves).all()
    assert got_curves[2, :2].tolist() == [0.0, 0.0] and got_curves[2, 4] == 2.0
    assert got_curves[1, :2].tolist() == [float(table[0, 1, 0]), 1.0] and got_curves[3, :2].tolist() == [float(table[0, 3, 0]), 1.0]
    assert torch.allclose(got_curves, _rule(frames, 3, 4, 1)[1], rtol=1e-12, atol=0)
    assert torch.allclose(got_curves, curves, rtol=0, atol=PSNR_TOL_DB * 3)           # (sums of three values each within the bounds)

    # through the evaluator: the frames as a lookup table, codes = indices into it
    cfg = dsfvt_cfg()
    cfg.TEST.VT_SAMPLER.N_PRIME = 1
    vs = cfg.TEST.VT_SAMPLER.VQ_VAE
    vs.CFG = os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml")
    vs.ENCODER_WEIGHTS = vs.GENERATOR_WEIGHTS = vs.CODEBOOK_WEIGHTS = ""
    stub = _TableVQVAE(torch.cat([target, samples.flatten(0, 1)]).cuda())             # rows 0..3 the target, 4 + 4 s + t the samples
    ev = PredictionQualityEvaluator(cfg, "d", distributed=False, vqvae=stub)
    ev.reset()
    codes = torch.arange(4).view(4, 1, 1, 1).expand(4, 2, 1, 1).contiguous()
    outs = [(4 + 4 * s + torch.arange(4)).view(1, 4, 1, 1).expand(2, 4, 1, 1).contiguous() for s in range(3)]
    ev.process([{"image_sequence": codes.numpy()}], [{"samples": outs}])
    assert ev._acc.is_cuda and torch.equal(_bits(ev._acc), _bits(got_curves.cuda()))
    res = ev.evaluate()["prediction_quality"]
    assert res["identical_best_frames"] == 1 and res["clips"] == 1 and res["samples"] == 3 and res["per_frame"]["t"] == [1, 2, 3]
    assert res["per_frame"]["PSNR_best"][1] != res["per_frame"]["PSNR_best"][1]       # no finite best PSNR at t = 2: nan, not inf
    assert res["per_frame"]["SSIM_best"] == [float(table[2, t, 1]) for t in (1, 2, 3)]
    assert abs(res["PSNR_best"] - float((table[0, 1, 0] + table[0, 3, 0]) / 2)) <= 1e-12 * res["PSNR_best"]


def test_accumulating_over_clips():
    from lvt_amd.hip import ew
    L = 255.0
    a, b = (3, 4, 3, 17, 45, 1), (3, 4, 3, 17, 45, 1)
    s1, t1 = (x.cuda() for x in case(a, L)[:2])
    s2, t2 = (x.cuda() for x in make_clip(b, L, seed=1)[:2])
    _, _, c1 = ew.prediction_quality(s1, t1, 1, L)
    _, _, c2 = ew.prediction_quality(s2, t2, 1, L)
    acc = torch.zeros(4, 8, dtype=torch.float64, device="cuda")
    _, _, r1 = ew.prediction_quality(s1, t1, 1, L, curves=acc)
    _, _, r2 = ew.prediction_quality(s2, t2, 1, L, curves=acc)
    assert r1 is acc and r2 is acc
    assert torch.allclose(acc, c1 + c2, rtol=1e-12, atol=0)
    assert (acc[0] == 0).all() and (acc[1:, 6] == 2).all() and (acc[1:, 7] == 6).all()


def test_refusals_launch_nothing():
    from lvt_amd.hip import binding as B, ew
    from lvt_amd.hip.binding import LvtError
    # F % Fb != 0 through the C entry
    z = torch.rand(6, 3, 16, 16, device="cuda")
    n = B.lib().lvt_frame_quality_partials(3, 16, 16)
    ws = torch.full((6 * n * 2,), float("nan"), dtype=torch.float64, device="cuda")
    for F, Fb in ((6, 4), (6, 5), (5, 2), (6, 0), (3, 6)):
        rc = B.lib().lvt_frame_quality_vs(B.ptr(z), B.ptr(z), F, Fb, 3, 16, 16, 1.0, B.ptr(ws), n, B.stream_ptr())
        assert rc == -1 and b"multiple of Fb" in B.lib().lvt_last_error(), (F, Fb)
    torch.cuda.synchronize()
    assert torch.isnan(ws).all()
    # through ew.prediction_quality
    s, t = torch.rand(2, 3, 3, 16, 16, device="cuda"), torch.rand(3, 3, 16, 16, device="cuda")
    pattern = torch.arange(24, dtype=torch.float64, device="cuda").view(3, 8) + 0.5
    for samples, target, n_prime, L, curves, why in (
            (s, t, -1, 1.0, None, "n_prime"), (s, t, 3, 1.0, None, "n_prime"), (s, t, 17, 1.0, None, "n_prime"),
            (s, t[:2].contiguous(), 0, 1.0, None, "shapes differ"), (s, t[:, :2].contiguous(), 0, 1.0, None, "shapes differ"),
            (s[0], t, 0, 1.0, None, "shapes differ"), (s, t[0], 0, 1.0, None, "shapes differ"),
            (s.double(), t.double(), 0, 1.0, None, "float32"), (s, t.half(), 0, 1.0, None, "float32"),
            (s[..., :10, :].contiguous(), t[..., :10, :].contiguous(), 0, 1.0, None, "H=10"),
            (s[..., :10].contiguous(), t[..., :10].contiguous(), 0, 1.0, None, "W=10"),
            (s, t, 0, 0.0, None, "data_range"), (s, t, 0, float("nan"), None, "data_range"), (s, t, 0, float("inf"), None, "data_range"),
            (s, t, 0, 1.0, torch.zeros(2, 8, dtype=torch.float64, device="cuda"), "curves"),
            (s, t, 0, 1.0, torch.zeros(8, 3, dtype=torch.float64, device="cuda"), "curves"),
            (s, t, 0, 1.0, torch.zeros(3, 8, dtype=torch.float32, device="cuda"), "curves"),
            (s, t, 0, 1.0, torch.zeros(3, 8, dtype=torch.float64), "MI355X")):
        acc = pattern.clone() if curves is None else curves
        before = acc.clone()
        with pytest.raises(LvtError, match=why):
            ew.prediction_quality(samples, target, n_prime, L, curves=acc)
        torch.cuda.synchronize()
        assert torch.equal(acc, before), why
    with pytest.raises(LvtError):
        ew.prediction_quality(s.cpu(), t.cpu(), 0, 1.0)                   # no CPU fallback behind the device op
    with pytest.raises(LvtError, match="chunk_frames"):
        ew.prediction_quality(s, t, 0, 1.0, chunk_frames=0)


def test_decode_pixels():
    """`decode_pixels(codes)` is `back_normalizer(decode(codes))` clamped to [0, hi], on the route the `inference` mode ends with:
    PSNR / SSIM of both against the frames the codes were taken from agree within the bounds
    tests/test_gpu_frame_quality.py::test_evaluator_end_to_end gives that route (PSNR_TOL_DB; max(4 e, SSIM_FLOOR))."""
    import seeded
    from lvt_amd.evaluation import frame_quality_reference
    from util_models import vqvae_seeded
    model, _, _, _ = vqvae_seeded(11, scale=0.05)
    model.eval()
    clip = seeded.seeded_input("dp0", (16, 3, 64, 64), 11)
    with torch.no_grad():
        codes = model([{"image_sequence": clip.numpy()}])[0]["latent"]
        assert tuple(codes.shape) == (16, 4, 16, 16) and codes.dtype == torch.int64
        got = model.decode_pixels(codes)
        want = model.back_normalizer(model.decode(codes)).clamp(0.0, 1.0)
    assert model.cfg.INPUT.SCALE_TO_ZEROONE and got.dtype == torch.float32 and tuple(got.shape) == (16, 3, 64, 64)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    got, want = got.cpu(), want.cpu()
    p1, s1 = frame_quality_reference(got, clip, 1.0)
    p2, s2 = frame_quality_reference(want, clip, 1.0)
    e = (ssim_fp32_pivoted(want, clip, 1.0) - s2).abs()
    print("decode_pixels: max |pixel difference| %.3g, |psnr| %.3g dB, |ssim| %.3g"
          % (float((got - want).abs().max()), float((p1 - p2).abs().max()), float((s1 - s2).abs().max())))
    assert bool(((p1 - p2).abs() <= PSNR_TOL_DB).all())
    assert bool(((s1 - s2).abs() <= torch.clamp(4 * e, min=SSIM_FLOOR)).all())
    # 255 scale: the same frames times 255, and the single-frame call
    model.cfg.INPUT.SCALE_TO_ZEROONE = False
    try:
        with torch.no_grad():
            big = model.decode_pixels(codes[:1])
            want255 = model.back_normalizer(model.decode(codes[:1])).clamp(0.0, 255.0)
    finally:
        model.cfg.INPUT.SCALE_TO_ZEROONE = True
    assert tuple(big.shape) == (1, 3, 64, 64) and float(big.min()) >= 0.0 and float(big.max()) <= 255.0
    p3, s3 = frame_quality_reference(big.cpu(), want255.cpu() + 0.0, 255.0)
    assert float(p3) >= 10 * 14.0 and abs(float(s3) - 1.0) <= SSIM_FLOOR              # equal to 1e-7 of the range (mse <= 1e-14 L^2), or identical


# ---- end to end -------------------------------------------------------------------------------------------------------------------
SEED = 21          # of the transformer's seeded weights, the clip's codes and torch's generator (see test_evaluator_end_to_end)
_e2e = {}


def _setup(tmp_path, seed=SEED):
    """DSFVT with seeded weights, PR-DVQVAE2 with initialised weights, NUM_SAMPLES 2, N_PRIME 14, one clip of seeded codes."""
    import seeded
    from lvt_amd.modeling import build_model
    from util_models import ROOT, dsfvt_cfg
    if seed not in _e2e:
        cfg = dsfvt_cfg()
        cfg.TEST.EVALUATORS = "PredictionQualityEvaluator"
        cfg.TEST.VT_SAMPLER.NUM_SAMPLES = 2
        cfg.TEST.VT_SAMPLER.N_PRIME = 14
        vs = cfg.TEST.VT_SAMPLER.VQ_VAE
        vs.CFG = os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml")
        vs.ENCODER_WEIGHTS = vs.GENERATOR_WEIGHTS = vs.CODEBOOK_WEIGHTS = ""
        model = build_model(cfg)
        model.model.load_state_dict(seeded.seeded_params(seeded.dsfvt_shapes(), seed), strict=False)
        _e2e[seed] = (cfg, model, seeded.seeded_codes("pq", (16, 4, 16, 16), seed))
    _e2e[seed][0].OUTPUT_DIR = str(tmp_path)
    return _e2e[seed]


def end_to_end(tmp_path, seed=SEED):
    """One `inference_on_dataset` with "PredictionQualityEvaluator" -> (the report, the evaluator, and the reference's psnr, ssim,
    best on `decode_pixels` of the captured samples and of the input codes, decoded in the evaluator's own batches)."""
    from lvt_amd.evaluation import PredictionQualityEvaluator, build_evaluator, inference_on_dataset, prediction_quality_reference
    cfg, model, codes = _setup(tmp_path, seed)
    cfg.TEST.EVALUATORS = "PredictionQualityEvaluator"
    torch.manual_seed(seed)                          # the VQ-VAE's initialised weights and the sampler's draws
    ev = build_evaluator(cfg, "prdvqvae_test")
    assert isinstance(ev, PredictionQualityEvaluator)
    captured, orig = [], model.sample_videos

    def wrapped(data, output, **kw):
        out = orig(data, output, **kw)
        captured.append([[s.clone() for s in o["samples"]] for o in out])
        return out

    model.sample_videos = wrapped
    try:
        res = inference_on_dataset(model, [[{"image_sequence": codes, "video_idx": 7}]], ev)["prediction_quality"]
    finally:
        del model.sample_videos
    assert len(captured) == 1 and len(captured[0]) == 1 and len(captured[0][0]) == 2
    stacked = torch.cat([s.transpose(0, 1) for s in captured[0][0]]).contiguous()        # (2 * 16, 4, 16, 16)
    assert torch.equal(stacked.view(2, 16, 4, 16, 16)[:, :14].cpu(), codes[:14].expand(2, 14, 4, 16, 16))
    with torch.no_grad():
        target = ev.vqvae.decode_pixels(codes).cpu()
        samples = ev.vqvae.decode_pixels(stacked).cpu().view(2, 16, 3, 64, 64)
    psnr, ssim, best, _ = prediction_quality_reference(samples, target, 14, 1.0)
    gap_p = float((psnr[:, 14:].sum(1) / 2).sort().values.diff())
    gap_s = float((ssim[:, 14:].sum(1) / 2).sort().values.diff())
    print("prediction_quality end to end (seed %d):" % seed, res, "reference best", best.tolist(), "gaps %.4g dB %.4g" % (gap_p, gap_s))
    return res, ev, samples, target, psnr, ssim, best, gap_p, gap_s


def test_evaluator_end_to_end(tmp_path):
    """The report of one `inference_on_dataset` against the reference on the same decoded pixels: per-step SSIM within 1e-5, PSNR
    within PSNR_TOL_DB, and `best` equal where the reference's gap between the two samples' scores exceeds those tolerances.
    An initialised PR-DVQVAE2 decoder renders nearly constant frames (PSNR 79 dB, SSIM 0.99998 between any two decodes), so the
    gaps are small.  Measured, reference alone, seeds 21 / 22 / 23: PSNR gap 0.103 / 0.046 / 0.020 dB (all above 1e-4 dB: seed
    21, the first, is fixed and `best[0]` is demanded); SSIM gap 3.2e-7 / 1.6e-7 / 1.2e-7 -- none of the three exceeds 1e-5, so
    `best[1]` is demanded only under the proviso, which these weights do not meet; the SSIM figures themselves are held to 1e-5
    either way, and the choice by SSIM is demanded without proviso in test_against_fp64 (gaps >= 4.7e-3)."""
    res, ev, samples, target, psnr, ssim, best, gap_p, gap_s = end_to_end(tmp_path)
    assert torch.isfinite(psnr[:, 14:]).all() and torch.isinf(psnr[:, :14]).all()        # the priming frames are the target's own
    assert gap_p > PSNR_TOL_DB, "the reference's PSNR gap does not exceed the tolerance: take the next seed"
    assert res["per_frame"]["t"] == [14, 15] and res["clips"] == 1 and res["samples"] == 2 and res["n_prime"] == 14
    assert res["identical_best_frames"] == 0 and res["target"] == "decoded_codes"
    bp, bs = best.tolist()
    for i, t in enumerate((14, 15)):
        assert abs(res["per_frame"]["PSNR_best"][i] - float(psnr[bp, t])) <= PSNR_TOL_DB       # (which also says WHICH sample was chosen)
        assert abs(res["per_frame"]["SSIM_best"][i] - float(ssim[bs, t])) <= 1e-5
        assert abs(res["per_frame"]["PSNR_mean"][i] - float(psnr[:, t].mean())) <= PSNR_TOL_DB
        assert abs(res["per_frame"]["SSIM_mean"][i] - float(ssim[:, t].mean())) <= 1e-5
    assert abs(res["PSNR_best"] - float(psnr[bp, 14:].mean())) <= PSNR_TOL_DB and abs(res["SSIM_best"] - float(ssim[bs, 14:].mean())) <= 1e-5
    assert abs(res["PSNR_mean"] - float(psnr[:, 14:].mean())) <= PSNR_TOL_DB and abs(res["SSIM_mean"] - float(ssim[:, 14:].mean())) <= 1e-5
    # `best` itself, from the device op on the same pixels
    from lvt_amd.hip import ew
    frames, got_best, _ = ew.prediction_quality(samples.cuda(), target.cuda(), 14, 1.0)
    assert int(got_best[0]) == bp and (gap_s <= 1e-5 or int(got_best[1]) == bs)
    assert got_best.cpu().tolist() == _rule(frames, 2, 16, 14)[0].tolist()
    assert os.path.exists(os.path.join(str(tmp_path), "inference", "prediction_quality_prdvqvae_test.json"))


def test_one_sampling_pass_feeds_both_evaluators(tmp_path):
    from lvt_amd.evaluation import DatasetEvaluators, build_evaluator, inference_on_dataset
    cfg, model, codes = _setup(tmp_path)
    cfg.TEST.EVALUATORS = "VTSampler,PredictionQualityEvaluator"
    try:
        ev = build_evaluator(cfg, "prdvqvae_test")
        assert isinstance(ev, DatasetEvaluators)
        calls, orig = [], model.sample_video

        def counted(*a, **kw):
            calls.append(1)
            return orig(*a, **kw)

        model.sample_video = counted
        try:
            res = inference_on_dataset(model, [[{"image_sequence": codes, "video_idx": 7}]], ev)
        finally:
            del model.sample_video
    finally:
        cfg.TEST.EVALUATORS = "PredictionQualityEvaluator"
    assert len(calls) == cfg.TEST.VT_SAMPLER.NUM_SAMPLES == 2
    assert res["prediction_quality"]["samples"] == 2
    root = os.path.join(str(tmp_path), "inference", "samples", "prdvqvae_test")
    assert sorted(os.listdir(root)) == ["video_0_7", "video_1_7"]
