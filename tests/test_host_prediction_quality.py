"""Host side of the best-of-N prediction quality: the rule of `prediction_quality_reference` on hand-made tables of
per-frame values and on tiny frames, its refusals, PredictionQualityEvaluator on CPU tensors with a stub VQ-VAE (alone, its JSON
file, under two gloo ranks), build_evaluator's dispatch, and the C-ABI table and argument validation of the two new entries
(which comes before any device work, so it runs without a GPU)."""
import ctypes
import json
import math
import os

import pytest
import torch

from conftest import ROOT
from test_dp_gloo import _run
from test_host_frame_quality import _header_signature

INF, NAN = float("inf"), float("nan")
NEW = ("lvt_frame_quality_vs", "lvt_prediction_select")


# ---- the rule on hand-made tables ------------------------------------------------------------------------------------------------
def _on_tables(monkeypatch, psnr, ssim, n_prime):
    """prediction_quality_reference with the per-frame values given: sample s is a frame stack filled with s, and the patched
    per-frame function looks its rows up."""
    from lvt_amd.evaluation import quality
    psnr, ssim = torch.tensor(psnr, dtype=torch.float64), torch.tensor(ssim, dtype=torch.float64)
    S, T = psnr.shape
    monkeypatch.setattr(quality, "frame_quality_reference", lambda a, b, L, dtype=torch.float64: (psnr[int(a[0, 0, 0, 0])],
                                                                                                   ssim[int(a[0, 0, 0, 0])]))
    samples = torch.arange(S, dtype=torch.float32).view(S, 1, 1, 1, 1).expand(S, T, 1, 11, 11)
    p, q, best, curves = quality.prediction_quality_reference(samples, torch.zeros(T, 1, 11, 11), n_prime, 1.0)
    assert torch.allclose(p, psnr, rtol=0, atol=0, equal_nan=True) and torch.allclose(q, ssim, rtol=0, atol=0, equal_nan=True)
    assert best.dtype == torch.int64 and curves.dtype == torch.float64 and tuple(curves.shape) == (T, 8)
    return best.tolist(), curves


def test_each_metric_chooses_its_own_sample(monkeypatch):
    psnr = [[20.0, 21.0, 22.0], [30.0, 10.0, 40.0], [20.0, 25.0, 24.0]]          # means over t >= 1: 21.5, 25, 24.5
    ssim = [[0.5, 0.9, 0.8], [0.9, 0.1, 0.2], [0.1, 0.7, 0.9]]                   # 0.85, 0.15, 0.8
    best, curves = _on_tables(monkeypatch, psnr, ssim, 1)
    assert best == [1, 0]
    assert curves[0].tolist() == [0.0] * 8                                       # the priming row is exactly 0
    assert curves[1].tolist() == [10.0, 1.0, 0.9, 21.0 + 10.0 + 25.0, 3.0, 0.9 + 0.1 + 0.7, 1.0, 3.0]
    assert curves[2].tolist() == [40.0, 1.0, 0.8, 22.0 + 40.0 + 24.0, 3.0, 0.8 + 0.2 + 0.9, 1.0, 3.0]
    # with the priming frame counted, PSNR prefers sample 1 still (80 / 3) and SSIM sample 0 (2.2 / 3)
    best0, curves0 = _on_tables(monkeypatch, psnr, ssim, 0)
    assert best0 == [1, 0] and curves0[0].tolist() == [30.0, 1.0, 0.5, 70.0, 3.0, 0.5 + 0.9 + 0.1, 1.0, 3.0]
    assert torch.equal(curves0[1:], curves[1:])


def test_n_prime_bounds_and_zero_rows(monkeypatch):
    psnr = [[50.0, 1.0, 1.0, 2.0], [1.0, 9.0, 9.0, 1.0]]
    ssim = [[0.9, 0.1, 0.1, 0.3], [0.1, 0.8, 0.8, 0.2]]
    best, curves = _on_tables(monkeypatch, psnr, ssim, 3)                        # n_prime = T - 1: only the last step decides
    assert best == [0, 0]
    assert (curves[:3] == 0).all() and curves[3].tolist() == [2.0, 1.0, 0.3, 3.0, 2.0, 0.5, 1.0, 2.0]
    best, curves = _on_tables(monkeypatch, psnr, ssim, 0)                        # n_prime = 0: 54 / 4 against 20 / 4, 1.4 / 4 against 1.9 / 4
    assert best == [0, 1] and (curves[:, 6] == 1).all() and (curves[:, 7] == 2).all()
    assert curves[:, 0].tolist() == [50.0, 1.0, 1.0, 2.0] and curves[:, 2].tolist() == [0.1, 0.8, 0.8, 0.2]
    best, curves = _on_tables(monkeypatch, psnr, ssim, 1)                        # 4 / 3 against 19 / 3
    assert best == [1, 1] and (curves[0] == 0).all()


def test_equal_scores_resolve_to_the_lowest_index(monkeypatch):
    psnr = [[1.0, 10.0, 30.0], [1.0, 30.0, 10.0], [9.0, 20.0, 20.0], [1.0, 5.0, 5.0]]     # 20, 20, 20, 5
    ssim = [[0.0, 0.25, 0.25], [0.0, 0.5, 0.25], [0.0, 0.25, 0.5], [0.0, 0.5, 0.25]]      # .25, .375, .375, .375
    best, curves = _on_tables(monkeypatch, psnr, ssim, 1)
    assert best == [0, 1]
    assert curves[1, 0] == 10.0 and curves[2, 0] == 30.0 and curves[1, 2] == 0.5 and curves[2, 2] == 0.25


def test_an_identical_frame_wins_and_is_left_out_of_the_sums(monkeypatch):
    psnr = [[7.0, 40.0, 41.0, 42.0], [7.0, 12.0, INF, 14.0], [7.0, INF, INF, INF]]
    ssim = [[0.1, 0.9, 0.9, 0.9], [0.1, 0.2, 1.0, 0.3], [0.1, 1.0, 1.0, 1.0]]
    best, curves = _on_tables(monkeypatch, psnr, ssim, 1)
    assert best == [1, 2]                                                        # inf against inf: the lower index
    assert curves[1].tolist() == [12.0, 1.0, 1.0, 52.0, 2.0, 0.9 + 0.2 + 1.0, 1.0, 3.0]
    assert curves[2].tolist() == [0.0, 0.0, 1.0, 41.0, 1.0, 0.9 + 1.0 + 1.0, 1.0, 3.0]    # the identical best frame: not summed, not counted
    assert curves[3].tolist() == [14.0, 1.0, 1.0, 56.0, 2.0, 0.9 + 0.3 + 1.0, 1.0, 3.0]
    assert torch.isfinite(curves).all()


def test_a_nan_score_wins_only_among_nans(monkeypatch):
    best, _ = _on_tables(monkeypatch, [[NAN, NAN], [1.0, 2.0], [1.0, 3.0]], [[0.1, 0.1], [NAN, 0.2], [0.1, NAN]], 0)
    assert best == [2, 0]
    best, curves = _on_tables(monkeypatch, [[NAN, 1.0], [2.0, NAN]], [[NAN, 0.5], [NAN, 0.1]], 0)
    assert best == [0, 0]                                                        # every score NaN: sample 0
    assert curves[0, :2].tolist() == [0.0, 0.0] and curves[0, 3:5].tolist() == [2.0, 1.0] and math.isnan(float(curves[0, 2]))
    from lvt_amd.evaluation.quality import best_sample
    assert best_sample(torch.tensor([NAN, -INF, NAN])) == 1 and best_sample(torch.tensor([3.0])) == 0


def test_tiny_frames_and_the_per_frame_values():
    from lvt_amd.evaluation import frame_quality_reference, prediction_quality_reference
    g = torch.Generator().manual_seed(3)
    target = torch.rand(3, 2, 11, 12, generator=g)
    samples = torch.stack([(target + sg * torch.randn(target.shape, generator=g)).clamp(0, 1) for sg in (0.2, 0.05, 0.1)])
    samples[0, 2] = target[2]                                                    # the worst sample reproduces the last frame
    psnr, ssim, best, curves = prediction_quality_reference(samples, target, 1, 1.0)
    assert tuple(psnr.shape) == tuple(ssim.shape) == (3, 3) and psnr.dtype == torch.float64
    for s in range(3):
        p, q = frame_quality_reference(samples[s], target, 1.0)
        assert torch.equal(psnr[s], p) and torch.equal(ssim[s], q)
    assert psnr[0, 2] == INF and ssim[0, 2] == 1.0
    assert best.tolist() == [0, 1]                                               # inf + finite = inf wins PSNR; SSIM goes by the noise
    assert curves[2, :2].tolist() == [0.0, 0.0] and curves[1, 0] == psnr[0, 1] and curves[1, 1] == 1.0
    assert curves[2, 3] == psnr[1, 2] + psnr[2, 2] and curves[2, 4] == 2.0
    assert curves[1, 5] == (ssim[0, 1] + ssim[1, 1]) + ssim[2, 1] and (curves[0] == 0).all()
    p32 = prediction_quality_reference(samples, target, 1, 1.0, dtype=torch.float32)
    assert p32[0].dtype == torch.float32 and p32[3].dtype == torch.float64 and p32[2].tolist() == [0, 1]


def test_reference_refusals():
    from lvt_amd.evaluation import prediction_quality_reference
    s, t = torch.zeros(2, 3, 1, 12, 12), torch.zeros(3, 1, 12, 12)
    prediction_quality_reference(s + 0.5, t, 2, 1.0)
    for samples, target, n_prime, L in ((s[:0], t, 0, 1.0), (s, t, -1, 1.0), (s, t, 3, 1.0), (s, t, 7, 1.0), (s[0], t, 0, 1.0),
                                        (s, t[0], 0, 1.0), (s[..., :10, :], t[..., :10, :], 0, 1.0), (s[..., :10], t[..., :10], 0, 1.0),
                                        (s, t[:2], 0, 1.0), (s, t[:, :, :11], 0, 1.0), (s, t, 0, 0.0), (s, t, 0, -1.0),
                                        (s, t, 0, NAN), (s, t, 0, INF)):
        with pytest.raises(ValueError):
            prediction_quality_reference(samples, target, n_prime, L)


# ---- the evaluator on CPU tensors ------------------------------------------------------------------------------------------------
class _StubVQVAE:
    """`decode_pixels` as a seeded lookup table: a frame's first code picks one of 12 frames of 3 x 12 x 13 in [0, 1]."""
    encoder = generator = codebook = None

    def __init__(self):
        self.table = torch.rand(12, 3, 12, 13, generator=torch.Generator().manual_seed(5))
        self.calls = []

    def set_generator_requires_grad(self, flag):
        assert flag is False

    def eval(self):
        return self

    def decode_pixels(self, codes):
        assert codes.dtype == torch.int64 and codes.dim() in (3, 4)
        self.calls.append(codes.shape[0])
        return self.table[codes.reshape(codes.shape[0], -1)[:, 0]]


T_, S_, N_PRIME = 5, 3, 2


def _cfg(evaluators="PredictionQualityEvaluator"):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.DEVICE = "cpu"
    cfg.TEST.EVALUATORS = evaluators
    cfg.TEST.VT_SAMPLER.N_PRIME = N_PRIME
    cfg.TEST.VT_SAMPLER.NUM_SAMPLES = S_
    cfg.TEST.VT_SAMPLER.VQ_VAE.CFG = os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml")
    vs = cfg.TEST.VT_SAMPLER.VQ_VAE
    vs.ENCODER_WEIGHTS = vs.GENERATOR_WEIGHTS = vs.CODEBOOK_WEIGHTS = ""
    return cfg


def _clips(n, first=0):
    """Clips `first` .. `first + n - 1`: (input dict, output dict) with codes (T, 2, 1, 1) and S samples (2, T, 1, 1) that keep the
    priming frames; clip 1's sample 2 repeats the target's code at t = 3 (an identical frame)."""
    out = []
    for i in range(first, first + n):
        g = torch.Generator().manual_seed(40 + i)
        codes = torch.randint(0, 12, (T_, 2, 1, 1), generator=g)
        samples = []
        for s in range(S_):
            smp = torch.randint(0, 12, (T_, 2, 1, 1), generator=g)
            smp[:N_PRIME] = codes[:N_PRIME]
            clash = smp[N_PRIME:, 0] == codes[N_PRIME:, 0]                       # no identical frame by accident
            smp[N_PRIME:, 0] = torch.where(clash, (smp[N_PRIME:, 0] + 1) % 12, smp[N_PRIME:, 0])
            if i == 1 and s == 2:
                smp[3] = codes[3]
            samples.append(smp.transpose(0, 1).contiguous())
        out.append(({"image_sequence": codes.numpy(), "video_idx": i}, {"samples": samples}))
    return out


def _expected(clips):
    """The report, from prediction_quality_reference per clip and the column definitions."""
    from lvt_amd.evaluation import prediction_quality_reference
    table = _StubVQVAE().table
    curves = torch.zeros(T_, 8, dtype=torch.float64)
    for inp, out in clips:
        target = table[torch.as_tensor(inp["image_sequence"])[:, 0, 0, 0]]
        samples = torch.stack([table[s[0, :, 0, 0]] for s in out["samples"]])
        curves += prediction_quality_reference(samples, target, N_PRIME, 1.0)[3]
    r = curves[N_PRIME:]
    tot = r.sum(dim=0)
    return {"PSNR_best": float(tot[0] / tot[1]), "SSIM_best": float(tot[2] / tot[6]), "PSNR_mean": float(tot[3] / tot[4]),
            "SSIM_mean": float(tot[5] / tot[7]),
            "per_frame": {"t": list(range(N_PRIME, T_)), "PSNR_best": (r[:, 0] / r[:, 1]).tolist(), "SSIM_best": (r[:, 2] / r[:, 6]).tolist(),
                          "PSNR_mean": (r[:, 3] / r[:, 4]).tolist(), "SSIM_mean": (r[:, 5] / r[:, 7]).tolist()},
            "clips": len(clips), "samples": S_ * len(clips), "n_prime": N_PRIME, "identical_best_frames": int(tot[6] - tot[1]),
            "target": "decoded_codes"}


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b)


def _close(got, want):
    assert sorted(got.keys()) == sorted(want.keys())
    for k, w in want.items():
        if k == "per_frame":
            assert sorted(got[k].keys()) == sorted(w.keys()) and got[k]["t"] == w["t"]
            for name in ("PSNR_best", "SSIM_best", "PSNR_mean", "SSIM_mean"):
                assert len(got[k][name]) == len(w[name])
                assert all(_same(a, b) for a, b in zip(got[k][name], w[name])), name
        elif isinstance(w, float):
            assert _same(got[k], w), k
        else:
            assert got[k] == w, k


def _feed(ev, clips):
    for inp, out in clips:
        ev.process([inp], [out])


def test_build_evaluator_dispatch(tmp_path):
    from lvt_amd.evaluation import DatasetEvaluators, PredictionQualityEvaluator, VTSampler, build_evaluator
    cfg = _cfg()
    cfg.OUTPUT_DIR = str(tmp_path)
    ev = build_evaluator(cfg, "d", str(tmp_path))
    assert type(ev) is PredictionQualityEvaluator and ev._n_prime == N_PRIME and ev._data_range == 1.0
    assert type(ev.vqvae).__name__ == "VQVAEModel" and not ev.vqvae.training
    cfg.TEST.EVALUATORS = "VTSampler,PredictionQualityEvaluator"
    both = build_evaluator(cfg, "d", str(tmp_path))
    assert isinstance(both, DatasetEvaluators)
    assert [type(e) for e in both._evaluators] == [VTSampler, PredictionQualityEvaluator]
    cfg.TEST.EVALUATORS = "QualityEvaluator"                                     # a substring of two names, the name of none
    with pytest.raises(NotImplementedError):
        build_evaluator(cfg, "d", str(tmp_path))
    cfg.TEST.EVALUATORS = "PredictionQualityEvaluator"
    cfg.TEST.VT_SAMPLER.VQ_VAE.GENERATOR_WEIGHTS = os.path.join(str(tmp_path), "missing.pth")
    with pytest.raises(FileNotFoundError):                                       # the shared construction: as VTSampler refuses
        build_evaluator(cfg, "d", str(tmp_path))


def test_evaluator_equals_the_reference_summed_over_clips(tmp_path):
    from lvt_amd.evaluation import PredictionQualityEvaluator
    clips = _clips(3)
    want = _expected(clips)
    assert want["identical_best_frames"] == 1 and want["clips"] == 3 and want["samples"] == 9
    stub = _StubVQVAE()
    ev = PredictionQualityEvaluator(_cfg(), "bair", distributed=False, output_dir=str(tmp_path), vqvae=stub)
    assert ev.vqvae is stub
    ev.reset()
    _feed(ev, clips)
    assert stub.calls == [T_, S_ * T_] * 3                                       # the target, then every sample in one stacked call
    res = ev.evaluate()
    assert list(res.keys()) == ["prediction_quality"]
    _close(res["prediction_quality"], want)
    with open(os.path.join(str(tmp_path), "prediction_quality_bair.json")) as f:
        assert json.load(f) == res["prediction_quality"]
    # reset() forgets; without an output directory nothing is written
    ev2 = PredictionQualityEvaluator(_cfg(), "other", distributed=False, vqvae=stub)
    _feed(ev2, clips[:1])
    _close(ev2.evaluate()["prediction_quality"], _expected(clips[:1]))
    assert os.listdir(str(tmp_path)) == ["prediction_quality_bair.json"]
    ev.reset()
    _feed(ev, clips[1:2])
    alone = ev.evaluate()["prediction_quality"]                                  # the clip whose best PSNR sample reproduces frame 3
    _close(alone, _expected(clips[1:2]))
    assert math.isnan(alone["per_frame"]["PSNR_best"][1]) and alone["identical_best_frames"] == 1


def test_stacked_decode_is_chunked_and_clip_lengths_must_agree():
    from lvt_amd.evaluation import PredictionQualityEvaluator
    clips = _clips(1)
    stub = _StubVQVAE()
    ev = PredictionQualityEvaluator(_cfg(), "d", distributed=False, vqvae=stub)
    ev.DECODE_FRAMES = 4
    _feed(ev, clips)
    assert stub.calls == [T_, 4, 4, 4, 3]
    _close(ev.evaluate()["prediction_quality"], _expected(clips))
    inp, out = clips[0]
    short = ({"image_sequence": inp["image_sequence"][:4]}, {"samples": [s[:, :4] for s in out["samples"]]})
    with pytest.raises(ValueError, match="frames"):
        _feed(ev, [short])
    with pytest.raises(ValueError):
        _feed(ev, [(inp, {"samples": [out["samples"][0][:, :3]]})])              # samples of another length than their clip


def _two_rank_case(rank, world):
    from lvt_amd.evaluation import PredictionQualityEvaluator
    ev = PredictionQualityEvaluator(_cfg(), "d", distributed=True, vqvae=_StubVQVAE())
    ev.reset()
    _feed(ev, _clips(2, first=0) if rank == 0 else _clips(1, first=2))
    res = ev.evaluate()
    empty = PredictionQualityEvaluator(_cfg(), "d", distributed=True, vqvae=_StubVQVAE())
    if rank == 1:                                                                # only rank 1 saw a clip: rank 0 learns T from it
        _feed(empty, _clips(1, first=2))
    return res, empty.evaluate()


def test_two_gloo_ranks_over_disjoint_clips():
    res = _run(_two_rank_case)
    assert res[1] == (None, None)                                                # the main process reports
    union, one = res[0]
    _close(union["prediction_quality"], _expected(_clips(3)))
    _close(one["prediction_quality"], _expected(_clips(1, first=2)))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_table_and_argument_validation():
    from lvt_amd.hip import binding as L
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = L.lib()
    assert L.ABI_VERSION == 680 == lib.lvt_version()
    assert set(NEW) <= set(L.declared_symbols())
    for name in NEW:
        assert name in integration, name
        res, args = _header_signature(header, name)
        assert lib._lvt_sigs[name] == (res, args), name

    p = 4096                                                                     # a non-null, 16-byte aligned address
    n = lib.lvt_frame_quality_partials(3, 64, 64)
    ok = dict(a=p, b=p, F=6, Fb=3, C=3, H=64, W=64, L=1.0, parts=p, n=n)

    def vs(**kw):
        v = dict(ok, **kw)
        return lib.lvt_frame_quality_vs(v["a"], v["b"], v["F"], v["Fb"], v["C"], v["H"], v["W"], v["L"], v["parts"], v["n"], None)

    for bad in (dict(Fb=4), dict(Fb=5), dict(Fb=12), dict(F=7, Fb=2), dict(Fb=0), dict(Fb=-3)):
        assert vs(**bad) == -1 and b"frame_quality_vs:" in lib.lvt_last_error() and b"multiple of Fb" in lib.lvt_last_error(), bad
    for key in ("a", "b", "parts"):
        assert vs(**{key: None}) == -1 and b"frame_quality_vs:" in lib.lvt_last_error() and b"null" in lib.lvt_last_error(), key
    for bad in (dict(H=10), dict(W=10)):
        assert vs(**bad) == -1 and b">= 11" in lib.lvt_last_error(), bad
    for bad in (0.0, -1.0, NAN, INF):
        assert vs(L=bad) == -1 and b"data_range" in lib.lvt_last_error(), bad
    for bad in (dict(n=n - 1), dict(n=0), dict(F=0, Fb=1), dict(C=0), dict(parts=p + 8), dict(a=p + 2)):
        assert vs(**bad) == -1 and b"frame_quality_vs:" in lib.lvt_last_error(), bad

    def select(frames=p, S=3, T=4, n_prime=1, curves=p, best=p):
        return lib.lvt_prediction_select(frames, S, T, n_prime, curves, best, None)

    for key in ("frames", "curves", "best"):
        assert select(**{key: None}) == -1 and b"prediction_select:" in lib.lvt_last_error() and b"null" in lib.lvt_last_error(), key
    for bad in (dict(n_prime=-1), dict(n_prime=4), dict(n_prime=9), dict(T=1, n_prime=1)):
        assert select(**bad) == -1 and b"n_prime" in lib.lvt_last_error(), bad
    for bad in (dict(S=0), dict(S=-2), dict(T=0, n_prime=0), dict(frames=p + 4), dict(curves=p + 4), dict(best=p + 2)):
        assert select(**bad) == -1 and b"prediction_select:" in lib.lvt_last_error(), bad
    assert ctypes.sizeof(ctypes.c_int) == 4                                      # `best` is two int32 on the Python side
