"""Host side of truncated sampling (TEST.VT_SAMPLER.{TEMPERATURE, TOP_K, TOP_P}): the rule stated in plain torch
(lvt_amd/modeling/autoregressive/sampling.py) on hand-made rows, the argument check, the config keys and their refusals when a
model is built.  No GPU: nothing here launches."""
import os

import pytest
import torch

from conftest import ROOT
from lvt_amd.modeling.autoregressive import sampling as S

KEYS = {"temp": "TEST.VT_SAMPLER.TEMPERATURE", "top_k": "TEST.VT_SAMPLER.TOP_K", "top_p": "TEST.VT_SAMPLER.TOP_P"}


def _kept(logits, temp, top_k, top_p):
    p = S.truncated_probs_reference(torch.tensor(logits, dtype=torch.float64), temp, top_k, top_p)
    assert p.dtype == torch.float64 and abs(float(p.sum()) - 1.0) < 1e-12
    return [i for i, v in enumerate(p.tolist()) if v > 0], p


# ---- the rule ---------------------------------------------------------------------------------------------------------
def test_tie_at_the_kth_logit_keeps_both():
    row = [1.0, 3.0, 2.0, 2.0, 0.5]
    assert _kept(row, 1.0, 2, 1.0)[0] == [1, 2, 3]              # the 2nd largest is 2.0, twice: |A| = 3 > k
    assert _kept(row, 1.0, 3, 1.0)[0] == [1, 2, 3]
    assert _kept(row, 1.0, 1, 1.0)[0] == [1]
    assert _kept(row, 1.0, 4, 1.0)[0] == [0, 1, 2, 3]


def test_top_k_off_keeps_everything():
    row = [0.3, -1.0, 2.0, 0.0]
    full = torch.softmax(torch.tensor(row, dtype=torch.float64) / 0.7, 0)
    for k in (0, 4, 9):
        kept, p = _kept(row, 0.7, k, 1.0)
        assert kept == [0, 1, 2, 3] and torch.allclose(p, full, rtol=1e-12, atol=0)


def test_small_top_p_keeps_only_the_argmax():
    kept, p = _kept([0.0, 1.0, 5.0, 1.0], 1.0, 0, 1e-6)
    assert kept == [2] and p.tolist() == [0.0, 0.0, 1.0, 0.0]


def test_top_p_one_is_the_identity_and_probs_are_renormalised():
    row = [2.0, 1.0, 0.0, -1.0]
    full = torch.softmax(torch.tensor(row, dtype=torch.float64), 0)
    assert torch.equal(_kept(row, 1.0, 0, 1.0)[1], S.truncated_probs_reference(torch.tensor(row), 1.0, 0, 1.0))
    assert torch.allclose(_kept(row, 1.0, 0, 1.0)[1], full, rtol=1e-12, atol=0)
    # masses 0.644, 0.237, 0.087, 0.032: 0.85 needs two codes, 0.9 three
    kept, p = _kept(row, 1.0, 0, 0.85)
    assert kept == [0, 1] and torch.allclose(p[:2], full[:2] / full[:2].sum(), rtol=1e-12, atol=0) and p[2:].tolist() == [0.0, 0.0]
    assert _kept(row, 1.0, 0, 0.9)[0] == [0, 1, 2]
    # a tie class at the boundary is kept whole
    assert _kept([2.0, 1.0, 1.0, -3.0], 1.0, 0, 0.7)[0] == [0, 1, 2]


def test_top_k_is_applied_before_top_p():
    """w = 4, 3, 2, 1 (mass 0.4, 0.3, 0.2, 0.1) with k = 3, p = 0.75, where the two orders give different sets.
    k first: A = {0, 1, 2}, masses over A 4/9, 7/9 = 0.778 >= 0.75 -> {0, 1}.
    p first on the full row: 0.4, 0.7 < 0.75, 0.9 -> {0, 1, 2}, and k = 3 leaves it: {0, 1, 2}."""
    row = torch.log(torch.tensor([4.0, 3.0, 2.0, 1.0], dtype=torch.float64)).tolist()
    assert _kept(row, 1.0, 3, 0.75)[0] == [0, 1]
    assert _kept(row, 1.0, 0, 0.75)[0] == [0, 1, 2]              # what top-p alone (hence top-p first) would have kept
    kept, p = _kept(row, 1.0, 3, 0.75)
    assert torch.allclose(p[:2], torch.tensor([4.0 / 7, 3.0 / 7], dtype=torch.float64), rtol=1e-12, atol=0)


def test_selection_is_on_logits_whatever_the_temperature():
    row = [0.0, 0.25, 0.5, 0.75]
    for temp in (1e-3, 1.0, 50.0):
        assert _kept(row, temp, 2, 1.0)[0] == [2, 3]


def test_draw_never_leaves_the_kept_set():
    # first and last indices cut
    logits = torch.tensor([[-9.0, 2.0, 1.0, 2.5, -9.0, -9.0], [-5.0, -4.0, 3.0, 0.0, 2.0, -6.0]])
    probs = S.truncated_probs_reference(logits, 0.9, 3, 1.0)
    assert (probs[:, 0] == 0).all() and (probs[:, -1] == 0).all()
    for u in (0.0, 1.0 - 2.0 ** -24):
        codes = S.truncated_draw_reference(probs, torch.full((2,), u, dtype=torch.float64))
        assert codes.dtype == torch.int64
        assert bool((probs.gather(1, codes[:, None]) > 0).all()), (u, codes)
    assert S.truncated_draw_reference(probs, torch.zeros(2)).tolist() == [1, 2]
    assert S.truncated_draw_reference(probs, torch.full((2,), 1.0 - 2.0 ** -24, dtype=torch.float64)).tolist() == [3, 4]
    # a threshold that rounding lifts to the total itself stops at the last kept index, not at V - 1
    assert S.truncated_draw_reference(probs, torch.ones(2, dtype=torch.float64)).tolist() == [3, 4]
    # the inverse-CDF rule in memory order: thresholds inside each kept code's step
    p = torch.tensor([[0.0, 0.25, 0.0, 0.5, 0.25, 0.0]], dtype=torch.float64)
    for u, want in ((0.1, 1), (0.25, 3), (0.5, 3), (0.75, 4), (0.99, 4)):
        assert S.truncated_draw_reference(p, torch.tensor([u], dtype=torch.float64)).tolist() == [want], u


def test_reference_takes_batches():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 7, 33, generator=g)
    p = S.truncated_probs_reference(x, 0.8, 6, 0.9)
    assert p.shape == x.shape
    for i in (0, 4):
        for j in (0, 6):
            assert torch.equal(p[i, j], S.truncated_probs_reference(x[i, j], 0.8, 6, 0.9))
    assert int((p > 0).sum(-1).max()) <= 6 and bool((p.argmax(-1) == x.argmax(-1)).all())


# ---- the argument check -----------------------------------------------------------------------------------------------
BAD = [("temp", 0.0), ("temp", -1.0), ("temp", float("nan")), ("temp", float("inf")), ("temp", "hot"),
       ("top_k", -1), ("top_k", 2.5), ("top_k", "8"), ("top_k", True),
       ("top_p", 0.0), ("top_p", -0.1), ("top_p", 1.5), ("top_p", float("nan")), ("top_p", float("inf"))]


@pytest.mark.parametrize("which,bad", BAD, ids=lambda v: str(v))
def test_check_sampling_refuses(which, bad):
    args = {"temp": 1.0, "top_k": 0, "top_p": 1.0}
    args[which] = bad
    with pytest.raises(ValueError, match=KEYS[which].replace(".", r"\.")):
        S.check_sampling(**args)


def test_check_sampling_accepts():
    assert S.check_sampling(1.0, 0, 1.0) == (1.0, 0, 1.0)
    t, k, p = S.check_sampling(1, 8, 1)
    assert (t, k, p) == (1.0, 8, 1.0) and isinstance(t, float) and isinstance(k, int) and isinstance(p, float)
    assert S.check_sampling(1e-4, 100000, 1e-9) == (1e-4, 100000, 1e-9)
    assert S.truncation_off(0, 1.0) and not S.truncation_off(1, 1.0) and not S.truncation_off(0, 0.99)


# ---- config -----------------------------------------------------------------------------------------------------------
def _cfg(path="configs/vt/DSFVT.yaml"):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, path))
    cfg.MODEL.DEVICE = "cpu"
    cfg.OUTPUT_DIR = "/tmp/lvt_test_out"
    return cfg


def _small_cfg(**sampler):
    cfg = _cfg()
    vt = cfg.MODEL.AUTOREGRESSIVE.VT
    vt.BLOCKS_E, vt.N_HEAD_E = ((1, 16, 16),) * 2, (2, 2)
    vt.BLOCKS_D, vt.N_HEAD_D = ((1, 16, 16),) * 3, (2, 2, 2)
    vt.D, vt.DA, vt.DE = 64, 32, 32
    for k, v in sampler.items():
        setattr(cfg.TEST.VT_SAMPLER, k, v)
    return cfg


def test_config_keys(tmp_path):
    from lvt_amd.config import get_cfg
    s = get_cfg().TEST.VT_SAMPLER
    assert (s.TEMPERATURE, s.TOP_K, s.TOP_P) == (1.0, 0, 1.0)
    assert isinstance(s.TEMPERATURE, float) and isinstance(s.TOP_K, int) and isinstance(s.TOP_P, float)
    for name in ("DSFVT", "DSSVT", "KDSFVT", "DSTSVT"):
        s = _cfg("configs/vt/%s.yaml" % name).TEST.VT_SAMPLER
        assert (s.TEMPERATURE, s.TOP_K, s.TOP_P) == (1.0, 0, 1.0), name
    y = tmp_path / "trunc.yaml"
    y.write_text("_BASE_: %s\nTEST:\n  VT_SAMPLER:\n    TEMPERATURE: 0.9\n    TOP_K: 8\n    TOP_P: 0.95\n"
                 % os.path.join(ROOT, "configs/vt/DSFVT.yaml"))
    cfg = get_cfg()
    cfg.merge_from_file(str(y))
    s = cfg.TEST.VT_SAMPLER
    assert (s.TEMPERATURE, s.TOP_K, s.TOP_P) == (0.9, 8, 0.95) and cfg.MODEL.AUTOREGRESSIVE.VT.D == 512
    cfg.merge_from_list([KEYS["top_k"], "16", KEYS["top_p"], "0.5", KEYS["temp"], "0.7"])
    assert (s.TEMPERATURE, s.TOP_K, s.TOP_P) == (0.7, 16, 0.5)
    cfg.merge_from_list([KEYS["top_p"], 1, KEYS["temp"], 1])
    assert (s.TEMPERATURE, s.TOP_P) == (1.0, 1.0) and isinstance(s.TOP_P, float) and isinstance(s.TEMPERATURE, float)


def test_defaults_build():
    from lvt_amd.modeling import build_model
    model = build_model(_small_cfg())
    assert model._sampling_settings() == (1.0, 0, 1.0)
    assert build_model(_small_cfg(TEMPERATURE=0.9, TOP_K=8, TOP_P=0.9))._sampling_settings() == (0.9, 8, 0.9)


@pytest.mark.parametrize("key,which,bad", [("TEMPERATURE", "temp", 0.0), ("TEMPERATURE", "temp", -2.0),
                                           ("TEMPERATURE", "temp", float("nan")), ("TEMPERATURE", "temp", float("inf")),
                                           ("TOP_K", "top_k", -1), ("TOP_P", "top_p", 0.0), ("TOP_P", "top_p", 1.5),
                                           ("TOP_P", "top_p", -0.5), ("TOP_P", "top_p", float("nan"))], ids=lambda v: str(v))
def test_bad_config_value_is_refused_at_build(key, which, bad):
    from lvt_amd.modeling import build_model
    with pytest.raises(ValueError, match=KEYS[which].replace(".", r"\.")):
        build_model(_small_cfg(**{key: bad}))


def test_sample_video_checks_its_arguments_before_anything_else():
    from lvt_amd.modeling import build_model
    model = build_model(_small_cfg())
    video = torch.zeros(1, 4, 16, 16, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"TEST\.VT_SAMPLER\.TOP_K"):
        model.sample_video(video, top_k=-1)
    with pytest.raises(ValueError, match=r"TEST\.VT_SAMPLER\.TOP_P"):
        model.sample_video(video, top_p=0.0)
    with pytest.raises(ValueError, match=r"TEST\.VT_SAMPLER\.TEMPERATURE"):
        model.sample_video(video, temp=0.0)


def test_evaluator_reports_sampling_only_when_set():
    """PredictionQualityEvaluator names the settings in its result only when one differs from its default (no VQ-VAE is built: the
    one passed in is used as it is)."""
    from lvt_amd.evaluation import PredictionQualityEvaluator

    class _Decoder:
        encoder = generator = codebook = None

        def set_generator_requires_grad(self, flag):
            pass

        def eval(self):
            return self

        def decode_pixels(self, codes):
            return codes.float().mean(1, keepdim=True).expand(-1, 3, -1, -1).contiguous() / 8.0

    def run(**sampler):
        cfg = _small_cfg(**sampler)
        cfg.TEST.VT_SAMPLER.N_PRIME = 1
        vs = cfg.TEST.VT_SAMPLER.VQ_VAE
        vs.CFG = os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml")
        vs.ENCODER_WEIGHTS = vs.GENERATOR_WEIGHTS = vs.CODEBOOK_WEIGHTS = ""
        ev = PredictionQualityEvaluator(cfg, "x", distributed=False, output_dir=None, vqvae=_Decoder())
        g = torch.Generator().manual_seed(0)
        clip = torch.randint(0, 8, (3, 4, 16, 16), generator=g)
        ev.process([{"image_sequence": clip}], [{"samples": [torch.randint(0, 8, (4, 3, 16, 16), generator=g)]}])
        return ev.evaluate()["prediction_quality"]

    assert "sampling" not in run()
    assert run(TOP_K=8)["sampling"] == {"temperature": 1.0, "top_k": 8, "top_p": 1.0}
    assert run(TEMPERATURE=0.9, TOP_P=0.95)["sampling"] == {"temperature": 0.9, "top_k": 0, "top_p": 0.95}
