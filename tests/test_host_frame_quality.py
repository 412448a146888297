"""Host side of the frame-quality evaluation: the plain-torch statement of PSNR / SSIM (evaluation/quality.py) on hand-checkable
cases, FrameQualityEvaluator on CPU tensors (alone, combined, under two gloo ranks), build_evaluator's dispatch, the C-ABI table
and the argument validation of the three entries (which comes before any device work, so it runs without a GPU)."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from test_dp_gloo import _run

NEW = ("lvt_frame_quality_partials", "lvt_frame_quality", "lvt_frame_quality_finish")


def _clip(seed, shape, noise):
    """A clip in [0, 1] and a copy whose frame f carries noise of strength noise * (f + 1)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g)
    s = noise * torch.arange(1, shape[0] + 1, dtype=torch.float32).view(-1, 1, 1, 1)
    return a, (a + s * torch.randn(shape, generator=g)).clamp(0, 1)


# ---- the definitions -------------------------------------------------------------------------------------------------------------
def test_window_sums_to_one():
    from lvt_amd.evaluation.quality import gaussian_window
    w = gaussian_window()
    assert w.dtype == torch.float64 and w.numel() == 11
    assert abs(float(w.sum()) - 1.0) < 1e-15
    assert torch.equal(w, w.flip(0)) and float(w[5]) == float(w.max())
    assert abs(float(w[4] / w[5]) - math.exp(-1 / (2 * 1.5 ** 2))) < 1e-15


def test_identical_frames():
    from lvt_amd.evaluation import frame_quality_reference
    a, _ = _clip(0, (3, 3, 17, 23), 0.1)
    for L in (1.0, 255.0):
        psnr, ssim = frame_quality_reference(a * L, (a * L).clone(), L)
        assert psnr.dtype == torch.float64 and tuple(psnr.shape) == tuple(ssim.shape) == (3,)
        assert torch.isinf(psnr).all() and (psnr > 0).all()
        assert (ssim == 1.0).all()


@pytest.mark.parametrize("L,m,d", [(1.0, 0.25, 0.125), (255.0, 100.0, 3.0), (1.0, 0.5, -0.01)])
def test_constant_offset_on_a_constant_frame(L, m, d):
    from lvt_amd.evaluation import frame_quality_reference
    a = torch.full((2, 3, 13, 16), m, dtype=torch.float64)
    psnr, ssim = frame_quality_reference(a, a + d, L)
    c1 = (0.01 * L) ** 2
    assert torch.allclose(psnr, torch.full((2,), 20 * math.log10(L / abs(d)), dtype=torch.float64), rtol=0, atol=1e-9)
    want = (2 * m * (m + d) + c1) / (m * m + (m + d) ** 2 + c1)
    assert torch.allclose(ssim, torch.full((2,), want, dtype=torch.float64), rtol=0, atol=1e-12)


def test_single_window_frame():
    """An 11x11 frame has one map position: the SSIM is the formula on the window's own weighted moments."""
    from lvt_amd.evaluation import frame_quality_reference
    from lvt_amd.evaluation.quality import gaussian_window, windowed
    a, b = _clip(1, (1, 1, 11, 11), 0.2)
    assert tuple(windowed(a.double(), gaussian_window()).shape) == (1, 1, 1, 1)
    assert tuple(windowed(torch.zeros(2, 3, 17, 23, dtype=torch.float64), gaussian_window()).shape) == (2, 3, 7, 13)
    w2 = torch.outer(gaussian_window(), gaussian_window())
    x, y = a[0, 0].double(), b[0, 0].double()
    mx, my = (w2 * x).sum(), (w2 * y).sum()
    sxx, syy, sxy = (w2 * x * x).sum() - mx * mx, (w2 * y * y).sum() - my * my, (w2 * x * y).sum() - mx * my
    want = (2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    psnr, ssim = frame_quality_reference(a, b, 1.0)
    assert abs(float(ssim[0]) - float(want)) < 1e-13
    assert abs(float(psnr[0]) - 10 * math.log10(1.0 / float(((x - y) ** 2).mean()))) < 1e-10
    # (C, H, W) is one frame
    p3, s3 = frame_quality_reference(a[0], b[0], 1.0)
    assert torch.equal(p3, psnr) and torch.equal(s3, ssim)


def test_reference_refusals():
    from lvt_amd.evaluation import frame_quality_reference
    z = torch.zeros(1, 3, 16, 16)
    for a, b, L in ((z[..., :10, :], z[..., :10, :], 1.0), (z[..., :10], z[..., :10], 1.0), (z, z[:, :2], 1.0), (z, z, 0.0),
                    (z, z, -1.0), (z, z, float("nan")), (z, z, float("inf")), (z[0, 0], z[0, 0], 1.0)):
        with pytest.raises(ValueError):
            frame_quality_reference(a, b, L)


def test_package_does_not_import_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "lvt_amd")):
        for name in files:
            if name.endswith(".py"):
                text = open(os.path.join(dirpath, name)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), os.path.join(dirpath, name)


# ---- the evaluator on CPU tensors ------------------------------------------------------------------------------------------------
def _three_clips():
    clips = [_clip(10, (4, 3, 32, 32), 0.02), _clip(11, (2, 3, 17, 23), 0.05), _clip(12, (3, 1, 11, 12), 0.1)]
    clips[1][1][1] = clips[1][0][1]                      # one frame reproduced exactly
    return clips


def _feed(ev, clips):
    for a, b in clips:
        ev.process([{"image_sequence": a.numpy()}], [{"reconstruction": b}])


def _expected(clips, L=1.0):
    from lvt_amd.evaluation import frame_quality_reference
    ps, ss = zip(*(frame_quality_reference(b, a, L) for a, b in clips))
    ps, ss = torch.cat(ps), torch.cat(ss)
    finite = ~torch.isinf(ps)
    return float(ps[finite].mean()), float(ss.mean()), ps.numel(), int((~finite).sum())


def test_evaluator_is_the_mean_of_the_per_frame_values():
    from lvt_amd.evaluation import DatasetEvaluators, FrameQualityEvaluator, MSEEvaluator
    clips = _three_clips()
    psnr, ssim, n, ident = _expected(clips)
    assert n == 9 and ident == 1
    ev = FrameQualityEvaluator("d", distributed=False)
    ev.reset()
    _feed(ev, clips)
    res = ev.evaluate()
    assert list(res.keys()) == ["frame_quality"]
    fq = res["frame_quality"]
    assert sorted(fq.keys()) == ["PSNR", "SSIM", "frames", "identical_frames"]
    assert fq["frames"] == 9 and fq["identical_frames"] == 1
    assert abs(fq["PSNR"] - psnr) < 1e-12 * psnr and abs(fq["SSIM"] - ssim) < 1e-14
    # reset() forgets; single images ("image": (C, H, W)) count as one frame each
    ev.reset()
    a, b = clips[0]
    ev.process([{"image": a[0].numpy()}, {"image": a[1].numpy()}], [{"reconstruction": b[0]}, {"reconstruction": b[1]}])
    fq2 = ev.evaluate()["frame_quality"]
    p2, s2, _, _ = _expected([(a[:2], b[:2])])
    assert fq2["frames"] == 2 and abs(fq2["PSNR"] - p2) < 1e-12 * p2 and abs(fq2["SSIM"] - s2) < 1e-14
    # next to MSEEvaluator: two top-level keys, each what its evaluator reports alone
    both = DatasetEvaluators([MSEEvaluator("d", False), FrameQualityEvaluator("d", False)])
    both.reset()
    _feed(both, clips)
    res2 = both.evaluate()
    assert list(res2.keys()) == ["reconstruction", "frame_quality"]
    assert res2["frame_quality"] == fq
    alone = MSEEvaluator("d", False)
    _feed(alone, clips)
    assert res2["reconstruction"] == alone.evaluate()["reconstruction"]


def test_evaluator_without_a_finite_psnr_and_data_range():
    from lvt_amd.evaluation import FrameQualityEvaluator
    a, _ = _clip(3, (2, 3, 16, 16), 0.1)
    ev = FrameQualityEvaluator("d", distributed=False)
    ev.process([{"image_sequence": a.numpy()}], [{"reconstruction": a.clone()}])
    fq = ev.evaluate()["frame_quality"]
    assert math.isnan(fq["PSNR"]) and fq["SSIM"] == 1.0 and fq["frames"] == 2 and fq["identical_frames"] == 2
    # the same frames on the 0..255 scale: the same SSIM and PSNR as on 0..1 (both are scale-free given the range)
    a, b = _clip(4, (2, 3, 16, 16), 0.05)
    lo, hi = FrameQualityEvaluator("d", False, data_range=1.0), FrameQualityEvaluator("d", False, data_range=255.0)
    lo.process([{"image_sequence": a.numpy()}], [{"reconstruction": b}])
    hi.process([{"image_sequence": (a.double() * 255).numpy()}], [{"reconstruction": b.double() * 255}])
    r_lo, r_hi = lo.evaluate()["frame_quality"], hi.evaluate()["frame_quality"]
    assert abs(r_lo["PSNR"] - r_hi["PSNR"]) < 1e-9 and abs(r_lo["SSIM"] - r_hi["SSIM"]) < 1e-12
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            FrameQualityEvaluator("d", False, data_range=bad)


def test_build_evaluator_dispatch():
    from lvt_amd.config import get_cfg
    from lvt_amd.evaluation import DatasetEvaluators, FrameQualityEvaluator, MSEEvaluator, build_evaluator
    cfg = get_cfg()
    cfg.TEST.EVALUATORS = "FrameQualityEvaluator"
    assert cfg.INPUT.SCALE_TO_ZEROONE is True
    ev = build_evaluator(cfg, "d", "/tmp/lvt_test_out")
    assert isinstance(ev, FrameQualityEvaluator) and ev._data_range == 1.0
    cfg.INPUT.SCALE_TO_ZEROONE = False
    assert build_evaluator(cfg, "d", "/tmp/lvt_test_out")._data_range == 255.0
    cfg.TEST.EVALUATORS = "MSEEvaluator,FrameQualityEvaluator"
    ev = build_evaluator(cfg, "d", "/tmp/lvt_test_out")
    assert isinstance(ev, DatasetEvaluators)
    assert [type(e) for e in ev._evaluators] == [MSEEvaluator, FrameQualityEvaluator]
    cfg.TEST.EVALUATORS = "MSEEvaluator"
    assert type(build_evaluator(cfg, "d", "/tmp/lvt_test_out")) is MSEEvaluator
    cfg.TEST.EVALUATORS = "QualityEvaluator"
    with pytest.raises(NotImplementedError):
        build_evaluator(cfg, "d", "/tmp/lvt_test_out")


def _two_rank_case(rank, world):
    from lvt_amd.evaluation import DatasetEvaluators, FrameQualityEvaluator, MSEEvaluator
    ev = DatasetEvaluators([MSEEvaluator("d", True), FrameQualityEvaluator("d", True)])
    ev.reset()
    if rank == 0:                                   # rank 1 sees no sample and still takes part in the all-reduce
        _feed(ev, _three_clips()[:2])
    single = FrameQualityEvaluator("d", True).evaluate()           # a rank-local evaluator with nothing in it: both ranks call
    return dict(ev.evaluate()), single


def test_two_gloo_ranks_one_without_samples():
    res = _run(_two_rank_case)
    psnr, ssim, n, ident = _expected(_three_clips()[:2])
    main, empty = res[0]
    assert res[1][0] == {} and res[1][1] is None    # DatasetEvaluators collects on the main process only; the evaluator returns None
    fq = main["frame_quality"]
    assert fq["frames"] == n == 6 and fq["identical_frames"] == ident == 1
    assert abs(fq["PSNR"] - psnr) < 1e-12 * psnr and abs(fq["SSIM"] - ssim) < 1e-14
    assert "reconstruction" in main
    assert empty["frame_quality"]["frames"] == 0 and math.isnan(empty["frame_quality"]["PSNR"])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
_CTYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double}


def _header_signature(header, name):
    m = re.search(r"^([a-z ]+?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, header, re.M)
    assert m, name
    args = []
    for arg in m.group(2).replace("\n", " ").split(","):
        arg = arg.strip()
        if "*" in arg:
            args.append(ctypes.c_void_p)
        else:
            args.append(_CTYPES[arg.rsplit(" ", 1)[0].strip()])
    return _CTYPES[m.group(1).strip()], args


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

    assert lib.lvt_frame_quality_partials(3, 64, 64) > 0
    assert lib.lvt_frame_quality_partials(1, 11, 11) == 1
    assert lib.lvt_frame_quality_partials(3, 10, 64) == -1
    assert lib.lvt_frame_quality_partials(3, 64, 10) == -1
    assert lib.lvt_frame_quality_partials(0, 64, 64) == -1
    # more frame rows / columns never means fewer tiles, and channels multiply
    assert lib.lvt_frame_quality_partials(3, 75, 43) == 3 * lib.lvt_frame_quality_partials(1, 75, 43)
    assert lib.lvt_frame_quality_partials(1, 75, 43) > lib.lvt_frame_quality_partials(1, 26, 42) == 1

    p = 4096                                                               # a non-null, 16-byte aligned address
    n = lib.lvt_frame_quality_partials(3, 64, 64)
    ok = dict(a=p, b=p, F=2, C=3, H=64, W=64, L=1.0, parts=p, n=n, frames=p, acc=p)

    def run(**kw):
        v = dict(ok, **kw)
        return lib.lvt_frame_quality(v["a"], v["b"], v["F"], v["C"], v["H"], v["W"], v["L"], v["parts"], v["n"], None)

    def finish(**kw):
        v = dict(ok, **kw)
        return lib.lvt_frame_quality_finish(v["parts"], v["F"], v["C"], v["H"], v["W"], v["L"], v["n"], v["frames"], v["acc"], None)

    for fn, fname, nulls in ((run, b"frame_quality:", ("a", "b", "parts")), (finish, b"frame_quality_finish:", ("parts", "frames", "acc"))):
        for key in nulls:
            assert fn(**{key: None}) == -1 and fname in lib.lvt_last_error() and b"null" in lib.lvt_last_error(), key
        for bad in (dict(H=10), dict(W=10)):
            assert fn(**bad) == -1 and fname in lib.lvt_last_error() and b">= 11" in lib.lvt_last_error(), bad
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(L=bad) == -1 and fname in lib.lvt_last_error() and b"data_range" in lib.lvt_last_error(), bad
        for bad in (n - 1, n + 1, 0):
            assert fn(n=bad) == -1 and fname in lib.lvt_last_error() and b"partials" in lib.lvt_last_error(), bad
        for bad in (dict(F=0), dict(C=0), dict(parts=p + 8)):
            assert fn(**bad) == -1 and fname in lib.lvt_last_error(), bad
