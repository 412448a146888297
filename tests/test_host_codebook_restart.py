"""Host side of codebook restart (MODEL.CODEBOOK.RESTART): config keys, the model's refusals, state-dict keys, the plain-Python
statement of the draw (hip/vq.py restart_row), the C-ABI table."""
import glob
import os
import re

import pytest

from conftest import ROOT


def _cfg(num=4, **restart):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.CODEBOOK.NUM = num
    for k, v in restart.items():
        cfg.MODEL.CODEBOOK.RESTART[k] = v
    return cfg


def test_defaults_and_shipped_yamls():
    from lvt_amd.config import get_cfg
    r = get_cfg().MODEL.CODEBOOK.RESTART
    assert r.ENABLED is False and r.THRESHOLD == 1.0
    assert sorted(r.keys()) == ["ENABLED", "THRESHOLD"]
    yamls = sorted(glob.glob(os.path.join(ROOT, "configs", "*", "*.yaml")))
    assert len(yamls) == 7
    for path in yamls:
        cfg = get_cfg()
        cfg.merge_from_file(path)
        assert cfg.MODEL.CODEBOOK.RESTART.ENABLED is False, path
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.CODEBOOK.RESTART.ENABLED", "True", "MODEL.CODEBOOK.RESTART.THRESHOLD", "0.25"])
    assert cfg.MODEL.CODEBOOK.RESTART.ENABLED is True and cfg.MODEL.CODEBOOK.RESTART.THRESHOLD == 0.25


@pytest.mark.parametrize("num", [4, 1])
def test_refusals(num):
    from lvt_amd.modeling import build_model
    cfg = _cfg(num, ENABLED=True)
    cfg.MODEL.CODEBOOK.EMA = False
    with pytest.raises(ValueError):
        build_model(cfg)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            build_model(_cfg(num, ENABLED=True, THRESHOLD=bad))
    # a bad threshold with the feature off is not looked at: off is today's model
    assert not build_model(_cfg(num, THRESHOLD=-1.0)).codebook.restart_enabled


@pytest.mark.parametrize("num", [4, 1])
def test_state_dict_keys_are_the_reference_s(num):
    from lvt_amd.modeling import build_model
    off = build_model(_cfg(num))
    on = build_model(_cfg(num, ENABLED=True, THRESHOLD=0.5))
    assert on.codebook.restart_enabled and not off.codebook.restart_enabled
    assert off.codebook_health() is None
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    assert list(on.codebook.state_dict().keys()) == list(off.codebook.state_dict().keys())
    # the counters exist, as non-persistent buffers
    names = dict(on.codebook.named_buffers())
    assert {"restart_pass", "restart_health", "restart_total"} <= set(names)
    assert int(names["restart_pass"]) == 0
    # and loading a checkpoint written without the feature is strict-clean
    on.codebook.load_state_dict(off.codebook.state_dict())


def test_seed_is_the_unoffset_config_seed():
    from lvt_amd.modeling import build_model
    cfg = _cfg(4, ENABLED=True)
    cfg.SEED = -1                          # "no seed": the draw still needs one
    assert build_model(cfg).codebook._restart == (1.0, 0)
    cfg = _cfg(4, ENABLED=True, THRESHOLD=0.0)
    cfg.SEED = 1234
    assert build_model(cfg).codebook._restart == (0.0, 1234)


def test_restart_row():
    from lvt_amd.hip.vq import restart_row
    K = 512
    for R in (K, K + 1, 4 * K + 3):
        for i in (0, 3):
            rows = [restart_row(7, 2, i, k, R, K) for k in range(K)]
            assert len(set(rows)) == K, (R, i)
            assert min(rows) >= 0 and max(rows) < R
            assert all(k * R // K <= r < (k + 1) * R // K for k, r in enumerate(rows))      # its own stratum
    for R in (1, 8, K - 1):
        rows = [restart_row(7, 2, 1, k, R, K) for k in range(K)]
        assert min(rows) >= 0 and max(rows) < R, R
    # the stream moves with the pass, the codebook and the seed (strata of 64 rows: a repeat has probability 1/64 per code)
    R = 64 * K
    base = [restart_row(7, 0, 0, k, R, K) for k in range(K)]
    for other in ([restart_row(7, 1, 0, k, R, K) for k in range(K)], [restart_row(7, 0, 1, k, R, K) for k in range(K)],
                  [restart_row(8, 0, 0, k, R, K) for k in range(K)]):
        assert sum(a != b for a, b in zip(base, other)) > 0.9 * K
    # pinned values: the kernel states the same function (tests/test_gpu_codebook_restart.py compares them on the device)
    z = 0 ^ (0 * 0x9E3779B97F4A7C15) ^ (0 << 32 | 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    z ^= z >> 31
    assert restart_row(0, 0, 0, 1, 2 * 1000, 2) == 1000 + z % 1000


def test_enable_restart_on_the_quantisers():
    from lvt_amd.modeling.vq import DVQEmbedding, SingleVQEmbedding
    for q in (DVQEmbedding(2, 64, 32, True), SingleVQEmbedding(128, 128, True)):
        assert not q.restart_enabled and q.health_scalars() is None
        keys = list(q.state_dict().keys())
        q.enable_restart(0.5, 3)
        assert q.restart_enabled and list(q.state_dict().keys()) == keys
    with pytest.raises(ValueError):
        DVQEmbedding(2, 64, 32, False).enable_restart(1.0, 0)
    with pytest.raises(ValueError):
        SingleVQEmbedding(128, 128, True).enable_restart(-0.5, 0)


def test_abi_table_and_argument_validation():
    from lvt_amd.hip import binding as L
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    assert L.ABI_VERSION == 680 == L.lib().lvt_version()
    new = {"lvt_vq_restart_candidates", "lvt_vq_ema_finalize_restart"}
    assert new <= set(L.declared_symbols())
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, header), name
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`lvt_version()` == 680" in text
    for name in new:
        assert name in text, name
    # argument validation comes before any device work (no GPU here: a launch would fail differently)
    lib = L.lib()
    p = 4096                                                               # a non-null, 16-byte aligned address
    ok_c = dict(z=p, rows=8, ldz=64, num=1, D=64, K=64, P=4, rank=0, world=1, seed=0, pas=p, shared=0, cand=p)

    def cand(**kw):
        a = dict(ok_c, **kw)
        return lib.lvt_vq_restart_candidates(a["z"], a["rows"], a["ldz"], a["num"], a["D"], a["K"], a["P"], a["rank"], a["world"],
                                             a["seed"], a["pas"], a["shared"], a["cand"], None)
    for bad in (dict(z=None), dict(pas=None), dict(cand=None), dict(D=24), dict(D=272), dict(K=96), dict(K=4096), dict(rows=0),
                dict(rows=6), dict(rank=1), dict(world=0), dict(ldz=32), dict(cand=p + 4)):
        assert cand(**bad) == -1, bad
    assert b"vq_restart_candidates" in lib.lvt_last_error()

    ok_f = dict(stats=p, cand=p, num=1, D=64, K=64, thr=1.0, rs=p, rsum=p, w=p, health=p, total=p, pas=p)

    def fin(**kw):
        a = dict(ok_f, **kw)
        return lib.lvt_vq_ema_finalize_restart(a["stats"], a["cand"], a["num"], a["D"], a["K"], 0.99, 1e-5, a["thr"], a["rs"],
                                               a["rsum"], a["w"], a["health"], a["total"], a["pas"], None)
    for bad in (dict(stats=None), dict(cand=None), dict(rs=None), dict(rsum=None), dict(w=None), dict(health=None),
                dict(total=None), dict(pas=None), dict(num=0), dict(D=8), dict(K=32), dict(K=2112)):
        assert fin(**bad) == -1, bad
    for thr in (-1.0, float("nan"), float("inf")):
        assert fin(thr=thr) == -1 and b"threshold" in lib.lvt_last_error(), thr
