"""Host side of the video transformer's residual dropout (MODEL.AUTOREGRESSIVE.VT.DROPOUT): the Philox stream stated
in plain Python (lvt_amd/hip/dropout.py) against known answers, threshold / scale / mask properties, the config key and its
refusals, and the model surface (constructor keywords, state-dict keys, init checksums, site numbering, the pass counter).  No
GPU: nothing here launches."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from lvt_amd.hip import dropout as D

KEY = "MODEL.AUTOREGRESSIVE.VT.DROPOUT"


# ---- the generator -----------------------------------------------------------------------------------------------------
KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % w for w in D.philox4x32_10(counter, key)) == want
    # the array form gives the same words
    arr = D.philox4x32_10(tuple(np.array([c, c], dtype=np.uint64) for c in counter), key)
    assert all(a.dtype == np.uint32 and a.shape == (2,) for a in arr)
    assert " ".join("%08x" % int(a[1]) for a in arr) == want


def test_threshold_and_scale():
    assert D.threshold(0.0) == 0 and D.threshold(0.5) == 2 ** 31
    ps = [0.0, 1e-12, 0.1, 0.25, 0.5, 0.75, 0.9, 1 - 2.0 ** -40, math.nextafter(1.0, 0.0)]
    ts = [D.threshold(p) for p in ps]
    assert ts == sorted(ts) and ts[-1] <= 2 ** 32 - 1
    for p in ps:
        assert D.threshold(p) == int(math.floor(p * 2.0 ** 32))
        s = D.scale(p)
        assert isinstance(s, np.float32) and s == np.float32(1.0 / (1.0 - p))
    assert D.scale(0.0) == 1.0
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            D.threshold(bad)


def test_keep_mask_prefix_and_word_order():
    seed, sr, pass_ = 0xfeedfacecafebeef, D.site_rank(5, 1, 3), 7
    for n in (1, 5, 4096, 4099):
        m, m5 = D.keep_mask(seed, sr, pass_, n, 0.3), D.keep_mask(seed, sr, pass_, n + 5, 0.3)
        assert m.dtype == bool and m.shape == (n,) and np.array_equal(m, m5[:n])
    w = D.words(seed, sr, pass_, 23)
    T = D.threshold(0.3)
    for i in (0, 1, 4, 7, 18, 22):
        g, j = divmod(i, 4)
        out = D.philox4x32_10((g, 0, sr, pass_), (seed & 0xffffffff, seed >> 32))
        assert int(w[i]) == out[j]
        assert bool(D.keep_mask(seed, sr, pass_, 23, 0.3)[i]) == (out[j] >= T)
    # the group index is 64 bits wide: its high word is counter word 1
    g = (1 << 32) + 9
    a = D.philox4x32_10((np.array([g], dtype=np.uint64) & np.uint64(0xffffffff), np.array([g], dtype=np.uint64) >> np.uint64(32), sr, 0),
                        (1, 2))
    assert tuple(int(x[0]) for x in a) == D.philox4x32_10((9, 1, sr, 0), (1, 2))
    assert D.keep_mask(seed, sr, pass_, 64, 0.0).all()


@pytest.mark.parametrize("n", [32792, 65868])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_and_site_independence(p, n):
    m3, m4 = (D.keep_mask(0x1234567, sr, 0, n, p) for sr in (3, 4))
    sigma = math.sqrt(p * (1 - p) / n)
    for m in (m3, m4):
        dev = abs(float(m.sum()) / n - (1 - p))
        print("p %.1f n %d: kept %.6f, %.2f sigma" % (p, n, float(m.sum()) / n, dev / sigma))
        assert dev <= 4 * sigma
    q = p * p + (1 - p) * (1 - p)
    dev = abs(float((m3 == m4).sum()) / n - q)
    print("agreement %.6f, %.2f sigma" % (float((m3 == m4).sum()) / n, dev / math.sqrt(q * (1 - q) / n)))
    assert dev <= 4 * math.sqrt(q * (1 - q) / n)


def test_masks_differ_between_passes_ranks_and_seeds():
    n, p, seed = 4096, 0.5, 0x1234567
    base = D.keep_mask(seed, D.site_rank(2, 0, 0), 0, n, p)
    assert np.array_equal(base, D.keep_mask(seed, D.site_rank(2, 0, 0), 0, n, p))
    others = [D.keep_mask(seed, D.site_rank(2, 0, 0), 1, n, p), D.keep_mask(seed, D.site_rank(2, 0, 1), 0, n, p),
              D.keep_mask(seed + 1, D.site_rank(2, 0, 0), 0, n, p), D.keep_mask(seed + (1 << 32), D.site_rank(2, 0, 0), 0, n, p),
              D.keep_mask(seed, D.site_rank(2, 1, 0), 0, n, p)]
    for o in others:
        assert 0.4 < float((o != base).mean()) < 0.6


def test_site_rank_limits():
    assert D.site_rank(0, 0) == 0 and D.site_rank(3, 1) == 7 and D.site_rank(2047, 1, (1 << 20) - 1) == 2 ** 32 - 1
    for bad in ((2048, 0, 0), (-1, 0, 0), (0, 2, 0), (0, 0, 1 << 20), (0, 0, -1)):
        with pytest.raises(ValueError):
            D.site_rank(*bad)


def test_reference_statement():
    z = np.linspace(-2, 2, 37, dtype=np.float32)
    r = np.linspace(5, 6, 37, dtype=np.float32)
    keep = D.keep_mask(11, 4, 2, 37, 0.25)
    out = D.dropout_add_reference(z, r, 11, 4, 2, 0.25)
    assert out.dtype == np.float32 and np.array_equal(out[~keep], r[~keep])
    assert np.array_equal(out[keep], (r + z * np.float32(1.0 / 0.75))[keep])
    bwd = D.dropout_add_reference(z, None, 11, 4, 2, 0.25)
    assert np.array_equal(bwd == 0, ~keep | (z == 0)) and not np.signbit(bwd[~keep]).any()
    assert np.array_equal(D.dropout_add_reference(z, r, 11, 4, 2, 0.0), r + z)


# ---- config -----------------------------------------------------------------------------------------------------------
def _cfg(path="configs/vt/DSFVT.yaml"):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, path))
    cfg.MODEL.DEVICE = "cpu"
    cfg.OUTPUT_DIR = "/tmp/lvt_test_out"
    return cfg


def test_config_key(tmp_path):
    from lvt_amd.config import get_cfg
    assert get_cfg().MODEL.AUTOREGRESSIVE.VT.DROPOUT == 0.0
    for name in ("DSFVT", "DSSVT", "KDSFVT", "DSTSVT"):
        assert _cfg("configs/vt/%s.yaml" % name).MODEL.AUTOREGRESSIVE.VT.DROPOUT == 0.0, name
    y = tmp_path / "drop.yaml"
    y.write_text("_BASE_: %s\nMODEL:\n  AUTOREGRESSIVE:\n    VT:\n      DROPOUT: 0.2\n" % os.path.join(ROOT, "configs/vt/DSFVT.yaml"))
    cfg = get_cfg()
    cfg.merge_from_file(str(y))
    assert cfg.MODEL.AUTOREGRESSIVE.VT.DROPOUT == 0.2 and cfg.MODEL.AUTOREGRESSIVE.VT.D == 512
    cfg.merge_from_list([KEY, "0.1"])
    assert cfg.MODEL.AUTOREGRESSIVE.VT.DROPOUT == 0.1
    cfg.merge_from_list([KEY, 0])
    assert cfg.MODEL.AUTOREGRESSIVE.VT.DROPOUT == 0.0 and isinstance(cfg.MODEL.AUTOREGRESSIVE.VT.DROPOUT, float)


def _small_cfg(dropout=None):
    cfg = _cfg()
    vt = cfg.MODEL.AUTOREGRESSIVE.VT
    vt.BLOCKS_E, vt.N_HEAD_E = ((1, 16, 16),) * 2, (2, 2)
    vt.BLOCKS_D, vt.N_HEAD_D = ((1, 16, 16),) * 3, (2, 2, 2)
    vt.D, vt.DA, vt.DE = 64, 32, 32
    if dropout is not None:
        vt.DROPOUT = dropout
    return cfg


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf")], ids=str)
def test_bad_rate_is_refused_at_build(bad):
    from lvt_amd.modeling import build_model
    with pytest.raises(ValueError, match=KEY):
        build_model(_small_cfg(bad))


# ---- model surface ----------------------------------------------------------------------------------------------------
def _vt_positional(*extra, **kw):
    from lvt_amd.modeling.autoregressive.videotransformer import VideoTransformer
    return VideoTransformer(4, 8, 16, 16, 32, ((1, 4, 4),) * 2, (2, 2), (3, 1, 1), (4, 1, 1), ((1, 4, 4),) * 3, (2, 2, 2), -1,
                            True, False, 0, *extra, **kw)


def test_positional_construction_still_works():
    from lvt_amd.modeling.autoregressive.videotransformer import VTDecoder, VTEncoder
    from lvt_amd.modeling.autoregressive.vt_attention import BlockLocalAttention
    m = _vt_positional()
    assert m.dropout == 0.0 and all(l.dropout == 0.0 for l in m.encoder.block_local_attention)
    assert _vt_positional(0.25).dropout == 0.25 and _vt_positional(dropout=0.25).decoder.block_local_attention[2].dropout == 0.25
    VTEncoder(4, 8, 16, 16, 32, ((1, 4, 4),), (2,), (3, 1, 1), (4, 1, 1), -1, 0)
    assert VTEncoder(4, 8, 16, 16, 32, ((1, 4, 4),), (2,), (3, 1, 1), (4, 1, 1), dropout=0.5).block_local_attention[0].dropout == 0.5
    VTDecoder(4, 8, 16, 16, 32, ((1, 4, 4),), (2,))
    assert VTDecoder(4, 8, 16, 16, 32, ((1, 4, 4),), (2,), dropout=0.5).block_local_attention[0].dropout == 0.5
    lay = BlockLocalAttention((1, 4, 4), 16, 32, 2, True)
    assert lay.masked and lay.dropout == 0.0 and lay.dropout_layer == 0 and lay._dropout_state.pass_ == 0
    with pytest.raises(ValueError, match=KEY):
        BlockLocalAttention((1, 4, 4), 16, 32, 2, dropout=1.0)


def test_dropout_adds_no_state_and_leaves_the_init_alone():
    from lvt_amd.modeling import build_model

    def build(p):
        torch.manual_seed(1234)
        model = build_model(_small_cfg(p))
        after = torch.rand(1)
        return model, after

    m0, r0 = build(0.0)
    m3, r3 = build(0.3)
    sd0, sd3 = m0.state_dict(), m3.state_dict()
    assert list(sd0) == list(sd3)
    for k in sd0:
        assert sd0[k].shape == sd3[k].shape and sd0[k].dtype == sd3[k].dtype and torch.equal(sd0[k], sd3[k]), k
    assert [n for n, _ in m0.named_buffers()] == [n for n, _ in m3.named_buffers()]
    assert torch.equal(r0, r3), "building with dropout advanced torch's generator"
    assert m3.model.dropout == 0.3 and m3.model.dropout_state.seed == 1234 and m0.model.dropout_state.seed == 1234
    m3.model.set_dropout_seed((1 << 64) + 5)
    assert m3.model.dropout_state.seed == 5


def test_site_numbering_and_pass_counter():
    m = _vt_positional(0.5)
    layers = list(m.encoder.block_local_attention) + list(m.decoder.block_local_attention)
    assert len(layers) == 5 and [l.dropout_layer for l in layers] == [0, 1, 2, 3, 4]
    assert all(l._dropout_state is m.dropout_state for l in layers)
    m.train()
    m.set_dropout_seed(99)
    sites = []
    for l in layers:
        p, seed, sr, pass_ = l._drop_args()
        assert (p, seed, pass_) == (0.5, 99, 0)
        sites += [sr, sr + 1]
    assert sites == list(range(10))
    # the counter: the first training-mode pass uses 0, the next 1; eval and rate 0 leave it alone
    assert [m.begin_dropout_pass(), m.begin_dropout_pass(), m.begin_dropout_pass()] == [0, 1, 2]
    assert layers[4]._drop_args()[3] == 2
    m.eval()
    assert m.begin_dropout_pass() == 2 and all(l._drop_args() is None for l in layers)
    m.train()
    assert m.begin_dropout_pass() == 3
    off = _vt_positional()
    off.train()
    assert [off.begin_dropout_pass(), off.begin_dropout_pass()] == [0, 0]
    assert all(l._drop_args() is None for l in off.encoder.block_local_attention)
    # logits_tokens is what advances it: without a GPU the forward refuses right after
    from lvt_amd.hip import LvtError
    ctx, sl, sidx = torch.zeros(1, 4, 7, 4, 4, dtype=torch.long), torch.zeros(1, 4, 1, 4, 4, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    for want in (4, 5):
        with pytest.raises(LvtError):
            m.logits_tokens(ctx, sl, sidx)
        assert m.dropout_state.pass_ == want
    m.eval()
    with pytest.raises(LvtError):
        m.logits_tokens(ctx, sl, sidx)
    assert m.dropout_state.pass_ == 5


def test_abi_is_additive():
    import re
    from lvt_amd.hip import binding as L
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    declared = set(re.findall(r"\b(lvt_[a-z0-9_]+)\s*\(", header))
    new = {"lvt_dropout_add", "lvt_dropout_bwd"}
    assert new <= declared and new <= set(L.declared_symbols())
    assert L.ABI_VERSION == 680 and L.lib().lvt_version() == 680
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all("`%s(" % n in text for n in new)
    # the refusals need no device: nothing is launched
    buf = (torch.zeros(8) + 3).contiguous()
    p = buf.data_ptr() if buf.data_ptr() % 16 == 0 else buf.data_ptr() + (16 - buf.data_ptr() % 16)
    lib = L.lib()
    assert lib.lvt_dropout_add(p, None, 0, 1, 0, 0, 0, 1.0, p, None, None) == -1 and b"lvt_dropout_add" in lib.lvt_last_error()
    assert lib.lvt_dropout_add(None, None, 4, 1, 0, 0, 0, 1.0, p, None, None) == -1
    assert lib.lvt_dropout_add(p, None, 4, 1, 0, 0, 0, 1.0, None, None, None) == -1
    assert lib.lvt_dropout_add(p + 4, None, 4, 1, 0, 0, 0, 1.0, p, None, None) == -1 and b"aligned" in lib.lvt_last_error()
    assert lib.lvt_dropout_add(p, p + 8, 4, 1, 0, 0, 0, 1.0, p, None, None) == -1
    assert lib.lvt_dropout_bwd(p, -3, 1, 0, 0, 0, 1.0, p, None, None) == -1 and b"lvt_dropout_bwd" in lib.lvt_last_error()
    assert lib.lvt_dropout_bwd(p, 4, 1, 0, 0, 0, 1.0, p + 4, None, None) == -1
    assert bool((buf == 3).all())
