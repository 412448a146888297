"""Host side of finite scalar quantisation (MODEL.CODEBOOK.FSQ.LEVELS): the rule of lvt_amd/modeling/vq/fsq.py in
float64 (digit range, the index as a bijection, decode of encode, the gradient against autograd of the smooth part), the config
key and every refusal of the model, off is off, state-dict keys and optimizer groups, the exempt share of the GPU tests' cases
on the float64 rule alone, and the null-launch refusals of the three entry points."""
import glob
import math
import os
import re

import pytest
import torch

import util_fsq as U
from conftest import ROOT, rel_err

LEVEL_SETS = [(8, 8, 8), (8, 5, 5), (8, 5, 5, 5), (2,) * 11, (64,), (7, 5, 5, 5, 2), (3, 2, 4)]


def _cfg(levels=None, **kw):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.CODEBOOK.EMA = False
    if levels is not None:
        cfg.MODEL.CODEBOOK.FSQ.LEVELS = levels
    for k, v in kw.items():
        node, parts = cfg.MODEL.CODEBOOK, k.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    return cfg


# ---- the rule in float64 -------------------------------------------------------------------------------------------------
def test_digits_stay_in_range_for_every_level_and_scale():
    """L from 2 to 64 at input scales 1 to 30, and at the ends of the float64 range of tanh: digit = round(b) + w in [0, L - 1]."""
    from lvt_amd.modeling.vq import fsq as R
    gen = torch.Generator().manual_seed(0)
    for L in range(2, 65):
        for scale in (1.0, 3.0, 10.0, 30.0):
            z = torch.cat([torch.randn(2000, 1, dtype=torch.float64, generator=gen) * scale,
                           torch.tensor([[-1e3], [1e3], [0.0], [-40.0], [40.0]], dtype=torch.float64)])
            d = R.digits(z, (L,))
            assert int(d.min()) >= 0 and int(d.max()) <= L - 1, (L, scale)
            if scale == 30.0:
                assert int(d.min()) == 0 and int(d.max()) == L - 1, L             # saturation reaches both ends
            v = R.value_of(d, (L,))
            assert float(v.min()) >= -1.0 and float(v.max()) <= 1.0


@pytest.mark.parametrize("levels", LEVEL_SETS, ids=str)
def test_index_is_a_bijection_and_decode_inverts_encode(levels):
    from lvt_amd.modeling.vq import fsq as R
    V = math.prod(levels)
    codes = torch.arange(V)
    dig = R.digits_of(codes.unsqueeze(-1), levels)                              # (V, d)
    assert all(int(dig[:, i].min()) == 0 and int(dig[:, i].max()) == L - 1 for i, L in enumerate(levels))
    assert torch.equal(R.index(dig, levels).squeeze(-1), codes)                   # index o digits_of = id on all V codes
    assert len({tuple(r) for r in dig.tolist()}) == V                             # and digits_of is injective
    assert int(dig[1, 0]) == 1 and int(dig[1, 1:].sum()) == 0                     # first level fastest
    # every code is reached: the z_p whose bound is the digit's centre encodes to that digit
    half_l, offset, shift, w, _ = R.constants(levels)
    z_p = torch.atanh((dig - w + offset) / half_l) - shift
    z_q, idx = R.quantise(z_p, levels)
    assert torch.equal(idx.squeeze(-1), codes)
    assert torch.equal(z_q, R.value_of(dig, levels))
    # decode(encode) on random rows of 3 groups: the values the encoder produced, bit for bit
    z = torch.randn(500, 3 * len(levels), dtype=torch.float64, generator=torch.Generator().manual_seed(V)) * 2.0
    z_q, idx = R.quantise(z, levels)
    assert tuple(idx.shape) == (500, 3) and int(idx.min()) >= 0 and int(idx.max()) < V
    assert torch.equal(R.value_of(R.digits_of(idx, levels), levels), z_q)
    w_out = torch.randn(16, 3 * len(levels), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    b_out = torch.randn(16, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    assert torch.equal(R.decode(idx, w_out, b_out, levels), R.project_out(z_q, w_out, b_out))


@pytest.mark.parametrize("levels", LEVEL_SETS, ids=str)
def test_gradient_is_autograd_of_the_smooth_part(levels):
    """The straight-through estimator goes through the rounding only: the gradient of quantise is that of bound / w."""
    from lvt_amd.modeling.vq import fsq as R
    gen = torch.Generator().manual_seed(len(levels))
    z = torch.randn(64, 2 * len(levels), dtype=torch.float64, generator=gen) * 1.5
    g = torch.randn(64, 2 * len(levels), dtype=torch.float64, generator=gen)
    w = R.constants(levels)[3].double().repeat(2)
    smooth = z.clone().requires_grad_(True)
    (R.bound(smooth, levels) / w).backward(g)
    st = z.clone().requires_grad_(True)
    R.quantise(st, levels)[0].backward(g)
    assert rel_err(st.grad, smooth.grad) < 1e-14
    assert rel_err(R.quantise_backward(g, z, levels), smooth.grad) < 1e-14
    # through both projections: ordinary linear backward around it
    D = 24
    w_in, b_in = torch.randn(2 * len(levels), D, dtype=torch.float64, generator=gen), torch.randn(2 * len(levels), dtype=torch.float64, generator=gen)
    w_out, b_out = torch.randn(D, 2 * len(levels), dtype=torch.float64, generator=gen), torch.randn(D, dtype=torch.float64, generator=gen)
    z_e = torch.randn(64, D, dtype=torch.float64, generator=gen).requires_grad_(True)
    g_out = torch.randn(64, D, dtype=torch.float64, generator=gen)
    out = R.step(z_e, w_in, b_in, w_out, b_out, levels)
    out["z_out"].backward(g_out)
    want = R.quantise_backward(g_out @ w_out, out["z_p"].detach(), levels) @ w_in
    assert rel_err(z_e.grad, want) < 1e-13
    # force_idx: the value of the forced codes, the gradient of the rule
    z_e2 = z_e.detach().clone().requires_grad_(True)
    forced = (out["idx"] + 1) % math.prod(levels)
    out2 = R.step(z_e2, w_in, b_in, w_out, b_out, levels, force_idx=forced)
    assert torch.equal(out2["z_q"].detach(), R.value_of(R.digits_of(forced, levels), levels))
    out2["z_out"].backward(g_out)
    assert rel_err(z_e2.grad, want) < 1e-13


def test_constants_are_the_issue_s():
    from lvt_amd.modeling.vq import fsq as R
    half_l, offset, shift, w, basis = R.constants((8, 5, 2))
    assert half_l.tolist() == [7 * 1.001 / 2, 4 * 1.001 / 2, 1 * 1.001 / 2]
    assert offset.tolist() == [0.5, 0.0, 0.5] and w.tolist() == [4, 2, 1] and basis.tolist() == [1, 8, 40]
    assert shift.tolist() == [math.atanh(0.5 / (7 * 1.001 / 2)), 0.0, math.atanh(0.5 / (1.001 / 2))]
    # round half to even
    assert torch.round(torch.tensor([0.5, 1.5, 2.5, -0.5], dtype=torch.float64)).tolist() == [0.0, 2.0, 2.0, -0.0]


@pytest.mark.parametrize("c", U.KERNEL_CASES, ids=U.case_id)
def test_gpu_cases_keep_the_exempt_share_on_the_float64_rule(c):
    """The condition of tests/test_gpu_fsq.py, checked where no device takes part: at most 1 % of a case's elements lie within
    2^-14 of a rounding boundary (a one-row case must have none)."""
    k = U.kernel_case(*c)
    share = float(k["exempt"].double().mean())
    print("%s: %d of %d elements exempt" % (U.case_id(c), int(k["exempt"].sum()), k["exempt"].numel()))
    assert share <= U.EXEMPT_SHARE
    assert torch.equal(k["z_p"][:, k["nd"]:], torch.zeros(c[0], k["ld"] - k["nd"]))
    assert int(k["idx"].min()) >= 0 and int(k["idx"].max()) < math.prod(c[2])


@pytest.mark.parametrize("c", U.MODULE_CASES, ids=U.module_case_id)
def test_gpu_module_cases_keep_the_exempt_share(c):
    """The same condition for the FSQEmbedding cases, whose exempt set is wider by the engine's bound on the projection."""
    e = U.module_case(*c)["exempt"]
    print("%s: %d of %d elements exempt" % (U.module_case_id(c), int(e.sum()), e.numel()))
    assert float(e.double().mean()) <= U.EXEMPT_SHARE


# ---- config and model ------------------------------------------------------------------------------------------------------
def test_default_and_shipped_yamls():
    from lvt_amd.config import get_cfg
    assert get_cfg().MODEL.CODEBOOK.FSQ.LEVELS == []
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "*", "*.yaml"))):
        cfg = get_cfg()
        cfg.merge_from_file(path)
        assert cfg.MODEL.CODEBOOK.FSQ.LEVELS == [], path
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.CODEBOOK.FSQ.LEVELS", "[8, 8, 8]"])
    assert cfg.MODEL.CODEBOOK.FSQ.LEVELS == [8, 8, 8]
    cfg.merge_from_list(["MODEL.CODEBOOK.FSQ.LEVELS", "(8, 5, 5)"])
    assert cfg.MODEL.CODEBOOK.FSQ.LEVELS == [8, 5, 5]


@pytest.mark.parametrize("levels,kw,names", [
    ([8, 8, 8.5], {}, ["MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 8, "8"], {}, ["MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 8, True], {}, ["MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([512, 1], {}, ["MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 65], {"SIZE": 520}, ["MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 8, -8], {}, ["MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([2] * 12, {"SIZE": 4096}, ["MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 8, 8, 8], {"SIZE": 4096}, ["MODEL.CODEBOOK.FSQ.LEVELS", "2048"]),
    ([8, 8, 8], {"SIZE": 1024}, ["MODEL.CODEBOOK.SIZE", "MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 5, 5], {}, ["MODEL.CODEBOOK.SIZE", "MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 8, 8], {"EMA": True}, ["MODEL.CODEBOOK.EMA", "False", "MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 8, 8], {"COSINE": True}, ["MODEL.CODEBOOK.COSINE", "MODEL.CODEBOOK.FSQ.LEVELS"]),
    ([8, 8, 8], {"RESTART.ENABLED": True}, ["MODEL.CODEBOOK.RESTART.ENABLED", "MODEL.CODEBOOK.FSQ.LEVELS"]),
], ids=lambda v: re.sub(r"[^0-9A-Za-z_.]+", "-", str(v)))
def test_refusals_name_the_keys(levels, kw, names):
    from lvt_amd.modeling import build_model
    with pytest.raises(ValueError) as e:
        build_model(_cfg(levels, **kw))
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_base_yaml_needs_ema_false():
    """Base-VQVAE.yaml sets EMA True: FSQ on top of a shipped config says what to change."""
    from lvt_amd.config import get_cfg
    from lvt_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    assert cfg.MODEL.CODEBOOK.EMA is True
    cfg.MODEL.CODEBOOK.FSQ.LEVELS = [8, 8, 8]
    with pytest.raises(ValueError, match="MODEL.CODEBOOK.EMA to False"):
        build_model(cfg)


@pytest.mark.parametrize("levels,size,num", [([8, 8, 8], 512, 4), ([8, 5, 5], 200, 1), ([2] * 11, 2048, 2), ([64], 64, 4),
                                             ([8, 5, 5, 5], 1000, 4)])
def test_accepted_geometries_keys_and_optimizer_groups(levels, size, num, tmp_path):
    from lvt_amd.modeling import build_model
    from lvt_amd.modeling.vq import FSQEmbedding
    cfg = _cfg(levels, SIZE=size, NUM=num)
    cfg.OUTPUT_DIR = str(tmp_path)
    torch.manual_seed(0)
    model = build_model(cfg)
    q = model.codebook
    nd = num * len(levels)
    assert isinstance(q, FSQEmbedding) and (q.num, q.levels, q.D, q.K) == (num, tuple(levels), 256, size)
    assert q.width == (nd + 3) // 4 * 4
    assert list(q.state_dict().keys()) == ["proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias"]
    assert [tuple(v.shape) for v in q.state_dict().values()] == [(nd, 256), (nd,), (256, nd), (256,)]
    assert list(q.named_buffers()) == []
    assert [k for k in model.state_dict() if k.startswith("codebook.")] == ["codebook." + k for k in q.state_dict()]
    # initialised by INIT_TYPE like every other Linear (PR-DVQVAE2: xavier_uniform, std sqrt(2 / (fan_in + fan_out))), zero biases
    assert cfg.MODEL.INIT_TYPE == "xavier_uniform"
    assert bool((q.proj_in.bias == 0).all()) and bool((q.proj_out.bias == 0).all())
    for w in (q.proj_in.weight.detach(), q.proj_out.weight.detach()):
        want = math.sqrt(2.0 / (256 + nd))
        assert abs(float(w.std()) - want) < 0.2 * want and float(w.abs().max()) <= want * math.sqrt(3.0) * (1 + 1e-6)
    assert all(p.requires_grad for p in q.parameters())
    assert model.codebook_health() is None and q.health_scalars() is None
    assert len(q._flat()) == 4 and all(a.data_ptr() == b.data_ptr() for a, b in zip(q._flat(), q.parameters()))
    z = torch.zeros(1, 1, 2, 2, 256)
    assert q.normalise_cl(z) is z
    # the trained-codebook route: a third optimizer over exactly the four tensors, the netC checkpointer
    opts, ckpts = model.configure_optimizers_and_checkpointers()
    assert len(opts) == 3 and len(ckpts) == 3
    own = [p for g in opts[2]["optimizer"].param_groups for p in g["params"]]
    assert len(own) == 4 and {id(p) for p in own} == {id(p) for p in q.parameters()}
    assert ckpts[2]["checkpointer"].model is q if hasattr(ckpts[2]["checkpointer"], "model") else True
    assert os.path.isdir(os.path.join(str(tmp_path), "netC"))
    gen_ids = {id(p) for p in model._generator_parameters()}
    assert {id(p) for p in q.parameters()} <= gen_ids


def test_off_is_off_on_the_host():
    """LEVELS [] (the default, or set): the module tree, the state-dict keys and shapes, and the initial weights bit for bit are
    those of a model whose config never heard of the key; no FSQ module exists."""
    from lvt_amd.modeling import build_model
    from lvt_amd.modeling.vq import DVQEmbedding, SingleVQEmbedding

    def build(num, ema, levels):
        cfg = _cfg(levels, NUM=num, EMA=ema)
        torch.manual_seed(5)
        return build_model(cfg)

    for num, ema in ((4, True), (4, False), (1, True)):
        a, b = build(num, ema, None), build(num, ema, [])
        assert type(a.codebook) is type(b.codebook) is (SingleVQEmbedding if num == 1 else DVQEmbedding)
        assert a.fsq is False and b.fsq is False
        assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
        pre = ["ve.%d." % i for i in range(num)] if num > 1 else [""]
        want = [p + k for p in pre for k in ((["running_size", "running_sum"] if ema else []) + ["embedding.weight"])]
        assert sorted(a.codebook.state_dict().keys()) == sorted(want)               # the reference's names, as ever
        assert not any("proj_" in k for k in sa)


def test_module_refuses_what_the_kernels_do_not_take():
    from lvt_amd.hip import binding as L
    from lvt_amd.modeling.vq import FSQEmbedding
    for bad in ([], [1, 8], [65], [8.0, 8], [2] * 12, [8, 8, 8, 8]):
        with pytest.raises(ValueError):
            FSQEmbedding(4, bad, 256)
    with pytest.raises(ValueError):
        FSQEmbedding(0, [8, 8, 8], 256)
    with pytest.raises(NotImplementedError):
        FSQEmbedding(4, [8, 8, 8], 130)
    q = FSQEmbedding(1, [8, 5, 5], 64)
    assert q.width == 4 and tuple(w.shape for w in q._operands()) == ((4, 64), (4,), (64, 4))
    wi, bi, wo = q._operands()
    assert bool((wi[3] == 0).all()) and float(bi[3]) == 0 and bool((wo[:, 3] == 0).all())
    assert torch.equal(wi[:3], q.proj_in.weight) and torch.equal(wo[:, :3], q.proj_out.weight)
    with pytest.raises(L.LvtError):                                                # no CPU path
        q(torch.zeros(1, 64, 2, 2))
    with pytest.raises(L.LvtError):
        q(torch.zeros(1, 1, 2, 2, dtype=torch.int64), "emb")


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_table_and_null_launch_refusals():
    from lvt_amd.hip import binding as L, fsq as K
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    new = {"lvt_fsq_fwd", "lvt_fsq_bwd", "lvt_fsq_decode"}
    assert new <= set(L.declared_symbols())
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in text, name
    assert L.FSQ_MAX_LEVELS == 11 and "#define LVT_FSQ_MAX_LEVELS 11" in header
    lib = L.lib()
    p = 4096                                                               # a non-null, 16-byte aligned address
    ok = dict(x=p, rows=8, num=4, ld=12, lv=(8, 8, 8), P=4, zq=p, idx=p, am=None, g=p)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.lvt_fsq_fwd(a["x"], a["rows"], a["num"], a["ld"], K.table(a["lv"]), a["P"], a["zq"], a["idx"], a["am"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.lvt_fsq_bwd(a["g"], a["x"], a["rows"], a["num"], a["ld"], K.table(a["lv"]), a["zq"], a["am"], None)

    def dec(**kw):
        a = dict(ok, **kw)
        return lib.lvt_fsq_decode(a["idx"], a["rows"], a["num"], a["ld"], K.table(a["lv"]), a["P"], a["zq"], a["am"], None)

    empty = L.FsqLevels()
    geometry = (dict(rows=0), dict(rows=-3), dict(num=0), dict(ld=8), dict(ld=14), dict(ld=4100), dict(lv=(8, 8, 1)),
                dict(lv=(8, 65, 8)), dict(lv=(8, 0, 8)), dict(lv=(64,) * 6, ld=24), dict(am=p + 1), dict(zq=p + 4))
    for name, fn, extra in (("lvt_fsq_fwd", fwd, (dict(x=None), dict(zq=None, idx=None), dict(x=p + 8), dict(P=3), dict(P=0),
                                                  dict(idx=p + 4))),
                            ("lvt_fsq_bwd", bwd, (dict(x=None), dict(g=None), dict(zq=None), dict(g=p + 4), dict(x=p + 8))),
                            ("lvt_fsq_decode", dec, (dict(idx=None), dict(zq=None), dict(P=3), dict(P=-1), dict(idx=p + 2)))):
        for bad in geometry + extra:
            assert fn(**bad) == -1, (name, bad)
            assert name.encode() in lib.lvt_last_error(), (name, bad)
    # an empty table (d = 0) and more than 11 levels never reach a launch
    assert lib.lvt_fsq_fwd(p, 8, 4, 12, empty, 4, p, p, None, None) == -1
    empty.d = 12
    assert lib.lvt_fsq_decode(p, 8, 1, 12, empty, 4, p, None, None) == -1
    with pytest.raises(L.LvtError):
        K.table(())
    with pytest.raises(L.LvtError):
        K.table((2,) * 12)


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from lvt_amd.hip import binding as L, fsq as K
    with pytest.raises(L.LvtError):
        K.fsq_fwd(torch.zeros(4, 12), 4, (8, 8, 8))
    with pytest.raises(L.LvtError):
        K.fsq_bwd(torch.zeros(4, 12), torch.zeros(4, 12), 4, (8, 8, 8))
    with pytest.raises(L.LvtError):
        K.fsq_decode(torch.zeros(1, 4, 4, dtype=torch.int64), (8, 8, 8))
