"""Cosine codebook lookup (MODEL.CODEBOOK.COSINE, csrc/l2norm.hip) on the device.  The reference has no such lookup:
the yardsticks are float64 torch on the CPU (F.normalize and autograd) for the two kernels and lvt_amd/modeling/vq/cosine.py,
fed the device's own z_e and pre-step codebook state, for the model.

Bounds.  Kernels: rel_err(y) < 1e-6, | ||y|| - 1 | <= 1e-6, inv 1e-6 relative, rel_err(dx) < 1e-5 -- what tests/test_gpu_norm.py
holds the batch-norm apply and backward kernels to; a sum of at most 1024 squares and one reciprocal square root stay inside them.
Model: indices equal on every row that passes util_models.margin_ok(rel=1e-4), which may leave out at most 2 % of the rows
(tests/test_host_cosine_codebook.py measures 0.07 .. 0.64 % on random unit vectors); z_q_st, z_q_bar and the codebook state
rel_err < 1e-5 and the commitment loss 2e-4 relative, as tests/test_gpu_vq_geometry.py holds the same quantities; the gradient at
z_e within max(2e-5, 4 x the CPU fp32 evaluation's distance) of the float64 evaluation of the same graph with the same indices."""
import functools

import pytest
import torch
import torch.nn.functional as F

import seeded
from conftest import rel_err
from util_models import margin_ok, vqvae_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-12
SHAPES = [(1, 1, 16), (3, 4, 64), (257, 4, 64), (130, 3, 48), (65, 1, 256), (4099, 2, 128), (33, 1, 1024), (70001, 4, 64)]


def _gen(tag):
    g = torch.Generator()
    g.manual_seed(tag)
    return g


@functools.lru_cache(maxsize=None)
def _kernel_case(rows, G, d):
    """(x, g, float64 y, float64 dx, float64 inv) of one shape: computed once on the CPU, shared by the tests, never written."""
    x = torch.randn(rows, G * d, generator=_gen(rows + G + d)) * 1.5
    g = torch.randn(rows, G * d, generator=_gen(rows + G + d + 1))
    return (x, g) + _fp64_rule(x, g, d)


def _fp64_rule(x, g, d):
    leaf = x.double().requires_grad_(True)
    y = F.normalize(leaf.view(x.shape[0], -1, d), dim=-1, eps=EPS).flatten(-2)
    y.backward(g.double())
    inv = 1.0 / x.double().view(x.shape[0], -1, d).norm(dim=-1).clamp_min(EPS)
    return y.detach(), leaf.grad, inv


def _run(x, g, d, **kw):
    from lvt_amd.hip import l2norm
    xd = x.to(DEV)
    y, inv = l2norm.l2norm_groups_fwd(xd, d, **kw)
    dx = l2norm.l2norm_groups_bwd(g.to(DEV), y, inv, d) if inv is not None else None
    return xd, y, inv, dx


# ---- the kernels against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,G,d", SHAPES)
def test_kernels_against_fp64(rows, G, d):
    """One row, a lane segment that is no power of two wide (d 48), a looping lane (d 1024), row counts off every block size, the
    shipped geometry."""
    x, g, y64, dx64, inv64 = _kernel_case(rows, G, d)
    xd, y, inv, dx = _run(x, g, d)
    assert torch.equal(xd.cpu(), x)                                           # out of place: the input is untouched
    e_y, e_dx = rel_err(y, y64), rel_err(dx, dx64)
    e_n = float((y.double().view(rows, G, d).norm(dim=-1) - 1).abs().max())
    e_inv = float(((inv.double().cpu() - inv64) / inv64).abs().max())
    print("(%d, %d, %d): y %.3g  | |y| - 1 | %.3g  inv %.3g  dx %.3g" % (rows, G, d, e_y, e_n, e_inv, e_dx))
    assert tuple(inv.shape) == (rows, G)
    assert e_y < 1e-6
    assert e_n <= 1e-6
    assert e_inv <= 1e-6
    assert e_dx < 1e-5


@pytest.mark.parametrize("G,d", [(4, 64), (1, 1024), (3, 48)])
def test_clamped_groups(G, d):
    """A zero group and a group of elements around 1e-20 (norm below eps): y = x / eps and dx = g / eps, inv == 1 / eps exactly.
    Their dx = g * 1e12 would swamp a max-relative error over a tensor with ordinary groups in it, so the clamped groups and
    the ordinary ones are compared separately, and a tensor in which every group is clamped is compared whole."""
    rows = 5
    x = torch.randn(rows, G * d, generator=_gen(7)) * 0.7
    x[1, :d] = 0.0
    x[3, -d:] = torch.randn(d, generator=_gen(8)) * 1e-20
    clamped = torch.zeros(rows, G, dtype=torch.bool)
    clamped[1, 0] = clamped[3, G - 1] = True
    g = torch.randn(rows, G * d, generator=_gen(9))
    r_eps = (torch.ones(1) / torch.tensor(EPS, dtype=torch.float32)).item()   # the fp32 quotient
    for xs, mask in ((x, clamped), (torch.randn(rows, G * d, generator=_gen(10)) * 1e-20, torch.ones(rows, G, dtype=torch.bool)),
                     (torch.zeros(rows, G * d), torch.ones(rows, G, dtype=torch.bool))):
        y64, dx64, inv64 = _fp64_rule(xs, g, d)
        _, y, inv, dx = _run(xs, g, d)
        el = mask[:, :, None].expand(rows, G, d).reshape(rows, G * d)
        assert bool((inv.cpu()[mask] == r_eps).all())
        assert bool((inv.cpu()[~mask] != r_eps).all())
        assert torch.isfinite(y).all() and torch.isfinite(dx).all()
        for part in (el, ~el):
            if bool(part.any()):
                if float(y64[part].abs().max()) > 0:
                    assert rel_err(y.cpu()[part], y64[part]) < 1e-6
                else:
                    assert bool((y.cpu()[part] == 0).all())
                assert rel_err(dx.cpu()[part], dx64[part]) < 1e-5
        if bool((~mask).any()):
            assert float(((inv.double().cpu() - inv64) / inv64).abs()[~mask].max()) <= 1e-6


@pytest.mark.parametrize("rows,G,d", [(257, 4, 64), (33, 1, 1024), (130, 3, 48)])
def test_in_place_and_null_inv(rows, G, d):
    from lvt_amd.hip import l2norm
    x, g, _, _, _ = _kernel_case(rows, G, d)
    _, y, inv, _ = _run(x, g, d)
    xd = x.to(DEV)
    y2, inv2 = l2norm.l2norm_groups_fwd(xd, d, inplace=True)
    assert y2 is xd and torch.equal(y2, y) and torch.equal(inv2, inv)
    y3, inv3 = l2norm.l2norm_groups_fwd(x.to(DEV), d, want_inv=False)
    assert inv3 is None and torch.equal(y3, y)
    # a 3-D tensor is rows x groups of its last dimension (the flat codebook buffer)
    y4, _ = l2norm.l2norm_groups_fwd(x.to(DEV).view(rows * G, 1, d), d, want_inv=False)
    assert torch.equal(y4.view(rows, G * d), y)


def test_max_records_and_run_to_run_bits():
    """f16x2 mode: both launches leave a valid max-|.| record that bounds the tensor, without a stand-alone scan; two runs at
    (70001, 4, 64) give the same bits."""
    from lvt_amd.hip import binding as L
    assert L.get_math_mode() == "f16x2"
    rows, G, d = 70001, 4, 64
    x, g, _, _, _ = _kernel_case(rows, G, d)
    before = L.AMAX_FALLBACKS[0]
    _, y, inv, dx = _run(x, g, d)
    assert float(L.amax_of(y)) >= float(y.abs().max()) > 0
    assert float(L.amax_of(dx)) >= float(dx.abs().max()) > 0
    assert float(L.amax_of(y)) <= 1.0 + 1e-6
    assert L.AMAX_FALLBACKS[0] == before
    _, y2, inv2, dx2 = _run(x, g, d)
    assert torch.equal(y, y2) and torch.equal(inv, inv2) and torch.equal(dx, dx2)
    for rows, G, d in ((33, 1, 1024), (130, 3, 48)):
        x, g, _, _, _ = _kernel_case(rows, G, d)
        _, y, _, dx = _run(x, g, d)
        assert float(L.amax_of(y)) >= float(y.abs().max()) and float(L.amax_of(dx)) >= float(dx.abs().max())


# ---- the model ------------------------------------------------------------------------------------------------------------------------
SEED = 31


def _unit_state(num, K, d):
    """tests/golden/seeded.py's codebook state put on the sphere: unit rows, its running_size, running_sum = weight * size."""
    st = seeded.seeded_codebook_state(SEED, num=num, K=K, D=d, scale=1.0)
    for i in range(num):
        w = F.normalize(st["ve.%d.embedding.weight" % i], dim=-1)
        st["ve.%d.embedding.weight" % i] = w
        st["ve.%d.running_sum" % i] = w * st["ve.%d.running_size" % i][:, None]
    return st


def _model(num=4, K=512, dim=256, cosine=True, restart=False, key=True):
    from lvt_amd.modeling import build_model
    cfg = vqvae_cfg(DEV)
    cb = cfg.MODEL.CODEBOOK
    cb.NUM, cb.SIZE, cb.DIM = num, K, dim
    if key:
        cb.COSINE = cosine
    if restart:
        cb.RESTART.ENABLED, cb.RESTART.THRESHOLD = True, 1.0
    if dim != 256:
        # a generic width needs coders of that many channels: the plain conv family at NF 16 (16 x 16 latents)
        import convcoders_cfg as CC
        CC.apply(cfg, dict(CC.overrides("a"), **{"MODEL.ENCODER.NF": 16, "MODEL.GENERATOR.NF": 16, "MODEL.ENCODER.OUT_CHANNELS": dim,
                                                 "MODEL.GENERATOR.IN_CHANNELS": dim}))
        torch.manual_seed(SEED)
    model = build_model(cfg)
    if dim == 256:
        model.encoder.load_state_dict(seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, SEED, "enc."))
        model.generator.load_state_dict(seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, SEED, "dec."))
    st = _unit_state(num, K, dim // num)
    model.codebook.load_state_dict({k[len("ve.0."):]: v for k, v in st.items()} if num == 1 else st)
    return model.train()


def _frames(tag, n=4):
    return torch.stack([seeded.seeded_input("cosine.%s.%d" % (tag, i), (3, 64, 64), SEED) for i in range(n)])


def _state(model):
    """(weight (num, K, d), running_size (num, K), running_sum (num, K, d)) on the CPU, copies."""
    sd = {k: v.detach().cpu().clone() for k, v in model.codebook.state_dict().items()}
    num = model.codebook.num
    pre = ["ve.%d." % i for i in range(num)] if hasattr(model.codebook, "ve") else [""]
    return tuple(torch.stack([sd[p + k] for p in pre]) for k in ("embedding.weight", "running_size", "running_sum"))


def _step(model, x):
    """One supervised step (forward + backward) -> (losses, what passed between the encoder, the quantiser and the decoder)."""
    from lvt_amd.utils.events import EventStorage
    seen = {}
    enc, cbk = model.encoder, model.codebook
    enc_fwd, st_cl, fin = enc.forward_cl, cbk.straight_through_cl, cbk.finish_ema

    def forward_cl(x_cl):
        z = enc_fwd(x_cl)
        z.retain_grad()
        seen["z_e"] = z
        return z

    def straight_through_cl(u, defer=False):
        seen["u"] = u
        out = st_cl(u, defer=defer)
        seen["z_q_st"] = out.detach().clone()
        out.register_hook(lambda g: seen.__setitem__("g_st", g.detach().clone()))
        return out

    def finish_ema():
        seen["z_q_bar"] = fin()
        return seen["z_q_bar"]

    enc.forward_cl, cbk.straight_through_cl, cbk.finish_ema = forward_cl, straight_through_cl, finish_ema
    try:
        for p in model.parameters():
            p.grad = None
        with EventStorage(0):
            losses = model([{"image": x[i].numpy()} for i in range(x.shape[0])], mode="supervised")
        sum(losses.values()).backward()
    finally:
        del enc.forward_cl, cbk.straight_through_cl, cbk.finish_ema
    idx = cbk.last_indices.cpu()
    idx = idx.unsqueeze(1) if idx.dim() == 3 else idx                              # (N, num, h, w)
    D = seen["z_e"].shape[-1]
    out = {k: seen[k].detach().cpu().reshape(-1, D) for k in ("z_e", "u", "z_q_st", "z_q_bar", "g_st")}
    out["dz"] = seen["z_e"].grad.detach().cpu().reshape(-1, D)
    out["idx"] = idx.permute(0, 2, 3, 1).reshape(-1, idx.shape[1])                  # (rows, num)
    return losses, out


def _check_indices(tag, pre_w, z_e, idx):
    """The device's codes == the float64 rule's on every margin row; the margin rule leaves out at most 2 % of the rows."""
    from lvt_amd.modeling.vq import cosine as C
    num, K, d = pre_w.shape
    u64 = C.normalise(z_e.double(), d)
    left_out = 0
    for i in range(num):
        ui = u64[:, d * i:d * (i + 1)]
        ok = margin_ok(ui, pre_w[i], rel=1e-4)
        left_out += int((~ok).sum())
        want = C.nearest(ui, pre_w[i].double())
        assert torch.equal(idx[:, i][ok], want[ok]), (tag, i)
    share = left_out / float(num * z_e.shape[0])
    print("%s: margin rule leaves out %.3f %% of %d rows" % (tag, 100 * share, num * z_e.shape[0]))
    assert share <= 0.02, (tag, share)
    return u64


def _check_step(model, x, tag, numerics=True):
    from lvt_amd.modeling.vq import cosine as C
    pre = _state(model)
    num, K, d = pre[0].shape
    beta = model.beta
    losses, got = _step(model, x)
    post = _state(model)
    u64 = _check_indices(tag, pre[0], got["z_e"], got["idx"])
    assert rel_err(got["u"], u64) < 1e-6
    unit = float((post[0].double().norm(dim=-1) - 1).abs().max())
    print("%s: | |e| - 1 | %.3g" % (tag, unit))
    assert unit <= 1e-6
    # z_q_st is a pure gather of the pre-step codebook, z_q_bar of the post-step one
    own = torch.cat([pre[0][i][got["idx"][:, i]] for i in range(num)], -1)
    assert torch.equal(got["z_q_st"], own)
    assert torch.equal(got["z_q_bar"], torch.cat([post[0][i][got["idx"][:, i]] for i in range(num)], -1))
    if not numerics:
        return losses, got

    def rule(dtype):
        z = got["z_e"].to(dtype).requires_grad_(True)
        out = C.step(*(t.to(dtype) for t in pre), z, beta=beta, force_idx=got["idx"])
        ((out["z_q_st"] * got["g_st"].to(dtype)).sum() + out["loss_commitment"]).backward()
        return out, z.grad

    ref, dz64 = rule(torch.float64)
    _, dz32 = rule(torch.float32)
    assert rel_err(got["z_q_st"], ref["z_q_st"].detach()) < 1e-5
    assert rel_err(got["z_q_bar"], ref["z_q_bar"]) < 1e-5
    for name, mine, want in (("weight", post[0], ref["weight"]), ("running_size", post[1], ref["running_size"]),
                             ("running_sum", post[2], ref["running_sum"])):
        e = max(rel_err(mine[i], want[i]) for i in range(num))
        print("%s: %s %.3g" % (tag, name, e))
        assert e < 1e-5, (tag, name)
    a, b = float(losses["loss_commitment"]), float(ref["loss_commitment"])
    print("%s: loss_commitment %.9g float64 %.9g" % (tag, a, b))
    assert abs(a - b) < 2e-4 * b
    e_mine, e_cpu = rel_err(got["dz"], dz64), rel_err(dz32, dz64)
    print("%s: gradient at z_e %.3g (CPU fp32 %.3g)" % (tag, e_mine, e_cpu))
    assert e_mine <= max(2e-5, 4 * e_cpu), (tag, e_mine, e_cpu)
    return losses, got


def test_shipped_geometry_three_steps():
    """PR-DVQVAE2 (4 codebooks of 512 x 64), 4 frames, three consecutive train steps, each against cosine.py in float64 fed the
    device's own z_e and pre-step codebook state."""
    model = _model()
    assert model.codebook.cosine
    for step in range(3):
        _check_step(model, _frames("s%d" % step), "step %d" % step)


def test_shipped_geometry_with_restart():
    """The same three steps with RESTART.ENABLED, THRESHOLD 1.0: the rows stay unit (a restarted code is a row of u), the health
    record is written, the indices agree with the rule."""
    model = _model(restart=True)
    assert model.codebook.restart_enabled and model.codebook_health() is not None
    for step in range(3):
        _check_step(model, _frames("s%d" % step), "restart step %d" % step, numerics=False)
        perplexity, dead, restarts = (float(v) for v in model.codebook_health())
        print("restart step %d: perplexity %.4g dead %d restarts %d" % (step, perplexity, dead, restarts))
        assert 1.0 <= perplexity <= 512.0 and dead >= 0
    assert int(model.codebook.restart_pass) == 3
    assert restarts > 0                                  # (seeded running_size 0.5 .. 4 decays below 1.0 on unused codes)


@pytest.mark.parametrize("num,K,dim", [(1, 512, 256), (2, 128, 96)], ids=["single-256", "generic-2x48"])
def test_other_geometries_one_step(num, K, dim):
    """NUM 1: SingleVQEmbedding, the whole 256-wide row is one group.  NUM 2, DIM 96, SIZE 128: the generic search and a lane
    segment that is no power of two wide."""
    model = _model(num, K, dim)
    assert model.codebook.cosine and type(model.codebook).__name__ == ("SingleVQEmbedding" if num == 1 else "DVQEmbedding")
    _check_step(model, _frames("g%d" % num), "NUM %d DIM %d" % (num, dim))


# ---- off, eval, reproducibility --------------------------------------------------------------------------------------------------------
class _Counter:
    def __init__(self, monkeypatch):
        from lvt_amd.hip import l2norm
        self.n = {"fwd": 0, "bwd": 0}
        for short, name in (("fwd", "l2norm_groups_fwd"), ("bwd", "l2norm_groups_bwd")):
            monkeypatch.setattr(l2norm, name, self._wrap(short, getattr(l2norm, name)))

    def _wrap(self, short, fn):
        def wrapped(*a, **kw):
            self.n[short] += 1
            return fn(*a, **kw)
        return wrapped


def _three_steps(model):
    out = []
    for step in range(3):
        losses, got = _step(model, _frames("s%d" % step))
        out.append(([float(v) for _, v in sorted(losses.items())], got["dz"], got["idx"]))
    return out, _state(model), [p.grad.detach().cpu().clone() for p in model.encoder.parameters()]


def test_off_launches_nothing_new_and_changes_no_bit(monkeypatch):
    """COSINE False: a train step calls neither wrapper, and losses, gradients and codebook bits after three steps are those of a
    model whose config never set the key."""
    calls = _Counter(monkeypatch)
    a = _three_steps(_model(cosine=False))
    b = _three_steps(_model(key=False))
    assert calls.n == {"fwd": 0, "bwd": 0}
    for (la, da, ia), (lb, db, ib) in zip(a[0], b[0]):
        assert la == lb and torch.equal(da, db) and torch.equal(ia, ib)
    assert all(torch.equal(s, t) for s, t in zip(a[1], b[1]))
    assert all(torch.equal(s, t) for s, t in zip(a[2], b[2]))
    # the codebook was not put on the sphere by anything
    assert float((a[1][0].norm(dim=-1) - 1).abs().max()) > 1e-4


def test_train_step_is_bit_reproducible(monkeypatch):
    """COSINE True: two models from the same state give the same bits over three steps; a step launches the forward kernel twice
    (z_e, the codebook) and the backward kernel once."""
    calls = _Counter(monkeypatch)
    a = _three_steps(_model())
    assert calls.n == {"fwd": 6, "bwd": 3}
    b = _three_steps(_model())
    for (la, da, ia), (lb, db, ib) in zip(a[0], b[0]):
        assert la == lb and torch.equal(da, db) and torch.equal(ia, ib)
    assert all(torch.equal(s, t) for s, t in zip(a[1], b[1]))
    assert all(torch.equal(s, t) for s, t in zip(a[2], b[2]))


@pytest.mark.parametrize("num", [4, 1])
def test_eval_encode_inference_decode(num):
    """encode, mode="inference" and the quantiser's forward(z, "") normalise before the search: the codes of the float64 rule on
    margin rows; decode(encode(x)) runs (the codebook already holds unit rows)."""
    from oracle import lvt_oracle as O
    from util_models import MEAN, STD
    model = _model(num, 512, 256).eval()
    x = _frames("eval", 2)
    xn = O.normalize(x, MEAN, STD).to(DEV)
    w = _state(model)[0]
    with torch.no_grad():
        z_e = model.encoder(xn)                                                  # (2, 256, 16, 16)
        lat = model.encode(xn)
        out = model([{"image": x[i].numpy()} for i in range(2)], mode="inference")
        direct = model.codebook(z_e)
        rec = model.decode(lat)
    assert torch.equal(w, _state(model)[0])                                      # no EMA update in any of these
    shape = (2, 16, 16) if num == 1 else (2, num, 16, 16)
    assert tuple(lat.shape) == shape and lat.dtype == torch.int64
    assert torch.equal(direct, lat)
    assert torch.equal(torch.stack([o["latent"] for o in out]), lat)
    assert tuple(rec.shape) == (2, 3, 64, 64) and bool(torch.isfinite(rec).all())
    rows = z_e.cpu().permute(0, 2, 3, 1).reshape(-1, 256)
    idx = (lat.unsqueeze(1) if num == 1 else lat).cpu().permute(0, 2, 3, 1).reshape(-1, num)
    _check_indices("eval NUM %d" % num, w, rows, idx)
