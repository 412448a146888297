"""GPU parity of the generic-geometry quantiser (csrc/vq.hip, "GENERIC GEOMETRY"): any sub-vector width 16..256 (multiple
of 16) and codebook size 64..2048 (multiple of 64).  Tolerances as in test_gpu_vqvae.py: indices bit-exact on rows whose fp64
top-2 margin exceeds 1e-5 (|x|^2 + max |e|^2), losses 1e-5 relative, EMA sums 1e-6 relative of a float64 reference."""
import pytest
import torch

import seeded
from conftest import rel_err
from oracle import lvt_oracle as O
from util_models import MEAN, STD, margin_ok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("f16x2", "f32", "bf16x3")
SCALES = ((1.0, 1.0), (1e-20, 1e10), (1e12, 1e12), (1e-15, 1e-15), (3.0, 1.0 / 512))


def _search_all_modes(z, cb, P, **kw):
    from lvt_amd.hip import binding as L, vq
    assert L.get_math_mode() == "f16x2"
    out = {}
    for mode in MODES:
        L.set_math_mode(mode)
        try:
            out[mode] = vq.nearest(z.to(DEV), cb.to(DEV), P, **kw).cpu()
        finally:
            L.set_math_mode("f16x2")
    return out


GRID = [(dg, k) for dg in (16, 32, 128, 256) for k in (64, 1024, 2048)] + [(64, 1024), (64, 2048), (32, 512)]


@pytest.mark.parametrize("Dg,K", GRID)
def test_generic_search_shapes_and_scales(Dg, K):
    """Margin rows == the fp64 search in all three arithmetic modes; three groups, 112 rows (no multiple of the 32-row tile),
    operands 1e-20 .. 1e12 in size, an all-zero row (-> the code of smallest norm)."""
    torch.manual_seed(1000 * Dg + K)
    P, n, num = 16, 7, 3
    for zs, es in SCALES:
        z = torch.randn(n * P, num * Dg) * zs
        z[5] = 0
        cb = torch.randn(num, K, Dg) * es
        res = _search_all_modes(z, cb, P)
        for g in range(num):
            rows = z[:, Dg * g:Dg * (g + 1)]
            ok = margin_ok(rows, cb[g]).view(n, P)
            assert ok.float().mean() > 0.5, (Dg, K, zs, es, float(ok.float().mean()))
            ref = O.vq_margin_fp64(rows, cb[g])[2].view(n, P)
            for mode, idx in res.items():
                assert torch.equal(idx[:, g][ok], ref[ok]), (mode, Dg, K, zs, es, g)
                assert int(idx[0, g, 5]) == int((cb[g].double() ** 2).sum(-1).argmin()), (mode, Dg, K, zs, es, g)


@pytest.mark.parametrize("Dg", [16, 64, 256])
def test_generic_search_ties_across_code_tiles(Dg):
    """Exact duplicates of one code placed far apart (different LDS code tiles for every tile size) resolve to the lowest
    index, in every mode."""
    torch.manual_seed(Dg)
    K = 2048
    cb = torch.randn(K, Dg)
    # code mod 32 = 5, 28, 28, 31, 2, 9: duplicates in both half-waves of the f16x2 32-code sub-tile (registers 4 q + e hold
    # codes 8 q + e + 4 half), so the final exchange between the half-waves has to break a tie as well
    for j in (700, 1500, 2047, 1026, 1609):
        cb[j] = cb[5]
    pick = [5, 700, 9, 1500, 2047, 1000, 1026, 1609]
    z = cb[pick].repeat(32, 2).contiguous()                      # (256, 2 Dg): two groups
    for mode, idx in _search_all_modes(z, torch.stack([cb, cb]), 64).items():
        got = idx.permute(0, 2, 1).reshape(-1, 2)
        want = torch.tensor([5, 5, 9, 5, 5, 1000, 5, 5]).repeat(32)
        assert torch.equal(got[:, 0], want) and torch.equal(got[:, 1], want), mode


def test_forced_generic_matches_specialised_kernel():
    """LVT_VQ_GENERIC on the shipped geometry (Dg 64, K 512): the indices equal the f16x2 kernel's on every margin row."""
    from lvt_amd.hip import vq
    torch.manual_seed(3)
    P, n, num = 256, 16, 4
    z = torch.randn(n * P, num * 64)
    cb = torch.randn(num, 512, 64)
    zd, cbd = z.to(DEV), cb.to(DEV)
    a = vq.nearest(zd, cbd, P).cpu()
    b = vq.nearest(zd, cbd, P, generic=True).cpu()
    differ = 0
    for g in range(num):
        ok = margin_ok(z[:, 64 * g:64 * (g + 1)], cb[g]).view(n, P)
        assert torch.equal(a[:, g][ok], b[:, g][ok]), g
        differ += int((a[:, g][~ok] != b[:, g][~ok]).sum())
    print("forced generic vs f16x2 kernel: %d sub-margin rows differ" % differ)


@pytest.mark.parametrize("Dg,K", [(16, 2048), (32, 1024), (64, 2048), (128, 256), (256, 1024), (64, 512), (64, 128), (64, 1024)])
def test_generic_gather_exact(Dg, K):
    """Both instantiations of the gather kernel: the compile-time width 64 at the three codebook sizes that route the search
    and the statistics differently (512, 128: whole-codebook kernels; 1024, 2048: generic), and run-time widths."""
    from lvt_amd.hip import vq
    torch.manual_seed(Dg + K)
    n, num, P = 5, 3, 48
    cb = torch.randn(num, K, Dg)
    idx = torch.randint(0, K, (n, num, P))
    out = vq.gather(idx.to(DEV), cb.to(DEV)).cpu()
    ref = torch.stack([cb[g][idx[:, g]] for g in range(num)], 2)      # (n, P, num, Dg)
    assert torch.equal(out, ref.reshape(n * P, num * Dg))


EMA_GEOMETRIES = [(16, 2048), (32, 1024), (64, 2048), (64, 1024), (128, 256), (256, 1024), (256, 64), (64, 128), (64, 256), (64, 512)]


@pytest.mark.parametrize("Dg,K", EMA_GEOMETRIES)
def test_generic_ema_accumulate(Dg, K):
    """Counts exact, sums within 1e-6 relative of a float64 index_add_, two runs bit-identical (skewed code histogram).
    (64, 128 | 256 | 512) is the whole-codebook family of the statistics kernel, the rest the ranged one (width 16: threads with
    nothing to stage; width 256: all eight staging registers)."""
    _check_ema_accumulate(Dg, K, 24, 256)


@pytest.mark.parametrize("n,P", [(5, 48), (1, 48)])
@pytest.mark.parametrize("Dg,K", EMA_GEOMETRIES)
def test_generic_ema_accumulate_few_rows(Dg, K, n, P):
    """As test_generic_ema_accumulate on 240 rows (below the 256-row chunk floor, the last tile 48 rows) and on 48 rows (less
    than one 64-row tile)."""
    _check_ema_accumulate(Dg, K, n, P)


def _check_ema_accumulate(Dg, K, n, P):
    from lvt_amd.hip import vq
    torch.manual_seed(Dg * K)
    num = 3
    rows = n * P
    z = torch.randn(rows, num * Dg)
    idx = torch.randint(0, K, (n, num, P))
    idx[:, 1, ::3] = K - 1                                          # one code takes a third of group 1
    zd, idd = z.to(DEV), idx.to(DEV)
    s1 = vq.ema_accumulate(idd, zd, K).cpu()
    s2 = vq.ema_accumulate(idd, zd, K).cpu()
    assert torch.equal(s1, s2)
    for g in range(num):
        flat = idx[:, g].reshape(-1)
        cnt = torch.zeros(K, dtype=torch.float64).index_add_(0, flat, torch.ones(rows, dtype=torch.float64))
        tot = torch.zeros(K, Dg, dtype=torch.float64).index_add_(0, flat, z[:, Dg * g:Dg * (g + 1)].double())
        assert torch.equal(s1[g, :, Dg].double(), cnt), g
        assert rel_err(s1[g, :, :Dg], tot) < 1e-6, g


@pytest.mark.parametrize("num,K,D", [(3, 128, 64), (2, 64, 16), (1, 2048, 256)])
def test_ema_finalize_against_fp64(num, K, D):
    """vq.ema_finalize (both instantiations: compile-time width 64, run-time width) against the reference's update
    (vq_embedding.py:48-59) in float64: decay-lerp of running_size and running_sum, Laplace-smoothed sizes, new codebook."""
    from lvt_amd.hip import vq
    torch.manual_seed(num * K + D)
    decay, eps = 0.99, 1e-5
    rs = torch.rand(num, K) * 4 + 0.1
    rsum = torch.randn(num, K, D)
    stats = torch.randn(num, K, D + 1)
    stats[:, :, D] = torch.randint(0, 40, (num, K)).float()        # counts
    rs_d, rsum_d, w_d = rs.to(DEV), rsum.to(DEV), torch.zeros(num, K, D, device=DEV)
    vq.ema_finalize(stats.to(DEV), rs_d, rsum_d, w_d, decay=decay, eps=eps)
    rs64 = rs.double() * decay + (1 - decay) * stats[:, :, D].double()
    rsum64 = rsum.double() * decay + (1 - decay) * stats[:, :, :D].double()
    n = rs64.sum(1, keepdim=True)
    size_ = (rs64 + eps) / (n + K * eps) * n
    for g in range(num):
        assert rel_err(rs_d[g], rs64[g]) < 1e-5, g
        assert rel_err(rsum_d[g], rsum64[g]) < 1e-5, g
        assert rel_err(w_d[g], rsum64[g] / size_[g].unsqueeze(1)) < 1e-5, g


@pytest.mark.parametrize("num,K,D", [(8, 1024, 256), (2, 256, 256), (4, 2048, 256)])
def test_generic_ema_three_steps_against_oracle(num, K, D):
    """DVQEmbedding straight-through + EMA update, three steps: z_q_st, z_q_bar and the EMA state against O.vq_ema_step on the
    same indices (and the indices against the fp64 search on margin rows)."""
    from lvt_amd.modeling.vq import DVQEmbedding
    torch.manual_seed(num * K)
    m = DVQEmbedding(num, K, D, True).to(DEV)
    st = seeded.seeded_codebook_state(5, num=num, K=K, D=D // num, scale=0.5)
    m.load_state_dict(st)
    ref = {k: v.clone() for k, v in st.items()}
    for step in range(3):
        z = torch.randn(2, D, 16, 16) * 0.5
        with torch.no_grad():
            z_q_st, z_q_bar = m(z.to(DEV), "st")
        mine = m.last_indices.cpu()                                   # (2, num, 16, 16)
        r_st, r_bar, ref, _ = O.dvq_straight_through(ref, z, num, force_idx=mine)
        for g in range(num):
            rows = z[:, (D // num) * g:(D // num) * (g + 1)].permute(0, 2, 3, 1).reshape(-1, D // num)
            ok = margin_ok(rows, st["ve.%d.embedding.weight" % g] if step == 0 else prev["ve.%d.embedding.weight" % g])
            want = O.vq_margin_fp64(rows, st["ve.%d.embedding.weight" % g] if step == 0 else prev["ve.%d.embedding.weight" % g])[2]
            assert torch.equal(mine[:, g].reshape(-1)[ok], want[ok]), (step, g)
        # z_q_st is a pure gather of the pre-step codebook: exact against the module's own codebook, and against the oracle's
        # (which differs from it by the fp32 rounding of the previous EMA updates)
        pre = st if step == 0 else prev
        own = torch.cat([pre["ve.%d.embedding.weight" % g][mine[:, g]] for g in range(num)], -1).permute(0, 3, 1, 2)
        assert torch.equal(z_q_st.cpu(), own)
        assert rel_err(z_q_st, r_st) < 1e-5
        assert rel_err(z_q_bar, r_bar) < 1e-5
        prev = {k: v.cpu() for k, v in m.state_dict().items()}
        for k, v in prev.items():
            assert rel_err(v, ref[k]) < 1e-5, (step, k)


def _model(num, K, ema=True):
    from lvt_amd.modeling import build_model
    from util_models import vqvae_cfg
    cfg = vqvae_cfg(DEV)
    cfg.MODEL.CODEBOOK.NUM, cfg.MODEL.CODEBOOK.SIZE, cfg.MODEL.CODEBOOK.EMA = num, K, ema
    model = build_model(cfg)
    seed = 31
    model.encoder.load_state_dict(seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, seed, "enc."))
    model.generator.load_state_dict(seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, seed, "dec."))
    D = cfg.MODEL.CODEBOOK.DIM
    st = seeded.seeded_codebook_state(seed, num=num, K=K, D=D // num, scale=0.05)
    if not ema:
        st = {k: v for k, v in st.items() if k.endswith("embedding.weight")}
    if num == 1:
        model.codebook.load_state_dict({k[len("ve.0."):]: v for k, v in st.items()})
    else:
        model.codebook.load_state_dict(st)
    return model, st, seed


@pytest.mark.parametrize("num,K,ema", [(8, 1024, True), (2, 256, True), (1, 1024, True), (2, 256, False)])
def test_vqvae_end_to_end_geometry(num, K, ema):
    """PR-DVQVAE2 with (NUM, SIZE) overridden, 8 frames, three supervised steps: losses, encoder / decoder gradients and the
    codebook state after every step against O.vqvae_supervised_loss from the same state on the same indices."""
    from lvt_amd.utils.events import EventStorage
    model, _, seed = _model(num, K, ema)
    model.train()
    for step in range(3):
        # every step starts the oracle from the module's own pre-step codebook state (the two EMA updates agree to fp32
        # rounding only, which the commitment loss's cancellation z_e - z_q would amplify into the gradients)
        ref = {k: v.detach().cpu().clone() for k, v in model.codebook.state_dict().items()}
        if num == 1:
            ref = {"ve.0." + k: v for k, v in ref.items()}
        x = torch.stack([seeded.seeded_input("geo.%d.%d" % (step, i), (3, 64, 64), seed) for i in range(8)])
        for p in model.parameters():
            p.grad = None
        with EventStorage(0):
            losses = model([{"image": x[i].numpy()} for i in range(8)], mode="supervised")
        sum(losses.values()).backward()
        mine = model.codebook.last_indices.cpu()
        if num == 1:
            mine = mine.unsqueeze(1)

        def oracle(dtype):
            enc = {k: v.to(dtype).requires_grad_(True) for k, v in seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, seed, "enc.").items()}
            dec = {k: v.to(dtype).requires_grad_(True) for k, v in seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, seed, "dec.").items()}
            cb_in = {k: (v.to(dtype).clone().requires_grad_(True) if not ema else v.to(dtype)) for k, v in ref.items()}
            lo, new_state, aux = O.vqvae_supervised_loss(enc, dec, cb_in, O.normalize(x, MEAN, STD).to(dtype), num=num,
                                                         force_idx=mine, ema=ema)
            sum(lo.values()).backward()
            return lo, new_state, aux, enc, dec, cb_in

        lo, new_state, aux, enc, dec, cb_in = oracle(torch.float32)
        _, _, _, enc64, dec64, cb64 = oracle(torch.float64)
        assert set(losses) == set(lo), (set(losses), set(lo))
        assert abs(float(losses["loss_reconstruction"]) - float(lo["loss_reconstruction"])) < 1e-5 * float(lo["loss_reconstruction"])
        assert abs(float(losses["loss_commitment"]) - float(lo["loss_commitment"])) < 2e-4 * float(lo["loss_commitment"])
        # indices: the fp64 search of the oracle's z_e on margin rows
        z = aux["z_e"].detach()
        dg = z.size(1) // num
        for g in range(num):
            rows = z[:, dg * g:dg * (g + 1)].permute(0, 2, 3, 1).reshape(-1, dg)
            w = ref["ve.%d.embedding.weight" % g]
            ok = margin_ok(rows, w.detach(), rel=1e-4)
            assert ok.float().mean() > 0.5
            assert torch.equal(mine[:, g].reshape(-1)[ok], O.vq_margin_fp64(rows, w.detach())[2][ok]), (step, g)
        # gradients against an fp64 evaluation of the same graph (same indices): as close to it as 4 x the CPU fp32 oracle is
        # (floor 2e-5; see test_gpu_vqvae.py: cancellation in z_e - z_q and ReLU units within an ulp of zero)
        E, G = dict(model.encoder.named_parameters()), dict(model.generator.named_parameters())
        for mod, r32, r64 in ((E, enc, enc64), (G, dec, dec64)):
            for n_, p in r64.items():
                e_mine, e_cpu = rel_err(mod[n_].grad, p.grad), rel_err(r32[n_].grad, p.grad)
                assert e_mine < max(4 * e_cpu, 2e-5), (step, n_, e_mine, e_cpu)
        sd = {k: v.detach().cpu() for k, v in model.codebook.state_dict().items()}
        if num == 1:
            sd = {"ve.0." + k: v for k, v in sd.items()}
        if ema:
            for k, v in new_state.items():
                assert rel_err(sd[k], v) < 1e-5, (step, k)
        else:
            cbp = [p for p in model.codebook.parameters()]
            assert len(cbp) == num
            for g in range(num):
                ref64 = cb64["ve.%d.embedding.weight" % g].grad
                e_mine, e_cpu = rel_err(cbp[g].grad, ref64), rel_err(cb_in["ve.%d.embedding.weight" % g].grad, ref64)
                assert e_mine < max(4 * e_cpu, 2e-5), (step, g, e_mine, e_cpu)


def test_sample_categorical_v2048():
    """lvt_sample_categorical at V = 2048 (the wide instantiation) == oracle.multinomial_from_uniform on rows whose threshold
    is not within rounding of a cdf step; probabilities == softmax."""
    from lvt_amd.hip import tx
    g = torch.Generator().manual_seed(12)
    V, rows = 2048, 300
    logits = torch.randn(rows, V, generator=g) * 3
    u = torch.rand(rows, generator=g)
    u[0], u[1] = 0.0, 0.999999
    temp = 0.9
    prob = torch.softmax(logits.double() / temp, 1)
    want = O.multinomial_from_uniform(prob, u.double())
    cdf = torch.cumsum(prob, 1)
    margin = (cdf - (u.double() * cdf[:, -1]).unsqueeze(1)).abs().min(1).values
    out = torch.full((rows, 2), -1, dtype=torch.int64, device=DEV)
    pr = tx.sample_categorical(logits.to(DEV), temp, u.to(DEV), out.view(-1)[1:], 2, want_probs=True)
    got = out[:, 1].cpu()
    safe = margin > 1e-5
    assert int(safe.sum()) > 280
    assert torch.equal(got[safe], want[safe])
    assert bool(((got - want).abs() <= 1).all())
    assert bool((out[:, 0] == -1).all())
    assert rel_err(pr, prob.float()) < 1e-5


@pytest.mark.parametrize("num,K", [(8, 1024), (2, 256), (1, 1024)])
def test_g25_codebook_geometry(golden, num, K):
    """Fixture G25, captured from the reference (tests/golden/make_golden_geometry.py): PR-DVQVAE2 with (NUM, SIZE)
    overridden, two frames.  Indices bit-exact on clear-margin rows, one supervised step (losses, first / last layer
    gradients) and the codebook state after its EMA update, as G3 / G23 are checked."""
    from lvt_amd.modeling import build_model
    from lvt_amd.utils.events import EventStorage
    from util_models import vqvae_cfg
    g = golden("g25_codebook_geometry")
    t = "n%d_k%d." % (num, K)
    seed, scale = int(g["seed"]), float(g[t + "scale"])
    cfg = vqvae_cfg(DEV)
    cfg.MODEL.CODEBOOK.NUM, cfg.MODEL.CODEBOOK.SIZE = num, K
    model = build_model(cfg)
    model.encoder.load_state_dict(seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, seed, "enc."))
    model.generator.load_state_dict(seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, seed, "dec."))
    D = cfg.MODEL.CODEBOOK.DIM
    st = seeded.seeded_codebook_state(seed, num=num, K=K, D=D // num, scale=scale)
    model.codebook.load_state_dict({k[len("ve.0."):]: v for k, v in st.items()} if num == 1 else st)
    x = torch.stack([seeded.seeded_input("g25.f%d" % i, (3, 64, 64), seed) for i in range(2)])
    xn = O.normalize(x, MEAN, STD).to(DEV)
    model.eval()
    with torch.no_grad():
        z_e = model.encoder(xn).cpu()
        lat = model.encode(xn).cpu()
    lat = lat.unsqueeze(1) if num == 1 else lat
    dg = D // num
    clear = []
    for i in range(num):
        rows = z_e[:, dg * i:dg * (i + 1)].permute(0, 2, 3, 1).reshape(-1, dg)
        clear.append(margin_ok(rows, st["ve.%d.embedding.weight" % i], rel=1e-4).view(2, 16, 16))
    clear = torch.stack(clear, 1)
    assert int((~clear).sum()) < 8 * num
    assert torch.equal(lat[clear], g[t + "idx"][clear])
    model.train()
    with EventStorage(0):
        losses = model([{"image": x[i].numpy()} for i in range(2)], mode="supervised")
    sum(losses.values()).backward()
    assert abs(float(losses["loss_reconstruction"]) - float(g[t + "loss_reconstruction"])) < 1e-5 * float(g[t + "loss_reconstruction"])
    assert abs(float(losses["loss_commitment"]) - float(g[t + "loss_commitment"])) < 2e-4 * float(g[t + "loss_commitment"])
    mine = model.codebook.last_indices.cpu()
    mine = mine.unsqueeze(1) if num == 1 else mine
    assert torch.equal(mine[clear], g[t + "idx"][clear])
    assert rel_err(model.encoder.layers[0].weight.grad, g[t + "grad_enc_first"]) < 1e-3
    assert rel_err(model.encoder.layers[0].bias.grad, g[t + "grad_enc_first_bias"]) < 1e-3
    assert rel_err(model.generator.layers[6].weight.grad, g[t + "grad_dec_last"]) < 1e-4
    assert rel_err(model.generator.layers[6].bias.grad, g[t + "grad_dec_last_bias"]) < 1e-4
    new = {k: v.detach().cpu() for k, v in model.codebook.state_dict().items()}
    new = {"ve.0." + k: v for k, v in new.items()} if num == 1 else new
    nrows = int(g["nrows"])
    for k, v in new.items():
        ref = g[t + "new." + k]
        assert rel_err(v if k.endswith("running_size") else v[:nrows], ref) < 1e-5, k
