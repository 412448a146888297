"""Codebook restart (MODEL.CODEBOOK.RESTART, csrc/vq_restart.hip) on the device: the parent's lvt_vq_ema_finalize and fp64 torch on
the CPU are the yardsticks (the reference has no such feature).  Quantiser level over the geometries and row counts that take
different paths, then the model and the Trainer."""
import logging
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 5
P = 4
# (num, K, d): the shipped geometry, the smallest of the generic path, the largest; "single": SingleVQEmbedding K=128 D=128 (two groups)
GEOMS = [(4, 512, 64), (2, 64, 16), (1, 2048, 256), "single"]
ROWS = ["R8", "RK", "R4K3P"]             # R = 8 < K (empty strata), R = K, R = 4 K + 3 P (not a multiple of K)


def _gen(tag):
    """A CPU generator of its own per integer tag: every input of this file is a function of its tag alone."""
    g = torch.Generator()
    g.manual_seed(tag)
    return g


def _shape(geom):
    return (1, 128, 128) if geom == "single" else geom


def _nframes(geom, rows):
    K = _shape(geom)[1]
    return {"R8": 2, "RK": K // P, "R4K3P": K + 3}[rows]


def _make(geom, threshold=None):
    from lvt_amd.modeling.vq import DVQEmbedding, SingleVQEmbedding
    num, K, d = _shape(geom)
    q = SingleVQEmbedding(K, d, True) if geom == "single" else DVQEmbedding(num, K, num * d, True)
    q = q.to(DEV)
    if threshold is not None:
        q.enable_restart(threshold, SEED)
    return q.train()


def _books(q):
    """[(weight, running_size, running_sum)] per codebook, as the module's own tensors."""
    if hasattr(q, "ve"):
        return [(v.embedding.weight.data, v.running_size, v.running_sum) for v in q.ve]
    return [(q.embedding.weight.data, q.running_size, q.running_sum)]


def _set_state(q, state):
    """state: [(w, rs)] per codebook (CPU); running_sum = w * rs."""
    with torch.no_grad():
        for (w, rs, rsum), (w0, rs0) in zip(_books(q), state):
            w.copy_(w0)
            rs.copy_(rs0)
            rsum.copy_(w0 * rs0[:, None])


def _snapshot(q):
    return [tuple(t.detach().cpu().clone() for t in b) for b in _books(q)]


def _z(geom, n, seed):
    num, K, d = _shape(geom)
    return torch.randn(n, 1, 2, 2, num * d, generator=_gen(seed))


def _pass(q, z):
    st, bar = q.straight_through_cl(z.to(DEV).contiguous())
    return st, bar, q.last_indices.cpu()


def _counts(geom, idx, K):
    """(num, K) int64 assignment counts of a pass from the returned indices."""
    if geom == "single":
        return torch.bincount(idx.reshape(-1), minlength=K)[None]
    return torch.stack([torch.bincount(idx[:, i].reshape(-1), minlength=K) for i in range(idx.shape[1])])


def _perplexity64(counts):
    p = counts.double() / counts.double().sum()
    p = p[p > 0]
    return math.exp(-float((p * p.log()).sum()))


def _random_state(geom, seed):
    num, K, d = _shape(geom)
    g = _gen(seed)
    return [(torch.randn(K, d, generator=g), torch.rand(K, generator=g) * 3.0) for _ in range(num)]


# ---- 1. monitoring is exact, 3. health ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_threshold_zero_is_the_plain_finalize_bit_for_bit(geom, rows):
    """THRESHOLD 0: three passes leave weight, running_size and running_sum bit-equal to the plain module's; nothing restarts; the
    perplexity is that of the returned indices."""
    num, K, d = _shape(geom)
    plain, mon = _make(geom), _make(geom, 0.0)
    state = _random_state(geom, 100)
    _set_state(plain, state)
    _set_state(mon, state)
    n = _nframes(geom, rows)
    for p in range(3):
        z = _z(geom, n, 200 + p)
        sa, ba, ia = _pass(plain, z)
        sb, bb, ib = _pass(mon, z)
        assert torch.equal(ia, ib) and torch.equal(sa, sb) and torch.equal(ba, bb)
        for (w0, r0, s0), (w1, r1, s1) in zip(_snapshot(plain), _snapshot(mon)):
            assert torch.equal(w0, w1) and torch.equal(r0, r1) and torch.equal(s0, s1), p
        h = mon.restart_health.cpu()
        counts = _counts(geom, ib, K)
        for i in range(num):
            want = _perplexity64(counts[i])
            print("pass %d codebook %d perplexity %.9g fp64 %.9g" % (p, i, float(h[i, 0]), want))
            assert abs(float(h[i, 0]) - want) <= 1e-5 * want
        assert torch.equal(h[:, 1:], torch.zeros_like(h[:, 1:]))           # nothing is below 0
        if geom == "single":
            assert torch.equal(h, h[:1].expand_as(h))                      # every 64-d group carries the same record
    assert int(mon.restart_pass) == 3 and int(mon.restart_total.sum()) == 0


# ---- 2. the draw, 3. counts ------------------------------------------------------------------------------------------------------
def _far_state(geom, seed, z_first_row):
    """A quarter of the codes (k % 4 == 0) offset by 1e3 from rows of N(0, 1) with running_size 0, the others running_size 10.
    Code 4: far, but running_size 5 (above the threshold after decay).  Code 1: running_size 0 (below the threshold) and placed
    on top of row 0, which it therefore wins."""
    num, K, d = _shape(geom)
    g = _gen(seed)
    state = []
    for i in range(num):
        w = torch.randn(K, d, generator=g)
        rs = torch.full((K,), 10.0)
        w[0::4] += 1e3
        rs[0::4] = 0.0
        rs[4] = 5.0
        w[1] = z_first_row[i * d:(i + 1) * d]
        rs[1] = 0.0
        state.append((w, rs))
    return state


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_dead_codes_take_the_predicted_rows(geom, rows):
    from lvt_amd.hip.vq import restart_row
    num, K, d = _shape(geom)
    n = _nframes(geom, rows)
    R = n * P
    zs = [_z(geom, n, 300 + p) for p in range(3)]
    state = _far_state(geom, 301, zs[0].reshape(R, -1)[0])
    plain, rst = _make(geom), _make(geom, 1.0)
    _set_state(plain, state)
    _set_state(rst, state)
    far = [k for k in range(0, K, 4) if k != 4]
    total = torch.zeros(num, dtype=torch.int64)
    for p, z in enumerate(zs):
        before = _snapshot(rst)
        _set_state(plain, [(w, rs) for w, rs, _ in before])
        with torch.no_grad():                                              # (running_sum as it is, not w * rs)
            for (_, _, s1), (_, _, s0) in zip(_books(plain), before):
                s1.copy_(s0)
        sa, ba, ia = _pass(plain, z)
        sb, bb, ib = _pass(rst, z)
        assert torch.equal(ia, ib) and torch.equal(sa, sb)
        rows2d = z.reshape(R, -1)
        counts = _counts(geom, ib, K)
        h = rst.restart_health.cpu()
        for i, ((w0, r0, s0), (w1, r1, s1)) in enumerate(zip(_snapshot(plain), _snapshot(rst))):
            dead = r0 < 1.0                                                # the plain finalize's running_size IS the updated one
            restart = dead & (counts[i] == 0)
            if p == 0:
                assert sorted(torch.nonzero(restart).reshape(-1).tolist()) == far
                assert bool(dead[1]) and counts[i][1] >= 1                 # below the threshold, but it won row 0: kept
                assert not bool(dead[4]) and counts[i][4] == 0             # far, but running_size 4.95: kept
            for k in torch.nonzero(restart).reshape(-1).tolist():
                r = restart_row(SEED, p, 0 if geom == "single" else i, k, R, K)
                assert torch.equal(w1[k], rows2d[r, i * d:(i + 1) * d]), (p, i, k, r)
            assert torch.equal(r1[restart], torch.ones(int(restart.sum())))
            assert torch.equal(s1[restart], w1[restart] * 1.0)
            keep = ~restart
            assert torch.equal(w1[keep], w0[keep]) and torch.equal(r1[keep], r0[keep]) and torch.equal(s1[keep], s0[keep])
            ngroups = rst.restart_health.shape[0] // num
            for gi in range(i * ngroups, (i + 1) * ngroups):
                assert float(h[gi, 1]) == float(dead.sum()) and float(h[gi, 2]) == float(restart.sum()), (p, i)
            assert abs(float(h[i, 0]) - _perplexity64(counts[i])) <= 1e-5 * _perplexity64(counts[i])
            total[i] += int(restart.sum())
        # z_q_bar: no row refers to a restarted code
        assert torch.equal(ba, bb)
    assert int(rst.restart_pass) == 3
    assert torch.equal(rst.restart_total.cpu()[:num], total) and int(total.sum()) >= len(far) * num


def test_a_code_that_stays_dead_draws_another_row_each_pass():
    from lvt_amd.hip.vq import restart_row
    geom = (2, 64, 16)
    num, K, d = geom
    n = _nframes(geom, "R4K3P")
    R = n * P
    z = _z(geom, n, 400)
    state = _far_state(geom, 401, z.reshape(R, -1)[0])
    rst = _make(geom, 1.0)
    _set_state(rst, state)
    k = next(k for k in range(8, K, 4) if restart_row(SEED, 0, 0, k, R, K) != restart_row(SEED, 1, 0, k, R, K))
    rows2d = z.reshape(R, -1)
    for p in range(2):
        _pass(rst, z)
        w = _snapshot(rst)[0][0]
        assert torch.equal(w[k], rows2d[restart_row(SEED, p, 0, k, R, K), :d]), p
        with torch.no_grad():                                              # dead again: far away, nothing accumulated
            for wi, rs, rsum in _books(rst):
                wi[k] = 1e3
                rs[k] = 0.0
                rsum[k] = 0.0
    assert int(rst.restart_pass) == 2


def test_abandoned_pass_advances_nothing():
    geom = (2, 64, 16)
    z = _z(geom, 8, 500)
    rst = _make(geom, 1.0)
    _set_state(rst, _far_state(geom, 501, z.reshape(32, -1)[0]))
    before = _snapshot(rst)
    rst.straight_through_cl(z.to(DEV), defer=True)
    rst.abandon_ema()
    assert int(rst.restart_pass) == 0 and int(rst.restart_total.sum()) == 0
    for a, b in zip(before, _snapshot(rst)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    _pass(rst, z)                                                          # and the quantiser is usable again
    assert int(rst.restart_pass) == 1 and int(rst.restart_total.sum()) > 0


# ---- 7. recovery -----------------------------------------------------------------------------------------------------------------
def _recovery_sim(z, state, passes, thr=1.0, decay=0.99, eps=1e-5):
    """The rule in fp64 on the CPU for ONE codebook (restart_row + exact nearest search) -> [(perplexity, dead, restarted)]."""
    from lvt_amd.hip.vq import restart_row
    w, rs = state[0].double().clone(), state[1].double().clone()
    rsum = w * rs[:, None]
    K, R = w.shape[0], z.shape[0]
    z = z.double()
    out = []
    for p in range(passes):
        idx = torch.cdist(z, w).argmin(1)
        counts = torch.bincount(idx, minlength=K)
        sums = torch.zeros_like(w).index_add_(0, idx, z)
        rs = rs * decay + (1 - decay) * counts
        n = rs.sum()
        rsum = rsum * decay + (1 - decay) * sums
        w = rsum / ((rs + eps) / (n + K * eps) * n)[:, None]
        dead = rs < thr
        restart = dead & (counts == 0)
        for k in torch.nonzero(restart).reshape(-1).tolist():
            w[k] = z[restart_row(SEED, p, 0, k, R, K)]
            rsum[k] = w[k] * thr
            rs[k] = thr
        out.append((_perplexity64(counts), int(dead.sum()), int(restart.sum())))
    return out


def test_recovery_from_a_half_dead_codebook():
    """Rows from 2 K clusters 20 sigma apart, laid out cluster by cluster, so that the stratum of code k is clusters 2 k and
    2 k + 1: every restarted code lands in a cluster of its own, wins its 4 rows from the second pass on (running_size 0.99 +
    0.04 >= 1) and is dead no more.  The live half sits on the centres of clusters 2 k of ITS strata."""
    num, K, d = 1, 64, 16
    m = 4
    g = _gen(700)
    cl = torch.arange(2 * K)
    centres = torch.zeros(2 * K, d)
    for b in range(7):
        centres[:, b] = 20.0 * ((cl >> b) & 1)
    z = centres.repeat_interleave(m, 0) + torch.randn(2 * K * m, d, generator=g)         # (512, 16): R = 8 K
    w = torch.randn(K, d, generator=g) + 1e3
    rs = torch.zeros(K)
    w[1::2] = centres[2 * torch.arange(1, K, 2)]
    rs[1::2] = 10.0
    sim = _recovery_sim(z, (w, rs), 5)
    assert sim[0][1] == K // 2 and sim[0][2] == K // 2
    assert sim[-1][1] == 0 and sim[-1][0] > sim[0][0]                      # the inputs meet the condition on their own
    rst = _make((num, K, d), 1.0)
    _set_state(rst, [(w, rs)])
    got = []
    for p in range(5):
        _pass(rst, z.view(-1, 1, 2, 2, d))
        h = rst.restart_health.cpu()[0]
        got.append((float(h[0]), int(h[1]), int(h[2])))
    print("kernel", got, "fp64", sim)
    assert got[0][1] == K // 2 and got[0][2] == K // 2
    assert got[-1][1] == 0 and got[-1][0] > got[0][0]
    for a, b in zip(got, sim):
        assert a[1:] == b[1:] and abs(a[0] - b[0]) <= 1e-5 * b[0]
    assert int(rst.restart_total) == sum(a[2] for a in got)


# ---- 4. - 6., 8.: the model and the Trainer ---------------------------------------------------------------------------------------
def _model(restart, threshold=1.0):
    import seeded
    from util_models import vqvae_cfg
    from lvt_amd.modeling import build_model
    cfg = vqvae_cfg(DEV)
    cfg.SEED = 11
    if restart:
        cfg.MODEL.CODEBOOK.RESTART.ENABLED = True
        cfg.MODEL.CODEBOOK.RESTART.THRESHOLD = threshold
    torch.manual_seed(11)
    model = build_model(cfg)
    model.encoder.load_state_dict(seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, 11, "enc."))
    model.generator.load_state_dict(seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, 11, "dec."))
    model.codebook.load_state_dict(seeded.seeded_codebook_state(11, scale=0.05))
    return cfg, model


def _batch():
    import seeded
    x = seeded.seeded_input("restart", (4, 3, 64, 64), 12)
    return [{"image": x[i].numpy()} for i in range(4)]


def _supervised(model):
    from lvt_amd.utils.events import EventStorage
    with EventStorage(0):
        losses = model(_batch(), mode="supervised")
    return losses


def test_losses_and_gradients_are_untouched():
    out = {}
    for on in (False, True):
        _, model = _model(on)
        model.train()
        losses = _supervised(model)
        sum(losses.values()).backward()
        out[on] = ({k: v.detach().cpu() for k, v in losses.items()}, model.encoder.layers[0].weight.grad.detach().cpu().clone(),
                   _snapshot(model.codebook), model.codebook.last_indices.cpu(), model)
    (la, ga, ca, ia, _), (lb, gb, cb, ib, mb) = out[False], out[True]
    assert la.keys() == lb.keys()
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    assert torch.equal(ga, gb) and torch.equal(ia, ib)
    h = mb.codebook.restart_health.cpu()
    counts = _counts((4, 512, 64), ib, 512)
    nrest = 0
    for i, ((w0, r0, s0), (w1, r1, s1)) in enumerate(zip(ca, cb)):
        restart = (r0 < 1.0) & (counts[i] == 0)
        differ = (w0 != w1).any(1) | (r0 != r1) | (s0 != s1).any(1)
        assert not bool((differ & ~restart).any()), i
        assert float(h[i, 2]) == float(restart.sum()) and int(differ.sum()) <= int(h[i, 2])
        assert torch.equal(r1[restart], torch.ones(int(restart.sum())))
        nrest += int(restart.sum())
    assert nrest > 0                                                       # (the seeded state has running sizes from 0.5 up)
    assert int(mb.codebook.restart_total.sum()) == nrest and int(mb.codebook.restart_pass) == 1


def test_eval_mode_runs_the_plain_finalize():
    out = {}
    for on in (False, True):
        _, model = _model(on)
        model.eval()
        with torch.no_grad():
            losses = _supervised(model)
        out[on] = ({k: v.detach().cpu() for k, v in losses.items()}, _snapshot(model.codebook), model)
    (la, ca, _), (lb, cb, mb) = out[False], out[True]
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    for a, b in zip(ca, cb):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    q = mb.codebook
    assert int(q.restart_pass) == 0 and int(q.restart_total.sum()) == 0 and not bool(q.restart_health.any())


def _trainer(tmp_path, restart):
    from lvt_amd.engine.trainer import Trainer
    cfg, model = _model(restart)
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.SOLVER.CHECKPOINT_PERIOD = 10 ** 6
    return Trainer(cfg, model, iter([_batch()] * 3), log_period=10 ** 6)


def _count_host_reads(monkeypatch, fn):
    calls = {"item": 0, "tolist": 0, "float": 0}
    for name, key in (("item", "item"), ("tolist", "tolist"), ("__float__", "float")):
        orig = getattr(torch.Tensor, name)

        def wrapped(self, *a, _orig=orig, _key=key, **kw):
            if self.is_cuda:
                calls[_key] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapped)
    fn()
    monkeypatch.undo()
    return calls


def test_trainer_logs_the_health_in_the_existing_copy_and_is_reproducible(tmp_path, monkeypatch, caplog):
    off = _trainer(tmp_path / "off", False)
    reads_off = _count_host_reads(monkeypatch, lambda: off.train(max_iter=3))
    runs = []
    for tag in ("a", "b"):
        on = _trainer(tmp_path / tag, True)
        with caplog.at_level(logging.INFO, logger="lvt_amd"):
            reads_on = _count_host_reads(monkeypatch, lambda: on.train(max_iter=3))
        runs.append((on, reads_on))
    lines = [r.getMessage() for r in caplog.records if "codebook_perplexity" in r.getMessage()]
    assert len(lines) == 2, caplog.text
    for key in ("codebook_perplexity: ", "codebook_dead: ", "codebook_restarts: ", "loss_reconstruction: ", "loss_commitment: "):
        assert key in lines[0], lines[0]
    # the losses came over in two float() reads; now everything comes in ONE stacked copy, and nothing else reads the device
    print("host reads off", reads_off, "on", runs[0][1])
    assert runs[0][1]["tolist"] == reads_off["tolist"] + 1
    assert runs[0][1]["item"] == reads_off["item"] and runs[0][1]["float"] == reads_off["float"] - 2
    q = runs[0][0].model.codebook
    total = int(q.restart_total.sum())
    assert int(q.restart_pass) == 3 and total > 0
    assert "codebook_restarts: %.5f" % total in lines[0]
    # 5. two runs leave the same bits
    qa, qb = runs[0][0].model.codebook, runs[1][0].model.codebook
    for a, b in zip(_snapshot(qa), _snapshot(qb)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for name in ("restart_pass", "restart_health", "restart_total"):
        assert torch.equal(getattr(qa, name), getattr(qb, name)), name
    for pa, pb in zip(runs[0][0].model.parameters(), runs[1][0].model.parameters()):
        assert torch.equal(pa, pb)
    assert lines[0].split("  ")[1:-1] == lines[1].split("  ")[1:-1]         # (all but the iteration prefix and the s/it suffix)
    # off is today's trainer: no health keys in its model
    assert off.model.codebook_health() is None
