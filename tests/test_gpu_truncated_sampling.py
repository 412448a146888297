"""lvt_sample_truncated (top-k, then top-p, then the inverse-CDF draw on what is left) against the rule stated in fp64 by
lvt_amd/modeling/autoregressive/sampling.py, and the settings through the model: ChannelPredictor, GraphedSliceSampler,
VideoTransformerModel.sample_video and TEST.VT_SAMPLER.{TEMPERATURE, TOP_K, TOP_P}.

300 rows per case, temp = 0.9, two classes of logits from torch.Generator().manual_seed(11): `randn * 3` ("randn") and the same
rounded to multiples of 0.5 ("ties": runs of bit-equal logits everywhere, the k-th and the nucleus boundary included)."""
import functools

import pytest
import torch

import seeded
from conftest import rel_err
from lvt_amd.modeling.autoregressive.sampling import truncated_draw_reference, truncated_probs_reference
from util_models import dsfvt_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, TEMP = 300, 0.9
VS = [7, 64, 65, 512, 1000, 1024, 1025, 2048]
KINDS = ["randn", "ties"]
MARGIN = 1e-5                       # what the existing draw tests give fp32 sums (test_sample_categorical_matches_oracle_rule)


@functools.lru_cache(maxsize=None)
def _inputs(V, kind):
    """(logits (300, V) fp32, u (300,)): computed once per (V, kind) and never modified."""
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(ROWS, V, generator=g) * 3
    u = torch.rand(ROWS, generator=g)
    if kind == "ties":
        logits = torch.round(logits * 2) / 2
    return logits, u


@functools.lru_cache(maxsize=None)
def _reference(V, kind, top_k, top_p):
    return truncated_probs_reference(_inputs(V, kind)[0], TEMP, top_k, top_p)


def _run(logits, top_k, top_p, u, temp=TEMP, stride=4, slot=2, **kw):
    """-> (codes (rows,), probs (rows, V)) on the CPU; the codes are written at `stride` into a buffer of -1 whose other slots
    must stay -1."""
    from lvt_amd.hip import tx
    rows = logits.shape[0]
    out = torch.full((rows, stride), -1, dtype=torch.int64, device=DEV)
    pr = tx.sample_truncated(logits.to(DEV), temp, top_k, top_p, u.to(DEV), out.view(-1)[slot:], stride, want_probs=True, **kw)
    torch.cuda.synchronize()
    others = [i for i in range(stride) if i != slot]
    assert bool((out[:, others] == -1).all()), "a neighbouring slot of the strided output was written"
    return out[:, slot].cpu(), pr.cpu()


def unsafe_rows(V, kind, top_k, top_p):
    """Rows in which a cumulative mass at a boundary between tie classes (the reference's, fp64, normalised over the top-k set A)
    lies within MARGIN of top_p: there fp32 sums may legitimately stop one tie class away."""
    x = _inputs(V, kind)[0].double()
    w = torch.exp((x - x.amax(1, keepdim=True)) / TEMP)
    keep = torch.ones_like(x, dtype=torch.bool)
    if 0 < top_k < V:
        keep = x >= torch.topk(x, top_k, dim=1).values[:, -1:]
    xs, order = torch.sort(x, dim=1, descending=True, stable=True)
    ws = torch.gather(torch.where(keep, w, torch.zeros_like(w)), 1, order)
    mass = torch.cumsum(ws, 1) / ws.sum(1, keepdim=True)
    boundary = torch.ones_like(keep)
    boundary[:, :-1] = xs[:, :-1] != xs[:, 1:]
    boundary &= torch.gather(keep, 1, order)
    return (boundary & ((mass - top_p).abs() <= MARGIN)).any(1)


def _sets_one_class_away(x, ref_keep, a_keep):
    """The reference's kept set with the boundary one tie class lower and one higher (inside A)."""
    inf = float("inf")
    t = torch.where(ref_keep, x, torch.full_like(x, inf)).amin(1, keepdim=True)
    lower = torch.where(a_keep & (x < t), x, torch.full_like(x, -inf)).amax(1, keepdim=True)
    upper = torch.where(x > t, x, torch.full_like(x, inf)).amin(1, keepdim=True)
    return a_keep & (x >= lower), a_keep & (x >= upper)


# ---- 1. top-k alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", VS)
def test_top_k_set_is_exact(V, kind):
    """top_k in 1, 2, 8, V/2, V-1, V, V+5: the set probs > 0 is the reference's on every row (selection on the logits is exact in
    fp32; ties at the k-th logit all stay) and the probabilities are the reference's to 1e-5, the bound of
    test_sample_categorical_matches_oracle_rule for this arithmetic."""
    logits, u = _inputs(V, kind)
    for top_k in sorted({1, 2, 8, V // 2, V - 1, V, V + 5}):
        want = _reference(V, kind, top_k, 1.0)
        codes, pr = _run(logits, top_k, 1.0, u)
        diff = int(((pr > 0) != (want > 0)).any(1).sum())
        err = rel_err(pr, want)
        print("top-k V=%d %s k=%d: rows with another set %d, kept per row %d..%d, probs rel_err %.3g"
              % (V, kind, top_k, diff, int((want > 0).sum(1).min()), int((want > 0).sum(1).max()), err))
        assert diff == 0, (top_k, diff)
        assert err < 1e-5, (top_k, err)
        assert bool((pr.gather(1, codes[:, None]) > 0).all()), top_k
        assert float((pr.double().sum(1) - 1).abs().max()) < 1e-5


# ---- 2. top-p alone, and behind top-k -----------------------------------------------------------------------------------
def _top_p_cases(V, kind):
    cases = [(0, 0.5), (0, 0.9), (8, 0.9), (V // 2, 0.9)]
    return cases + [(0, 0.99)] if kind == "ties" else cases


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", VS)
def test_top_p_set(V, kind):
    """(top_k, top_p) in (0, 0.5), (0, 0.9), (8, 0.9), (V/2, 0.9), and (0, 0.99) on the tie-heavy class.  A row is safe when no
    cumulative mass at a boundary between tie classes is within 1e-5 of top_p (`unsafe_rows`).  Safe rows: the kept set is the
    reference's.  Every row: the kept set is the reference's for t_p or for the tie class next to it.  At least 285 of 300 rows
    are safe in every case; the reference alone on these inputs gives, as the largest number of unsafe rows over the eight V:
    randn (0, 0.5) 1, (0, 0.9) 4, (8, 0.9) 1, (V/2, 0.9) 8; ties (0, 0.5) 0, (0, 0.9) 0, (8, 0.9) 0, (V/2, 0.9) 0, (0, 0.99) 3
    ((0, 0.99) on randn: 110 at V = 2048 -- a long tail of tiny steps -- which is why that case is not run).
    On the rows whose set is the reference's the probabilities are held to 1e-5 as in the top-k test."""
    logits, u = _inputs(V, kind)
    x = logits.double()
    for top_k, top_p in _top_p_cases(V, kind):
        want = _reference(V, kind, top_k, top_p)
        a_keep = _reference(V, kind, top_k, 1.0) > 0
        unsafe = unsafe_rows(V, kind, top_k, top_p)
        codes, pr = _run(logits, top_k, top_p, u)
        got, ref = pr > 0, want > 0
        same = (got == ref).all(1)
        lower, upper = _sets_one_class_away(x, ref, a_keep)
        near = same | (got == lower).all(1) | (got == upper).all(1)
        err = rel_err(pr[same], want[same])
        print("top-p V=%d %s k=%d p=%g: unsafe rows %d, rows with another set %d (of them safe %d, further than one tie class %d), "
              "kept per row %d..%d, probs rel_err %.3g"
              % (V, kind, top_k, top_p, int(unsafe.sum()), int((~same).sum()), int((~same & ~unsafe).sum()), int((~near).sum()),
                 int(ref.sum(1).min()), int(ref.sum(1).max()), err))
        assert int((~unsafe).sum()) >= 285, (top_k, top_p, int(unsafe.sum()))
        assert bool(same[~unsafe].all()), (top_k, top_p)
        assert bool(near.all()), (top_k, top_p)
        assert err < 1e-5, (top_k, top_p, err)
        assert bool((pr.gather(1, codes[:, None]) > 0).all()), (top_k, top_p)
        assert bool((got & ~a_keep).sum() == 0), (top_k, top_p)          # never outside the top-k set
        assert bool(pr.gather(1, x.argmax(1, keepdim=True)).gt(0).all())  # the arg-max always stays


# ---- 3. the draw --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,kind,top_k,top_p", [(512, "randn", 8, 1.0), (512, "randn", 0, 0.9), (512, "randn", 8, 0.9),
                                                (512, "ties", 8, 0.9), (2048, "randn", 8, 0.9), (2048, "ties", 0, 0.9),
                                                (65, "randn", 8, 0.9)])
def test_draw(V, kind, top_k, top_p):
    """codes == truncated_draw_reference on the rows that qualify: the kept set is the reference's and the threshold u * total_B
    is further than 1e-5 from every cdf step (at least 280 of 300 rows).  On every row the code is a kept one.  The first two
    rows whose first and last indices are both cut draw with u = 0 and u = 1 - 2^-24: the first and the last kept index, never
    index 0 or V - 1.  The codes go out at stride 4; the other slots stay untouched (`_run`)."""
    logits, u = _inputs(V, kind)
    u = u.clone()
    want = _reference(V, kind, top_k, top_p)
    r0, r1 = torch.nonzero((want[:, 0] == 0) & (want[:, -1] == 0)).view(-1)[:2].tolist()
    u[r0], u[r1] = 0.0, 1.0 - 2.0 ** -24
    codes, pr = _run(logits, top_k, top_p, u)
    ref_codes = truncated_draw_reference(want, u.double())
    cdf = torch.cumsum(want, 1)
    margin = (cdf - (u.double() * cdf[:, -1]).unsqueeze(1)).abs().min(1).values
    same = ((pr > 0) == (want > 0)).all(1)
    ok = same & (margin > MARGIN)
    print("draw V=%d %s k=%d p=%g: %d rows qualify, %d of them differ, %d rows differ in all"
          % (V, kind, top_k, top_p, int(ok.sum()), int((codes != ref_codes)[ok].sum()), int((codes != ref_codes).sum())))
    assert int(ok.sum()) >= 280, int(ok.sum())
    assert torch.equal(codes[ok], ref_codes[ok])
    assert bool((pr.gather(1, codes[:, None]) > 0).all())
    assert bool((want.gather(1, codes[:, None]) > 0)[same].all())
    assert bool(same[r0]) and bool(same[r1])
    kept = [torch.nonzero(want[r] > 0).view(-1) for r in (r0, r1)]
    assert int(codes[r0]) == int(kept[0][0]) and int(codes[r1]) == int(kept[1][-1])


# ---- 4. off means off ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [512, 2048])
def test_off_is_lvt_sample_categorical(V):
    """top_k = 0 with top_p = 1 (and top_k >= V): the codes and the bits of probs are lvt_sample_categorical's, with the uniforms
    passed directly and read from a table at the device cursor."""
    from lvt_amd.hip import tx
    logits, u = _inputs(V, "randn")
    u = u.clone()
    u[0], u[1] = 0.0, 1.0 - 2.0 ** -24
    lg, ud = logits.to(DEV), u.to(DEV)
    table = torch.rand(4, ROWS, generator=torch.Generator().manual_seed(V))
    table[3] = u
    td, pos = table.to(DEV), torch.full((1,), 3, dtype=torch.int32, device=DEV)
    for kw in ({}, {"pos": pos, "u_pos": ROWS}):
        src = td if kw else ud
        out = torch.full((ROWS, 4), -1, dtype=torch.int64, device=DEV)
        pr = tx.sample_categorical(lg, TEMP, src, out.view(-1)[2:], 4, want_probs=True, **kw)
        for top_k in (0, V, V + 5):
            codes, pt = _run(logits, top_k, 1.0, table if kw else u, **kw)
            assert torch.equal(codes, out[:, 2].cpu()), (top_k, bool(kw))
            assert torch.equal(pt.view(torch.int32), pr.cpu().view(torch.int32)), (top_k, bool(kw))
    # the table form reads the row the cursor names
    codes_t, _ = _run(logits, 8, 0.9, table, pos=pos, u_pos=ROWS)
    codes_d, _ = _run(logits, 8, 0.9, u)
    assert torch.equal(codes_t, codes_d)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,temp,top_k,top_p", [(2049, 0.9, 8, 0.9), (64, 0.9, -1, 0.9), (64, 0.9, 8, 0.0), (64, 0.9, 8, 1.5),
                                                (64, 0.0, 8, 0.9), (64, 0.9, 8, float("nan"))])
def test_refusals(V, temp, top_k, top_p):
    from lvt_amd.hip import binding as L
    from lvt_amd.hip import tx
    logits = torch.zeros(4, V, device=DEV)
    out = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    with pytest.raises(L.LvtError):
        tx.sample_truncated(logits, temp, top_k, top_p, torch.zeros(4, device=DEV), out)
    torch.cuda.synchronize()
    assert bool((out == -1).all())                          # nothing was launched


# ---- 6. frequencies -----------------------------------------------------------------------------------------------------
def test_frequencies():
    """One row of 64 logits 20000 times with independent uniforms, top_k = 8, top_p = 0.9: no cut code is ever drawn and every
    kept code's frequency is within 5 binomial standard deviations of its reference probability."""
    n = 20000
    # of the 300 rows at V = 64, the safe one (see test_top_p_set) in which the reference keeps the most codes
    kept = (_reference(64, "randn", 8, 0.9) > 0).sum(1)
    kept[unsafe_rows(64, "randn", 8, 0.9)] = 0
    row = _inputs(64, "randn")[0][int(kept.argmax())]
    u = torch.rand(n, generator=torch.Generator().manual_seed(12))
    q = truncated_probs_reference(row, TEMP, 8, 0.9)
    codes, pr = _run(row.expand(n, 64).contiguous(), 8, 0.9, u)
    assert bool(((pr > 0) == (q > 0)).all())
    freq = torch.bincount(codes, minlength=64).double() / n
    sd = torch.sqrt(q * (1 - q) / n)
    print("frequencies: kept", torch.nonzero(q > 0).view(-1).tolist(), "q", q[q > 0].tolist(), "freq", freq[q > 0].tolist(),
          "worst deviation in sd %.3g" % float(((freq - q).abs() / sd.clamp_min(1e-30))[q > 0].max()))
    assert int((q > 0).sum()) >= 4
    assert float(freq[q == 0].sum()) == 0.0
    assert bool(((freq - q).abs() <= 5 * sd)[q > 0].all())


# ---- 7. through the model -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vt():
    from lvt_amd.modeling import build_model
    cfg = dsfvt_cfg()
    cfg.TEST.EVALUATORS = "VTSampler"
    model = build_model(cfg)
    model.model.load_state_dict(seeded.seeded_params(seeded.dsfvt_shapes(), 4321), strict=False)
    model.eval()
    return model


def _clips():
    codes = torch.stack([seeded.seeded_codes("t%d" % i, (16, 4, 16, 16), 31) for i in range(3)])
    video = codes.transpose(1, 2).contiguous().to(DEV)
    video[:, :, 15:] = 0
    return codes, video


def _changed(a, b):
    return float((a != b)[:, :, 15:].float().mean())


def test_top_k_one_is_the_argmax_whatever_the_seed(vt):
    """top_k = 1 leaves one code per draw (exact ties aside): the same video under two seeds, the `_samplers` key carries the
    settings, and temp = 1e-4 sampling differs in fewer than 1 % of the generated codes (near-ties, the existing allowance).
    TEST.VT_SAMPLER.TOP_K = 1 gives the same video through mode="inference"."""
    codes, video = _clips()
    s = vt.cfg.TEST.VT_SAMPLER
    saved = (s.N_PRIME, s.NUM_SAMPLES, s.TEMPERATURE, s.TOP_K, s.TOP_P)
    try:
        with torch.no_grad():
            vt._samplers = {}
            torch.manual_seed(1)
            a = vt.sample_video(video, n_prime=15, top_k=1)
            assert list(vt._samplers) == [(3, 1, 16, 16, 1.0, 1, 1.0)]
            torch.manual_seed(2)
            b = vt.sample_video(video, n_prime=15, top_k=1)
            assert torch.equal(a, b)
            assert torch.equal(a[:, :, :15].cpu(), codes.transpose(1, 2)[:, :, :15])
            cold = vt.sample_video(video, n_prime=15, temp=1e-4)
            assert list(vt._samplers) == [(3, 1, 16, 16, 1e-4)]             # truncation off: the 5-tuple
            print("top_k=1 vs temp=1e-4: %.4f of the generated codes differ" % _changed(a, cold))
            assert _changed(a, cold) < 0.01
            s.N_PRIME, s.NUM_SAMPLES, s.TOP_K = 15, 1, 1
            torch.manual_seed(3)
            res = vt([{"image_sequence": codes[i]} for i in range(3)], mode="inference")
            assert list(vt._samplers) == [(3, 1, 16, 16, 1.0, 1, 1.0)]
            assert torch.equal(torch.stack([r["samples"][0] for r in res]), a)
            s.TOP_K = 0
            vt([{"image_sequence": codes[i]} for i in range(3)], mode="inference")
            assert list(vt._samplers) == [(3, 1, 16, 16, 1.0)]
    finally:
        s.N_PRIME, s.NUM_SAMPLES, s.TEMPERATURE, s.TOP_K, s.TOP_P = saved
        vt._samplers = {}


def test_truncated_graph_replay_equals_eager_steps(vt, monkeypatch):
    """top_k = 8, top_p = 0.9 with one seed: the captured step replayed for 256 positions == the same steps launched eagerly
    (LVT_DECODE_GRAPHS=0), bit for bit; the settings are arguments of the captured launches."""
    _, video = _clips()
    key = (3, 1, 16, 16, 1.0, 8, 0.9)
    try:
        with torch.no_grad():
            vt._samplers = {}
            torch.manual_seed(5)
            graphed = vt.sample_video(video, n_prime=15, top_k=8, top_p=0.9)
            (_, _, smp, _), = vt._samplers[key]
            assert set(smp.graphs) == {True} and (smp.top_k, smp.top_p) == (8, 0.9)
            monkeypatch.setenv("LVT_DECODE_GRAPHS", "0")
            vt._samplers = {}
            torch.manual_seed(5)
            eager = vt.sample_video(video, n_prime=15, top_k=8, top_p=0.9)
            (_, _, smp, _), = vt._samplers[key]
            assert not smp.graphs
            torch.manual_seed(6)
            other = vt.sample_video(video, n_prime=15, top_k=8, top_p=0.9)
    finally:
        vt._samplers = {}
    print("truncated graph replay vs eager: %d codes differ; another seed changes %.3f of the generated codes"
          % (int((graphed != eager).sum()), _changed(eager, other)))
    assert torch.equal(graphed, eager)
    assert _changed(eager, other) > 0                      # it is a sampler: eight codes at most, not one


def test_full_pass_schedule_honours_the_settings(vt):
    """temp = 1e-4 with top_k = 2 and one seed: the reference's full-pass schedule (incremental=False) differs from the K/V-cache
    path in fewer than 1 % of the generated codes -- both cut to the same sets and draw the arg-max but for near-ties."""
    _, video = _clips()
    try:
        with torch.no_grad():
            vt._samplers = {}
            torch.manual_seed(7)
            a = vt.sample_video(video, n_prime=15, temp=1e-4, top_k=2, incremental=True)
            assert list(vt._samplers) == [(3, 1, 16, 16, 1e-4, 2, 1.0)]
            torch.manual_seed(7)
            b = vt.sample_video(video, n_prime=15, temp=1e-4, top_k=2, incremental=False)
    finally:
        vt._samplers = {}
    print("full-pass vs incremental at top_k=2: %.4f of the generated codes differ" % _changed(a, b))
    assert _changed(a, b) < 0.01


def test_forced_codes_return_the_truncated_probabilities(vt):
    """ChannelPredictor.sample_from_rows(forced_codes=...) with truncation on: the codes are the forced ones and the probabilities
    are the kernel's truncated ones.  Against the untruncated probabilities of the same call (torch.softmax, as before): the
    support lies inside their eight largest, it is the smallest run of the largest whose mass reaches 0.9 of those eight (to
    1e-5, the fp32-sum margin), and on it the probabilities are the full ones renormalised."""
    pred = vt.model.ch_predictor
    g = torch.Generator().manual_seed(17)
    rows = torch.randn(5, 512, generator=g).to(DEV)
    forced = torch.randint(0, 512, (5, 4), generator=g)
    with torch.no_grad():
        codes0, full = pred.sample_from_rows(rows, TEMP, forced_codes=forced, return_probs=True)
        codes, cut = pred.sample_from_rows(rows, TEMP, forced_codes=forced, return_probs=True, top_k=8, top_p=0.9)
    assert torch.equal(codes.cpu(), forced) and torch.equal(codes0.cpu(), forced)
    full, got = full.double().cpu(), cut.double().cpu()
    assert tuple(got.shape) == (5, 4, 512)
    top8 = torch.topk(full, 8, dim=-1).values
    support = got > 0
    n = support.sum(-1)
    assert int(n.min()) >= 1 and int(n.max()) <= 8
    assert bool((torch.where(support, full, torch.ones_like(full)).amin(-1) >= torch.gather(top8, -1, n[..., None] - 1)[..., 0]).all())
    mass = torch.cumsum(top8, -1) / top8.sum(-1, keepdim=True)
    reached = torch.gather(mass, -1, n[..., None] - 1)[..., 0]
    before = torch.where(n > 1, torch.gather(mass, -1, (n[..., None] - 2).clamp_min(0))[..., 0], torch.zeros_like(reached))
    assert bool((reached >= 0.9 - MARGIN).all()) and bool((before < 0.9 + MARGIN).all())
    want = torch.where(support, full, torch.zeros_like(full))
    want = want / want.sum(-1, keepdim=True)
    assert rel_err(got, want) < 1e-5
