"""The kernels of one decode step, each on its own against a plain formula: the single-query attention over a K/V cache
(csrc/transformer.hip: attn_decode_body behind lvt_attn_decode and lvt_attn_decode_blocks) against

    o = softmax_{j <= i}( q . K_j / temper + (dt[ti - tj + bt - 1] + dh[hi - hj + bh - 1]) + dw[wi - wj + bw - 1] ) V_j

evaluated in fp64 (accepted: err < max(2e-5 * max |o_ref|, 4 * err32), err32 = the error of the same formula in fp32 torch), at
the key counts where the kernel changes its path -- fewer keys than its four waves, the 16-key score pass, entry into and exit
from the 8 x 4-row unrolled P.V loop, all 1024 entries of the score table, a head count that is no power of two -- and
lvt_sample_categorical at vocabulary sizes where lanes run past the end of a row and across the switch to the wide
instantiation."""
import ctypes as C
import math

import pytest
import torch

from conftest import rel_err
from oracle import lvt_oracle as O
from util_attention import judge, rand
from util_guard import IBuf, obuf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, DA = 2, 3, 128
HD = H * DA
TEMPER = math.sqrt(DA)


def _coords(j, blk):
    return j // (blk[1] * blk[2]), (j // blk[2]) % blk[1], j % blk[2]


def _formula(q, Kc, Vc, banks, blk, li, rows, dtype):
    """The formula above on the CPU in `dtype`: q (B, HD); the keys are the cache rows `rows`, key n at block-local raster
    index n; the query at local index li = len(rows) - 1.  -> o (B, HD)."""
    n = len(rows)
    qh = q.to(dtype).view(B, H, DA)
    K = Kc[:, rows].to(dtype).view(B, n, H, DA)
    V = Vc[:, rows].to(dtype).view(B, n, H, DA)
    dt, dh, dw = (t.to(dtype) for t in banks)
    ti, hi, wi = _coords(li, blk)
    tj, hj, wj = _coords(torch.arange(n), blk)
    bias = (dt[:, ti - tj + blk[0] - 1] + dh[:, hi - hj + blk[1] - 1]) + dw[:, wi - wj + blk[2] - 1]          # (H, n)
    sc = torch.einsum("bhd,bnhd->bhn", qh, K) / math.sqrt(DA) + bias
    return torch.einsum("bhn,bnhd->bhd", torch.softmax(sc, -1), V).reshape(B, HD)


def _case(blk, seed, qscale=3.0, bank_scale=0.5):
    """-> q for every position (B, S, HD), Kc, Vc (B, S, HD), banks: uniform draws, scores of a few units."""
    Sn = blk[0] * blk[1] * blk[2]
    q = rand(B, Sn, HD, seed=seed) * qscale
    Kc, Vc = rand(B, Sn, HD, seed=seed + 1), rand(B, Sn, HD, seed=seed + 2)
    banks = [rand(H, 2 * n - 1, seed=seed + 3 + i) * bank_scale for i, n in enumerate(blk)]
    return q, Kc, Vc, banks


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


D1_CASES = [((1, 16, 16), [0, 1, 2, 3, 4, 14, 15, 16, 17, 27, 28, 31, 32, 33, 59, 60, 255]),
            ((4, 8, 8), [63, 64, 65, 255]),
            ((2, 4, 6), list(range(48))),
            ((4, 16, 16), [1023])]


@pytest.mark.parametrize("blk,positions", D1_CASES, ids=["x".join(map(str, c[0])) for c in D1_CASES])
def test_attn_decode_vs_fp64(blk, positions):
    """lvt_attn_decode against the fp64 formula at every listed position; at (1,16,16) also through a padded query pitch (NaN
    between the rows) and through the device cursor, both bit-equal to the plain call.

    Worst err / err32 of o on an MI355X (printed per geometry): (1,16,16) 0.81, (4,8,8) 0.64, (2,4,6) 1.43, (4,16,16) 0.21;
    test_attn_decode_blocks_vs_fp64: 0.97 (leading-axis split), 1.27 (full split)."""
    from lvt_amd.hip import tx
    Sn = blk[0] * blk[1] * blk[2]
    q, Kc, Vc, banks = _case(blk, seed=40)
    qd, Kd, Vd = _dev(q, Kc, Vc)
    bd = _dev(*banks)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for qi in positions:
        rows = list(range(qi + 1))
        ref = _formula(q[:, qi], Kc, Vc, banks, blk, qi, rows, torch.float64)
        ref32 = _formula(q[:, qi], Kc, Vc, banks, blk, qi, rows, torch.float32)
        got = tx.attn_decode(qd[:, qi].contiguous(), Kd, Vd, H, qi, TEMPER, *bd, blk)
        assert torch.isfinite(got).all(), qi
        err, err32, _ = judge(("o", blk, qi), got, ref, ref32)
        worst = max(worst, err / max(err32, 1e-300))
        if blk == (1, 16, 16):
            wide = torch.full((B, 2 * HD), float("nan"), device=DEV)
            wide[:, :HD] = qd[:, qi]
            assert torch.equal(tx.attn_decode(wide, Kd, Vd, H, qi, TEMPER, *bd, blk, ldq=2 * HD), got), (qi, "ldq")
            pos.fill_(qi)
            cur = tx.attn_decode(qd, Kd, Vd, H, 0, TEMPER, *bd, blk, ldq=Sn * HD, pos=pos, q_pos=HD)
            assert torch.equal(cur, got), (qi, "cursor")
    print("attn_decode_vs_fp64 %s worst err/err32 = %.3f" % (blk, worst))


@pytest.mark.parametrize("qi", [0, 17, 100])
def test_attn_decode_reads_no_key_past_the_query(qi):
    from lvt_amd.hip import tx
    blk = (1, 16, 16)
    q, Kc, Vc, banks = _case(blk, seed=50)
    bd = _dev(*banks)
    qd, = _dev(q[:, qi])
    outs = []
    for fill in (0.0, float("nan")):
        K2, V2 = Kc.clone(), Vc.clone()
        K2[:, qi + 1:] = fill
        V2[:, qi + 1:] = fill
        outs.append(tx.attn_decode(qd, *_dev(K2, V2), H, qi, TEMPER, *bd, blk))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("kind", ["shifted", "spread", "equal_keys"])
def test_attn_decode_extreme_scores(kind):
    """Scores near +200 (exp overflows without the max subtraction), scores spread over +-80 (a one-hot softmax) and equal keys
    (uniform weights: o is the mean of V)."""
    from lvt_amd.hip import tx
    blk, qi = (1, 16, 16), 200
    q, Kc, Vc, banks = _case(blk, seed=60, qscale=120.0 if kind == "spread" else 3.0)
    if kind == "shifted":
        banks[0] = banks[0] + 200.0
    elif kind == "equal_keys":
        Kc[:] = Kc[:, :1]
        banks = [torch.zeros_like(t) for t in banks]
    rows = list(range(qi + 1))
    ref = _formula(q[:, qi], Kc, Vc, banks, blk, qi, rows, torch.float64)
    ref32 = _formula(q[:, qi], Kc, Vc, banks, blk, qi, rows, torch.float32)
    if kind == "spread":                                                 # the premise: one key takes (nearly) everything
        sc = torch.einsum("bhd,bnhd->bhn", q[:, qi].double().view(B, H, DA), Kc[:, rows].double().view(B, qi + 1, H, DA)) / TEMPER
        assert float(sc.max()) > 80 and float(sc.min()) < -80
    if kind == "equal_keys":
        mean = Vc[:, rows].double().mean(1)
        assert float((ref - mean).abs().max()) < 1e-12
    got = tx.attn_decode(*_dev(q[:, qi], Kc, Vc), H, qi, TEMPER, *_dev(*banks), blk)
    assert torch.isfinite(got).all()
    judge(("o", kind), got, ref, ref32)


def _block_keys(thw, blk, qi):
    """-> the cache rows (slice raster order) of the keys of slice position qi: those of its block, in the block's raster order,
    up to the query itself."""
    T, Hs, W = thw
    t, h, w = blk
    tq, hq, wq = qi // (Hs * W), (qi // W) % Hs, qi % W
    ot, oh, ow = tq - tq % t, hq - hq % h, wq - wq % w
    li = ((tq - ot) * h + (hq - oh)) * w + (wq - ow)
    rows = [((ot + a) * Hs + oh + b) * W + ow + c for a in range(t) for b in range(h) for c in range(w)]
    assert rows[li] == qi
    return rows[:li + 1]


@pytest.mark.parametrize("thw,blk", [((8, 4, 4), (2, 4, 4)), ((2, 4, 6), (1, 2, 3))], ids=["leading_axis", "full_split"])
def test_attn_decode_blocks_vs_fp64(thw, blk):
    """lvt_attn_decode_blocks (a leading-axis split: contiguous key rows; a full split with extents that are no powers of two:
    the row table) against the fp64 formula restricted to the keys of the query's block at or before it."""
    from lvt_amd.hip import tx
    Sn, vol = thw[0] * thw[1] * thw[2], blk[0] * blk[1] * blk[2]
    q, Kc, Vc = rand(B, Sn, HD, seed=70) * 3.0, rand(B, Sn, HD, seed=71), rand(B, Sn, HD, seed=72)
    banks = [rand(H, 2 * n - 1, seed=73 + i) * 0.5 for i, n in enumerate(blk)]
    qd, Kd, Vd = _dev(q, Kc, Vc)
    bd = _dev(*banks)
    positions = range(Sn) if Sn <= 48 else sorted({0, 1, vol - 1, vol, vol + 1, Sn // 2 + 3, Sn - vol, Sn - 1})
    worst = 0.0
    for qi in positions:
        rows = _block_keys(thw, blk, qi)
        ref = _formula(q[:, qi], Kc, Vc, banks, blk, len(rows) - 1, rows, torch.float64)
        ref32 = _formula(q[:, qi], Kc, Vc, banks, blk, len(rows) - 1, rows, torch.float32)
        got = tx.attn_decode_blocks(qd[:, qi].contiguous(), Kd, Vd, H, qi, TEMPER, *bd, thw, blk)
        assert torch.isfinite(got).all(), qi
        err, err32, _ = judge(("o", thw, blk, qi), got, ref, ref32)
        worst = max(worst, err / max(err32, 1e-300))
    print("attn_decode_blocks_vs_fp64 %s %s worst err/err32 = %.3f" % (thw, blk, worst))


def test_attn_decode_in_guard_buffers():
    """One launch of each of the three kernels through the C entry with `o` in a NaN-payload buffer: every logical element is
    written and nothing outside it."""
    from lvt_amd.hip import binding as L
    lib = L.lib()
    null = C.c_void_p(0)
    for thw, blk in (((1, 16, 16), (1, 16, 16)), ((8, 4, 4), (2, 4, 4)), ((2, 4, 6), (1, 2, 3))):
        Sn = thw[0] * thw[1] * thw[2]
        qi = Sn - 2
        q, Kc, Vc = rand(B, HD, seed=80) * 3.0, rand(B, Sn, HD, seed=81), rand(B, Sn, HD, seed=82)
        banks = [rand(H, 2 * n - 1, seed=83 + i) * 0.5 for i, n in enumerate(blk)]
        qd, Kd, Vd = _dev(q, Kc, Vc)
        bd = _dev(*banks)
        o = obuf(B, HD)
        if thw == blk:
            rc = lib.lvt_attn_decode(L.ptr(qd), HD, L.ptr(Kd), L.ptr(Vd), B, H, Sn, DA, qi, TEMPER, L.ptr(bd[0]), L.ptr(bd[1]),
                                     L.ptr(bd[2]), blk[0], blk[1], blk[2], L.ptr(o.view), null, 0, L.stream_ptr())
            rows = list(range(qi + 1))
        else:
            rc = lib.lvt_attn_decode_blocks(L.ptr(qd), HD, L.ptr(Kd), L.ptr(Vd), B, H, DA, qi, TEMPER, L.ptr(bd[0]), L.ptr(bd[1]),
                                            L.ptr(bd[2]), thw[0], thw[1], thw[2], blk[0], blk[1], blk[2], L.ptr(o.view), null, 0,
                                            L.stream_ptr())
            rows = _block_keys(thw, blk, qi)
        L.check(rc, "decode %s %s" % (thw, blk))
        torch.cuda.synchronize()
        assert o.outside_untouched(), (thw, blk)
        val = o.logical()
        assert not torch.isnan(val).any(), (thw, blk)
        ref = _formula(q, Kc, Vc, banks, blk, len(rows) - 1, rows, torch.float64)
        assert float((val.double() - ref).abs().max()) < 2e-5 * float(ref.abs().max()), (thw, blk)


ROWS = 200


def _draws(V):
    g = torch.Generator().manual_seed(1000 + V)
    logits = torch.randn(ROWS, V, generator=g) * 3
    u = torch.rand(ROWS, generator=g)
    u[0], u[1] = 0.0, 0.999999
    return logits, u


def _sample(logits, temp, u, **kw):
    """-> codes (rows,), probabilities; the codes go at stride 3 into an int64 guard buffer that must not change elsewhere."""
    from lvt_amd.hip import tx
    out = IBuf(torch.arange(logits.shape[0]) * 3)
    pr = tx.sample_categorical(logits.to(DEV), temp, u.to(DEV), out.view, 3, want_probs=True, **kw)
    torch.cuda.synchronize()
    assert out.outside_untouched()
    return out.logical(), pr.cpu()


@pytest.mark.parametrize("temp", [0.25, 1.0, 4.0])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 100, 1000, 1024, 1025, 2047])
def test_sample_categorical_edges(V, temp):
    """Vocabulary sizes around the lane count (lanes past the end of the row), a ragged last lane, and both sides of the switch
    to the wide instantiation (1024 / 1025), against oracle.multinomial_from_uniform on the fp64 softmax.  A row is safe when its
    threshold is more than 1e-5 away from every cdf step."""
    logits, u = _draws(V)
    prob = torch.softmax(logits.double() / temp, 1)
    want = O.multinomial_from_uniform(prob, u.double())
    cdf = torch.cumsum(prob, 1)
    safe = (cdf - (u.double() * cdf[:, -1]).unsqueeze(1)).abs().min(1).values > 1e-5
    assert int(safe.sum()) >= 185, int(safe.sum())
    got, pr = _sample(logits, temp, u)
    assert got.dtype == torch.int64 and int(got.min()) >= 0 and int(got.max()) < V
    assert torch.equal(got[safe], want[safe])
    assert bool(((got - want).abs() <= 1).all())
    assert rel_err(pr, prob.float()) < 1e-5
    assert float((pr.double().sum(1) - 1).abs().max()) < 1e-5
    if V not in (100, 1025):
        return
    # the device-cursor form: the uniforms are read pos * u_pos elements in
    ubig = torch.rand(4, ROWS, generator=torch.Generator().manual_seed(V))
    ubig[2] = u
    got2, pr2 = _sample(logits, temp, ubig, pos=torch.full((1,), 2, dtype=torch.int32, device=DEV), u_pos=ROWS)
    assert torch.equal(got2, got) and torch.equal(pr2, pr)
    # one logit 60 above the rest (after the temperature): that index for every u < 0.999 (u >= 1e-6: at u == 0 the rule itself
    # returns the first index whose probability is not 0)
    idx = torch.arange(ROWS) * 7 % V
    peak = logits.clone()
    peak[torch.arange(ROWS), idx] = logits.max() + 60.0 * temp
    up = 1e-6 + u * (0.999 - 2e-6)
    up[1] = 0.99899
    got3, _ = _sample(peak, temp, up)
    assert torch.equal(got3, idx)
    # equal logits: cdf_j = (j + 1) / V, so the draw is floor(u V)
    flat = torch.full((ROWS, V), 1.25)
    got4, pr4 = _sample(flat, temp, u)
    steps = (torch.arange(1, V + 1).double() / V)
    safe4 = (steps.unsqueeze(0) - u.double().unsqueeze(1)).abs().min(1).values > 1e-5
    assert int(safe4.sum()) >= 185
    assert torch.equal(got4[safe4], torch.floor(u.double() * V).long()[safe4])
    assert float((pr4 - 1.0 / V).abs().max()) < 1e-5 / V
