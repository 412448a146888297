"""Flash attention backward (csrc/attention_flash.hip, kernels A and B) after the per-lane loop invariants of kernel A moved
from registers to an LDS array: (1) the bit patterns of dq / dk / dv / delta and the bank gradients against the fixture that
tests/golden/make_golden_flash_bwd_bits.py wrote with the kernels as they were before that change (the change moves values, it
does not touch arithmetic); (2) the LDS array against its neighbours -- masked launch (two bodies share one shared-memory
block) and unmasked, outputs prefilled with NaN, a bias bank that is different for every query -- against the fp64 evaluation
of tests/test_gpu_flash_attention.py at that file's tolerances."""
import numpy as np
import pytest
import torch

import make_golden_flash_bwd_bits as MK
from test_gpu_flash_attention import _rand, _reference

pytestmark = pytest.mark.gpu
S, DA = MK.S, MK.DA


@pytest.fixture(scope="module")
def bits(golden):
    return golden("g_flash_bwd_bits")


@pytest.mark.parametrize("blk,masked,onepass", MK.CASES, ids=[MK.case_tag(*c) for c in MK.CASES])
def test_flash_bwd_bits_equal_parent(bits, blk, masked, onepass):
    q, k, v, go, banks = MK.inputs(blk, int(bits["seed"]))
    # the inputs do what the fixture was made for: rows from 1e-6 to 1e4, one zero q row, one zero dO row, non-zero banks
    rmax = torch.cat([t.abs().amax(1) for t in (q, k, v, go)])
    assert float(rmax[rmax > 0].min()) < 1e-5 and float(rmax.max()) > 1e3
    assert float(q[MK.ZERO_Q_ROW].abs().max()) == 0.0 and float(go[MK.ZERO_DO_ROW].abs().max()) == 0.0
    assert all(float(b.abs().min()) > 0 for b in banks)
    got = MK.flash_bwd(q, k, v, go, banks, blk, masked, onepass)
    tag = MK.case_tag(blk, masked, onepass)
    bad = []
    for n in MK.OUTPUTS:
        want, have = bits[tag + "." + n].numpy().astype(np.uint32), MK.checksum(got[n])
        print(tag, n, "sum / xor / weighted sum", have.tolist(), "fixture", want.tolist())
        if not np.array_equal(want, have):
            bad.append(n)
    for n in MK.BANKS:
        want, have = bits[tag + "." + n].numpy(), got[n].numpy()
        if not np.array_equal(want.view(np.uint32), have.view(np.uint32)):
            bad.append(n)
    assert not bad, (tag, bad)


@pytest.mark.parametrize("onepass", [True, False], ids=["onepass", "twopass"])
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "full"])
def test_flash_bwd_lane_slots_vs_fp64(masked, onepass):
    """(1, 16, 16) blocks: the h and w banks together give each of the 256 queries of a block its own bias row, q rows carry a
    per-query scale, so m, 1 / l, delta / l and qinv c1 differ from lane to lane -- a slot read from another lane, or one left
    by the first body of the masked launch, moves dq, delta and the bank gradients far beyond the tolerance."""
    blk, B, H = (1, 16, 16), MK.B, MK.H
    q, k, v, go = (_rand(B * S, H * DA, seed=s) for s in (21, 22, 23, 24))
    q = q * (1.0 + 2.0 * torch.arange(B * S).float().view(-1, 1) / (B * S))          # scores of a few units, per-query scale
    go = go * (0.25 + torch.arange(B * S).flip(0).float().view(-1, 1) / (B * S))
    banks = [_rand(H, 2 * n - 1, seed=25 + i) * 1.5 for i, n in enumerate(blk)]
    ref = _reference(q, k, v, go, banks, blk, masked)
    _, _, _, rdq, _, _, rdt, rdh, rdw = ref[:9]                                 # (ref[9] is the attention matrix)
    # delta_i = dO_i . O_i per (sample, head, query)
    o64 = ref[0].view(B, S, H, DA)
    rdelta = (o64 * go.double().view(B, S, H, DA)).sum(-1).permute(0, 2, 1).reshape(-1)
    got = MK.flash_bwd(q, k, v, go, banks, blk, masked, onepass)               # NaN-prefilled outputs and workspace
    bank_scale = max(float(t.abs().max()) for t in (rdt, rdh, rdw))
    for n, r, scale in (("dq", rdq, None), ("delta", rdelta, None), ("ddt", rdt, bank_scale), ("ddh", rdh, bank_scale),
                        ("ddw", rdw, bank_scale)):
        a = got[n]
        assert torch.isfinite(a).all(), n
        scale = float(r.abs().max()) if scale is None else scale
        err = float((a.double() - r).abs().max())
        print(n, "err", err, "bound", 2e-5 * scale)
        assert err < 2e-5 * scale, (n, err, scale)
