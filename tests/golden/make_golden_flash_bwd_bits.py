#!/usr/bin/env python
"""Generate g_flash_bwd_bits.npz: checksums of the BIT PATTERNS that the flash attention backward (csrc/attention_flash.hip:
lvt_attn_bwd_flash, kernels A and B) writes -- dq, dk, dv and delta -- and the three bias-bank gradients verbatim, for both block
geometries, masked and not, one-pass (o given) and two-pass.  The fixture is written by this project's own kernels: run it on an
MI355X at the commit whose results are to be pinned, before a change that must leave the arithmetic bit for bit.

    python tests/golden/make_golden_flash_bwd_bits.py

tests/test_gpu_flash_bwd_loop.py imports the inputs, the launcher and the checksum from here and asserts equality."""
import math
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
S, DA = 256, 128
B, H = 1, 8                 # 8 (sample, head) pairs: the smallest batch tx.attn_flash_supported accepts (pairs % 8 == 0)
SEED = 4242
ZERO_Q_ROW, ZERO_DO_ROW = 5, 200
CASES = [(blk, masked, onepass) for blk in ((1, 16, 16), (4, 8, 8)) for masked in (False, True) for onepass in (True, False)]
OUTPUTS = ("dq", "dk", "dv", "delta")
BANKS = ("ddt", "ddh", "ddw")


def case_tag(blk, masked, onepass):
    return "b%d_%d_%d.%s.%s" % (blk + ("masked" if masked else "full", "onepass" if onepass else "twopass"))


def inputs(blk, seed=SEED):
    """Host-seeded q, k, v, dO (B*S, H*DA) and the three bias banks.  Every row has its own magnitude: v and dO rows between
    1e-6 and 1e4, q and k rows between 1e-6 and 10 (peaked, soft and flat softmax rows all occur); q row ZERO_Q_ROW and dO row
    ZERO_DO_ROW are zero in every head."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, go = (torch.randn(B * S, H * DA, generator=g) for _ in range(4))

    def ladder(lo, hi):
        return torch.pow(10.0, lo + (hi - lo) * torch.rand(B * S, 1, generator=g))
    q, k, v, go = q * ladder(-6, 1), k * ladder(-6, 1), v * ladder(-6, 4), go * ladder(-6, 4)
    q[ZERO_Q_ROW] = 0
    go[ZERO_DO_ROW] = 0
    banks = [torch.randn(H, 2 * n - 1, generator=g) * 0.5 for n in blk]
    return q, k, v, go, banks


def flash_bwd(q, k, v, go, banks, blk, masked, onepass, prefill=float("nan")):
    """Forward, then lvt_attn_bwd_flash into buffers (outputs AND workspace) prefilled with `prefill`.
    -> dict of CPU tensors: dq, dk, dv, delta (B*H*S), ddt, ddh, ddw."""
    from lvt_amd.hip import binding as L, tx
    assert tx.attn_flash_supported(S, DA, blk, B * H)
    qkv = torch.stack([q, k, v]).to(DEV).contiguous()
    bd = [t.to(DEV).contiguous() for t in banks]
    do = go.to(DEV).contiguous()
    temper = math.sqrt(DA)
    o, stats = tx.attn_fwd_flash(qkv, B, H, S, DA, temper, bd[0], bd[1], bd[2], blk, masked)
    M, hd = B * S, H * DA
    dqkv = torch.full((3, M, hd), prefill, dtype=torch.float32, device=DEV)
    dd = [torch.full((H, 2 * n - 1), prefill, dtype=torch.float32, device=DEV) for n in blk]
    lib = L.lib()
    nws = lib.lvt_attn_bwd_flash_workspace_bytes(B, H, S, blk[0], blk[1], blk[2])
    assert nws % 4 == 0
    ws = torch.full((nws // 4,), prefill, dtype=torch.float32, device=DEV)
    L.check(lib.lvt_attn_bwd_flash(L.ptr(qkv[0]), L.ptr(qkv[1]), L.ptr(qkv[2]), L.ptr(do), hd, L.ptr(stats),
                                   L.ptr(o if onepass else None), B, H, S, DA, temper, L.ptr(bd[0]), L.ptr(bd[1]), L.ptr(bd[2]),
                                   blk[0], blk[1], blk[2], 1 if masked else 0, -1e4, L.ptr(dqkv[0]), L.ptr(dqkv[1]), L.ptr(dqkv[2]),
                                   L.ptr(dd[0]), L.ptr(dd[1]), L.ptr(dd[2]), L.out_amax(dqkv), L.ptr(ws), nws, L.stream_ptr()),
            "lvt_attn_bwd_flash")
    torch.cuda.synchronize()
    out = {"dq": dqkv[0], "dk": dqkv[1], "dv": dqkv[2], "delta": ws[:B * H * S], "ddt": dd[0], "ddh": dd[1], "ddw": dd[2]}
    return {n: t.cpu() for n, t in out.items()}


def checksum(t):
    """uint32 [sum, xor, position-weighted sum] over the int32 view of the bit pattern (the third sees a permutation)."""
    u = t.contiguous().numpy().view(np.uint32).reshape(-1).astype(np.uint64)
    w = 2 * np.arange(u.size, dtype=np.uint64) + 1
    mask = np.uint64(0xFFFFFFFF)
    return np.array([int(u.sum() & mask), int(np.bitwise_xor.reduce(u)), int(((u * w) & mask).sum() & mask)], dtype=np.uint32)


if __name__ == "__main__":
    arrays = {"seed": np.int64(SEED)}
    for blk, masked, onepass in CASES:
        q, k, v, go, banks = inputs(blk)
        got = flash_bwd(q, k, v, go, banks, blk, masked, onepass)
        tag = case_tag(blk, masked, onepass)
        for n in OUTPUTS:
            assert torch.isfinite(got[n]).all(), (tag, n)
            assert float(got[n].abs().max()) > 0, (tag, n)
            arrays[tag + "." + n] = checksum(got[n])
        for n in BANKS:
            assert torch.isfinite(got[n]).all(), (tag, n)
            arrays[tag + "." + n] = got[n].numpy()
        print(tag, {n: arrays[tag + "." + n].tolist() for n in OUTPUTS})
    out = os.environ.get("LVT_GOLDEN_OUT", os.path.join(HERE, "g_flash_bwd_bits.npz"))
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
