"""Shared by the attention kernel tests (test_gpu_flash_attention.py, test_gpu_flash_matrix.py, test_gpu_plane_attention.py,
test_gpu_decode_kernels.py):
the fp64 autograd evaluation of the reference formula for one 256-token x 128-dim block layer
(vidgen/modeling/autoregressive/vt_attention.py:59-81 with the bias of :169-174), the exact 3-way bf16 split that the plane
kernels take their operands in, and the acceptance rule of the attention tests."""
import math

import torch

from oracle import lvt_oracle as O

S, DA = 256, 128


def rand(*shape, seed=0):
    """Uniform in (-1, 1), seeded by `seed` and the shape (the draw of the flash tests)."""
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * 2 - 1


def reference(q, k, v, go, banks, blk, masked, dtype=torch.float64, temper=None):
    """-> o, m, linv, dq, dk, dv, dbanks (3), P in `dtype` on the CPU (autograd of the reference formula).  q / k / v / go are
    token-major (B*S, H*DA), P is (B, H, S, S).  temper: what the scores are divided by (None: sqrt(DA), the layer's value)."""
    B = q.shape[0] // S
    H = q.shape[1] // DA
    temper = math.sqrt(DA) if temper is None else temper
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (q, k, v)]
    bl = [t.to(dtype).clone().requires_grad_(True) for t in banks]
    qh, kh, vh = [t.view(B, S, H, DA).permute(0, 2, 1, 3) for t in leaves]
    bias = O.rel_position_bias(*bl, blk).transpose(0, 1)                                # (1, H, S, S)
    sc = qh @ kh.transpose(2, 3) / temper + bias
    if masked:
        sc = sc.masked_fill(torch.triu(torch.ones(S, S), 1).bool(), -1e4)
    P = torch.softmax(sc, -1)
    o = (P @ vh).permute(0, 2, 1, 3).reshape(B * S, H * DA)
    o.backward(go.to(dtype))
    m = sc.max(-1).values * math.log2(math.e)          # the kernels keep the row max in log2 units
    linv = 1.0 / torch.exp(sc - sc.max(-1, keepdim=True).values).sum(-1)
    return ([o.detach(), m.detach().reshape(-1), linv.detach().reshape(-1)] + [t.grad for t in leaves] + [t.grad for t in bl]
            + [P.detach()])


def bf16x3_split(x):
    """fp32 (...) -> bf16 (3, ...): p1 = RNE_bf16(v), p2 = RNE_bf16(v - p1), p3 = v - p1 - p2, the planes the PLANES epilogue
    of the engine writes (test_gpu_gemm_matrix.py::test_planes_are_the_exact_bf16_split)."""
    v = x.float()
    p1 = v.to(torch.bfloat16)
    p2 = (v - p1.float()).to(torch.bfloat16)
    p3 = (v - p1.float() - p2.float()).to(torch.bfloat16)
    return torch.stack([p1, p2, p3])


def split_restores(x, planes):
    """The three planes, added as fp32 smallest first, give back the fp32 operand bit for bit (a CPU check: the fp64 reference
    may then take the fp32 operand as it is)."""
    back = (planes[2].float() + planes[1].float()) + planes[0].float()
    return torch.equal(back.view(torch.int32), x.float().view(torch.int32))


ATTENTION_ENTRIES = ("attn_fwd_planes", "attn_bwd_planes", "attn_fwd_flash", "attn_bwd_flash", "attn_fwd", "attn_softmax_fwd_",
                     "attn_softmax_bwd_")


def count_attention_calls(monkeypatch):
    """Wrap the attention entry points of lvt_amd.hip.tx (vt_attention.py calls them through the module) -> dict of call counts
    that the wrappers keep up to date: which path a layer took is then a fact of the test, not an assumption."""
    from lvt_amd.hip import tx
    counts = dict.fromkeys(ATTENTION_ENTRIES, 0)

    def wrap(name, real):
        def counted(*args, **kwargs):
            counts[name] += 1
            return real(*args, **kwargs)
        return counted

    for name in ATTENTION_ENTRIES:
        monkeypatch.setattr(tx, name, wrap(name, getattr(tx, name)))
    return counts


def calls(counts, **expected):
    """True when `counts` holds exactly `expected` and zero everywhere else."""
    return all(counts[n] == expected.get(n, 0) for n in ATTENTION_ENTRIES)


def judge(name, got, ref, ref32, scale=None):
    """The attention tests' rule: |got - fp64| < max(2e-5 * scale, 4 * |fp32 evaluation - fp64|).  -> (err, err32, scale)
    after asserting; scale defaults to the tensor's max."""
    ref = ref.double()
    scale = float(ref.abs().max()) if scale is None else scale
    err = float((got.double().cpu() - ref).abs().max())
    err32 = float((ref32.double() - ref).abs().max())
    assert err < max(2e-5 * scale, 4 * err32), (name, err, err32, scale)
    return err, err32, scale
