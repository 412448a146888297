"""Typed wrappers over the batch-normalisation kernels (csrc/norm.hip).

Activations are channels-last (..., Cp) fp32 viewed as (M, Cp).  Per-channel vectors are Cp long; the statistics of one
rank are `stats` = (mean, biased var), a forward pass keeps `saved` = (mean, rstd) for its backward."""
import torch

from . import binding as L


def _rows(y):
    Cp = y.shape[-1]
    return y.numel() // Cp, Cp


def _ws(M, Cp, dev):
    n = L.lib().lvt_bn_workspace_bytes(M, Cp)
    return L.workspace(n, dev, "bn"), n


def stats(y):
    """-> (2, Cp) tensor: per-channel mean and biased variance of y over all its rows."""
    L.require(y)
    M, Cp = _rows(y)
    out = torch.empty(2, Cp, dtype=torch.float32, device=y.device)
    ws, n = _ws(M, Cp, y.device)
    L.check(L.lib().lvt_bn_stats(L.ptr(y), M, Cp, L.ptr(out), L.ptr(ws), n, L.stream_ptr()), "lvt_bn_stats")
    return out


def finalize(C, Cp, gamma, beta, running_mean, running_var, stats=None, nranks=1, count=0, num_batches_tracked=None,
             momentum=0.1, eps=1e-5, flags=0):
    """-> (scale, shift, saved): scale / shift (Cp) and saved = (2, Cp) (mean, rstd).  stats: (nranks, 2, Cp) or (2, Cp), over
    `count` rows per rank; ignored with BN_RUNNING."""
    L.require(stats, gamma, beta, running_mean, running_var, num_batches_tracked)
    dev = gamma.device
    buf = torch.empty(4, Cp, dtype=torch.float32, device=dev)
    scale, shift, saved = buf[0], buf[1], buf[2:]
    L.check(L.lib().lvt_bn_finalize(L.ptr(stats), nranks, count, C, Cp, L.ptr(gamma), L.ptr(beta), L.ptr(running_mean),
                                    L.ptr(running_var), L.ptr(num_batches_tracked), float(momentum), float(eps), flags,
                                    L.ptr(scale), L.ptr(shift), L.ptr(saved), L.stream_ptr()), "lvt_bn_finalize")
    if running_mean is not None and flags & L.BN_UPDATE:
        L.drop_amax(running_mean)
        L.drop_amax(running_var)
    return scale, shift, saved


def apply(y, scale, shift, res=None, act=0):
    """act(y * scale + shift (+ res)); act: 0, binding.EPI_RELU, binding.EPI_LEAKY, binding.EPI_TANH or binding.EPI_SIGMOID | binding.epi_pad(n)
    (the last n channels are zero pads and stay 0).  Reports max |out| (f16x2 mode)."""
    L.require(y, res)
    M, Cp = _rows(y)
    out = torch.empty_like(y)
    L.check(L.lib().lvt_bn_apply(L.ptr(y), L.ptr(res), M, Cp, L.ptr(scale), L.ptr(shift), act, L.ptr(out), L.out_amax(out),
                                 L.stream_ptr()), "lvt_bn_apply")
    return out


def bwd_reduce(g, y, saved):
    """-> (2, Cp) tensor: (sum g, sum g * xhat) per channel, i.e. (dbeta, dgamma)."""
    L.require(g, y)
    M, Cp = _rows(y)
    out = torch.empty(2, Cp, dtype=torch.float32, device=y.device)
    ws, n = _ws(M, Cp, y.device)
    L.check(L.lib().lvt_bn_bwd_reduce(L.ptr(g), L.ptr(y), M, Cp, L.ptr(saved), L.ptr(out), L.ptr(ws), n, L.stream_ptr()),
            "lvt_bn_bwd_reduce")
    return out


def bwd_apply(g, y, scale, saved=None, sums=None, n=0, train=True):
    """dL/dy from the gradient g at the normalised output: batch-statistics backward over n rows (all ranks) with
    `train`, else scale * g.  Reports max |dy| (f16x2 mode)."""
    L.require(g, y)
    M, Cp = _rows(g)
    dy = torch.empty_like(g)
    L.check(L.lib().lvt_bn_bwd_apply(L.ptr(g), L.ptr(y) if train else None, M, Cp, L.ptr(scale),
                                     L.ptr(saved) if train else None, L.ptr(sums) if train else None, int(n),
                                     L.BN_TRAIN if train else 0, L.ptr(dy), L.out_amax(dy), L.stream_ptr()), "lvt_bn_bwd_apply")
    return dy


def fold(layers):
    """Eval fold of many layers in one launch.  layers: [(weight, transposed, norm module, Cp)], weight in torch layout (a
    ConvTranspose weight is (Ci, Co, k..): its output channel is dim 1).  -> [(folded weight, bias (Cp,))]: the weight with
    every output channel scaled by gamma rstd of the running statistics, and the bias beta - running_mean gamma rstd."""
    sizes = [((w.numel() + 3) // 4 * 4, cp) for w, _, _, cp in layers]
    buf = torch.empty(sum(n + cp for n, cp in sizes), dtype=torch.float32, device=layers[0][0].device)
    arr = (L.BnFoldEntry * len(layers))()
    out, pos = [], 0
    for e, (w, transposed, nm, cp), (nw, _) in zip(arr, layers, sizes):
        L.require(w, nm.weight, nm.bias, nm.running_mean, nm.running_var)
        bias = buf[pos:pos + cp]                      # every piece starts on a 16-byte boundary
        wo = buf[pos + cp:pos + cp + w.numel()].view(w.shape)
        pos += cp + nw
        e.outer, e.Co = (w.shape[0], w.shape[1]) if transposed else (1, w.shape[0])
        e.inner, e.Cp = w.numel() // (e.outer * e.Co), cp
        e.w, e.w_out, e.bias_out = w.data_ptr(), wo.data_ptr(), bias.data_ptr()
        e.gamma, e.beta = nm.weight.data_ptr(), nm.bias.data_ptr()
        e.running_mean, e.running_var, e.eps = nm.running_mean.data_ptr(), nm.running_var.data_ptr(), float(nm.eps)
        e.w_amax = L.new_amax(wo).data_ptr() if L.f16x2() else None
        out.append((wo, bias))
    L.check(L.lib().lvt_bn_fold(arr, len(layers), L.stream_ptr()), "lvt_bn_fold")
    return out
