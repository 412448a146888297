"""Typed wrappers over the l2-normalisation kernels of the cosine codebook lookup (csrc/l2norm.hip).  The rule they
follow is stated in plain torch in lvt_amd/modeling/vq/cosine.py."""
import torch

from . import binding as L

EPS = 1e-12              # F.normalize's default, the eps of MODEL.CODEBOOK.COSINE


def _geometry(name, x, d):
    L.require(x)
    if x.dtype != torch.float32 or x.dim() < 1 or d <= 0 or x.shape[-1] % d:
        raise L.LvtError("%s: a float32 tensor whose last dimension is a multiple of the group width %r (got %s %s)"
                         % (name, d, x.dtype, tuple(x.shape)))
    width = x.shape[-1]
    return x.numel() // width, width // d


def l2norm_groups_fwd(x, d, eps=EPS, inplace=False, want_inv=True):
    """x (..., G * d) contiguous float32 -> (y, inv): every d-wide group of the last dimension divided by max(its l2 norm,
    eps), and inv (rows, G) = 1 / max(norm, eps) (None unless want_inv).  inplace: y is x.  Reports max |y| (f16x2 mode)."""
    rows, G = _geometry("l2norm_groups_fwd", x, d)
    y = x if inplace else torch.empty_like(x)
    inv = torch.empty(rows, G, dtype=torch.float32, device=x.device) if want_inv else None
    L.check(L.lib().lvt_l2norm_groups_fwd(L.ptr(x), rows, G, d, eps, L.ptr(y), L.ptr(inv), L.out_amax(y), L.stream_ptr()),
            "lvt_l2norm_groups_fwd")
    return y, inv


def l2norm_groups_bwd(g, y, inv, d, eps=EPS):
    """The gradient at x of l2norm_groups_fwd from the gradient g at y (the forward's y and inv; a group the forward clamped is
    recognised by inv == 1 / eps).  Reports max |dx| (f16x2 mode)."""
    rows, G = _geometry("l2norm_groups_bwd", g, d)
    L.require(y, inv)
    if y.shape != g.shape or y.dtype != torch.float32 or inv.dtype != torch.float32 or inv.numel() != rows * G:
        raise L.LvtError("l2norm_groups_bwd: y like g and inv (rows, G) float32 (got %s, %s for g %s)"
                         % (tuple(y.shape), tuple(inv.shape), tuple(g.shape)))
    dx = torch.empty_like(g)
    L.check(L.lib().lvt_l2norm_groups_bwd(L.ptr(g), L.ptr(y), L.ptr(inv), rows, G, d, eps, L.ptr(dx), L.out_amax(dx),
                                          L.stream_ptr()), "lvt_l2norm_groups_bwd")
    return dx
