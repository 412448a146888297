"""Typed wrappers over the finite-scalar-quantisation kernels (csrc/fsq.hip).  The rule they follow is stated in
plain torch in lvt_amd/modeling/vq/fsq.py.  Rows are (rows, ld) float32 with ld >= num * len(levels) a multiple of 4; the pad
columns are zero on entry and on exit.  Codes are int64 (rows / P, num, P), the layout of hip/vq.py nearest."""
import torch

from . import binding as L


def table(levels):
    """The by-value launch argument for a level tuple."""
    levels = tuple(int(l) for l in levels)
    if not 1 <= len(levels) <= L.FSQ_MAX_LEVELS:
        raise L.LvtError("fsq: from 1 to %d levels (got %d)" % (L.FSQ_MAX_LEVELS, len(levels)))
    t = L.FsqLevels()
    t.d = len(levels)
    for i, l in enumerate(levels):
        t.levels[i] = l
    return t


def padded_width(num, levels):
    """num * d rounded up to the multiple of 4 the engine and the 16-byte accesses want."""
    return (num * len(levels) + 3) // 4 * 4


def _rows(name, x, num, levels):
    L.require(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] % 4 or x.shape[1] < num * len(levels):
        raise L.LvtError("%s: a (rows, ld) float32 tensor with ld a multiple of 4 and at least num * d = %d (got %s %s)"
                         % (name, num * len(levels), x.dtype, tuple(x.shape)))
    return x.shape[0], x.shape[1]


def fsq_fwd(z_p, num, levels, P=None, want_zq=True, want_idx=True):
    """z_p (rows, ld) -> (z_q (rows, ld) or None, idx (rows / P, num, P) int64 or None).  Reports max |z_q| (f16x2 mode)."""
    rows, ld = _rows("fsq_fwd", z_p, num, levels)
    if not (want_zq or want_idx):
        raise L.LvtError("fsq_fwd: neither z_q nor idx wanted")
    P = rows if P is None else P
    if want_idx and (P < 1 or rows % P):
        raise L.LvtError("fsq_fwd: P = %r must divide rows = %d" % (P, rows))
    z_q = torch.empty_like(z_p) if want_zq else None
    idx = torch.empty(rows // P, num, P, dtype=torch.int64, device=z_p.device) if want_idx else None
    L.check(L.lib().lvt_fsq_fwd(L.ptr(z_p), rows, num, ld, table(levels), P, L.ptr(z_q), L.ptr(idx),
                                L.out_amax(z_q) if want_zq else None, L.stream_ptr()), "lvt_fsq_fwd")
    return z_q, idx


def fsq_bwd(g, z_p, num, levels):
    """The gradient at z_p from the gradient g at z_q (straight through the rounding).  Reports max |dz_p| (f16x2 mode)."""
    rows, ld = _rows("fsq_bwd", g, num, levels)
    L.require(z_p)
    if z_p.shape != g.shape or z_p.dtype != torch.float32:
        raise L.LvtError("fsq_bwd: z_p like g (got %s for g %s)" % (tuple(z_p.shape), tuple(g.shape)))
    dz_p = torch.empty_like(g)
    L.check(L.lib().lvt_fsq_bwd(L.ptr(g), L.ptr(z_p), rows, num, ld, table(levels), L.ptr(dz_p), L.out_amax(dz_p),
                                L.stream_ptr()), "lvt_fsq_bwd")
    return dz_p


def fsq_decode(idx, levels, ld=None):
    """idx (n, num, P) int64 -> z_q (n * P, ld) float32, ld = num * d rounded up to 4 unless given.  Reports max |z_q|."""
    L.require(idx)
    if idx.dtype != torch.int64 or idx.dim() != 3:
        raise L.LvtError("fsq_decode: idx (n, num, P) int64 (got %s %s)" % (idx.dtype, tuple(idx.shape)))
    n, num, P = idx.shape
    ld = padded_width(num, levels) if ld is None else ld
    z_q = torch.empty(n * P, ld, dtype=torch.float32, device=idx.device)
    L.check(L.lib().lvt_fsq_decode(L.ptr(idx), n * P, num, ld, table(levels), P, L.ptr(z_q), L.out_amax(z_q), L.stream_ptr()),
            "lvt_fsq_decode")
    return z_q
