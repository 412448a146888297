"""Residual dropout of the video transformer: the random stream stated once in plain Python (numpy), and the
typed wrappers over the two kernels of csrc/dropout.hip, which follow it bit for bit.

The stream is counter-based: element `i` of a flat tensor is kept iff word `i & 3` of Philox4x32-10 under

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (g & 0xffffffff, g >> 32, site + 4096 * rank, pass),        g = i >> 2

is >= T = floor(p 2^32); kept elements are scaled by s = fp32(1 / (1 - p)).  `site = 2 * layer + branch` (branch 0: the
attention branch, 1: the FFN branch; the encoder's layers count first), `rank` the process's rank in the default group, `pass`
the index of the training-mode forward.  The backward regenerates the mask from the same four numbers, so nothing mask-sized
is stored.
"""
import math

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MAX_LAYERS, MAX_RANKS = 2048, 1 << 20
CONFIG_KEY = "MODEL.AUTOREGRESSIVE.VT.DROPOUT"
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011).  counter: four 32-bit words, key: two; each an int or a numpy array of them (arrays
    broadcast).  -> the four output words: ints when every input is an int, else uint32 arrays."""
    scalar = all(isinstance(v, (int, np.integer)) for v in tuple(counter) + tuple(key))
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & np.uint64(_M32) for v in counter)
    k0, k1 = (np.asarray(v, dtype=np.uint64) & np.uint64(_M32) for v in key)
    m32, sh = np.uint64(_M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2          # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m32, (p0 >> sh) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m32, (k1 + np.uint64(PHILOX_W1)) & m32
    if scalar:
        return int(c0), int(c1), int(c2), int(c3)
    return tuple(np.broadcast_arrays(*(c.astype(np.uint32) for c in (c0, c1, c2, c3))))


def check_rate(p, key=CONFIG_KEY):
    """The dropout rate as a float; a negative, >= 1.0 or non-finite one is a ValueError that names `key`."""
    try:
        v = float(p)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number in [0, 1), got %r" % (key, p))
    if not (math.isfinite(v) and 0.0 <= v < 1.0):
        raise ValueError("%s must be finite and in [0, 1), got %r" % (key, p))
    return v


def threshold(p):
    """T = floor(p 2^32) in double: an element is kept iff its word is >= T (p = 0 keeps everything)."""
    return int(math.floor(check_rate(p) * 4294967296.0))


def scale(p):
    """s = the fp32 rounding of 1 / (1 - p)."""
    return np.float32(1.0 / (1.0 - check_rate(p)))


def site_rank(layer, branch, rank=0):
    """Counter word 2: site + 4096 * rank, site = 2 * layer + branch."""
    if not 0 <= layer < MAX_LAYERS:
        raise ValueError("dropout: layer %r, at most %d attention layers" % (layer, MAX_LAYERS))
    if branch not in (0, 1):
        raise ValueError("dropout: branch %r is neither 0 (attention) nor 1 (FFN)" % (branch,))
    if not 0 <= rank < MAX_RANKS:
        raise ValueError("dropout: rank %r, ranks below %d only" % (rank, MAX_RANKS))
    return 2 * layer + branch + 4096 * rank


def words(seed, site_rank_, pass_, n):
    """The stream's first n words as a uint32 array: word 4 g + j is output j of group g."""
    if n <= 0:
        return np.zeros(0, dtype=np.uint32)
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = philox4x32_10((g & np.uint64(_M32), g >> np.uint64(32), int(site_rank_) & _M32, int(pass_) & _M32),
                        (seed & _M32, seed >> 32))
    return np.stack(out, axis=1).reshape(-1)[:n]


def keep_mask(seed, site_rank_, pass_, n, p):
    """bool array of n: True where the element is kept."""
    return words(seed, site_rank_, pass_, n) >= np.uint32(threshold(p))


def dropout_add_reference(z, res, seed, site_rank_, pass_, p):
    """What lvt_dropout_add / lvt_dropout_bwd (res None) compute, as a float32 numpy statement: the product is rounded on its own."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    keep = keep_mask(seed, site_rank_, pass_, z.size, p).reshape(z.shape)
    zs = z * scale(p)
    if res is None:
        return np.where(keep, zs, np.float32(0.0))
    res = np.ascontiguousarray(res, dtype=np.float32)
    return np.where(keep, res + zs, res)


class DropoutState:
    """seed and pass index of one model's dropout stream: host integers, owned by VideoTransformer and shared by its layers (a
    layer built on its own makes one).  Neither is persistent: a resumed run starts the pass count again."""

    def __init__(self, seed=None):
        if seed is None:
            import torch
            seed = torch.initial_seed()          # (reads the default generator's seed; does not advance it)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.pass_ = 0                           # what the layers use
        self._next = 0

    def set_seed(self, seed):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def set_next_pass(self, n):
        """The index the next begin_pass() hands out (replaying a pass)."""
        self._next = int(n)

    def begin_pass(self):
        """Called once per training-mode forward: the first pass uses 0."""
        self.pass_ = self._next & _M32
        self._next += 1
        return self.pass_


def current_rank():
    """The process's rank in the default group, 0 without one."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return 0


def _launch(name, z, res, state_tuple, p, out):
    from . import binding as L
    import torch
    seed, sr, pass_ = state_tuple
    L.require(z, res)
    if z.dtype != torch.float32 or (res is not None and (res.dtype != torch.float32 or res.numel() != z.numel())):
        raise L.LvtError("%s: float32 tensors of one size" % name)
    if out is None:
        out = torch.empty_like(z)
    elif out is not z:
        raise L.LvtError("%s: out is a new tensor or z itself" % name)
    T, s = threshold(p), float(scale(p))
    seed, sr, pass_ = int(seed) & 0xFFFFFFFFFFFFFFFF, int(sr) & _M32, int(pass_) & _M32
    if name == "lvt_dropout_add":
        L.check(L.lib().lvt_dropout_add(L.ptr(z), L.ptr(res), z.numel(), seed, sr, pass_, T, s, L.ptr(out), L.out_amax(out),
                                        L.stream_ptr()), name)
    else:
        L.check(L.lib().lvt_dropout_bwd(L.ptr(z), z.numel(), seed, sr, pass_, T, s, L.ptr(out), L.out_amax(out), L.stream_ptr()),
                name)
    return out


def dropout_add(z, res, state_tuple, p, inplace=False):
    """res + D(z) (D(z) alone when res is None) under state_tuple = (seed, site_rank, pass) and rate p; `inplace` writes into z.
    Reports max |out| (f16x2 mode)."""
    return _launch("lvt_dropout_add", z, res, state_tuple, p, z if inplace else None)


def dropout_bwd(g, state_tuple, p):
    """D(g): the gradient through the mask the forward drew under the same state_tuple.  Reports max |out| (f16x2 mode)."""
    return _launch("lvt_dropout_bwd", g, None, state_tuple, p, None)
