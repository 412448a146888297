"""Finite scalar quantisation, MODEL.CODEBOOK.FSQ.LEVELS (Mentzer et al. 2023), stated once in plain torch.

This module is the rule of record: the kernels of csrc/fsq.hip and FSQEmbedding (fsq_embedding.py) follow it, and the tests hold
them to it in float64.  Nothing here runs on the training path; every function works in whatever dtype it is handed.

levels = (L_1 .. L_d); a row z_e of the encoder output has D = CODEBOOK.DIM entries:

  1. z_p = z_e W_in^T + b_in: NUM * d entries, NUM groups of d                                                  `project_in`
  2. per entry i of a group, with eps = 1e-3: half_l = (L_i - 1)(1 + eps) / 2, offset = 0.5 for an even L_i else 0,
     shift = atanh(offset / half_l),  b = tanh(z_p + shift) * half_l - offset                                   `bound`
     (the constants are formed in float64: `constants`)
  3. q = round(b), half to even; w_i = L_i // 2; digit_i = q + w_i in [0, L_i - 1]                              `digits`
  4. z_q[i] = q / w_i in [-1, 1]; index of the group = sum_i digit_i prod_{j<i} L_j (first level fastest);
     prod(levels) = V                                                                                            `quantise`, `index`
  5. z_out = z_q W_out^T + b_out: D entries, what the decoder receives                                           `project_out`
  6. the straight-through estimator goes through the rounding only:
     d z_q[i] / d z_p[i] = half_l (1 - tanh^2(z_p + shift)) / w_i                                               `quantise_backward`
     everything else is ordinary linear backward; train and eval mode are the same function
  7. decode from indices: digits by successive division, then z_q, then step 5                                  `digits_of`, `decode`
"""
import math

import torch

EPS = 1e-3
MAX_LEVELS, MIN_LEVEL, MAX_LEVEL, MAX_CODES = 11, 2, 64, 2048     # what csrc/fsq.hip and the sampling kernels take


def check_levels(levels):
    """-> tuple of ints, or ValueError naming MODEL.CODEBOOK.FSQ.LEVELS."""
    key = "MODEL.CODEBOOK.FSQ.LEVELS"
    levels = list(levels)
    if not levels:
        raise ValueError("%s is empty" % key)
    for l in levels:
        if isinstance(l, bool) or not isinstance(l, int):
            raise ValueError("%s: every level is an integer from %d to %d (got %r)" % (key, MIN_LEVEL, MAX_LEVEL, l))
        if not MIN_LEVEL <= l <= MAX_LEVEL:
            raise ValueError("%s: every level is an integer from %d to %d (got %r)" % (key, MIN_LEVEL, MAX_LEVEL, l))
    if len(levels) > MAX_LEVELS:
        raise ValueError("%s: at most %d levels (got %d)" % (key, MAX_LEVELS, len(levels)))
    if math.prod(levels) > MAX_CODES:
        raise ValueError("%s: prod(LEVELS) = %d codes, the sampling kernels take at most %d" % (key, math.prod(levels), MAX_CODES))
    return tuple(levels)


def constants(levels, dtype=torch.float64):
    """-> (half_l, offset, shift, w, basis), each (d,): formed in float64, then cast (w and basis stay int64)."""
    L = torch.tensor(list(levels), dtype=torch.float64)
    half_l = (L - 1.0) * (1.0 + EPS) / 2.0
    offset = torch.where(L.long() % 2 == 0, torch.full_like(L, 0.5), torch.zeros_like(L))
    shift = torch.atanh(offset / half_l)
    w = L.long() // 2
    basis = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.int64), L.long()[:-1]]), 0)
    return half_l.to(dtype), offset.to(dtype), shift.to(dtype), w, basis


def _groups(x, d):
    return x.unflatten(-1, (-1, d))


def bound(z_p, levels):
    """(..., G * d) -> the same shape (step 2)."""
    half_l, offset, shift, _, _ = constants(levels, z_p.dtype)
    return (torch.tanh(_groups(z_p, len(levels)) + shift) * half_l - offset).flatten(-2)


def digits(z_p, levels):
    """(..., G * d) -> int64 of the same shape: digit_i = round(b) + w_i (step 3)."""
    w = constants(levels)[3]
    return (_groups(torch.round(bound(z_p, levels)), len(levels)).long() + w).flatten(-2)


def value_of(dig, levels, dtype=torch.float64):
    """digits (..., G * d) int64 -> z_q = (digit - w) / w (step 4)."""
    w = constants(levels)[3]
    g = _groups(dig, len(levels))
    return ((g - w).to(dtype) / w.to(dtype)).flatten(-2)


def index(dig, levels):
    """digits (..., G * d) int64 -> (..., G) int64, first level fastest (step 4)."""
    return (_groups(dig, len(levels)) * constants(levels)[4]).sum(-1)


def digits_of(idx, levels):
    """(..., G) int64 -> digits (..., G * d) by successive division (step 7)."""
    out, rest = [], idx
    for l in levels:
        out.append(rest % l)
        rest = rest // l
    return torch.stack(out, -1).flatten(-2)


class _RoundST(torch.autograd.Function):
    """round half to even with the gradient of the identity (step 6)."""

    @staticmethod
    def forward(ctx, b):
        return torch.round(b)

    @staticmethod
    def backward(ctx, g):
        return g


def quantise(z_p, levels):
    """z_p (..., G * d) -> (z_q of the same shape, idx (..., G) int64); z_q carries the straight-through graph to z_p."""
    w = constants(levels)[3]
    q = _groups(_RoundST.apply(bound(z_p, levels)), len(levels))
    z_q = (q / w.to(z_p.dtype)).flatten(-2)
    return z_q, index((q.detach().long() + w).flatten(-2), levels)


def quantise_backward(g, z_p, levels):
    """The gradient at z_p from the gradient g at z_q, in closed form (step 6)."""
    half_l, _, shift, w, _ = constants(levels, z_p.dtype)
    t = torch.tanh(_groups(z_p, len(levels)) + shift)
    return (_groups(g, len(levels)) * (half_l * (1.0 - t * t) / w.to(z_p.dtype))).flatten(-2)


def project_in(z_e, w_in, b_in):
    return z_e @ w_in.t() + b_in


def project_out(z_q, w_out, b_out):
    return z_q @ w_out.t() + b_out


def step(z_e, w_in, b_in, w_out, b_out, levels, force_idx=None):
    """Rows z_e (rows, D) -> dict(z_p, z_q, idx (rows, NUM), z_out), steps 1 to 5 with the graph of step 6.  force_idx
    (rows, NUM): continue with these codes (isolates inputs on a rounding boundary from the rest): z_q takes their value, the
    gradient stays that of step 6."""
    z_p = project_in(z_e, w_in, b_in)
    z_q, idx = quantise(z_p, levels)
    if force_idx is not None:
        forced = value_of(digits_of(force_idx, levels), levels, z_p.dtype)
        z_q = z_q + (forced - z_q).detach()
        idx = force_idx
    return {"z_p": z_p, "z_q": z_q, "idx": idx, "z_out": project_out(z_q, w_out, b_out)}


def decode(idx, w_out, b_out, levels, dtype=torch.float64):
    """idx (..., NUM) int64 -> z_out (..., D) (step 7)."""
    return project_out(value_of(digits_of(idx, levels), levels, dtype), w_out, b_out)
