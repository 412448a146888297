"""Truncated sampling of the video transformer: the rule, stated once in plain torch (fp64), and the argument check.

For one row of V logits x, temp > 0, integer top_k >= 0 and 0 < top_p <= 1:

1. weights  w_j = exp((x_j - max x) / temp);
2. top-k first: with top_k == 0 or top_k >= V every index is kept; otherwise A = { j : x_j >= t_k } with t_k the k-th
   largest logit counting multiplicity -- logits equal to the k-th are all kept, so |A| may exceed k.  Selection is on the
   logits themselves (exact in fp32), not on w;
3. top-p on what top-k left, renormalised over it: with top_p == 1 B = A; otherwise M(t) = sum of w_j over j in A with
   x_j >= t, t_p is the largest logit value t in A with M(t) >= top_p * M(-inf), and B = { j in A : x_j >= t_p } -- the
   smallest set of most likely codes whose mass reaches top_p, ties at the boundary kept, the arg-max always in it;
4. probs_j = w_j / sum_B w on B and exactly 0 elsewhere;
5. the draw is the inverse-CDF rule in memory order on the truncated weights, code = #{ j : cdf_j <= u * total_B }; where
   rounding puts the count past the last kept index the result is the last kept index.  A code outside B is never drawn.

lvt_sample_truncated (csrc/transformer.hip) computes this on the GPU; these functions are what it is tested against.
"""
import math
import numbers

import torch

KEY_TEMPERATURE = "TEST.VT_SAMPLER.TEMPERATURE"
KEY_TOP_K = "TEST.VT_SAMPLER.TOP_K"
KEY_TOP_P = "TEST.VT_SAMPLER.TOP_P"


def check_sampling(temp, top_k, top_p):
    """(float temp, int top_k, float top_p); a ValueError that names the config key for temp <= 0 or not finite, top_k < 0 or
    not an integer, top_p outside (0, 1] or not finite."""
    try:
        t = float(temp)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number > 0, got %r" % (KEY_TEMPERATURE, temp))
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError("%s must be finite and > 0, got %r" % (KEY_TEMPERATURE, temp))
    if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral):
        raise ValueError("%s must be an integer >= 0 (0: off), got %r" % (KEY_TOP_K, top_k))
    if top_k < 0:
        raise ValueError("%s must be >= 0 (0: off), got %r" % (KEY_TOP_K, top_k))
    try:
        p = float(top_p)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number in (0, 1], got %r" % (KEY_TOP_P, top_p))
    if not (math.isfinite(p) and 0.0 < p <= 1.0):
        raise ValueError("%s must be finite and in (0, 1] (1.0: off), got %r" % (KEY_TOP_P, top_p))
    return t, int(top_k), p


def truncation_off(top_k, top_p):
    """True when neither cut is asked for: the callers then issue exactly the launches of untruncated sampling."""
    return top_k == 0 and top_p == 1.0


def truncated_probs_reference(logits, temp, top_k, top_p):
    """logits (..., V) -> fp64 probabilities of the rule above (exactly 0 on a cut code)."""
    x = logits.detach().to("cpu", torch.float64)
    V = x.shape[-1]
    w = torch.exp((x - x.amax(-1, keepdim=True)) / temp)
    keep = torch.ones_like(x, dtype=torch.bool)
    if 0 < top_k < V:
        t_k = torch.topk(x, top_k, dim=-1).values[..., -1:]
        keep = x >= t_k
    if top_p < 1.0:
        wa = torch.where(keep, w, torch.zeros_like(w))
        xs, order = torch.sort(x, dim=-1, descending=True, stable=True)
        ws = torch.gather(wa, -1, order)
        csum = torch.cumsum(ws, -1)
        # M(t) at t = xs_i is the running sum at the END of the run of equal logits that xs_i belongs to
        end = torch.ones_like(xs, dtype=torch.bool)
        end[..., :-1] = xs[..., :-1] != xs[..., 1:]
        idx = torch.arange(V).expand(xs.shape)
        run_end = torch.flip(torch.cummin(torch.flip(torch.where(end, idx, torch.full_like(idx, V)), (-1,)), -1).values, (-1,))
        m = torch.gather(csum, -1, run_end)
        ok = (m >= top_p * csum[..., -1:]) & torch.gather(keep, -1, order)
        # the largest kept logit value whose M reaches the target: the first such entry in descending order
        first = torch.argmax(ok.to(torch.int8), -1, keepdim=True)
        t_p = torch.gather(xs, -1, first)
        keep = keep & (x >= t_p)
    wb = torch.where(keep, w, torch.zeros_like(w))
    return wb / wb.sum(-1, keepdim=True)


def truncated_draw_reference(probs, u):
    """probs (rows, V) truncated probabilities (or weights), u (rows,) in [0, 1) -> int64 codes: the count of cdf steps at or
    below u * total in memory order, and the last index of non-zero probability where rounding takes the count past it."""
    p = probs.detach().to("cpu", torch.float64)
    cdf = torch.cumsum(p, -1)
    thr = u.detach().to("cpu", torch.float64).unsqueeze(-1) * cdf[..., -1:]
    cnt = (cdf <= thr).sum(-1)
    V = p.shape[-1]
    last = (V - 1) - torch.argmax(torch.flip(p > 0, (-1,)).to(torch.int8), -1)
    return torch.minimum(cnt, last)
