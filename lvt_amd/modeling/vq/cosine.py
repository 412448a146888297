"""The cosine (l2-normalised) codebook lookup, MODEL.CODEBOOK.COSINE, stated once in plain torch.

This module is the rule of record: the kernels of csrc/l2norm.hip and the quantisers of vq_embedding.py follow it, and the tests
hold them to it in float64.  Nothing here runs on the training path; every function works in whatever dtype it is handed.

For a row z (one latent position) and codebook i, with z_i the row's d-wide sub-vector (d = DIM / NUM; the whole row for the
single wide codebook):

  1. u_i = F.normalize(z_i, dim=-1, eps=1e-12) = z_i / max(||z_i||_2, 1e-12)                                       `normalise`
  2. idx_i = argmin_k ||u_i - e_k||^2 over the current codebook, ties to the lowest k                              `nearest`
     (the rows e_k are unit vectors by the invariant of step 4)
  3. z_q_st = u + sg(e[idx] - u), from the PRE-update codebook
  4. EMA: running_size and running_sum follow the reference's rule (vq_embedding.py:46-59) on the rows u, the restart rule
     applies unchanged where it is enabled (its candidates are rows of u), and the stored code is then
     weight = F.normalize(weight_raw, dim=-1, eps=1e-12); running_sum and running_size are NOT normalised          `ema_update`
  5. z_q_bar = weight[idx] from the POST-update codebook, loss_commitment = BETA * mse(u, sg(z_q_bar))             `step`
  6. the node z -> u has the backward of torch autograd's F.normalize: with r = 1 / max(||z||, eps),
     dz = r (g - u (u . g)) where ||z|| > eps and dz = r g where the norm was clamped                               `normalise_backward`
  7. encode / inference normalise before the search; embedding (decode) reads the codebook, which already holds unit rows
  8. at construction the rows of every codebook are normalised once after the reference's uniform init and running_sum starts
     as that normalised clone                                                                                       `init_`
"""
import torch
import torch.nn.functional as F

EPS = 1e-12                 # F.normalize's default
DECAY, EMA_EPS = 0.99, 1e-5  # the reference's EMA constants (vq_embedding.py:14)


def normalise(z, d, eps=EPS):
    """(..., G * d) -> the same shape, every d-wide group of the last dimension l2-normalised (step 1)."""
    return F.normalize(z.unflatten(-1, (-1, d)), dim=-1, eps=eps).flatten(-2)


def inverse_norm(z, d, eps=EPS):
    """(..., G * d) -> (..., G): r = 1 / max(||z_i||, eps)."""
    return 1.0 / z.unflatten(-1, (-1, d)).norm(dim=-1).clamp_min(eps)


def normalise_backward(g, z, d, eps=EPS):
    """The gradient at z of u = normalise(z, d) from the gradient g at u, in closed form (step 6)."""
    zg, gg = z.unflatten(-1, (-1, d)), g.unflatten(-1, (-1, d))
    norm = zg.norm(dim=-1, keepdim=True)
    r = 1.0 / norm.clamp_min(eps)
    u = zg * r
    free = r * (gg - u * (u * gg).sum(-1, keepdim=True))
    return torch.where(norm > eps, free, r * gg).flatten(-2)


def nearest(u, e):
    """u (rows, d), e (K, d) -> int64 (rows,): argmin_k ||u - e_k||^2 with the |e|^2 term kept, ties to the lowest k (step 2)."""
    dist = (e ** 2).sum(1)[None, :] + (u ** 2).sum(1, keepdim=True) - 2.0 * u @ e.t()
    return torch.min(dist, dim=1).indices


def ema_update(weight, running_size, running_sum, u, idx, decay=DECAY, eps=EMA_EPS):
    """One codebook: weight (K, d), running_size (K,), running_sum (K, d), the rows u (rows, d) and their codes idx (rows,) ->
    (weight, running_size, running_sum) after the pass (step 4 without restart): the reference's update, then unit rows."""
    K = weight.shape[0]
    size = torch.zeros(K, dtype=u.dtype).index_add_(0, idx, torch.ones(idx.shape[0], dtype=u.dtype))
    total = torch.zeros_like(weight).index_add_(0, idx, u)
    running_size = running_size * decay + (1 - decay) * size
    running_sum = running_sum * decay + (1 - decay) * total
    n = running_size.sum()
    size_ = (running_size + eps) / (n + K * eps) * n
    raw = running_sum / size_.unsqueeze(1)
    return F.normalize(raw, dim=-1, eps=EPS), running_size, running_sum


class _StraightThrough(torch.autograd.Function):
    """u + sg(e[idx] - u) without the rounding of the two additions: the value is e[idx] bit for bit, the gradient goes to u."""

    @staticmethod
    def forward(ctx, u, codes):
        return codes.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def step(weight, running_size, running_sum, z, beta=1.0, force_idx=None):
    """One training pass of the quantiser on rows z (rows, num * d) from the state weight (num, K, d), running_size (num, K),
    running_sum (num, K, d) -> dict(u, idx (rows, num), z_q_st, z_q_bar, weight, running_size, running_sum, loss_commitment).
    z_q_st carries the straight-through graph to z when z requires grad.  force_idx (rows, num): continue with these codes
    (isolates near-ties of the search from the rest)."""
    num, K, d = weight.shape
    u = normalise(z, d)
    ug = u.detach().unflatten(-1, (num, d))
    idx, new = [], []
    for i in range(num):
        k = nearest(ug[:, i], weight[i]) if force_idx is None else force_idx[:, i]
        idx.append(k)
        new.append(ema_update(weight[i], running_size[i], running_sum[i], ug[:, i], k))
    idx = torch.stack(idx, 1)
    w_new, rs_new, rsum_new = (torch.stack([n[j] for n in new]) for j in range(3))
    pre = torch.cat([weight[i][idx[:, i]] for i in range(num)], -1)
    z_q_bar = torch.cat([w_new[i][idx[:, i]] for i in range(num)], -1)
    return {"u": u, "idx": idx, "z_q_st": _StraightThrough.apply(u, pre),"z_q_bar": z_q_bar, "weight": w_new, "running_size": rs_new,
            "running_sum": rsum_new, "loss_commitment": beta * F.mse_loss(u, z_q_bar.detach())}


def init_(weight):
    """Step 8, in place: the rows of a freshly initialised codebook (K, d) become unit vectors."""
    with torch.no_grad():
        weight.copy_(F.normalize(weight, dim=-1, eps=EPS))
    return weight
