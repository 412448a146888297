"""Finite scalar quantiser (MODEL.CODEBOOK.FSQ.LEVELS; the reference has nothing like it, off by default).

The encoder rows are projected to NUM groups of d = len(LEVELS) entries, each entry is squashed and rounded to L_i levels and
the code of a group is the mixed-radix number of its digits; a second projection takes the rounded values back to DIM channels
for the decoder.  The codebook is implicit: no search, no EMA, no restart, no commitment loss, no cross-rank statistics.  The
rule in plain torch: fsq.py.  The two projections run on the GEMM engine as the transformer's linear layers do, the three
streaming kernels are csrc/fsq.hip; the projected width travels rounded up to a multiple of 4 (zero weight rows / columns)."""
import math

import torch
from torch import nn

from ...hip import binding as L
from ...hip import fsq as K
from ...hip import gemm as G
from . import fsq as rule
from .vq_embedding import Quantiser


def _rows4(t, rows):
    """`t` (rows, n) with zero rows appended up to a multiple of 4 (a copy), or `t` itself when rows already is one."""
    pad = -rows % 4
    if not pad:
        return t
    out = torch.zeros(rows + pad, t.shape[1], dtype=t.dtype, device=t.device)
    out[:rows].copy_(t)
    return out


def _wgrad(dy, x, n_out, k_in, rows):
    """(dW, db) of a linear layer on the engine, as the transformer's layers form them.  The reduction runs over the rows and
    the engine wants it a multiple of 4: a row count that is not (never the model's N * h * w of whole latent grids) is
    padded with zero rows, which add nothing to either sum."""
    from ..autoregressive.vt_attention import linear_wgrad
    return linear_wgrad(_rows4(dy, rows), _rows4(x, rows), n_out, k_in, rows + (-rows % 4), want_bias=True)


class _FSQFn(torch.autograd.Function):
    """rows z_e (rows, D) -> (z_out (rows, D), idx (rows / P, num, P)): fsq.py steps 1 to 5 in one node, step 6 as its backward.
    Saved: z_e and z_q (the inputs of the two linear layers, as any linear saves its input) and z_p, from which the backward
    kernel recomputes tanh."""

    @staticmethod
    def forward(ctx, z2d, w_in, b_in, w_out, b_out, owner, P):
        rows, D = z2d.shape
        wi, bi, wo = owner._operands(w_in, b_in, w_out)
        z_p = owner._project_in(z2d, wi, bi)
        z_q, idx = K.fsq_fwd(z_p, owner.num, owner.levels, P)
        out = owner._project_out(z_q, wo, b_out.detach())
        ctx.save_for_backward(z2d, z_p, z_q, wi, wo)
        ctx.owner = owner
        ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, g, g_idx):
        z2d, z_p, z_q, wi, wo = ctx.saved_tensors
        o = ctx.owner
        rows, D = z2d.shape
        wp, nd = o.width, o.num * o.d
        g = g.contiguous()
        dz_q = torch.empty(rows, wp, dtype=torch.float32, device=g.device)
        G.gemm(g, wo, dz_q, rows, wp, D, ta=0, tb=1, ldb=wp)                    # g W_out (pad columns of W_out are 0)
        dwo, dbo = _wgrad(g, z_q, D, wp, rows)
        dz_p = K.fsq_bwd(dz_q, z_p, o.num, o.levels)
        dwi, dbi = _wgrad(dz_p, z2d, wp, D, rows)
        dz = torch.empty(rows, D, dtype=torch.float32, device=g.device)
        G.gemm(dz_p, wi, dz, rows, D, wp, ta=0, tb=1, ldb=D)                    # dz_p W_in
        if wp != nd:
            dwo, dwi, dbi = dwo[:, :nd].contiguous(), dwi[:nd].contiguous(), dbi[:nd].contiguous()
        return dz, dwi, dbi, dwo, dbo, None, None


class FSQEmbedding(Quantiser):
    """FSQEmbedding(num, levels, dim): `num` code channels of prod(levels) codes each over `dim` encoder / decoder channels.
    Parameters proj_in (dim -> num * d) and proj_out (num * d -> dim); no buffers.  A `Quantiser` (vq_embedding.py) with nothing
    to normalise, update or restart; train and eval mode are the same function."""

    def __init__(self, num, levels, dim):
        super().__init__()
        self.levels = rule.check_levels(levels)
        if num < 1:
            raise ValueError("MODEL.CODEBOOK.NUM must be at least 1 (got %r)" % (num,))
        if dim < 4 or dim % 4:
            raise NotImplementedError("MODEL.CODEBOOK.FSQ.LEVELS: MODEL.CODEBOOK.DIM (%r) must be a positive multiple of 4" % (dim,))
        self.num, self.d, self.D, self.K = num, len(self.levels), dim, math.prod(self.levels)
        self.width = K.padded_width(num, self.levels)
        self.proj_in = nn.Linear(dim, num * self.d)
        self.proj_out = nn.Linear(num * self.d, dim)

    # ---- engine operands -------------------------------------------------------------------------------------------------
    def _operands(self, wi=None, bi=None, wo=None):
        """(W_in (width, D), b_in (width,), W_out (D, width)) as the launches read them: the parameters themselves (the
        objects that carry the max |.| records of the pass) when num * d is a multiple of 4, else copies with zero rows /
        columns up to it."""
        if wi is None:
            wi, bi, wo = self.proj_in.weight, self.proj_in.bias, self.proj_out.weight
        nd, wp = self.num * self.d, self.width
        if nd == wp:
            return wi, bi, wo
        wi_p = torch.zeros(wp, self.D, dtype=torch.float32, device=wi.device)
        bi_p = torch.zeros(wp, dtype=torch.float32, device=wi.device)
        wo_p = torch.zeros(self.D, wp, dtype=torch.float32, device=wi.device)
        with torch.no_grad():
            wi_p[:nd].copy_(wi)
            bi_p[:nd].copy_(bi)
            wo_p[:, :nd].copy_(wo)
        return wi_p, bi_p, wo_p

    def _project_in(self, z2d, wi, bi):
        z_p = torch.empty(z2d.shape[0], self.width, dtype=torch.float32, device=z2d.device)
        return G.gemm(z2d, wi, z_p, z2d.shape[0], self.width, self.D, flags=L.EPI_BIAS, bias=bi)

    def _project_out(self, z_q, wo, bo):
        out = torch.empty(z_q.shape[0], self.D, dtype=torch.float32, device=z_q.device)
        return G.gemm(z_q, wo, out, z_q.shape[0], self.D, self.width, flags=L.EPI_BIAS, bias=bo)

    def _flat(self):
        """The tensors a data-parallel run broadcasts from rank 0 (meta_arch/vqvae.py wrap_parallel)."""
        return (self.proj_in.weight.data, self.proj_in.bias.data, self.proj_out.weight.data, self.proj_out.bias.data)

    # ---- channels-last fast paths (the interface VQVAEModel uses: see CodebookQuantiser) ----------------------------------
    def _rows(self, z_cl):
        n, _, h, w, d = z_cl.shape
        L.require(z_cl)
        if d != self.D:
            raise L.LvtError("FSQEmbedding: rows of %d channels, MODEL.CODEBOOK.DIM is %d" % (d, self.D))
        return n, h, w, z_cl.view(n * h * w, d)

    def indices_cl(self, z_cl):
        """(N,1,H,W,D) -> (N,num,H,W) int64."""
        n, h, w, z2d = self._rows(z_cl)
        wi, bi, _ = self._operands()
        _, idx = K.fsq_fwd(self._project_in(z2d.detach(), wi, bi), self.num, self.levels, h * w, want_zq=False)
        return idx.view(n, self.num, h, w)

    def straight_through_cl(self, z_cl, defer=False):
        """(N,1,H,W,D) -> z_out channels-last, what the decoder receives, with the straight-through graph to z_cl and the two
        projections.  defer=False returns the pair (z_out, z_out), the shape of the other quantisers' (z_q_st, z_q_bar);
        after defer=True there is nothing to finish: no z_q_bar, hence no quantiser loss terms."""
        n, h, w, z2d = self._rows(z_cl)
        out, idx = _FSQFn.apply(z2d, self.proj_in.weight, self.proj_in.bias, self.proj_out.weight, self.proj_out.bias, self, h * w)
        self.last_indices = idx.view(n, self.num, h, w)      # kept for evaluators / tests
        out = out.view(n, 1, h, w, self.D)
        return out if defer else (out, out)

    def finish_ema(self):
        return None

    def abandon_ema(self):
        pass

    def embed_cl(self, latents):
        """(N,num,H,W) int64 -> (N,1,H,W,D) channels-last."""
        n, num, h, w = latents.shape
        L.require(latents)
        if num != self.num:
            raise L.LvtError("FSQEmbedding: %d code channels, MODEL.CODEBOOK.NUM is %d" % (num, self.num))
        z_q = K.fsq_decode(latents.contiguous().view(n, num, h * w), self.levels, self.width)
        _, _, wo = self._operands()
        return self._project_out(z_q, wo, self.proj_out.bias.detach()).view(n, 1, h, w, self.D)
