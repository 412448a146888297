"""Vector quantisers with EMA codebooks (reference: vidgen/modeling/vq/vq_embedding.py:9-99, vq_utils.py:5-65).

`Quantiser` is the call contract every quantiser offers (`forward(z, "" | "st" | "emb")` over the channels-last methods) with the
answers of one that has no codebook state; FSQEmbedding (fsq_embedding.py) is built on it directly.  `CodebookQuantiser` adds
what a learned codebook needs -- the pass lifecycle `straight_through_cl` / `finish_ema` / `abandon_ema`, codebook restart, the
cosine lookup, the two autograd nodes -- once, for the product quantiser `DVQEmbedding` and the one wide codebook
`SingleVQEmbedding`, which state only their geometry: how a row is searched and how their state looks to the kernels.

State layout is the reference's (`ve.i.embedding.weight`, `ve.i.running_size`, `ve.i.running_sum`; `embedding.weight`, ... for
the single codebook) but the kernels see (G, K, d) tensors, so that all codebooks / all 64-d groups are quantised, gathered and
EMA-updated by single kernel launches.

Deliberate, documented deviations:
  * `running_sum` owns its storage.  The reference registers it as `weight.detach()`, which on CPU
    aliases the codebook; on a GPU `.to(device)` de-aliases.  GPU semantics are kept.
  * multi-GPU EMA statistics are summed with ONE all-reduce of a packed (num, K, D+1) buffer instead of
    2*num all_gather+sum round trips (vq_embedding.py:46-47, 53-54); the sum is the same.
  * that all-reduce is OFF the critical path: the decoder only needs z_q_st, which comes from the pre-update codebook, so
    `straight_through_cl(z, defer=True)` starts the collective asynchronously right after the statistics kernel and returns;
    `finish_ema()` joins it, applies the EMA update and gathers z_q_bar for the commitment loss -- after the decoder forward
    has been enqueued (meta_arch/vqvae.py).  Same arithmetic, same order of updates as the reference (vq_embedding.py:46-59).
  * `enable_restart` (MODEL.CODEBOOK.RESTART; the reference has nothing like it, off by default): dead codes are re-seeded from
    encoder rows of the pass inside the finalize launch, and a health record is kept.
  * `cosine` (MODEL.CODEBOOK.COSINE; the reference has nothing like it, off by default): the lookup runs on the unit sphere.  The
    caller hands the quantiser u = normalise_cl(z_e) instead of z_e, and the finalize step leaves unit rows in the codebook
    (the rule in plain torch: cosine.py).
"""
from collections import namedtuple

import torch
from torch import nn

from ...hip import binding as L
from ...hip import l2norm, vq
from ...layers.all_reduce import all_reduce_sum_async_
from ...utils import comm
from .. import convstack
from . import cosine as cosine_rule

SUPPORTED_GEOMETRY = ("sub-vector width DIM / NUM: a multiple of 16 from 16 to 256 (product quantiser, DVQEmbedding) or "
                      "DIM a multiple of 64 (one wide codebook, SingleVQEmbedding); codebook size SIZE: a multiple of 64 "
                      "from 64 to 2048")


def check_geometry(num, K, D, single=False):
    """Raise NotImplementedError unless (NUM, SIZE, DIM) is a geometry the HIP quantiser kernels support (csrc/vq.hip).
    single=True: SingleVQEmbedding, which searches the whole DIM-wide codebook and gathers / updates it as DIM / 64 groups of
    64 dims; otherwise the product quantiser, whose kernels see sub-vectors of DIM / NUM dims (also when NUM == 1)."""
    if num < 1 or D % num:
        raise NotImplementedError("CODEBOOK.DIM (%d) must be a multiple of CODEBOOK.NUM (%d); supported: %s"
                                  % (D, num, SUPPORTED_GEOMETRY))
    dg = D // num
    if single:
        ok_d = D % 64 == 0 and D > 0
    else:
        ok_d = dg % 16 == 0 and 16 <= dg <= 256
    if not ok_d:
        raise NotImplementedError("unsupported codebook geometry NUM=%d DIM=%d (sub-vector width %d); supported: %s"
                                  % (num, D, dg, SUPPORTED_GEOMETRY))
    if K % 64 or not 64 <= K <= 2048:
        raise NotImplementedError("unsupported codebook SIZE=%d; supported: %s" % (K, SUPPORTED_GEOMETRY))


class Quantiser(nn.Module):
    """What VQVAEModel calls on a quantiser.  A subclass provides `indices_cl`, `straight_through_cl(z_cl, defer)`,
    `finish_ema`, `abandon_ema`, `embed_cl` and `_flat()`; the attributes below are the answers of one without EMA state,
    cosine lookup or restart."""

    ema = cosine = restart_enabled = False

    def normalise_cl(self, z_cl):
        return z_cl

    def health_scalars(self):
        return None

    def forward(self, z_e_x, mode=""):
        """The reference's call contract (vq_embedding.py:23-33, 77-99) on (N, D, H, W) tensors: "" -> codes, "st" ->
        (z_q_st, z_q_bar), "emb": codes -> (N, H, W, D) as nn.Embedding yields."""
        if mode == "emb":
            return self.embed_cl(z_e_x).squeeze(1)
        if mode not in ("", "st"):
            raise ValueError
        assert z_e_x.dim() == 4
        z_cl = self.normalise_cl(convstack._LayoutIn.apply(z_e_x))
        if mode == "":
            return self.indices_cl(z_cl)
        st, bar = self.straight_through_cl(z_cl)
        out = convstack._LayoutOut.apply(st, self.D)
        return out, (out if bar is st else convstack._LayoutOut.apply(bar, self.D))


class VQEmbedding(nn.Module):
    """One codebook: parameter / buffer container (vq_embedding.py:9-21).  unit: the rows are l2-normalised once after the
    reference's init (MODEL.CODEBOOK.COSINE, cosine.py step 8)."""

    def __init__(self, K, D, ema, unit=False):
        super().__init__()
        self.embedding = nn.Embedding(K, D)
        self.embedding.weight.data.uniform_(-1.0 / K, 1.0 / K)
        if unit:
            cosine_rule.init_(self.embedding.weight.data)
        self.K, self.D, self.ema = K, D, ema
        if ema:
            self.register_buffer("running_size", torch.zeros(K))
            self.register_buffer("running_sum", self.embedding.weight.detach().clone())


class _NormaliseFn(torch.autograd.Function):
    """u = F.normalize of every `d`-wide group of channels-last rows (rows, G d), with the backward of torch autograd's
    F.normalize (cosine.py step 6): lvt_l2norm_groups_fwd / _bwd."""

    @staticmethod
    def forward(ctx, z2d, d):
        u, inv = l2norm.l2norm_groups_fwd(z2d, d)
        ctx.save_for_backward(u, inv)
        ctx.d = d
        return u

    @staticmethod
    def backward(ctx, g):
        u, inv = ctx.saved_tensors
        return l2norm.l2norm_groups_bwd(g.contiguous(), u, inv, ctx.d), None


class _StraightThroughFn(torch.autograd.Function):
    """vq_st as an autograd node (vq_utils.py:34-65): nearest code + gather from the PRE-update codebook; with EMA the
    assignment statistics are accumulated and their all-reduce is STARTED here (joined by finish_ema)."""

    @staticmethod
    def forward(ctx, z2d, owner, P, shape):
        codes = owner._codes()                           # (fetched once: DVQEmbedding._flat() checks every slice)
        idx = owner._search(z2d, P, codes)
        idx_k = owner._kernel_idx(idx, P)
        z_q_st = vq.gather(idx_k, codes)
        stats, work, cand = owner._accumulate(idx_k, z2d, P) if owner.ema else (None, None, None)
        owner._pending = _Pending(idx_k, stats, work, cand, shape)
        ctx.mark_non_differentiable(idx)
        return z_q_st, idx

    @staticmethod
    def backward(ctx, g_st, g_idx):
        return g_st, None, None, None                    # straight-through (vq_utils.py:52-54)


class _GatherWithGradFn(torch.autograd.Function):
    """rows of `codes` (G, K, d) selected by idx, differentiable w.r.t. the `weights` the codes are made of (CODEBOOK.EMA False:
    vq_embedding.py:61-64): the backward pass is `grad_codebook.index_add_(0, indices, grad_rows)` (vq_utils.py:56-63) -- here
    the per-code row sums of the EMA-statistics kernel (fixed summation order, no atomics) applied to the gradient rows.
    shared: ONE weight (K, G d) whose 64-d groups sit side by side; otherwise one weight (K, d) per group."""

    @staticmethod
    def forward(ctx, idx, codes, K, shared, *weights):
        ctx.save_for_backward(idx)
        ctx.K, ctx.shared = K, shared
        return vq.gather(idx, codes)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        sums = vq.ema_accumulate(idx, g.contiguous(), ctx.K)[:, :, :-1]            # (G, K, d + 1) is sums | counts
        if ctx.shared:
            return (None,) * 4 + (sums.permute(1, 0, 2).reshape(ctx.K, -1).contiguous(),)
        return (None,) * 4 + tuple(s.contiguous() for s in sums)


# A pass between straight_through_cl and finish_ema / abandon_ema: the kernel-shaped index (n, G, P), the statistics, the
# handle of their all-reduce, the restart candidates (the last three None where the pass has none) and the shape of z_cl.
_Pending = namedtuple("_Pending", "idx stats work cand shape")


class CodebookQuantiser(Quantiser):
    """A quantiser with K learned codes per codebook, for one wide codebook and for `num` narrow ones alike.  The kernels work
    on G groups of d channels with a (G, K, d) codebook; a subclass says what its groups are:
      shared_index        every group selects with the same code (the restart then draws ONE row for all groups of a code)
      _search(z2d, P, codes=None)   rows -> the code indices as the search kernel leaves them (codes: `_codes()`, if at hand)
      _latents(idx, n, h, w)   those -> the public latents;  _kernel_idx(latents, P) -> (n, G, P), what gather / EMA take
      _codes()            the (G, K, d) codebook;  _ema_state() -> (codes, running_size (G, K), running_sum (G, K, d))
      _store(w, rsize, rsum)   after the finalize launch rewrote those three: back to where the state lives
      _grad_weights()     the parameters a trained codebook's gradient goes to (_GatherWithGradFn)
      _unit_codes(w)      (G, K, d) the finalize launch wrote -> unit rows (cosine)
      _flat()             the tensors a data-parallel run broadcasts from rank 0 (meta_arch/vqvae.py wrap_parallel)

    Restart (MODEL.CODEBOOK.RESTART) is off until `enable_restart` is called; then, in train mode, every pass
    gathers one candidate row per code next to the EMA statistics (same collective) and the finalize launch re-seeds the codes
    that won no row and whose running_size fell below the threshold.  The pass counter, the health record and the cumulative
    restart counter are NON-persistent buffers: the state-dict keys stay the reference's, and a resumed run draws a different
    stream of rows.  Cosine (MODEL.CODEBOOK.COSINE): `normalise_cl` is the node z_e -> u that the caller applies
    before `indices_cl` / `straight_through_cl`, and `_unit_codes` what the finalize step ends with.  Neither adds a parameter,
    a persistent buffer or a state-dict key."""

    decay, eps = 0.99, 1e-5
    COSINE_MAX_WIDTH = 1024        # the widest group of lvt_l2norm_groups_fwd

    def __init__(self, *args, cosine=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.cosine = bool(cosine)
        self._pending = None
        self._restart = None           # (threshold, seed) once enabled

    # ---- restart ---------------------------------------------------------------------------------------------------------
    def enable_restart(self, threshold=1.0, seed=0):
        """threshold: a code is dead when its updated running_size is below it (0.0: monitoring only); seed: of the draw, the
        same on every rank."""
        threshold = float(threshold)
        if not self.ema:
            raise ValueError("codebook restart needs CODEBOOK.EMA: a trained codebook has no running_size")
        if not (0.0 <= threshold < float("inf")):
            raise ValueError("codebook restart: THRESHOLD must be finite and >= 0 (got %r)" % (threshold,))
        dev = self._flat()[0].device
        self.register_buffer("restart_pass", torch.zeros(1, dtype=torch.int64, device=dev), persistent=False)
        self.register_buffer("restart_health", torch.zeros(self.groups, 3, device=dev), persistent=False)
        self.register_buffer("restart_total", torch.zeros(self.groups, dtype=torch.int64, device=dev), persistent=False)
        self._restart = (threshold, max(int(seed), 0))

    @property
    def restart_enabled(self):
        return self._restart is not None

    def _accumulate(self, idx, z2d, P):
        """EMA statistics of a pass (+ the restart candidates behind them in ONE buffer, when enabled and in train mode) and
        the start of their all-reduce -> (stats, work, cand or None)."""
        if self._restart is None or not self.training:
            stats = vq.ema_accumulate(idx, z2d, self.K)
            return stats, all_reduce_sum_async_(stats), None
        num = idx.shape[1]
        flat, stats, cand = vq.restart_buffer(num, self.K, z2d.shape[1] // num, z2d.device)
        vq.ema_accumulate(idx, z2d, self.K, out=stats)
        vq.restart_candidates(z2d, cand, P, comm.get_rank(), comm.get_world_size(), self._restart[1], self.restart_pass,
                              shared_index=self.shared_index)
        return stats, all_reduce_sum_async_(flat), cand

    def _finalize(self, stats, cand, rsize, rsum, w):
        if cand is None:
            vq.ema_finalize(stats, rsize, rsum, w, self.decay, self.eps)
        else:
            vq.ema_finalize_restart(stats, cand, rsize, rsum, w, self._restart[0], self.restart_health, self.restart_total,
                                    self.restart_pass, self.decay, self.eps)
        if self.cosine:
            self._unit_codes(w)                           # (running_sum and running_size stay as the launch left them)

    def health_scalars(self):
        """(perplexity: mean over codebooks, dead: sum, restarts: cumulative sum) of the last finalized train pass as device
        scalars -- no host synchronisation; None unless restart is enabled."""
        if self._restart is None:
            return None
        n = self.num                                      # (the groups of a single codebook carry the same record: take one)
        h = self.restart_health[:n].double()
        return h[:, 0].mean(), h[:, 1].sum(), self.restart_total[:n].sum().double()

    # ---- cosine ----------------------------------------------------------------------------------------------------------
    def _check_cosine(self, ema, width):
        if not ema:
            raise ValueError("MODEL.CODEBOOK.COSINE needs MODEL.CODEBOOK.EMA: a trained cosine codebook would need a "
                             "differentiable normalisation of its weights")
        if width > self.COSINE_MAX_WIDTH:
            raise NotImplementedError("MODEL.CODEBOOK.COSINE: one codebook of DIM %d; the normalisation kernels take groups of "
                                      "at most %d" % (width, self.COSINE_MAX_WIDTH))

    def normalise_cl(self, z_cl):
        """(N,1,H,W,D) channels-last -> u of the same shape: every sub-vector (the whole row for the single codebook) divided
        by its l2 norm.  The identity, and no launch, when the lookup is off."""
        if not self.cosine:
            return z_cl
        L.require(z_cl)
        return _NormaliseFn.apply(z_cl.view(-1, z_cl.shape[-1]), self.D // self.num).view(z_cl.shape)

    # ---- channels-last fast paths (the interface VQVAEModel uses) ----------------------------------------------------------
    def indices_cl(self, z_cl):
        """(N,1,H,W,D) -> int64 latents: (N,num,H,W), or (N,H,W) for the single codebook."""
        n, _, h, w, d = z_cl.shape
        L.require(z_cl)
        return self._latents(self._search(z_cl.view(n * h * w, d), h * w), n, h, w)

    def straight_through_cl(self, z_cl, defer=False):
        """(N,1,H,W,D) -> (z_q_st, z_q_bar) channels-last; updates the EMA state (vq_embedding.py:35-66).
        defer=True returns z_q_st only and leaves the EMA update + z_q_bar to `finish_ema()`: the statistics all-reduce of a
        data-parallel run then overlaps whatever the caller enqueues in between (the decoder forward)."""
        n, _, h, w, d = z_cl.shape
        L.require(z_cl)
        if self._pending is not None:
            raise L.LvtError("%s: the EMA update of the previous pass was never finished (finish_ema)" % type(self).__name__)
        z_q_st, idx = _StraightThroughFn.apply(z_cl.view(n * h * w, d), self, h * w, (n, 1, h, w, d))
        self.last_indices = self._latents(idx, n, h, w)      # kept for evaluators / tests
        z_q_st = z_q_st.view(n, 1, h, w, d)
        return z_q_st if defer else (z_q_st, self.finish_ema())

    def finish_ema(self):
        """Join the statistics all-reduce, apply the EMA update (vq_embedding.py:48-59) and return z_q_bar, the codes of this
        pass gathered from the UPDATED codebook (channels-last)."""
        pend, self._pending = self._pending, None
        if pend is None:
            raise L.LvtError("%s.finish_ema without a pending straight_through_cl" % type(self).__name__)
        if self.ema:
            if pend.work is not None:
                pend.work.wait()
            w, rsize, rsum = self._ema_state()
            self._finalize(pend.stats, pend.cand, rsize, rsum, w)
            self._store(w, rsize, rsum)
            z_q_bar = vq.gather(pend.idx, w)
        else:
            # a trained codebook: z_q_bar carries the graph to the weight parameters (vq_embedding.py:61-64); their gradient
            # is the reference's index_add_ of the incoming rows (vq_utils.py:56-63)
            z_q_bar = _GatherWithGradFn.apply(pend.idx, self._codes(), self.K, self.shared_index, *self._grad_weights())
        return z_q_bar.view(pend.shape)

    def abandon_ema(self):
        """Error path of a deferred pass: wait for the statistics all-reduce that was started and forget the pending update
        (the codebook stays as it was before the pass)."""
        pend, self._pending = self._pending, None
        if pend is not None and pend.work is not None:
            pend.work.wait()

    def embed_cl(self, latents):
        """int64 latents as `indices_cl` yields them -> (N,1,H,W,D) channels-last."""
        L.require(latents)
        n, (h, w) = latents.shape[0], latents.shape[-2:]
        return vq.gather(self._kernel_idx(latents.contiguous(), h * w), self._codes()).view(n, 1, h, w, self.D)


class SingleVQEmbedding(CodebookQuantiser, VQEmbedding):
    """`VQEmbedding` used directly as the quantiser: CODEBOOK.NUM == 1, the default of the config tree (config/defaults.py:79,
    meta_arch/vqvae.py:25-27).  Same parameters, buffers and state_dict keys as the reference's class (`embedding.weight`,
    `running_size`, `running_sum`); latents carry no codebook axis: (N, H, W).

    The search runs as engine GEMM + lvt_vq_argmax_scores (hip/vq.py nearest_single).  Gather and the EMA statistics reuse the
    product quantiser's kernels, which work on 64-d groups: the (K, D) codebook is viewed as D / 64 groups that all select with
    the SAME index -- group g of code k is e_k[64 g : 64 g + 64] -- so the gathered rows, the per-code sums and the counts (equal
    in every group) are exactly those of the wide codebook, and lvt_vq_ema_finalize applies the reference's update
    (vq_embedding.py:48-59) to every group with the same counts."""

    shared_index = True

    def __init__(self, K, D, ema, cosine=False):
        check_geometry(1, K, D, single=True)
        if cosine:
            self._check_cosine(ema, D)
        super().__init__(K, D, ema, unit=cosine, cosine=cosine)
        self.num, self.groups = 1, D // 64

    # ---- 64-d group views ------------------------------------------------------------------------------------------------
    def _grouped(self, t):
        """(K, D) -> (g, K, 64) contiguous; (K,) -> (g, K)."""
        if t.dim() == 1:
            return t.unsqueeze(0).expand(self.groups, self.K).contiguous()
        out = t.view(self.K, self.groups, 64).permute(1, 0, 2).contiguous()
        if L.f16x2() and L._valid_amax(t) is not None:
            L.set_amax(out, L._valid_amax(t))
        return out

    def _ungrouped(self, t):
        return t.permute(1, 0, 2).reshape(self.K, self.D)

    def _search(self, z2d, P, codes=None):
        return vq.nearest_single(z2d, self.embedding.weight)                  # (rows,): the (K, D) rows, not their groups

    def _latents(self, idx, n, h, w):
        return idx.view(n, h, w)

    def _kernel_idx(self, latents, P):
        return latents.view(-1, 1, P).expand(-1, self.groups, P).contiguous()

    def _codes(self):
        return self._grouped(self.embedding.weight.detach())

    def _ema_state(self):
        return self._codes(), self._grouped(self.running_size), self._grouped(self.running_sum)

    def _store(self, wg, rsize, rsum):
        w = self.embedding.weight
        with torch.no_grad():
            w.data.copy_(self._ungrouped(wg))
            self.running_size.copy_(rsize[0])
            self.running_sum.copy_(self._ungrouped(rsum))
        L.drop_amax(w)

    def _grad_weights(self):
        return (self.embedding.weight,)

    def _unit_codes(self, wg):
        """Normalised as the (K, D) rows they are."""
        rows = self._ungrouped(wg).contiguous()
        l2norm.l2norm_groups_fwd(rows, self.D, inplace=True, want_inv=False)
        with torch.no_grad():
            wg.copy_(self._grouped(rows))

    def _flat(self):
        return (self.embedding.weight.data, getattr(self, "running_size", None), getattr(self, "running_sum", None))


class DVQEmbedding(CodebookQuantiser):
    """The product quantiser: `num` codebooks `ve.i` of D / num channels each, latents (N, num, H, W).  The kernel-shaped state
    IS the state: three flat device buffers whose slices are the per-codebook parameters / buffers."""

    shared_index = False

    def __init__(self, num, K, D, ema, cosine=False):
        check_geometry(num, K, D)
        if cosine:
            self._check_cosine(ema, D // num)
        super().__init__(cosine=cosine)
        self.num, self.groups, self.D, self.K, self.ema = num, num, D, K, ema
        self.ve = nn.ModuleList([VQEmbedding(K, D // num, ema, unit=cosine) for _ in range(num)])
        self._flat_w = self._flat_rs = self._flat_rsum = None

    def _flat(self):
        """(weights (num,K,d), running_size (num,K), running_sum (num,K,d)) whose slices ARE the
        per-codebook parameters / buffers.  Rebuilt whenever a `.to()` / load replaced the storage."""
        w0 = self.ve[0].embedding.weight
        fw = self._flat_w
        ok = fw is not None and fw.device == w0.device and all(
            self.ve[i].embedding.weight.data_ptr() == fw[i].data_ptr()
            and (not self.ema or (self.ve[i].running_size.data_ptr() == self._flat_rs[i].data_ptr()
                                  and self.ve[i].running_sum.data_ptr() == self._flat_rsum[i].data_ptr()))
            for i in range(self.num))
        if not ok:
            with torch.no_grad():
                fw = torch.stack([v.embedding.weight.data for v in self.ve]).contiguous()
                frs = frsum = None
                if self.ema:                 # (a trained codebook, CODEBOOK.EMA False, has no running buffers: vq_embedding.py:17-21)
                    frs = torch.stack([v.running_size for v in self.ve]).contiguous()
                    frsum = torch.stack([v.running_sum for v in self.ve]).contiguous()
                for i, v in enumerate(self.ve):
                    v.embedding.weight.data = fw[i]
                    if self.ema:
                        v.running_size = frs[i]
                        v.running_sum = frsum[i]
            self._flat_w, self._flat_rs, self._flat_rsum = fw, frs, frsum
        return self._flat_w, self._flat_rs, self._flat_rsum

    def _search(self, z2d, P, codes=None):
        return vq.nearest(z2d, self._codes() if codes is None else codes, P)   # (rows / P, num, P)

    def _latents(self, idx, n, h, w):
        return idx.view(n, self.num, h, w)

    def _kernel_idx(self, latents, P):
        return latents.view(-1, self.num, P)

    def _codes(self):
        return self._flat()[0]

    _ema_state = _flat

    def _store(self, w, rsize, rsum):
        pass

    def _grad_weights(self):
        return [v.embedding.weight for v in self.ve]

    def _unit_codes(self, w):
        """In place on the flat buffer, one launch (which records max |w| in f16x2 mode and, as every raw-pointer write,
        retires the records of the other views of the buffer)."""
        l2norm.l2norm_groups_fwd(w, self.D // self.num, inplace=True, want_inv=False)
