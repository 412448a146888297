"""VQ-VAE meta-architecture (reference: vidgen/modeling/meta_arch/vqvae.py:17-124).

supervised step:  x -> ResEncoder -> z_e -> DVQ "st" (indices, z_q_st from the pre-update codebook,
EMA update, z_q_bar from the post-update codebook) -> ResDecoder -> x_tilde;
losses: lambda * mse(x_tilde, x)  and  beta * mse(z_e, sg(z_q_bar)).
With MODEL.CODEBOOK.COSINE the quantiser and the commitment loss see u = z_e with every sub-vector l2-normalised instead of z_e
(lvt_amd/modeling/vq/cosine.py).
With MODEL.CODEBOOK.FSQ.LEVELS the quantiser is FSQEmbedding: two trained projections around a fixed rounding rule, no codebook
state and no quantiser loss terms (lvt_amd/modeling/vq/fsq.py).
"""
import math
import os

from ...hip import ew
from ...solver import build_lr_scheduler, build_optimizer
from ...utils.checkpoint import Checkpointer
from ..loss import ReconstructionLoss
from ..loss.loss import mse
from ..vq import DVQEmbedding, FSQEmbedding, SingleVQEmbedding
from ..vq import fsq as fsq_rule
from .ae import AutoEncoderModel
from .build import META_ARCH_REGISTRY


@META_ARCH_REGISTRY.register()
class VQVAEModel(AutoEncoderModel):
    def __init__(self, cfg):
        super().__init__(cfg)
        cb = cfg.MODEL.CODEBOOK
        self.use_codebook_ema = cb.EMA
        self.fsq = bool(len(cb.FSQ.LEVELS))
        # (COSINE with EMA False is the quantisers' ValueError: a trained cosine codebook is not built)
        if self.fsq:
            self.codebook = self._build_fsq(cfg)
        elif cb.NUM == 1:          # the default of the config tree: `VQEmbedding` used directly (vqvae.py:25-27)
            self.codebook = SingleVQEmbedding(cb.SIZE, cb.DIM, self.use_codebook_ema, cosine=cb.COSINE)
        else:
            self.codebook = DVQEmbedding(cb.NUM, cb.SIZE, cb.DIM, self.use_codebook_ema, cosine=cb.COSINE)
        if self.use_codebook_ema:
            self._set_requires_grad(self.codebook.parameters(), False)
        if cb.RESTART.ENABLED:
            # (the un-offset config seed: every rank must draw the same rows)
            self.codebook.enable_restart(cb.RESTART.THRESHOLD, max(cfg.SEED, 0))
        self.reconstruction_loss = ReconstructionLoss(cfg)      # PixelLoss's choice (+ LOSS.SSIM.LAMBDA * (1 - SSIM))
        self.pixel_loss = self.reconstruction_loss.pixel_loss
        self.beta = cb.BETA
        self.to(self.device)

    def _build_fsq(self, cfg):
        """FSQEmbedding from MODEL.CODEBOOK.FSQ.LEVELS, or the ValueError that names the keys at odds with it."""
        cb = cfg.MODEL.CODEBOOK
        levels = fsq_rule.check_levels(cb.FSQ.LEVELS)
        if cb.SIZE != math.prod(levels):
            raise ValueError("MODEL.CODEBOOK.SIZE (%r) must equal prod(MODEL.CODEBOOK.FSQ.LEVELS) = %d"
                             % (cb.SIZE, math.prod(levels)))
        if cb.EMA:
            raise ValueError("MODEL.CODEBOOK.FSQ.LEVELS trains its two projections by gradient and keeps no EMA state: set "
                             "MODEL.CODEBOOK.EMA to False (Base-VQVAE.yaml sets it to True)")
        if cb.COSINE:
            raise ValueError("MODEL.CODEBOOK.FSQ.LEVELS has no learned codebook to search on the unit sphere: set "
                             "MODEL.CODEBOOK.COSINE to False")
        if cb.RESTART.ENABLED:
            raise ValueError("MODEL.CODEBOOK.FSQ.LEVELS has no codes that can die: set MODEL.CODEBOOK.RESTART.ENABLED to False")
        codebook = FSQEmbedding(cb.NUM, levels, cb.DIM)
        self.init_weights(codebook, cfg.MODEL.INIT_TYPE)
        return codebook

    def train(self, mode=True):
        super().train(mode)
        self.codebook.train(mode)
        return self

    def wrap_parallel(self, device_ids, broadcast_buffers):
        """Encoder / generator gradients are averaged by the bucketed reducer (see AutoEncoderModel).  The
        EMA codebook takes no gradient; its statistics are summed across ranks inside the quantiser.  The
        reference neither wraps nor synchronises the codebook, so with per-rank seeds (SEED + rank) the
        replicas start from different codebooks and only converge geometrically; here rank 0's codebook
        and EMA buffers are broadcast once so that all replicas stay bit-identical (documented deviation,
        single-GPU behaviour unaffected)."""
        import torch
        import torch.distributed as dist
        from ...utils import comm
        super().wrap_parallel(device_ids, broadcast_buffers)
        if not self.use_codebook_ema:
            # a trained codebook is a DDP module of its own in the reference (vqvae.py:46-49): its gradients are averaged too
            from ...engine.grad_reducer import BucketedGradReducer
            self._reducers.append(BucketedGradReducer(self.codebook.parameters()))
        if comm.get_world_size() > 1:
            with torch.no_grad():
                for t in self.codebook._flat():
                    if t is not None:
                        dist.broadcast(t, 0)

    def codebook_health(self):
        """Device scalars (codebook_perplexity, codebook_dead, codebook_restarts) of the last train pass, or None when
        MODEL.CODEBOOK.RESTART is off (engine/trainer.py logs them)."""
        return self.codebook.health_scalars()

    def _generator_parameters(self):
        params = super()._generator_parameters()
        if not self.use_codebook_ema:
            params += list(self.codebook.parameters())
        return params

    def forward(self, data, mode="inference"):
        return super().forward(data, mode)

    # ---- channels-last internals --------------------------------------------------------------------
    def _latent_cl(self, x):
        z_e = self.encoder.forward_cl(x)
        return self.codebook.indices_cl(self.codebook.normalise_cl(z_e))     # (N,num,h,w) int64

    def _latent_public(self, latent):
        return latent

    def _decode_cl(self, latent):
        return self.generator.forward_cl(self.codebook.embed_cl(latent))

    def _supervised_loss_cl(self, x, return_x=False):
        # (COSINE: u, the l2-normalised sub-vectors, takes the place of z_e from here on; the identity when the key is off)
        z_e = self.codebook.normalise_cl(self.encoder.forward_cl(x))
        # the decoder needs z_q_st only (pre-update codebook): the all-reduce of the EMA statistics that the quantiser
        # started runs beside the decoder forward and is joined afterwards (reference order of updates: vq_embedding.py:46-59)
        z_q_st = self.codebook.straight_through_cl(z_e, defer=True)
        try:
            x_tilde = self.generator.forward_cl(z_q_st)
        except BaseException:
            self.codebook.abandon_ema()     # (a failed decoder pass must not leave the quantiser unusable: join + drop the update)
            raise
        z_q_bar = self.codebook.finish_ema()
        c = len(self.cfg.MODEL.PIXEL_MEAN)
        loss = self.reconstruction_loss(x_tilde, x, denom=x.numel() // x.shape[-1] * c)
        if z_q_bar is not None:
            # (FSQ has none: it is a function of z_e and its two projections, and the reconstruction loss trains all of it)
            loss["loss_commitment"] = mse(z_e, z_q_bar.detach(), scale=self.beta)
            if not self.use_codebook_ema:
                # vector-quantisation objective of a TRAINED codebook, under the reference's key (vqvae.py:83-84)
                loss["loss_dict"] = mse(z_q_bar, z_e.detach())
        return (loss, x, x_tilde) if return_x else loss

    def _generator_loss_cl(self, x):
        return self._supervised_loss_cl(x)

    # ---- reference tensor-level API (vqvae.py:61-106) ----------------------------------------------
    def compute_supervised_loss(self, x, return_x=False):
        return self._supervised_loss_cl(self._as_cl(x), return_x)

    def decode(self, latents):
        """(N,num,h,w) int64 codes -> (N,C,H,W) in normalised space."""
        from .. import convstack
        self._require_gpu()
        y = self._decode_cl(latents.to(self.device))
        return convstack.cl_to_nchw(y, self.generator.out_channels)

    def decode_pixels(self, latents):
        """(N,num,h,w) int64 codes -> (N,C,H,W) fp32 pixels in [0, hi], hi = 1 with INPUT.SCALE_TO_ZEROONE and 255 without: the
        decoder's output de-normalised and clamped by the one kernel the `inference` mode ends with."""
        self._require_gpu()
        y = self._decode_cl(latents.to(self.device))
        n, _, h, w, cp = y.shape
        hi = 1.0 if self.cfg.INPUT.SCALE_TO_ZEROONE else 255.0
        return ew.to_channels_first(y.view(n, h * w, cp), self.generator.out_channels, 2, self._pixel_mean, self._pixel_std,
                                    0.0, hi).view(n, -1, h, w)

    def configure_optimizers_and_checkpointers(self):
        o, c = super().configure_optimizers_and_checkpointers()
        if not self.use_codebook_ema:
            opt = build_optimizer(self.codebook, self.cfg, suffix="_G")
            o.append({"optimizer": opt, "scheduler": build_lr_scheduler(self.cfg, opt), "type": "generator"})
        os.makedirs(os.path.join(self.cfg.OUTPUT_DIR, "netC"), exist_ok=True)
        c.append({"checkpointer": Checkpointer(self.codebook, os.path.join(self.cfg.OUTPUT_DIR, "netC")),
                  "pretrained": self.cfg.MODEL.CODEBOOK.WEIGHTS})
        return o, c
