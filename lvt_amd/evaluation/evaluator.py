"""Evaluation callers of the hot path (reference: vidgen/evaluation/evaluator.py:14-166,
codes_extractor.py:36-53, mse_evaluation.py:28-47, bits_evaluation.py:28-58).  They only consume the
dicts `model(inputs)` returns in inference mode; statistics are accumulated on the device and reduced across
ranks with one all-reduce at the end (the reference gathers pickled python objects over gloo)."""
import json
import logging
import math
import os
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from ..data.latents import save_video_codes
from ..layers import all_reduce_sum_
from ..utils import comm
from .quality import frame_quality_reference, prediction_quality_reference


class DatasetEvaluator:
    def reset(self):
        pass

    def process(self, inputs, outputs):
        pass

    def evaluate(self):
        pass


class DatasetEvaluators(DatasetEvaluator):
    def __init__(self, evaluators):
        self._evaluators = list(evaluators)

    def reset(self):
        for e in self._evaluators:
            e.reset()

    def process(self, inputs, outputs):
        for e in self._evaluators:
            e.process(inputs, outputs)

    def evaluate(self):
        results = OrderedDict()
        for e in self._evaluators:
            r = e.evaluate()
            if comm.is_main_process() and r is not None:
                for k, v in r.items():
                    assert k not in results, "Different evaluators produce results with the same key {}".format(k)
                    results[k] = v
        return results


class CodesExtractor(DatasetEvaluator):
    """Writes `output['latent']` (T, nc, h, w) as one .npy per frame under
    <output_dir>/<dataset_name>/video_<idx>/<frame>.npy -- the training data format of the transformer."""

    def __init__(self, dataset_name, distributed=True, output_dir=None):
        self._root = os.path.join(output_dir, dataset_name)

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            latent = out["latent"]
            if latent.dim() == 3:
                latent = latent.unsqueeze(1)
            save_video_codes(self._root, int(inp["video_idx"]), latent.detach().cpu().numpy())

    def evaluate(self):
        comm.synchronize()
        return {}


class _SumEvaluator(DatasetEvaluator):
    def __init__(self, dataset_name, distributed=True, output_dir=None):
        self._logger = logging.getLogger(__name__)
        self._distributed = distributed
        self.reset()

    def reset(self):
        self._acc = None                      # [sum, count] on the device of the first output

    def _add(self, s, n):
        v = torch.stack([s.double().reshape(()), torch.tensor(float(n), dtype=torch.float64, device=s.device)])
        self._acc = v if self._acc is None else self._acc + v

    def _totals(self):
        if self._acc is None:                 # a rank that saw no sample still takes part in the all-reduce
            dist_on = self._distributed and torch.distributed.is_available() and torch.distributed.is_initialized()
            dev = "cuda" if (dist_on and torch.cuda.is_available() and torch.distributed.get_backend() == "nccl") else "cpu"
            self._acc = torch.zeros(2, dtype=torch.float64, device=dev)
        acc = self._acc.clone()
        if self._distributed:
            all_reduce_sum_(acc)
        return float(acc[0]), float(acc[1])


class MSEEvaluator(_SumEvaluator):
    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            rec = out["reconstruction"].detach()
            tgt = torch.as_tensor(inp["image"] if "image" in inp else inp["image_sequence"], device=rec.device)
            if rec.is_cuda:       # sum of squared differences on the device: lvt_mse_fwd (F.mse_loss(reduction="sum"))
                from ..hip import ew
                sq = ew.mse_fwd(rec.contiguous().float(), tgt.to(torch.float32).contiguous(), denom=1.0)
            else:
                sq = F.mse_loss(rec, tgt.to(rec.dtype), reduction="sum")
            self._add(sq, tgt.numel())

    def evaluate(self):
        s, n = self._totals()
        if not comm.is_main_process():
            return None
        results = OrderedDict({"reconstruction": {"MSE": s / n}})
        self._logger.info(results)
        return results


class FrameQualityEvaluator(DatasetEvaluator):
    """Mean per-frame PSNR and SSIM of `out["reconstruction"]` against the input frames, the unit reconstructions are compared
    in (definitions: evaluation/quality.py).  Device tensors go through `ew.frame_quality` (csrc/quality.hip) into one device
    accumulator [sum psnr, sum ssim, frames with a finite psnr, frames]; CPU tensors through `frame_quality_reference` into the
    same four sums.  A frame that is reproduced exactly (mse == 0) has no finite PSNR: it is left out of the PSNR mean and
    counted as `identical_frames`; its SSIM of 1 counts."""

    def __init__(self, dataset_name, distributed=True, output_dir=None, data_range=1.0):
        self._logger = logging.getLogger(__name__)
        self._distributed = distributed
        self._data_range = float(data_range)
        if not (self._data_range > 0 and math.isfinite(self._data_range)):
            raise ValueError("FrameQualityEvaluator: data_range must be positive and finite, got %r" % (data_range,))
        self.reset()

    def reset(self):
        self._acc = None                      # the four sums on the device of the first output

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            rec = out["reconstruction"].detach()
            tgt = torch.as_tensor(inp["image"] if "image" in inp else inp["image_sequence"], device=rec.device)
            if self._acc is None:
                self._acc = torch.zeros(4, dtype=torch.float64, device=rec.device)
            if rec.is_cuda:
                from ..hip import ew
                ew.frame_quality(rec.contiguous().float(), tgt.to(torch.float32).contiguous(), self._data_range, acc=self._acc)
            else:
                psnr, ssim = frame_quality_reference(rec, tgt, self._data_range)
                finite = psnr != float("inf")                    # (mse != 0, as the kernel counts)
                self._acc += torch.stack([psnr[finite].sum(), ssim.sum(), finite.sum().double(),
                                          torch.tensor(float(psnr.numel()), dtype=torch.float64)])

    def evaluate(self):
        if self._acc is None:                 # a rank that saw no sample still takes part in the all-reduce
            dist_on = self._distributed and torch.distributed.is_available() and torch.distributed.is_initialized()
            dev = "cuda" if (dist_on and torch.cuda.is_available() and torch.distributed.get_backend() == "nccl") else "cpu"
            self._acc = torch.zeros(4, dtype=torch.float64, device=dev)
        acc = self._acc.clone()
        if self._distributed:
            all_reduce_sum_(acc)
        if not comm.is_main_process():
            return None
        psnr_sum, ssim_sum, finite, n = (float(v) for v in acc.cpu())
        results = OrderedDict({"frame_quality": {"PSNR": psnr_sum / finite if finite > 0 else float("nan"),
                                                 "SSIM": ssim_sum / n if n > 0 else float("nan"),
                                                 "frames": int(n), "identical_frames": int(n - finite)}})
        self._logger.info(results)
        return results


class BitsEvaluator(_SumEvaluator):
    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            logits = out["logits"]                                   # nc, nv, T, H, W
            target = torch.as_tensor(inp["image_sequence"], device=logits.device).transpose(0, 1)   # nc, T, H, W
            keep = ~out["ignore_mask"].expand(target.size(0), -1, -1, -1)
            if logits.is_cuda:
                # lvt_xent_fwd on token-major rows (vidgen/evaluation/bits_evaluation.py:28-58 sums F.cross_entropy over the
                # kept positions): (nc, nv, P) -> (nc * P, nv) by lvt_permute3, ignored positions carry the ignore index
                from ..hip import tx
                nc, nv = logits.shape[:2]
                P = target[0].numel()
                rows = tx.permute3(logits.contiguous().float().view(nc, nv, P), (nv * P, 1, P), (nc, P, nv)).view(nc * P, nv)
                tgt = torch.where(keep, target, torch.full_like(target, -100)).reshape(1, nc * P).contiguous()
                # the SUM over the kept rows (bits_evaluation.py:36-40), from the per-row terms in fp64: `mean * count` would be
                # 0/0 = NaN for a sample whose positions are all ignored, and rounds the mean to fp32 first
                _, _, _, row_loss = tx.xent_fwd(rows, tgt[0], 0, 1, nc * P, -100, 1.0, want_rows=True)
                self._add(row_loss.double().sum(), int(keep.sum()))
            else:
                ce = F.cross_entropy(logits.permute(1, 0, 2, 3, 4).unsqueeze(0), target.unsqueeze(0), reduction="none")[0]
                self._add(ce[keep].sum(), int(keep.sum()))

    def evaluate(self):
        s, n = self._totals()
        if not comm.is_main_process():
            return None
        results = OrderedDict({"likelihood": {"bits_per_dim": (s / math.log(2)) / n}})
        self._logger.info(results)
        return results


def build_sampler_vqvae(cfg, vqvae=None):
    """The VQ-VAE named by cfg.TEST.VT_SAMPLER.VQ_VAE.* (or the one passed in), its weights loaded, frozen and in eval mode, as
    vt_sampler.py:18-58 builds it -> (vqvae, INPUT.SCALE_TO_ZEROONE of its config).  An empty weight path keeps the initialised
    weights, as fvcore's Checkpointer does."""
    from ..config import get_cfg
    from ..modeling import build_model
    from ..utils.checkpoint import Checkpointer
    vs = cfg.TEST.VT_SAMPLER.VQ_VAE
    vq_cfg = get_cfg()
    vq_cfg.merge_from_file(vs.CFG)
    vq_cfg.MODEL.DEVICE = cfg.MODEL.DEVICE
    vq_cfg.OUTPUT_DIR = cfg.OUTPUT_DIR
    vqvae = vqvae if vqvae is not None else build_model(vq_cfg)
    for module, path in ((vqvae.encoder, vs.ENCODER_WEIGHTS), (vqvae.generator, vs.GENERATOR_WEIGHTS),
                         (vqvae.codebook, vs.CODEBOOK_WEIGHTS)):
        if path:
            Checkpointer(module).resume_or_load(path, resume=False)
    vqvae.set_generator_requires_grad(False)
    vqvae.eval()
    return vqvae, vq_cfg.INPUT.SCALE_TO_ZEROONE


class VTSampler(DatasetEvaluator):
    """Decodes and saves the videos `VideoTransformerModel` sampled in inference mode (reference:
    vidgen/evaluation/vt_sampler.py:18-81): builds the VQ-VAE named by cfg.TEST.VT_SAMPLER.VQ_VAE.*, and for every input writes
    `<output_dir>/samples/<dataset>/video_<sample>_<video_idx>/{codes.npy, <frame>.png}`.  The decode runs on the HIP path
    (`vqvae.decode` -> gather + ResDecoder); an empty weight path keeps the initialised weights, as fvcore's Checkpointer does."""

    def __init__(self, cfg, dataset_name, distributed=True, output_dir=None, vqvae=None):
        self._logger = logging.getLogger(__name__)
        self._dataset_name, self._distributed, self._output_dir = dataset_name, distributed, output_dir
        self.vqvae, self.scale_to_zeroone = build_sampler_vqvae(cfg, vqvae)

    @torch.no_grad()
    def process(self, inputs, outputs):
        from PIL import Image
        for inp, out in zip(inputs, outputs):
            v_idx = inp["video_idx"]
            for sample_idx, sample in enumerate(out["samples"]):        # each (nc, T, h, w), or (1, T, h, w) -> (T, h, w)
                sample = sample.squeeze(0)
                if sample.dim() == 4:
                    sample = sample.transpose(0, 1).contiguous()         # (T, nc, h, w)
                code = sample.detach().cpu().numpy()
                frames = self.vqvae.back_normalizer(self.vqvae.decode(sample))           # (T, 3, H, W)
                if self.scale_to_zeroone:
                    frames = frames * 255
                frames = frames.clamp_(0.0, 255.0).permute(0, 2, 3, 1).contiguous().cpu().numpy().astype(np.uint8)
                video_dir = os.path.join(self._output_dir, "samples", self._dataset_name, "video_%d_%s" % (sample_idx, v_idx))
                os.makedirs(video_dir, exist_ok=True)
                np.save(os.path.join(video_dir, "codes.npy"), code)
                for frame_idx in range(len(frames)):
                    path = os.path.join(video_dir, "%d.png" % frame_idx)
                    for attempt in range(10):                            # (vt_sampler.py:74-81: shared file systems hiccup)
                        try:
                            Image.fromarray(frames[frame_idx]).save(path)
                            break
                        except OSError:
                            if attempt == 9:
                                raise
                            time.sleep(3)

    def evaluate(self):
        if self._distributed:
            comm.synchronize()
        return None


class PredictionQualityEvaluator(DatasetEvaluator):
    """Per-time-step PSNR and SSIM of the videos `VideoTransformerModel` sampled in inference mode, for the best of the
    NUM_SAMPLES sampled futures of a clip and for their mean (the SVG / SAVP / SV2P protocol; the rule and the eight columns:
    evaluation/quality.py prediction_quality_reference).  The target is the clip's own codes as the VQ-VAE renders
    them (`decode_pixels(inp["image_sequence"])`: the mapper feeds codes, not pixels), the samples `decode_pixels` of
    `out["samples"]`; the first TEST.VT_SAMPLER.N_PRIME frames are left out.  The best sample is chosen per metric by its mean
    over the predicted steps.  Device frames go through `ew.prediction_quality` (csrc/quality.hip) into one (T, 8) device
    accumulator, CPU frames through `prediction_quality_reference` into the same sums; nothing is read on the host before
    `evaluate`.  A best frame that equals its target (mse == 0) has no finite PSNR: it is left out of the PSNR means and counted
    as `identical_best_frames`.  The VQ-VAE is the one VTSampler builds (TEST.VT_SAMPLER.VQ_VAE.*)."""
    DECODE_FRAMES = 512                       # frames per decode_pixels call

    def __init__(self, cfg, dataset_name, distributed=True, output_dir=None, vqvae=None):
        self._logger = logging.getLogger(__name__)
        self._dataset_name, self._distributed, self._output_dir = dataset_name, distributed, output_dir
        self.vqvae, scale_to_zeroone = build_sampler_vqvae(cfg, vqvae)
        self._data_range = 1.0 if scale_to_zeroone else 255.0
        self._n_prime = int(cfg.TEST.VT_SAMPLER.N_PRIME)
        s = cfg.TEST.VT_SAMPLER             # how the samples were drawn: reported only when it is not the default
        self._sampling = {"temperature": float(s.TEMPERATURE), "top_k": int(s.TOP_K), "top_p": float(s.TOP_P)}
        self.reset()

    def reset(self):
        self._acc = None                      # (T, 8) sums on the device of the first decoded clip

    @staticmethod
    def _frames_of(codes, time_first):
        """Codes of one video as `decode_pixels` takes them: (T, nc, h, w), or (T, h, w) for a single codebook (as VTSampler)."""
        codes = torch.as_tensor(codes)
        if time_first:                        # the input clip: (T, nc, h, w)
            return codes.squeeze(1) if codes.dim() == 4 and codes.shape[1] == 1 else codes
        codes = codes.squeeze(0)              # a sample: (nc, T, h, w), or (1, T, h, w) -> (T, h, w)
        return codes.transpose(0, 1).contiguous() if codes.dim() == 4 else codes

    @torch.no_grad()
    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            target = self.vqvae.decode_pixels(self._frames_of(inp["image_sequence"], True))
            T = target.shape[0]
            codes = torch.cat([self._frames_of(s, False) for s in out["samples"]])
            S = codes.shape[0] // T
            if S < 1 or codes.shape[0] != S * T:
                raise ValueError("PredictionQualityEvaluator: %d sampled frames for a clip of %d" % (codes.shape[0], T))
            samples = torch.cat([self.vqvae.decode_pixels(codes[i:i + self.DECODE_FRAMES])
                                 for i in range(0, S * T, self.DECODE_FRAMES)]).view(S, *target.shape)
            if self._acc is None:
                self._acc = torch.zeros(T, 8, dtype=torch.float64, device=target.device)
            elif self._acc.shape[0] != T:
                raise ValueError("PredictionQualityEvaluator: a clip of %d frames after clips of %d" % (T, self._acc.shape[0]))
            if target.is_cuda:
                from ..hip import ew
                ew.prediction_quality(samples.float().contiguous(), target.float().contiguous(), self._n_prime, self._data_range,
                                      curves=self._acc)
            else:
                self._acc += prediction_quality_reference(samples, target, self._n_prime, self._data_range)[3]

    def _agree_on_steps(self):
        """T of this run.  A rank that saw no clip does not know it, and the all-reduce needs one shape everywhere: with more than
        one rank, two integers (max T, -min T over the ranks that saw a clip) are agreed on first."""
        T = -1 if self._acc is None else self._acc.shape[0]
        dist_on = self._distributed and torch.distributed.is_available() and torch.distributed.is_initialized()
        if not dist_on or comm.get_world_size() == 1:
            return max(T, 0), "cpu" if self._acc is None else self._acc.device
        dev = "cuda" if (torch.cuda.is_available() and torch.distributed.get_backend() == "nccl") else "cpu"
        span = torch.tensor([T, -T if T >= 0 else -(1 << 30)], dtype=torch.int64, device=dev)
        torch.distributed.all_reduce(span, op=torch.distributed.ReduceOp.MAX)
        hi, lo = int(span[0]), -int(span[1])
        if hi >= 0 and lo != hi:
            raise ValueError("PredictionQualityEvaluator: clips of %d and of %d frames on different ranks" % (lo, hi))
        return max(hi, 0), dev if self._acc is None else self._acc.device

    def evaluate(self):
        T, dev = self._agree_on_steps()
        if self._acc is None:                 # a rank that saw no clip still takes part in the all-reduce
            self._acc = torch.zeros(T, 8, dtype=torch.float64, device=dev)
        acc = self._acc.clone()
        if self._distributed:
            all_reduce_sum_(acc)
        if not comm.is_main_process():
            return None
        acc = acc.cpu()
        n0 = min(self._n_prime, T)
        rows = acc[n0:]

        def ratio(num, den):
            return float(num) / float(den) if float(den) > 0 else float("nan")

        steps = list(range(n0, T))
        per_frame = {"t": steps,
                     "PSNR_best": [ratio(r[0], r[1]) for r in rows], "SSIM_best": [ratio(r[2], r[6]) for r in rows],
                     "PSNR_mean": [ratio(r[3], r[4]) for r in rows], "SSIM_mean": [ratio(r[5], r[7]) for r in rows]}
        tot = rows.sum(dim=0) if len(steps) else torch.zeros(8, dtype=torch.float64)
        clips = int(rows[0, 6]) if len(steps) else 0
        res = {"PSNR_best": ratio(tot[0], tot[1]), "SSIM_best": ratio(tot[2], tot[6]),
               "PSNR_mean": ratio(tot[3], tot[4]), "SSIM_mean": ratio(tot[5], tot[7]), "per_frame": per_frame,
               "clips": clips, "samples": int(rows[0, 7]) if len(steps) else 0, "n_prime": self._n_prime,
               "identical_best_frames": int(tot[6] - tot[1]), "target": "decoded_codes"}
        if self._sampling != {"temperature": 1.0, "top_k": 0, "top_p": 1.0}:
            res["sampling"] = dict(self._sampling)
        results = OrderedDict({"prediction_quality": res})
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, "prediction_quality_%s.json" % self._dataset_name), "w") as f:
                json.dump(res, f, indent=1)
        self._logger.info(results)
        return results


def build_evaluator(cfg, dataset_name, output_folder=None):
    """Substring dispatch on cfg.TEST.EVALUATORS like tools/train_net.py:35-57 of the reference."""
    if output_folder is None:
        output_folder = os.path.join(cfg.OUTPUT_DIR, "inference")
    evs = []
    if "CodesExtractor" in cfg.TEST.EVALUATORS:
        evs.append(CodesExtractor(dataset_name, True, output_folder))
    if "MSEEvaluator" in cfg.TEST.EVALUATORS:
        evs.append(MSEEvaluator(dataset_name, True, output_folder))
    if "FrameQualityEvaluator" in cfg.TEST.EVALUATORS:    # the range AutoEncoderModel's inference clamps its reconstructions to
        evs.append(FrameQualityEvaluator(dataset_name, True, output_folder,
                                         data_range=1.0 if cfg.INPUT.SCALE_TO_ZEROONE else 255.0))
    if "BitsEvaluator" in cfg.TEST.EVALUATORS:
        evs.append(BitsEvaluator(dataset_name, True, output_folder))
    if "VTSampler" in cfg.TEST.EVALUATORS:
        evs.append(VTSampler(cfg, dataset_name, True, output_folder))
    if "PredictionQualityEvaluator" in cfg.TEST.EVALUATORS:
        evs.append(PredictionQualityEvaluator(cfg, dataset_name, True, output_folder))
    if not evs:
        raise NotImplementedError(cfg.TEST.EVALUATORS)
    return evs[0] if len(evs) == 1 else DatasetEvaluators(evs)


def inference_on_dataset(model, data_loader, evaluator):
    """Run `model(inputs)` in eval mode / no_grad over an iterable of batches and evaluate."""
    logger = logging.getLogger(__name__)
    evaluator = evaluator or DatasetEvaluators([])
    evaluator.reset()
    was_training = model.training
    model.eval()
    n, t0 = 0, time.perf_counter()
    with torch.no_grad():
        for inputs in data_loader:
            outputs = model(inputs)
            evaluator.process(inputs, outputs)
            n += len(inputs)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    model.train(was_training)
    logger.info("Total inference time: %.3f s (%.6f s / sample per device, on %d devices)",
                time.perf_counter() - t0, (time.perf_counter() - t0) / max(n, 1), comm.get_world_size())
    results = evaluator.evaluate()
    return {} if results is None else results
