#!/usr/bin/env python
"""Generate G26 (g26_batchnorm.npz): the reference's PR-DVQVAE2 with MODEL.ENCODER.NORM and MODEL.GENERATOR.NORM set to
"BN" and to "FrozenBN", over 4 frames.  Same route as make_golden.py (the reference imported through oracle/shim, seeded
weights from seeded.py, CPU, plain arrays out), whose helpers it reuses.

Per norm it records the state-dict key list, shapes and per-tensor checksums of `build_model(cfg)` at the config seed;
then, with seeded conv weights and non-trivial gamma / beta / running statistics: the train-mode `supervised` losses and
gradients of one step, the running statistics and num_batches_tracked after it, and in eval mode after that step the
`encode` latents, the `inference` reconstructions and one `supervised` forward + backward (running statistics with
gradients).

SyncBN is not captured: the reference's NaiveSyncBatchNorm reads its world size from vidgen.utils.comm and calls
torch.distributed collectives, which would need a two-process gloo group around the reference here.  The GPU test
tests/test_gpu_norm_dp.py checks its semantics against one process running BN on the concatenated batch instead.

    python tests/golden/make_golden_norm.py
"""
import os
import random
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (sets up the reference / shim import path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import seeded  # noqa: E402

SEED = 2626
PIN_SEED = 29871897         # the seed G19 builds PR-DVQVAE2 at
NORMS = ("BN", "FrozenBN")
NFRAMES = 4
# parameters whose gradients are stored: first encoder conv, a ResBlock 3x3 conv, the decoder's middle ConvTranspose
GRADS = {"enc_first": ("encoder", "layers.0.0.weight"), "enc_res3": ("encoder", "layers.5.block.1.0.weight"),
         "dec_ct1": ("generator", "layers.4.0.weight")}
NORM_LAYERS = {"enc0": ("encoder", "layers.0.1"), "enc_res1": ("encoder", "layers.6.block.3.1"),
               "dec_ct1": ("generator", "layers.4.1")}
ROWS = 4                    # leading rows of the large weight gradients


def seeded_norm_state(module, seed, prefix):
    """Non-trivial gamma / beta / running statistics for every norm layer of `module`."""
    st = {}
    for name, m in module.named_modules():
        if not hasattr(m, "running_mean"):
            continue
        c = m.running_mean.numel()
        r = seeded._rng(seed, prefix + name)
        st[name + ".weight"] = torch.from_numpy((1.0 + 0.2 * r.standard_normal(c)).astype(np.float32))
        st[name + ".bias"] = torch.from_numpy((0.1 * r.standard_normal(c)).astype(np.float32))
        st[name + ".running_mean"] = torch.from_numpy((0.05 * r.standard_normal(c)).astype(np.float32))
        st[name + ".running_var"] = torch.from_numpy(r.uniform(0.5, 2.0, c).astype(np.float32))
    return st


def seeded_conv_state(module, seed, prefix):
    """Seeded conv weights / biases for the keys that `module` has (normalised convs have no bias)."""
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()
              if (k.endswith(".weight") or k.endswith(".bias")) and v.dim() >= 1 and not _is_norm_key(module, k)}
    return seeded.seeded_params(shapes, seed, prefix)


def _is_norm_key(module, key):
    owner = module.get_submodule(key.rsplit(".", 1)[0])
    return hasattr(owner, "running_mean")


def clear_rows(z, cb, rel=1e-4):
    """(N, num, h, w) bool: latent positions whose fp64 best / second-best code distance gap exceeds rel * (|z|^2 +
    max |e|^2), the margin rule of the GPU tests (tests/util_models.margin_ok)."""
    n, _, h, w = z.shape
    out = []
    for i in range(4):
        rows = z[:, 64 * i:64 * (i + 1)].permute(0, 2, 3, 1).reshape(-1, 64).double()
        e = cb["ve.%d.embedding.weight" % i].double()
        dist = (e ** 2).sum(1)[None, :] + (rows ** 2).sum(1, keepdim=True) - 2.0 * rows @ e.t()
        top2 = torch.topk(dist, 2, dim=1, largest=False).values
        scale = (rows ** 2).sum(-1) + (e ** 2).sum(-1).max()
        out.append(((top2[:, 1] - top2[:, 0]) > rel * scale).view(n, h, w))
    return torch.stack(out, 1)


def capture(norm):
    from vidgen.modeling.meta_arch.build import build_model
    import vidgen.modeling.meta_arch  # noqa: F401
    from vidgen.utils.events import EventStorage
    cfg = MG.ref_cfg("configs/vqvae/PR-DVQVAE2.yaml", **{"MODEL.ENCODER.NORM": norm, "MODEL.GENERATOR.NORM": norm})
    tag = norm + "."
    out = {}
    torch.manual_seed(PIN_SEED)
    np.random.seed(PIN_SEED)
    random.seed(PIN_SEED)
    model = build_model(cfg)
    for part in ("encoder", "generator"):
        sd = getattr(model, part).state_dict()
        out[tag + part + ".keys"] = np.array(list(sd.keys()))
        out[tag + part + ".shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        names, rows = MG.tensor_pins(sd)
        out[tag + part + ".pin_names"], out[tag + part + ".pins"] = names, rows
    st = {}
    for part, pre in (("encoder", "enc."), ("generator", "dec.")):
        mod = getattr(model, part)
        s = seeded_conv_state(mod, SEED, pre)
        s.update(seeded_norm_state(mod, SEED, pre + "norm."))
        missing, unexpected = mod.load_state_dict(s, strict=False)
        assert not unexpected, unexpected
        assert all(k.endswith("num_batches_tracked") for k in missing), missing
        st[part] = s
    data = [{"image": seeded.seeded_input("g26.f%d" % i, (3, 64, 64), SEED).numpy()} for i in range(NFRAMES)]
    xin = model.normalizer(torch.stack([torch.from_numpy(d["image"]) for d in data]))
    model.eval()
    with torch.no_grad():
        zstd = float(model.encoder(xin.clone()).std())
    cb = seeded.seeded_codebook_state(SEED, scale=zstd)
    MG.dealias_codebook(model.codebook, cb)
    out[tag + "scale"] = zstd
    # ---- one train step (no optimizer: gradients and the running-statistics update) --------------------------------
    model.train()
    model.zero_grad()
    MG.dealias_codebook(model.codebook, cb)
    with EventStorage(0):
        losses = model(data, mode="supervised")
    sum(losses.values()).backward()
    for k in ("loss_reconstruction", "loss_commitment"):
        out[tag + "train." + k] = losses[k]
    for key, (part, name) in GRADS.items():
        g = dict(getattr(model, part).named_parameters())[name].grad
        out[tag + "train.grad." + key] = g[:ROWS]
    for key, (part, name) in NORM_LAYERS.items():
        m = getattr(model, part).get_submodule(name)
        for t in ("weight", "bias"):
            p = getattr(m, t)
            if isinstance(p, torch.nn.Parameter):
                out[tag + "train.grad.%s.%s" % (key, t)] = p.grad
    for part in ("encoder", "generator"):
        for k, v in getattr(model, part).state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
                out[tag + "after.%s.%s" % (part, k)] = v
    # ---- eval after the step -------------------------------------------------------------------------------------------
    model.eval()
    MG.dealias_codebook(model.codebook, cb)
    with torch.no_grad():
        z = model.encoder(xin.clone())
        out[tag + "eval.latent"] = model.codebook(z.clone())
        out[tag + "eval.clear"] = clear_rows(z, cb)
        res = model(data, mode="inference")
    out[tag + "eval.reconstruction"] = torch.stack([r["reconstruction"] for r in res])
    model.zero_grad()
    MG.dealias_codebook(model.codebook, cb)
    with EventStorage(0):
        losses = model(data, mode="supervised")
    sum(losses.values()).backward()
    for k in ("loss_reconstruction", "loss_commitment"):
        out[tag + "evalgrad." + k] = losses[k]
    for key, (part, name) in GRADS.items():
        out[tag + "evalgrad.grad." + key] = dict(getattr(model, part).named_parameters())[name].grad[:ROWS]
    for key, (part, name) in NORM_LAYERS.items():
        m = getattr(model, part).get_submodule(name)
        for t in ("weight", "bias"):
            p = getattr(m, t)
            if isinstance(p, torch.nn.Parameter):
                out[tag + "evalgrad.grad.%s.%s" % (key, t)] = p.grad
    return out


if __name__ == "__main__":
    arrays = {"seed": SEED, "norms": np.array(NORMS), "nframes": NFRAMES, "rows": ROWS}
    for n in NORMS:
        arrays.update(capture(n))
    MG.save("g26_batchnorm", **arrays)
