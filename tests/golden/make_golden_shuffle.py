#!/usr/bin/env python
"""Generate G29 (g29_res_shuffle.npz): the reference's PR-DVQVAE2 with MODEL.GENERATOR.NAME "ResShuffleDecoder", over 4 frames.
Same route as make_golden_norm.py (the reference imported through oracle/shim, seeded weights from seeded.py, CPU, plain arrays
out), whose helpers it reuses.

Three configs, p / b / s of shuffle_cfg.py.

Per config it records the state-dict key list, shapes and per-tensor checksums of `build_model(cfg)` at the config seed; then,
with seeded weights (and non-trivial gamma / beta / running statistics for b): the train-mode `supervised` losses, leading rows of
the gradients of the decoder's three convolutions outside the ResBlocks (layers.0, layers.4, layers.7) and the whole bias gradient
of layers.7; for b the gamma / beta gradients of generator.layers.4.1 and every running statistic after the step; in eval mode
after that step the `encode` latents with the fp64 "clear rows" mask of G26, `model.decode` of those latents (the call of
VTSampler: eval, no grad, (T, nc, h, w) codes), the `inference` reconstructions and one `supervised` forward + backward.

Two recordings would repeat bytes already in the file and are stored as the identity instead, each asserted here bit for bit
(a file added to the repository may not exceed 1 MiB -- a few older fixtures predate that limit; with both stored this one is
1.5 MiB, as it stands 0.9 MiB): the `inference` reconstruction IS decode * PIXEL_STD + PIXEL_MEAN in fp32 (the reference's
back_normaliser on the decode of the same latents; the tests form it from `eval.decode`), and without a norm the eval-mode step
IS the train-mode step (`<tag>.evalgrad.same_as_train` = 1, no `evalgrad.*` arrays; tag b stores them).

At least MIN_CLEAR of the latent positions of every config must be clear in the reference's own fp64 distances (asserted below);
the GPU test compares latents on those rows only.

    python tests/golden/make_golden_shuffle.py
"""
import os
import random
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (sets up the reference / shim import path)
import make_golden_norm as MGN  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

import seeded  # noqa: E402
import shuffle_cfg as SC  # noqa: E402

SEED = 2929
PIN_SEED = 29871897         # the seed G19 builds PR-DVQVAE2 at
NFRAMES = 4
ROWS = 4                    # leading rows of the weight gradients
MIN_CLEAR = 0.98


def grad_params(norm):
    """tag -> name of the generator parameter whose gradient is stored (layers.7 is never normalised)."""
    sub = ".0" if norm else ""
    return {"dec0": "layers.0%s.weight" % sub, "dec4": "layers.4%s.weight" % sub, "dec7": "layers.7.weight"}


def store_grads(out, pre, model, norm):
    params = dict(model.generator.named_parameters())
    for key, pname in grad_params(norm).items():
        out[pre + "grad." + key] = params[pname].grad[:ROWS]
    out[pre + "grad.dec7.bias"] = params["layers.7.bias"].grad
    if norm:
        m = model.generator.get_submodule("layers.4.1")
        for t in ("weight", "bias"):
            out[pre + "grad.dec4n.%s" % t] = getattr(m, t).grad


def capture(name, seed):
    from vidgen.modeling.meta_arch.build import build_model
    import vidgen.modeling.meta_arch  # noqa: F401
    from vidgen.utils.events import EventStorage
    norm = SC.CONFIGS[name]["norm"]
    cfg = MG.ref_cfg("configs/vqvae/PR-DVQVAE2.yaml", **SC.overrides(name))
    tag = name + "."
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
    for part, pre in (("encoder", "enc."), ("generator", "dec.")):
        mod = getattr(model, part)
        s = MGN.seeded_conv_state(mod, seed, pre)
        s.update(MGN.seeded_norm_state(mod, seed, pre + "norm."))
        missing, unexpected = mod.load_state_dict(s, strict=False)
        assert not unexpected, unexpected
        assert all(k.endswith("num_batches_tracked") for k in missing), missing
    data = [{"image": seeded.seeded_input("g29.f%d" % i, (3, 64, 64), seed).numpy()} for i in range(NFRAMES)]
    xin = model.normalizer(torch.stack([torch.from_numpy(d["image"]) for d in data]))
    model.eval()
    with torch.no_grad():
        zstd = float(model.encoder(xin.clone()).std())
    cb = seeded.seeded_codebook_state(seed, scale=zstd)
    out[tag + "scale"] = zstd
    # ---- one train step (no optimizer: gradients and the running-statistics update) ------------------------------------
    model.train()
    model.zero_grad()
    MG.dealias_codebook(model.codebook, cb)
    with EventStorage(0):
        losses = model(data, mode="supervised")
    sum(losses.values()).backward()
    for k in ("loss_reconstruction", "loss_commitment"):
        out[tag + "train." + k] = losses[k]
    store_grads(out, tag + "train.", model, norm)
    for part in ("encoder", "generator"):
        for k, v in getattr(model, part).state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
                out[tag + "after.%s.%s" % (part, k)] = v
    # ---- eval after the step -----------------------------------------------------------------------------------------------
    model.eval()
    MG.dealias_codebook(model.codebook, cb)
    with torch.no_grad():
        z = model.encoder(xin.clone())
        latent = model.codebook(z.clone())
        out[tag + "eval.latent"] = latent.to(torch.int16)         # codes < 512
        clear = MGN.clear_rows(z, cb)
        out[tag + "eval.clear"] = clear
        res = model(data, mode="inference")
        out[tag + "eval.decode"] = model.decode(latent)
    c = SC.CONFIGS[name]
    assert torch.equal(torch.stack([r["reconstruction"] for r in res]), out[tag + "eval.decode"] * c["std"] + c["mean"])
    model.zero_grad()
    MG.dealias_codebook(model.codebook, cb)
    with EventStorage(0):
        losses = model(data, mode="supervised")
    sum(losses.values()).backward()
    for k in ("loss_reconstruction", "loss_commitment"):
        out[tag + "evalgrad." + k] = losses[k]
    store_grads(out, tag + "evalgrad.", model, norm)
    ev = [k for k in out if k.startswith(tag + "evalgrad.")]
    same = all(torch.equal(torch.as_tensor(out[k]), torch.as_tensor(out[k.replace(".evalgrad.", ".train.")])) for k in ev)
    assert same == (not norm), (name, same)
    if same:
        for k in ev:
            del out[k]
    out[tag + "evalgrad.same_as_train"] = int(same)
    return out, float(clear.float().mean())


def capture_all(seed):
    arrays = {"seed": seed, "configs": np.array(SC.NAMES), "nframes": NFRAMES, "rows": ROWS}
    shares = {}
    for n in SC.NAMES:
        got, shares[n] = capture(n, seed)
        arrays.update(got)
        arrays[n + ".clear_share"] = shares[n]
    return arrays, shares


if __name__ == "__main__":
    arrays, shares = capture_all(SEED)
    print("clear share per config at seed %d: %s" % (SEED, shares))
    assert min(shares.values()) >= MIN_CLEAR, shares
    MG.save("g29_res_shuffle", **arrays)
