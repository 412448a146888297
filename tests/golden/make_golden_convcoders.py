#!/usr/bin/env python
"""Generate G28 (g28_conv_coders.npz): the reference's PR-DVQVAE2 with MODEL.ENCODER.NAME "ConvEncoder" and
MODEL.GENERATOR.NAME "ConvDecoder", over 4 frames.  Same route as make_golden_norm.py (the reference imported through
oracle/shim, seeded weights from seeded.py, CPU, plain arrays out), whose helpers it reuses.

Three configs, a / b / c of convcoders_cfg.py.

Per config it records the state-dict key list, shapes and per-tensor checksums of `build_model(cfg)` at the config seed;
then, with seeded weights (and non-trivial gamma / beta / running statistics for b): the train-mode `supervised` losses,
leading rows of the gradients of the first encoder conv, the encoder conv behind the first pool, the first decoder conv and the
decoder's last conv; for b the gamma / beta gradients of three norm layers and every running statistic after the step; in eval
mode after that step the `encode` latents with the fp64 "clear rows" mask of G26 and the `inference` reconstructions.

SEED is the first seed from 2828 on at which at least 99 % of the latent positions of every config are clear in the reference's
own fp64 distances (asserted below); the GPU test compares latents on those rows only.

    python tests/golden/make_golden_convcoders.py
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

import convcoders_cfg as CC  # noqa: E402
import seeded  # noqa: E402

SEED = 2828
PIN_SEED = 29871897         # the seed G19 builds PR-DVQVAE2 at
NFRAMES = 4
ROWS = 4                    # leading rows of the weight gradients
MIN_CLEAR = 0.99

def conv_names(module):
    """Names of the conv modules of `module` in order (the conv inside a normalised pair)."""
    return [n for n, m in module.named_modules() if isinstance(m, torch.nn.Conv2d)]


def grad_params(model):
    """tag -> (part, parameter name): first encoder conv, the encoder conv behind the first pool, first and last decoder conv."""
    enc, dec = conv_names(model.encoder), conv_names(model.generator)
    return {"enc_first": ("encoder", enc[0] + ".weight"), "enc_mid": ("encoder", enc[3] + ".weight"),
            "dec_first": ("generator", dec[0] + ".weight"), "dec_last": ("generator", dec[-1] + ".weight")}


def norm_layers(model):
    """tag -> (part, module name) of three norm layers: the first and last of the encoder, the second of the decoder."""
    enc = [n for n, m in model.encoder.named_modules() if hasattr(m, "running_mean")]
    dec = [n for n, m in model.generator.named_modules() if hasattr(m, "running_mean")]
    if not enc:
        return {}
    return {"enc0": ("encoder", enc[0]), "enc_last": ("encoder", enc[-1]), "dec1": ("generator", dec[1])}


def capture(name, seed):
    from vidgen.modeling.meta_arch.build import build_model
    import vidgen.modeling.meta_arch  # noqa: F401
    from vidgen.utils.events import EventStorage
    cfg = MG.ref_cfg("configs/vqvae/PR-DVQVAE2.yaml", **CC.overrides(name))
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
    data = [{"image": seeded.seeded_input("g28.f%d" % i, (3, 64, 64), seed).numpy()} for i in range(NFRAMES)]
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
    for key, (part, pname) in grad_params(model).items():
        out[tag + "train.grad." + key] = dict(getattr(model, part).named_parameters())[pname].grad[:ROWS]
    for key, (part, mname) in norm_layers(model).items():
        m = getattr(model, part).get_submodule(mname)
        for t in ("weight", "bias"):
            out[tag + "train.grad.%s.%s" % (key, t)] = getattr(m, t).grad
    for part in ("encoder", "generator"):
        for k, v in getattr(model, part).state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
                out[tag + "after.%s.%s" % (part, k)] = v
    # ---- eval after the step -----------------------------------------------------------------------------------------------
    model.eval()
    MG.dealias_codebook(model.codebook, cb)
    with torch.no_grad():
        z = model.encoder(xin.clone())
        out[tag + "eval.latent"] = model.codebook(z.clone()).to(torch.int16)         # codes < 512
        clear = MGN.clear_rows(z, cb)
        out[tag + "eval.clear"] = clear
        res = model(data, mode="inference")
    out[tag + "eval.reconstruction"] = torch.stack([r["reconstruction"] for r in res])
    return out, float(clear.float().mean())


def capture_all(seed):
    arrays = {"seed": seed, "configs": np.array(CC.NAMES), "nframes": NFRAMES, "rows": ROWS}
    shares = {}
    for n in CC.NAMES:
        got, shares[n] = capture(n, seed)
        arrays.update(got)
        arrays[n + ".clear_share"] = shares[n]
    return arrays, shares


if __name__ == "__main__":
    arrays, shares = capture_all(SEED)
    print("clear share per config at seed %d: %s" % (SEED, shares))
    assert min(shares.values()) >= MIN_CLEAR, shares
    MG.save("g28_conv_coders", **arrays)
