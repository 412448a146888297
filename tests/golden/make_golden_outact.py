#!/usr/bin/env python
"""Generate G27 (g27_out_activation.npz): the reference's PR-DVQVAE2 with every pair of MODEL.ENCODER.OUT_ACTIVATION /
MODEL.GENERATOR.OUT_ACTIVATION listed in COMBOS, over 4 frames.  Same route as make_golden_norm.py (the reference
imported through oracle/shim, seeded weights from seeded.py, CPU, plain arrays out), whose helpers it reuses.

Per combination it records, with seeded weights and the codebook scaled to the encoder's output std: the train-mode
`supervised` losses of one step and the leading rows of the gradients of the three tensors G26 stores; then in eval mode
the `encode` latents with their `clear_rows` mask and the share of clear positions (asserted >= 0.99 here), and the
`inference` reconstructions.  Inference treats every frame on its own (eval statistics), so the reconstructions of the
leading REC_FRAMES frames are stored: all four of all four combinations would not fit the size of G26.

    python tests/golden/make_golden_outact.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (sets up the reference / shim import path)
import make_golden_norm as MN  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

import seeded  # noqa: E402

SEED = 2727                 # the inputs
# weights, norm tensors and codebook: at 2727 the sigmoid-bounded encoder (outputs 0.5 +- 0.016, far from the zero-mean
# codebook) leaves only 0.949 of its latent positions clear; 2728 is the next seed at which every combination passes MIN_CLEAR
WSEED = 2728
NFRAMES = 4
REC_FRAMES = 2
ROWS = MN.ROWS
# (tag, NORM of both stacks, ENCODER.OUT_ACTIVATION, GENERATOR.OUT_ACTIVATION)
COMBOS = (("plain_sigmoid", "", "", "sigmoid"), ("tanh_plain", "", "tanh", ""), ("sigmoid_tanh", "", "sigmoid", "tanh"),
          ("bn.plain_sigmoid", "BN", "", "sigmoid"))
MIN_CLEAR = 0.99


def grad_names(norm):
    """GRADS of make_golden_norm.py; without a norm the conv is not wrapped, so its key loses the wrapper's index 0."""
    return {k: (part, name if norm else name.replace(".0.weight", ".weight")) for k, (part, name) in MN.GRADS.items()}


def capture(tag, norm, enc_act, dec_act):
    from vidgen.modeling.meta_arch.build import build_model
    import vidgen.modeling.meta_arch  # noqa: F401
    from vidgen.utils.events import EventStorage
    cfg = MG.ref_cfg("configs/vqvae/PR-DVQVAE2.yaml", **{"MODEL.ENCODER.NORM": norm, "MODEL.GENERATOR.NORM": norm,
                                                         "MODEL.ENCODER.OUT_ACTIVATION": enc_act,
                                                         "MODEL.GENERATOR.OUT_ACTIVATION": dec_act})
    tag += "."
    out = {}
    torch.manual_seed(WSEED)
    model = build_model(cfg)
    for part, pre in (("encoder", "enc."), ("generator", "dec.")):
        mod = getattr(model, part)
        s = MN.seeded_conv_state(mod, WSEED, pre)
        s.update(MN.seeded_norm_state(mod, WSEED, pre + "norm."))
        missing, unexpected = mod.load_state_dict(s, strict=False)
        assert not unexpected, unexpected
        assert all(k.endswith("num_batches_tracked") for k in missing), missing
        out[tag + part + ".keys"] = np.array(list(mod.state_dict().keys()))
        out[tag + part + ".children"] = np.array([type(m).__name__ for m in mod.layers])
    data = [{"image": seeded.seeded_input("g27.f%d" % i, (3, 64, 64), SEED).numpy()} for i in range(NFRAMES)]
    xin = model.normalizer(torch.stack([torch.from_numpy(d["image"]) for d in data]))
    model.eval()
    with torch.no_grad():
        zstd = float(model.encoder(xin.clone()).std())
    cb = seeded.seeded_codebook_state(WSEED, scale=zstd)
    out[tag + "scale"] = zstd
    # ---- one train step (no optimizer) -----------------------------------------------------------------------------
    model.train()
    model.zero_grad()
    MG.dealias_codebook(model.codebook, cb)
    with EventStorage(0):
        losses = model(data, mode="supervised")
    sum(losses.values()).backward()
    for k in ("loss_reconstruction", "loss_commitment"):
        out[tag + "train." + k] = losses[k]
    for key, (part, name) in grad_names(norm).items():
        out[tag + "train.grad." + key] = dict(getattr(model, part).named_parameters())[name].grad[:ROWS]
    # ---- eval (after the step: a BN combination normalises with the statistics that step left) -------------------------
    model.eval()
    MG.dealias_codebook(model.codebook, cb)
    with torch.no_grad():
        z = model.encoder(xin.clone())
        out[tag + "eval.latent"] = model.codebook(z.clone())
        clear = MN.clear_rows(z, cb)
        out[tag + "eval.clear"] = clear
        res = model(data, mode="inference")
    share = float(clear.float().mean())
    print("%-20s clear share %.4f  z std %.4f" % (tag, share, zstd))
    assert share >= MIN_CLEAR, (tag, share)
    out[tag + "eval.clear_share"] = share
    out[tag + "eval.reconstruction"] = torch.stack([r["reconstruction"] for r in res[:REC_FRAMES]])
    for part in ("encoder", "generator"):
        for k, v in getattr(model, part).state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                out[tag + "after.%s.%s" % (part, k)] = v
    return out


if __name__ == "__main__":
    arrays = {"seed": SEED, "wseed": WSEED, "nframes": NFRAMES, "rec_frames": REC_FRAMES, "rows": ROWS,
              "combos": np.array(["|".join(c) for c in COMBOS])}
    for c in COMBOS:
        arrays.update(capture(*c))
    MG.save("g27_out_activation", **arrays)
