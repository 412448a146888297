#!/usr/bin/env python
"""Generate G25 (g25_codebook_geometry.npz): the reference's PR-DVQVAE2 with the codebook geometry overridden to
(NUM 8, SIZE 1024), (NUM 2, SIZE 256) and (NUM 1, SIZE 1024) -- 32-d and 128-d sub-vectors and codebooks outside
{128, 256, 512}.  Same route as make_golden.py (the reference imported through oracle/shim, seeded weights from seeded.py,
CPU, plain arrays out), whose helpers it reuses.

    python tests/golden/make_golden_geometry.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (sets up the reference / shim import path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import seeded  # noqa: E402

SEED = 2525
GEOMETRIES = ((8, 1024), (2, 256), (1, 1024))
NROWS = 32                  # leading codes of every codebook stored after the update (the running sizes are stored whole)


def capture(num, K):
    from vidgen.modeling.meta_arch.build import build_model
    import vidgen.modeling.meta_arch  # noqa: F401
    from vidgen.utils.events import EventStorage
    cfg = MG.ref_cfg("configs/vqvae/PR-DVQVAE2.yaml", **{"MODEL.CODEBOOK.NUM": num, "MODEL.CODEBOOK.SIZE": K})
    model = build_model(cfg)
    D = cfg.MODEL.CODEBOOK.DIM
    MG.load_into(model.encoder, seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, SEED, "enc."))
    MG.load_into(model.generator, seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, SEED, "dec."))
    data = [{"image": seeded.seeded_input("g25.f%d" % i, (3, 64, 64), SEED).numpy()} for i in range(2)]
    xin = model.normalizer(torch.stack([torch.from_numpy(d["image"]) for d in data]))
    with torch.no_grad():
        zstd = float(model.encoder(xin.clone()).std())
    st = seeded.seeded_codebook_state(SEED, num=num, K=K, D=D // num, scale=zstd)

    def dealias():
        if num == 1:
            model.codebook.embedding.weight.data = st["ve.0.embedding.weight"].clone()
            model.codebook.running_size = st["ve.0.running_size"].clone()
            model.codebook.running_sum = st["ve.0.running_sum"].clone()
        else:
            MG.dealias_codebook(model.codebook, st)
    dealias()
    with torch.no_grad():
        idx = model.codebook(model.encoder(xin.clone()))             # (N, num, 16, 16) / (N, 16, 16)
    if num == 1:
        idx = idx.unsqueeze(1)
    dealias()
    model.train()
    model.zero_grad()
    with EventStorage(0):
        losses = model(data, mode="supervised")
    sum(losses.values()).backward()
    new = MG.cb_state_of(model.codebook)
    if num == 1:
        new = {"ve.0." + k: v for k, v in new.items()}
    tag = "n%d_k%d." % (num, K)
    out = {tag + "scale": zstd, tag + "idx": idx,
           tag + "loss_reconstruction": losses["loss_reconstruction"], tag + "loss_commitment": losses["loss_commitment"],
           tag + "grad_enc_first": model.encoder.layers[0].weight.grad, tag + "grad_enc_first_bias": model.encoder.layers[0].bias.grad,
           tag + "grad_dec_last": model.generator.layers[6].weight.grad, tag + "grad_dec_last_bias": model.generator.layers[6].bias.grad}
    for k, v in new.items():
        out[tag + "new." + k] = v if k.endswith("running_size") else v[:NROWS]
    return out


if __name__ == "__main__":
    arrays = {"seed": SEED, "geometries": np.array(GEOMETRIES), "nrows": NROWS}
    for num, K in GEOMETRIES:
        arrays.update(capture(num, K))
    MG.save("g25_codebook_geometry", **arrays)
