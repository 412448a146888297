"""The three ConvEncoder / ConvDecoder configs of fixture G28, as overrides of configs/vqvae/PR-DVQVAE2.yaml: shared by the script
that captures the fixture from the reference (make_golden_convcoders.py) and the tests that rebuild the models.

    a   NF 32, N_LAYERS 2, OUT_CHANNELS / IN_CHANNELS 256, NORM "", decoder tanh             (16x16 latents)
    b   the same with NORM "BN" on both sides
    c   NF 16, N_LAYERS 1 on both sides, decoder sigmoid, PIXEL_MEAN 0 / PIXEL_STD 1           (32x32 latents)
"""
CONFIGS = {
    "a": dict(nf=32, n_layers=2, norm="", act="tanh", mean=0.5, std=0.5),
    "b": dict(nf=32, n_layers=2, norm="BN", act="tanh", mean=0.5, std=0.5),
    "c": dict(nf=16, n_layers=1, norm="", act="sigmoid", mean=0.0, std=1.0),
}
NAMES = tuple(CONFIGS)


def overrides(name):
    c = CONFIGS[name]
    return {"MODEL.ENCODER.NAME": "ConvEncoder", "MODEL.ENCODER.NF": c["nf"], "MODEL.ENCODER.N_LAYERS": c["n_layers"],
            "MODEL.ENCODER.OUT_CHANNELS": 256, "MODEL.ENCODER.NORM": c["norm"],
            "MODEL.GENERATOR.NAME": "ConvDecoder", "MODEL.GENERATOR.IN_CHANNELS": 256, "MODEL.GENERATOR.NF": c["nf"],
            "MODEL.GENERATOR.N_LAYERS": c["n_layers"], "MODEL.GENERATOR.NORM": c["norm"],
            "MODEL.GENERATOR.OUT_ACTIVATION": c["act"],
            "MODEL.PIXEL_MEAN": [c["mean"]] * 3, "MODEL.PIXEL_STD": [c["std"]] * 3}


def apply(cfg, over):
    """Set dotted KEY -> value pairs on a config node tree; -> cfg."""
    for k, v in over.items():
        node = cfg
        ks = k.split(".")
        for s in ks[:-1]:
            node = node[s]
        node[ks[-1]] = v
    return cfg


def opts(name):
    """The overrides as the KEY VALUE list of a command line (tools/train_net.py)."""
    out = []
    for k, v in overrides(name).items():
        out += [k, repr(v) if not isinstance(v, str) else v]
    return out
