"""The three ResShuffleDecoder configs of fixture G29, as overrides of configs/vqvae/PR-DVQVAE2.yaml: shared by the script that
captures the fixture from the reference (make_golden_shuffle.py) and the tests that rebuild the models.

    p   NORM "" on both sides, decoder tanh, PIXEL_MEAN / PIXEL_STD 0.5
    b   the same with NORM "BN" on both sides
    s   NORM "", decoder sigmoid, PIXEL_MEAN 0 / PIXEL_STD 1
"""
CONFIGS = {
    "p": dict(norm="", act="tanh", mean=0.5, std=0.5),
    "b": dict(norm="BN", act="tanh", mean=0.5, std=0.5),
    "s": dict(norm="", act="sigmoid", mean=0.0, std=1.0),
}
NAMES = tuple(CONFIGS)


def overrides(name):
    c = CONFIGS[name]
    return {"MODEL.ENCODER.NORM": c["norm"], "MODEL.GENERATOR.NAME": "ResShuffleDecoder", "MODEL.GENERATOR.NORM": c["norm"],
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
