"""ResShuffleDecoder inside PR-DVQVAE2 at 32 clips x 16 frames against the shipped ResDecoder, same process, same box: train step
(per-step synchronised median and free-running mean, the method of leg_time.py, the two models alternating over `rounds`), and the
two pixel-shuffle kernels at the decoder's two tensors set beside lvt_upsample2x2 moving the same number of bytes (read once /
write once, kernels alternating over `rounds`).  Bytes are the algorithm's: every input and output element once.
python tools/profile/res_shuffle.py [steps] [rounds] [out.jsonl]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch, bench
from lvt_amd.hip import binding as L, ew
from lvt_amd.modeling import build_model

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "res_shuffle.jsonl")
dev = "cuda:0"; torch.cuda.set_device(0)
base = {"math": L.get_math_mode(), "device": torch.cuda.get_device_name(0)}
rows = []


def emit(row):
    rows.append(dict(row, **base))
    print(rows[-1], flush=True)


# ---- the train step ---------------------------------------------------------------------------------------------------------
def make_leg(generator):
    leg = bench.VqvaeLeg(dev, 1, 0, 0, 32, 2)
    leg.cfg.MODEL.GENERATOR.NAME = generator
    torch.manual_seed(bench.SEED)
    leg.model = build_model(leg.cfg)
    leg.model.train()
    leg.optimizers, _ = leg.model.configure_optimizers_and_checkpointers()
    for i in range(5): leg.step(i)
    torch.cuda.synchronize()
    return leg


legs = {name: make_leg(name) for name in ("ResDecoder", "ResShuffleDecoder")}
for r in range(rounds):
    for name, leg in legs.items():
        ts = []
        for i in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); leg.step(5 + i); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(steps): leg.step(5 + steps + i)
        torch.cuda.synchronize()
        emit({"kind": "train_step", "config": "PR-DVQVAE2 + " + name, "clips": 32, "frames": bench.CLIP_FRAMES, "round": r,
              "steps": steps, "median_ms": round(statistics.median(ts), 3),
              "free_running_ms": round((time.perf_counter() - t0) / steps * 1e3, 3)})
del legs, leg
torch.cuda.empty_cache()


# ---- the shuffle kernels beside lvt_upsample2x2 -------------------------------------------------------------------------------
def timed(fn, reps=50):
    for _ in range(5): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for shape, act in (((512, 16, 16, 128), "relu"), ((512, 32, 32, 3), "tanh")):
    n, h, w, c = shape
    cp = (c + 3) // 4 * 4
    coarse = torch.randn(n, h, w, 4 * c, device=dev)
    fine = torch.randn(n, 2 * h, 2 * w, cp, device=dev)
    nbytes = (coarse.numel() + fine.numel()) * 4
    # lvt_upsample2x2 reads one small tensor and writes four: a small tensor of a fifth of the shuffle's bytes, same rows and width
    n_up = round(nbytes / 5 / (h * w * cp * 4))
    small = torch.randn(n_up, h, w, cp, device=dev)
    cases = {
        "pixel_shuffle2 (%s)" % act: (lambda: ew.pixel_shuffle2(coarse, c, act), nbytes),
        "pixel_shuffle2 (copy)": (lambda: ew.pixel_shuffle2(coarse, c), nbytes),
        "pixel_unshuffle2": (lambda: ew.pixel_unshuffle2(fine, c), nbytes),
        "upsample2x2 (same bytes)": (lambda: ew.upsample2x2(small), 5 * small.numel() * 4),
    }
    for r in range(rounds):
        for name, (fn, nb) in cases.items():
            ms = timed(fn)
            emit({"kind": "kernel", "kernel": name, "coarse_tensor": [n, h, w, 4 * c], "fine_tensor": [n, 2 * h, 2 * w, cp], "round": r,
                  "bytes": nb, "us": round(ms * 1e3, 2), "GBps": round(nb / ms / 1e6, 1)})
with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
