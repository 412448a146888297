"""PR-DVQVAE2 train step with a sigmoid decoder head against the shipped tanh head, same box, same process (the method of
leg_time.py: per-step synchronised median and free-running mean of the bench's VQ-VAE leg, heads alternating over `rounds`):
python tools/profile/out_activation.py [steps] [rounds] [out.jsonl]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch, bench
from lvt_amd.hip import binding as L
from lvt_amd.modeling import build_model

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "out_activation.jsonl")
dev = "cuda:0"; torch.cuda.set_device(0)


def leg_of(act):
    leg = bench.VqvaeLeg(dev, 1, 0, 0, 32, 4)
    if act != leg.cfg.MODEL.GENERATOR.OUT_ACTIVATION:
        leg.cfg.MODEL.GENERATOR.OUT_ACTIVATION = act
        torch.manual_seed(bench.SEED)
        leg.model = build_model(leg.cfg)
        leg.model.train()
        leg.optimizers, _ = leg.model.configure_optimizers_and_checkpointers()
    for i in range(5): leg.step(i)
    torch.cuda.synchronize()
    return leg


def measure(leg):
    ts = []
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); leg.step(5 + i); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(steps): leg.step(5 + steps + i)
    torch.cuda.synchronize()
    return statistics.median(ts), (time.perf_counter() - t0) / steps * 1e3


legs = {act: leg_of(act) for act in ("tanh", "sigmoid")}
rows = []
for r in range(rounds):
    for act, leg in legs.items():
        med, free = measure(leg)
        rows.append({"kind": "train_step", "config": "PR-DVQVAE2", "clips": 32, "frames": bench.CLIP_FRAMES, "head": act, "round": r,
                     "steps": steps, "median_ms": round(med, 3), "free_running_ms": round(free, 3), "math": L.get_math_mode(),
                     "device": torch.cuda.get_device_name(0)})
        print(rows[-1], flush=True)
with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
