"""What codebook restart costs a train step: PR-DVQVAE2 at 32 clips x 16 frames with MODEL.CODEBOOK.RESTART off, on with THRESHOLD 0
(monitoring only: candidates gathered, health written, nothing restarted) and on with THRESHOLD 1.0 -- same process, same box,
three models of the same seed alternating over `rounds` (per-step synchronised median and free-running mean, the method of
grad_clip.py / res_shuffle.py).  "off" is bench.py's own leg, untouched; the other two are the same leg with
`codebook.enable_restart` called on its quantiser, which is what VQVAEModel does with the config keys.  Every mode is repeated
`rounds` times, so the file shows its own run-to-run spread.
python tools/profile/codebook_restart.py [steps] [rounds] [out.jsonl]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch, bench
from lvt_amd.hip import binding as L

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "codebook_restart.jsonl")
dev = "cuda:0"; torch.cuda.set_device(0)
base = {"math": L.get_math_mode(), "device": torch.cuda.get_device_name(0), "abi": L.lib().lvt_version()}
rows = []

legs = {}
for mode, thr in (("off", None), ("threshold_0", 0.0), ("threshold_1", 1.0)):
    leg = bench.VqvaeLeg(dev, 1, 0, 0, 32, 2)
    if thr is not None:
        leg.model.codebook.enable_restart(thr, 0)
    for i in range(5): leg.step(i)
    legs[mode] = leg
torch.cuda.synchronize()

for r in range(rounds):
    for mode, leg in legs.items():
        ts = []
        for i in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); leg.step(5 + i); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(steps): leg.step(5 + steps + i)
        torch.cuda.synchronize()
        row = {"kind": "train_step", "config": "PR-DVQVAE2", "clips": 32, "frames": bench.CLIP_FRAMES, "restart": mode, "round": r,
               "steps": steps, "median_ms": round(statistics.median(ts), 3),
               "free_running_ms": round((time.perf_counter() - t0) / steps * 1e3, 3)}
        health = leg.model.codebook_health()
        if health is not None:
            row.update(zip(("codebook_perplexity", "codebook_dead", "codebook_restarts"), torch.stack(list(health)).tolist()))
        rows.append(dict(row, **base))
        print(rows[-1], flush=True)

with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
