"""What the averaged weights (SOLVER.MODEL_EMA) cost the optimizer launches of a train step: PR-DVQVAE2 at 32 clips x 16 frames
and DSFVT at 64 slices, averaging off and on, same process, same box, the two modes alternating over `rounds` on ONE model per
workload (the method of grad_clip.py).  Timed are the optimizers' `step()` calls alone, on the gradients of one backward pass that
stay in place: `reps` back-to-back repetitions between two events, so the number is the launches' device time, and the bytes are
what the kernels move (Adam 28 -> 36 B per element: p, g, m, v read, p, m, v written, plus the shadow read and written; RMSprop
with momentum the same).  A last block times one `ModelEma.averaged()` enter + leave (two swaps).
python tools/profile/model_ema.py [reps] [rounds] [out.jsonl] [workloads: vqvae,dsfvt]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch, bench
from lvt_amd.hip import binding as L
from lvt_amd.solver.ema import ModelEma

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "model_ema.jsonl")
which = sys.argv[4].split(",") if len(sys.argv) > 4 else ["vqvae", "dsfvt"]
dev = "cuda:0"; torch.cuda.set_device(0)
base = {"math": L.get_math_mode(), "device": torch.cuda.get_device_name(0)}
rows = []


def emit(row):
    rows.append(dict(row, **base))
    print(rows[-1], flush=True)


def time_leg(name, leg, backward, extra):
    opts = [o["optimizer"] for o in leg.optimizers]
    for i in range(3): leg.step(i)                       # optimizer state exists, caches are warm
    backward()                                           # gradients that stay: step() does not consume them
    elems = sum(p.numel() for o in opts for g in o.param_groups for p in g["params"] if p.grad is not None)
    tensors = sum(1 for o in opts for g in o.param_groups for p in g["params"] if p.grad is not None)
    per = {"off": 28, "on": 36}
    ema = ModelEma(opts, 0.9999, True)                   # shadows for every parameter; toggled below

    def mode(on):
        for o in opts:
            o.enable_ema(0.9999, True) if on else o.disable_ema()

    def run():
        for o in opts: o.step()
    for on in (False, True):
        mode(on); run()
    torch.cuda.synchronize()
    for r in range(rounds):
        for tag, on in (("off", False), ("on", True)):
            mode(on)
            ts = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps): run()
                b.record(); torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) / reps)
            ms = statistics.median(ts)
            emit(dict({"kind": "optimizer_step", "config": name, "ema": tag, "round": r, "reps": reps, "tensors": tensors,
                       "elements": elems, "us": round(ms * 1e3, 2), "bytes": per[tag] * elems,
                       "GBps": round(per[tag] * elems / ms / 1e6, 1)}, **extra))
    mode(True)
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            with ema.averaged():
                pass
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    ms = statistics.median(ts)
    emit(dict({"kind": "averaged_enter_leave", "config": name, "tensors": tensors, "elements": elems, "us": round(ms * 1e3, 2),
               "bytes": 32 * elems, "GBps": round(32 * elems / ms / 1e6, 1)}, **extra))


if "vqvae" in which:
    leg = bench.VqvaeLeg(dev, 1, 0, 0, 32, 2)

    def bwd():
        from lvt_amd.utils.events import EventStorage
        with EventStorage(0):
            sum(leg.model(leg.batches[0], mode="supervised").values()).backward()
    time_leg("PR-DVQVAE2", leg, bwd, {"clips": 32, "frames": bench.CLIP_FRAMES})
    del leg
    torch.cuda.empty_cache()

if "dsfvt" in which:
    leg = bench.DsfvtLeg(dev, 1, 0, 0, 64, 2)

    def bwd():
        from lvt_amd.utils.events import EventStorage
        ctx, sl, sidx, ign = leg.batches[0]
        with EventStorage(0):
            leg.model.compute_supervised_loss(ctx, sl, sidx, ign)["loss_cross_entropy"].backward()
    time_leg("DSFVT", leg, bwd, {"slices": 64})

os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
