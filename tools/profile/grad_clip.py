"""What gradient clipping costs a train step: PR-DVQVAE2 at 32 clips x 16 frames and DSFVT at 64 slices with SOLVER.CLIP_GRADIENTS
off, "norm" and "value", same process, same box, the three modes alternating over `rounds` on ONE model per workload (per-step
synchronised median and free-running mean, the method of res_shuffle.py / leg_time.py).  "off" is bench.py's own step, untouched;
the other two put GradClipper.prepare() between the backward and the optimizers' step, where the Trainer puts it.  A last block
times the norm and coefficient launches alone on the DSFVT gradients (bytes: every gradient element read once).
python tools/profile/grad_clip.py [steps] [rounds] [out.jsonl] [workloads: vqvae,dsfvt]

The off path against another commit: `python tools/profile/grad_clip.py off <tree> <tag> [steps] [out.jsonl]` times bench.py's two
legs (no clipper anywhere) with the package, library and bench.py of the checkout at <tree> (`git archive <commit> | tar -x -C
<tree>`, then `make -C <tree>/lvt_amd/csrc`) and APPENDS `kind: "off_path"` rows; run it for both trees in turn, several times."""
import json, os, statistics, sys, time
OFF = sys.argv[1:2] == ["off"]
ROOT = os.path.abspath(sys.argv[2]) if OFF else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch, bench
from lvt_amd.hip import binding as L
assert os.path.abspath(bench.__file__).startswith(ROOT) and os.path.abspath(L._LIB_PATH).startswith(ROOT), (bench.__file__, L._LIB_PATH)

if OFF:
    tag, steps = sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 20
    out = sys.argv[5] if len(sys.argv) > 5 else os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                                                             "profiles", "grad_clip.jsonl")
    dev = "cuda:0"; torch.cuda.set_device(0)
    rows = []
    for name, cls, batch in (("PR-DVQVAE2", bench.VqvaeLeg, 32), ("DSFVT", bench.DsfvtLeg, 64)):
        leg = cls(dev, 1, 0, 0, batch, 2)
        for i in range(5): leg.step(i)
        torch.cuda.synchronize()
        for r in range(2):
            ts = []
            for i in range(steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); leg.step(5 + i); b.record(); torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(steps): leg.step(5 + steps + i)
            torch.cuda.synchronize()
            rows.append({"kind": "off_path", "tree": tag, "abi": L.lib().lvt_version(), "config": name, "round": r, "steps": steps,
                         "median_ms": round(statistics.median(ts), 3),
                         "free_running_ms": round((time.perf_counter() - t0) / steps * 1e3, 3),
                         "math": L.get_math_mode(), "device": torch.cuda.get_device_name(0)})
            print(rows[-1], flush=True)
        del leg
        torch.cuda.empty_cache()
    with open(out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    sys.exit(0)

from lvt_amd.solver.clip import GradClipper

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "grad_clip.jsonl")
which = sys.argv[4].split(",") if len(sys.argv) > 4 else ["vqvae", "dsfvt"]
dev = "cuda:0"; torch.cuda.set_device(0)
base = {"math": L.get_math_mode(), "device": torch.cuda.get_device_name(0)}
rows = []


def emit(row):
    rows.append(dict(row, **base))
    print(rows[-1], flush=True)


class Clipped:
    """A bench leg whose optimizers' first step is preceded by clipper.prepare() (a step pre-hook: leg.step itself stays as it is)."""

    def __init__(self, leg, clip_type):
        self.leg = leg
        opts = [o["optimizer"] for o in leg.optimizers]
        self.clipper = GradClipper(opts, clip_type, 1.0, 2.0) if clip_type != "off" else None
        self.first = opts[0]

    def step(self, i):
        if self.clipper is None:
            return self.leg.step(i)
        h = self.first.register_step_pre_hook(lambda *a: self.clipper.prepare())
        try:
            return self.leg.step(i)
        finally:
            h.remove()


def time_leg(name, leg, extra):
    modes = {m: Clipped(leg, m) for m in ("off", "norm", "value")}
    for i in range(5): leg.step(i)
    for m in modes.values(): m.step(0)
    torch.cuda.synchronize()
    for r in range(rounds):
        for mode, run in modes.items():
            ts = []
            for i in range(steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); run.step(5 + i); b.record(); torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(steps): run.step(5 + steps + i)
            torch.cuda.synchronize()
            row = {"kind": "train_step", "config": name, "clip": mode, "round": r, "steps": steps,
                   "median_ms": round(statistics.median(ts), 3),
                   "free_running_ms": round((time.perf_counter() - t0) / steps * 1e3, 3)}
            if run.clipper is not None and run.clipper.skipped is not None:
                row["skipped_steps"] = int(run.clipper.skipped)
            emit(dict(row, **extra))
    return modes


if "vqvae" in which:
    leg = bench.VqvaeLeg(dev, 1, 0, 0, 32, 2)
    time_leg("PR-DVQVAE2", leg, {"clips": 32, "frames": bench.CLIP_FRAMES})
    del leg
    torch.cuda.empty_cache()

if "dsfvt" in which:
    leg = bench.DsfvtLeg(dev, 1, 0, 0, 64, 2)
    modes = time_leg("DSFVT", leg, {"slices": 64})
    # ---- the two extra launches alone, on this model's gradients -------------------------------------------------------------
    from lvt_amd.utils.events import EventStorage
    ctx, sl, sidx, ign = leg.batches[0]
    with EventStorage(0):
        leg.model.compute_supervised_loss(ctx, sl, sidx, ign)["loss_cross_entropy"].backward()
    clipper = modes["norm"].clipper
    grads = clipper._gradients()
    nbytes = sum(g.numel() for g in grads) * 4
    for r in range(rounds):
        for _ in range(5): clipper.prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50): clipper.prepare()
        b.record(); torch.cuda.synchronize()
        ms = a.elapsed_time(b) / 50
        emit({"kind": "kernel", "kernel": "lvt_grad_sqnorm x %d + lvt_grad_clip_coef" % -(-len(grads) // 64), "config": "DSFVT",
              "tensors": len(grads), "round": r, "bytes": nbytes, "us": round(ms * 1e3, 2), "GBps": round(nbytes / ms / 1e6, 1)})

with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
