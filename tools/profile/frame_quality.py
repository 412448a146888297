"""What the frame-quality kernel costs and how accurate it is (csrc/quality.hip).
  kind "time":     microseconds per `ew.frame_quality` call (both launches) for a 16 x 3 x 64 x 64 clip and for one 3 x 128 x 128 frame,
                   and `ew.mse_fwd` on the same tensors, what the evaluator cost per clip before (median of `rounds` rounds of
                   `calls` back-to-back calls between two events, after a warm-up).
  kind "accuracy": per input class and data range, over the shapes of tests/test_gpu_frame_quality.py: the largest per-frame
                   |kernel - fp64| of SSIM and PSNR, the largest error e of the pivoted fp32 CPU restatement, and whether every frame
                   met the test's bounds.  Input classes, shapes, the restatement and the bounds are the test file's own, imported
                   from it, so the table is about exactly what the suite asserts.
python tools/profile/frame_quality.py [calls] [rounds] [out.jsonl]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch
import test_gpu_frame_quality as T
from lvt_amd.hip import binding as L, ew

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "frame_quality.jsonl")
torch.cuda.set_device(0)
base = {"device": torch.cuda.get_device_name(0), "abi": L.lib().lvt_version()}
rows = []


def emit(row):
    rows.append(dict(row, **base))
    print(rows[-1], flush=True)


def us_per_call(fn):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls): fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls * 1e3)
    return round(statistics.median(ts), 2), round(min(ts), 2), round(max(ts), 2)


for shape in ((16, 3, 64, 64), (1, 3, 128, 128)):
    a, b = (t.cuda() for t in T.make_pair("noised_copy", shape, 1.0))
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    frames = torch.empty(shape[0], 2, dtype=torch.float64, device="cuda")
    nbytes = 2 * a.numel() * 4
    for name, fn in (("ew.frame_quality", lambda: ew.frame_quality(a, b, 1.0, acc=acc, frames=frames)),
                     ("ew.mse_fwd", lambda: ew.mse_fwd(a, b, denom=1.0))):
        med, lo, hi = us_per_call(fn)
        emit({"kind": "time", "op": name, "shape": list(shape), "bytes_read": nbytes, "calls": calls, "rounds": rounds,
              "us_median": med, "us_min": lo, "us_max": hi,
              "workgroups": shape[0] * L.lib().lvt_frame_quality_partials(*shape[1:]) if name == "ew.frame_quality" else None})

for kind in T.CLASSES:
    for rng in T.RANGES:
        worst = [0.0, 0.0, 0.0]
        ok = True
        for shape in T.SHAPES:
            d_ssim, e, d_psnr, inside = T.kernel_errors(kind, shape, rng)
            worst = [max(worst[0], d_ssim), max(worst[1], e), max(worst[2], d_psnr)]
            ok = ok and inside
        emit({"kind": "accuracy", "class": kind, "data_range": rng, "shapes": [list(s) for s in T.SHAPES],
              "ssim_err_max": worst[0], "fp32_pivoted_cpu_err_max": worst[1], "ssim_floor": T.SSIM_FLOOR,
              "psnr_err_db_max": worst[2], "within_bounds": ok})

with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
