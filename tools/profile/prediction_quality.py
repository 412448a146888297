"""What the best-of-N comparison costs (csrc/quality.hip lvt_frame_quality_vs + lvt_prediction_select): microseconds per
clip of 16 x 3 x 64 x 64 frames with S = 10 and S = 100 sampled videos, for
  "ew.prediction_quality"          the broadcast compare in chunks of at most 512 frames, `finish` per chunk, one select launch; all
                                   on the device, nothing read on the host,
  "expanded target + host select"  what there was before: `ew.frame_quality` on the target expanded to S copies (the copy is part of the
                                   timed work), the (S T, 2) table read on the host and the selection rule evaluated there
                                   (`prediction_select_reference`),
  "expanded target, compare only"  the same without the host half: the copy and the two launches.
Median of `rounds` rounds; the device-only variants are `calls` back-to-back calls between two events, the one with a host half is
timed on the host clock around `calls` calls (each ends with a device-to-host copy, so it is synchronous).  Both variants are checked
to agree on `best` and, bit for bit, on the table before anything is timed.
python tools/profile/prediction_quality.py [calls] [rounds] [out.jsonl]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch
import test_gpu_prediction_quality as T
from lvt_amd.evaluation.quality import prediction_select_reference
from lvt_amd.hip import binding as L, ew

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "prediction_quality.jsonl")
torch.cuda.set_device(0)
base = {"device": torch.cuda.get_device_name(0), "abi": L.lib().lvt_version()}
rows = []
N_PRIME, RANGE = 14, 1.0


def emit(row):
    rows.append(dict(row, **base))
    print(rows[-1], flush=True)


def us_device(fn):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls): fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls * 1e3)
    return round(statistics.median(ts), 2), round(min(ts), 2), round(max(ts), 2)


def us_host(fn):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(calls): fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / calls * 1e6)
    return round(statistics.median(ts), 2), round(min(ts), 2), round(max(ts), 2)


for S in (10, 100):
    shape = (S, 16, 3, 64, 64, N_PRIME)
    samples, target, _ = T.make_clip(shape, RANGE)
    samples, target = samples.cuda(), target.cuda()
    curves = torch.zeros(16, 8, dtype=torch.float64, device="cuda")
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    table = torch.empty(S * 16, 2, dtype=torch.float64, device="cuda")

    def device_only():
        return ew.prediction_quality(samples, target, N_PRIME, RANGE, curves=curves)

    def expanded_compare():
        return ew.frame_quality(samples.flatten(0, 1), target.repeat(S, 1, 1, 1), RANGE, acc=acc, frames=table)

    def expanded_and_host():
        frames, _ = expanded_compare()
        t = frames.cpu().view(S, 16, 2)
        return frames, prediction_select_reference(t[..., 0], t[..., 1], N_PRIME)

    f1, b1, _ = device_only()
    f2, (b2, _) = expanded_and_host()
    assert torch.equal(f1.view(torch.int64), f2.view(torch.int64)) and b1.cpu().tolist() == b2.tolist()
    n = L.lib().lvt_frame_quality_partials(3, 64, 64)
    for name, timer, fn in (("ew.prediction_quality", us_device, device_only),
                            ("expanded target, compare only", us_device, expanded_compare),
                            ("expanded target + host select", us_host, expanded_and_host)):
        med, lo, hi = timer(fn)
        emit({"kind": "time", "op": name, "clock": "events" if timer is us_device else "host", "S": S, "shape": list(shape[:5]),
              "n_prime": N_PRIME, "frames": S * 16, "chunks": -(-S * 16 // 512) if name == "ew.prediction_quality" else 1,
              "workgroups": S * 16 * n, "target_bytes_copied": 0 if name == "ew.prediction_quality" else (S - 1) * target.numel() * 4,
              "calls": calls, "rounds": rounds, "us_median": med, "us_min": lo, "us_max": hi})

with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
