"""What the residual dropout of the video transformer costs, measured the way tools/profile/leg_time.py measures a
bench leg: same box, alternating rounds, one fresh process per arm and round.

    python tools/profile/vt_dropout.py [--parent DIR] [--rounds 3] [--steps 30] [--out profiles/vt_dropout.jsonl]

  (a) the DSFVT train step of the tree at DIR (a checkout of the parent commit with its library built; skipped without --parent),
  (b) the DSFVT train step here with MODEL.AUTOREGRESSIVE.VT.DROPOUT 0.0,
  (c) the same with DROPOUT 0.1,
  and the two kernels alone at 16384 x 512 with bytes moved / time (add: 3 streams, bwd: 2).

One JSON row per arm and round, one per kernel, and a `verdict` row: (b) must not differ from (a) by more than the spread of (a)'s
own rounds; (c) is recorded, not gated.  Needs a GPU: there is no fallback, and the first arm that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child_step(root, dropout, steps):
    sys.path.insert(0, root)
    import torch
    import bench
    if dropout > 0:
        from lvt_amd.config import defaults
        defaults._C.MODEL.AUTOREGRESSIVE.VT.DROPOUT = dropout          # (the bench leg builds its config from the defaults)
    torch.cuda.set_device(0)
    leg = bench.DsfvtLeg("cuda:0", 1, 0, 0, 64, 4)
    for i in range(5):
        leg.step(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); leg.step(5 + i); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(steps):
        leg.step(5 + steps + i)
    torch.cuda.synchronize()
    free = (time.perf_counter() - t0) / steps * 1e3
    ts.sort()
    print(json.dumps({"free_ms": round(free, 4), "median_ms": round(statistics.median(ts), 4), "p10_ms": round(ts[len(ts) // 10], 4),
                      "p90_ms": round(ts[-len(ts) // 10 - 1], 4), "steps": steps, "device": torch.cuda.get_device_name(0)}))


def child_kernels(calls=100, rounds=5):
    sys.path.insert(0, HERE)
    import torch
    from lvt_amd.hip import binding as L
    from lvt_amd.hip import dropout as D
    torch.cuda.set_device(0)
    M, d = 16384, 512
    g = torch.Generator(device="cuda:0").manual_seed(1)
    z, r = torch.randn(M, d, device="cuda:0", generator=g), torch.randn(M, d, device="cuda:0", generator=g)
    st = (0x1234567, D.site_rank(3, 1), 0)
    ops = (("lvt_dropout_add", 3, lambda: D.dropout_add(z, r, st, 0.1)), ("lvt_dropout_bwd", 2, lambda: D.dropout_bwd(z, st, 0.1)))
    for name, streams, fn in ops:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record(); torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / calls)
        nbytes = streams * M * d * 4
        print(json.dumps({"kind": "kernel", "op": name, "shape": [M, d], "p": 0.1, "calls": calls, "rounds": rounds,
                          "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                          "bytes": nbytes, "TB_per_s": round(nbytes / (statistics.median(us) * 1e-6) / 1e12, 3),
                          "device": torch.cuda.get_device_name(0), "abi": L.ABI_VERSION, "math": L.get_math_mode()}))


def run_child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit("vt_dropout: %s ended with status %d; nothing more is started" % (" ".join(args), r.returncode))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "vt_dropout.jsonl"))
    ap.add_argument("--child", nargs="*", default=None)
    a = ap.parse_args()
    if a.child is not None:
        if a.child[0] == "kernels":
            return child_kernels()
        return child_step(a.child[1], float(a.child[2]), int(a.child[3]))
    arms = [("b_dropout_0.0", HERE, 0.0), ("c_dropout_0.1", HERE, 0.1)]
    if a.parent:
        arms.insert(0, ("a_parent", os.path.abspath(a.parent), 0.0))
    rows = []
    for rnd in range(a.rounds):
        for name, root, p in arms:
            for row in run_child(["--child", "step", root, str(p), str(a.steps)], 600):
                rows.append(dict({"kind": "step", "arm": name, "round": rnd}, **row))
                print(rows[-1], flush=True)
    rows += run_child(["--child", "kernels"], 300)
    free = {name: [r["free_ms"] for r in rows if r.get("arm") == name] for name, _, _ in arms}
    mean = {k: sum(v) / len(v) for k, v in free.items()}
    verdict = {"kind": "verdict", "free_ms_mean": {k: round(v, 4) for k, v in mean.items()},
               "c_minus_b_ms": round(mean["c_dropout_0.1"] - mean["b_dropout_0.0"], 4)}
    if a.parent:
        spread = max(free["a_parent"]) - min(free["a_parent"])
        verdict.update({"a_spread_ms": round(spread, 4), "b_minus_a_ms": round(mean["b_dropout_0.0"] - mean["a_parent"], 4),
                        "off_path_within_spread": abs(mean["b_dropout_0.0"] - mean["a_parent"]) <= spread})
    rows.append(verdict)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print(verdict)


if __name__ == "__main__":
    main()
