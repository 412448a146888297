"""What the cosine codebook lookup (MODEL.CODEBOOK.COSINE) costs and what it does to codebook usage, measured the way
tools/profile/vt_dropout.py measures: same box, alternating rounds, one fresh process per arm and round.

    python tools/profile/cosine_codebook.py [--parent DIR] [--rounds 3] [--steps 30] [--out profiles/cosine_codebook.jsonl]

  1. the two kernels alone at 131072 x 4 x 64 (the bench's PR-DVQVAE2 shape) and at 512 x 4 x 64: us per launch and bytes moved /
     time (fwd: x, y and inv; bwd: g, y, inv and dx),
  2. the PR-DVQVAE2 train step at the bench shape (32 clips x 16 frames): (a) the tree at DIR (a checkout of the parent commit with
     its library built; skipped without --parent), (b) this tree with the key off, (c) with it on,
  3. codebook usage after the bench's 125 steps from the same seed: key off, key on, key on with RESTART THRESHOLD 1.0 -- the
     perplexity of the health record (off and on run restart in monitoring mode, THRESHOLD 0, which changes no bit of the step),
     the codes that won a row in the last pass and the codes whose running_size is below 1.

One JSON row per kernel, per arm and round, per usage arm, and a `verdict` row: (b) must not differ from (a) by more than the spread
of (a)'s own rounds; (c) is recorded as a difference, not gated.  Needs a GPU: there is no fallback, and the first arm that fails
ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CLIPS, NBATCHES = 32, 2


def _leg(root, cosine):
    sys.path.insert(0, root)
    import torch
    import bench
    if cosine:
        from lvt_amd.config import defaults
        defaults._C.MODEL.CODEBOOK.COSINE = True              # (the bench leg builds its config from the defaults)
    torch.cuda.set_device(0)
    return torch, bench, bench.VqvaeLeg("cuda:0", 1, 0, 0, CLIPS, NBATCHES)


def child_step(root, cosine, steps):
    torch, bench, leg = _leg(root, cosine)
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
                      "p90_ms": round(ts[-len(ts) // 10 - 1], 4), "steps": steps, "clips": CLIPS, "frames": bench.CLIP_FRAMES,
                      "device": torch.cuda.get_device_name(0)}))


def child_usage(cosine, threshold, steps=125):
    torch, bench, leg = _leg(HERE, cosine)
    q = leg.model.codebook
    q.enable_restart(threshold, 0)
    for i in range(steps):
        leg.step(i)
    torch.cuda.synchronize()
    perplexity, _, restarts = (float(v) for v in leg.model.codebook_health())
    idx = q.last_indices
    used = [int(torch.unique(idx[:, i]).numel()) for i in range(idx.shape[1])]
    low = [int((v.running_size < 1.0).sum()) for v in q.ve]
    w = torch.stack([v.embedding.weight.data for v in q.ve])
    print(json.dumps({"steps": steps, "cosine": bool(cosine), "restart_threshold": threshold, "size": q.K,
                      "codebook_perplexity_mean": round(perplexity, 3), "codes_used_last_pass": used,
                      "codes_running_size_below_1": low, "restarts_total": restarts,
                      "code_norm_min": round(float(w.norm(dim=-1).min()), 6), "code_norm_max": round(float(w.norm(dim=-1).max()), 6),
                      "device": torch.cuda.get_device_name(0)}))


def child_kernels(calls=100, rounds=5):
    sys.path.insert(0, HERE)
    import torch
    from lvt_amd.hip import binding as L
    from lvt_amd.hip import l2norm
    torch.cuda.set_device(0)
    G, d = 4, 64
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    for rows in (131072, 512):
        x = torch.randn(rows, G * d, device="cuda:0", generator=gen)
        g = torch.randn(rows, G * d, device="cuda:0", generator=gen)
        y, inv = l2norm.l2norm_groups_fwd(x, d)
        elems, groups = rows * G * d * 4, rows * G * 4
        ops = (("lvt_l2norm_groups_fwd", 2 * elems + groups, lambda: l2norm.l2norm_groups_fwd(x, d)),
               ("lvt_l2norm_groups_bwd", 3 * elems + groups, lambda: l2norm.l2norm_groups_bwd(g, y, inv, d)))
        for name, nbytes, fn in ops:
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
            print(json.dumps({"kind": "kernel", "op": name, "shape": [rows, G, d], "calls": calls, "rounds": rounds,
                              "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                              "bytes": nbytes, "TB_per_s": round(nbytes / (statistics.median(us) * 1e-6) / 1e12, 3),
                              "device": torch.cuda.get_device_name(0), "abi": L.ABI_VERSION, "math": L.get_math_mode()}))


def run_child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit("cosine_codebook: %s ended with status %d; nothing more is started" % (" ".join(args), r.returncode))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "cosine_codebook.jsonl"))
    ap.add_argument("--child", nargs="*", default=None)
    a = ap.parse_args()
    if a.child is not None:
        if a.child[0] == "kernels":
            return child_kernels()
        if a.child[0] == "usage":
            return child_usage(int(a.child[1]), float(a.child[2]))
        return child_step(a.child[1], int(a.child[2]), int(a.child[3]))
    rows = run_child(["--child", "kernels"], 300)
    for row in rows:
        print(row, flush=True)
    arms = [("b_cosine_off", HERE, 0), ("c_cosine_on", HERE, 1)]
    if a.parent:
        arms.insert(0, ("a_parent", os.path.abspath(a.parent), 0))
    for rnd in range(a.rounds):
        for name, root, cosine in arms:
            for row in run_child(["--child", "step", root, str(cosine), str(a.steps)], 600):
                rows.append(dict({"kind": "step", "arm": name, "round": rnd}, **row))
                print(rows[-1], flush=True)
    for name, cosine, thr in (("off", 0, 0.0), ("on", 1, 0.0), ("on_restart", 1, 1.0)):
        for row in run_child(["--child", "usage", str(cosine), str(thr)], 600):
            rows.append(dict({"kind": "usage", "arm": name}, **row))
            print(rows[-1], flush=True)
    free = {name: [r["free_ms"] for r in rows if r.get("arm") == name and r["kind"] == "step"] for name, _, _ in arms}
    med = {k: statistics.median(v) for k, v in free.items()}
    verdict = {"kind": "verdict", "free_ms_median": {k: round(v, 4) for k, v in med.items()},
               "c_minus_b_ms": round(med["c_cosine_on"] - med["b_cosine_off"], 4)}
    if a.parent:
        spread = max(free["a_parent"]) - min(free["a_parent"])
        verdict.update({"a_spread_ms": round(spread, 4), "b_minus_a_ms": round(med["b_cosine_off"] - med["a_parent"], 4),
                        "off_path_within_spread": abs(med["b_cosine_off"] - med["a_parent"]) <= spread})
    rows.append(verdict)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print(verdict)


if __name__ == "__main__":
    main()
