"""What finite scalar quantisation (MODEL.CODEBOOK.FSQ.LEVELS) costs and what it does to codebook usage, measured the
way tools/profile/cosine_codebook.py measures: same box, alternating rounds, one fresh process per arm and round.

    python tools/profile/fsq.py [--parent DIR] [--rounds 3] [--steps 30] [--out profiles/fsq.jsonl]

  1. the three kernels and the two projections alone at 131072 rows (the bench's PR-DVQVAE2 shape: 4 groups of [8, 8, 8], 12
     floats per row, DIM 256): us per launch and, for the kernels, bytes moved / time,
  2. the PR-DVQVAE2 train step at the bench shape (32 clips x 16 frames): (a) the tree at DIR (a checkout of the parent commit with
     its library built; skipped without --parent), (b) this tree with the key off, (c) this tree with EMA False and no FSQ (the
     trained-codebook route FSQ shares), (d) EMA False and LEVELS [8, 8, 8],
  3. codebook usage after the bench's 125 steps from the same seed with (d): the perplexity exp(-sum p log p) of the last pass's
     codes per code channel, computed here with torch on the device, and the codes that occur in it.  The figures to set it
     against are those of profiles/cosine_codebook.jsonl (same box-to-box caveat).

One JSON row per kernel, per arm and round, per usage arm, and a `verdict` row: (b) must not differ from (a) by more than the spread
of (a)'s own rounds; (c) and (d) are recorded, not gated.  Needs a GPU: there is no fallback, and the first arm that fails ends
the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CLIPS, NBATCHES = 32, 2
LEVELS = [8, 8, 8]
ARMS = {"a_parent": {}, "b_key_off": {}, "c_ema_false": {"EMA": False}, "d_fsq": {"EMA": False, "FSQ": LEVELS}}


def _leg(root, arm):
    sys.path.insert(0, root)
    import torch
    import bench
    import lvt_amd.modeling as M
    over, real = ARMS[arm], M.build_model

    def build_model(cfg):                                     # (the bench leg merges the YAML itself: override after it)
        if "EMA" in over:
            cfg.MODEL.CODEBOOK.EMA = over["EMA"]
        if "FSQ" in over:
            cfg.MODEL.CODEBOOK.FSQ.LEVELS = list(over["FSQ"])
        return real(cfg)
    M.build_model = build_model
    torch.cuda.set_device(0)
    return torch, bench, bench.VqvaeLeg("cuda:0", 1, 0, 0, CLIPS, NBATCHES)


def child_step(root, arm, steps):
    torch, bench, leg = _leg(root, arm)
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
                      "quantiser": type(leg.model.codebook).__name__, "device": torch.cuda.get_device_name(0)}))


def child_usage(arm, steps=125):
    torch, bench, leg = _leg(HERE, arm)
    for i in range(steps):
        losses = leg.step(i)
    torch.cuda.synchronize()
    idx = leg.model.codebook.last_indices                      # (N, num, h, w) of the last pass
    size = leg.cfg.MODEL.CODEBOOK.SIZE
    perplexity, used = [], []
    for i in range(idx.shape[1]):
        p = torch.bincount(idx[:, i].reshape(-1), minlength=size).double()
        p = p / p.sum()
        perplexity.append(float(torch.exp(-(p * torch.log(p.clamp_min(1e-300))).sum())))
        used.append(int((p > 0).sum()))
    print(json.dumps({"steps": steps, "size": size, "quantiser": type(leg.model.codebook).__name__,
                      "codebook_perplexity": [round(v, 3) for v in perplexity],
                      "codebook_perplexity_mean": round(statistics.mean(perplexity), 3), "codes_used_last_pass": used,
                      "loss_reconstruction_last": round(float(losses["loss_reconstruction"].detach()), 6),
                      "device": torch.cuda.get_device_name(0)}))


def child_kernels(calls=100, rounds=5):
    sys.path.insert(0, HERE)
    import torch
    from lvt_amd.hip import binding as L
    from lvt_amd.hip import fsq as K
    from lvt_amd.hip import gemm as G
    torch.cuda.set_device(0)
    rows, num, D = 131072, 4, 256
    wp = K.padded_width(num, LEVELS)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    z_e = torch.randn(rows, D, device="cuda:0", generator=gen)
    w_in = torch.randn(wp, D, device="cuda:0", generator=gen) / 16
    b_in = torch.zeros(wp, device="cuda:0")
    w_out = torch.randn(D, wp, device="cuda:0", generator=gen) / 4
    b_out = torch.zeros(D, device="cuda:0")
    z_p = torch.empty(rows, wp, device="cuda:0")
    out = torch.empty(rows, D, device="cuda:0")
    G.gemm(z_e, w_in, z_p, rows, wp, D, flags=L.EPI_BIAS, bias=b_in)
    g = torch.randn(rows, wp, device="cuda:0", generator=gen)
    z_q, idx = K.fsq_fwd(z_p, num, LEVELS, 256)
    f, i8 = rows * wp * 4, rows * num * 8
    ops = (("lvt_fsq_fwd", 2 * f + i8, lambda: K.fsq_fwd(z_p, num, LEVELS, 256)),
           ("lvt_fsq_fwd_idx_only", f + i8, lambda: K.fsq_fwd(z_p, num, LEVELS, 256, want_zq=False)),
           ("lvt_fsq_bwd", 3 * f, lambda: K.fsq_bwd(g, z_p, num, LEVELS)),
           ("lvt_fsq_decode", f + i8, lambda: K.fsq_decode(idx, LEVELS, wp)),
           ("proj_in_gemm", None, lambda: G.gemm(z_e, w_in, z_p, rows, wp, D, flags=L.EPI_BIAS, bias=b_in)),
           ("proj_out_gemm", None, lambda: G.gemm(z_q, w_out, out, rows, D, wp, flags=L.EPI_BIAS, bias=b_out)))
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
        row = {"kind": "kernel", "op": name, "shape": [rows, num, len(LEVELS)] if nbytes else [rows, wp, D], "calls": calls,
               "rounds": rounds, "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
               "device": torch.cuda.get_device_name(0), "abi": L.ABI_VERSION, "math": L.get_math_mode()}
        if nbytes:
            row.update({"bytes": nbytes, "TB_per_s": round(nbytes / (statistics.median(us) * 1e-6) / 1e12, 3)})
        print(json.dumps(row))


def run_child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit("fsq: %s ended with status %d; nothing more is started" % (" ".join(args), r.returncode))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "fsq.jsonl"))
    ap.add_argument("--child", nargs="*", default=None)
    a = ap.parse_args()
    if a.child is not None:
        if a.child[0] == "kernels":
            return child_kernels()
        if a.child[0] == "usage":
            return child_usage(a.child[1])
        return child_step(a.child[1], a.child[2], int(a.child[3]))
    rows = run_child(["--child", "kernels"], 300)
    for row in rows:
        print(row, flush=True)
    arms = [(name, HERE) for name in ("b_key_off", "c_ema_false", "d_fsq")]
    if a.parent:
        arms.insert(0, ("a_parent", os.path.abspath(a.parent)))
    for rnd in range(a.rounds):
        for name, root in arms:
            for row in run_child(["--child", "step", root, name, str(a.steps)], 600):
                rows.append(dict({"kind": "step", "arm": name, "round": rnd}, **row))
                print(rows[-1], flush=True)
    for name in ("c_ema_false", "d_fsq"):
        for row in run_child(["--child", "usage", name], 600):
            rows.append(dict({"kind": "usage", "arm": name}, **row))
            print(rows[-1], flush=True)
    free = {name: [r["free_ms"] for r in rows if r.get("arm") == name and r["kind"] == "step"] for name, _ in arms}
    med = {k: statistics.median(v) for k, v in free.items()}
    verdict = {"kind": "verdict", "free_ms_median": {k: round(v, 4) for k, v in med.items()},
               "d_minus_b_ms": round(med["d_fsq"] - med["b_key_off"], 4), "d_minus_c_ms": round(med["d_fsq"] - med["c_ema_false"], 4)}
    if a.parent:
        spread = max(free["a_parent"]) - min(free["a_parent"])
        verdict.update({"a_spread_ms": round(spread, 4), "b_minus_a_ms": round(med["b_key_off"] - med["a_parent"], 4),
                        "off_path_within_spread": abs(med["b_key_off"] - med["a_parent"]) <= spread})
    rows.append(verdict)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print(verdict)


if __name__ == "__main__":
    main()
