"""What truncated sampling costs, measured the way tools/profile/vt_dropout.py measures: same box, alternating
rounds, one fresh process per generation arm and round.

    python tools/profile/truncated_sampling.py [--parent DIR] [--rounds 3] [--videos 256] [--out profiles/truncated_sampling.jsonl]

  kernels: lvt_sample_categorical against lvt_sample_truncated at rows = 256, V = 512 and V = 2048, with truncation off
           (top_k 0, top_p 1), top_k = 8, top_p = 0.9 and both -- the five launches alternate inside every round;
  (a) generation frames/s of the seeded DSFVT at `--videos` clips, 5 priming frames, in the tree at DIR (a checkout of the parent
      commit with its library built; skipped without --parent),
  (b) the same here with truncation off,
  (c) the same here with top_k = 8, top_p = 0.9.

One JSON row per kernel form and per arm and round, and a `verdict` row: (b) must not differ from (a) by more than the spread of
(a)'s own rounds -- the same launches are issued; (c) is recorded, not gated.  Needs a GPU: there is no fallback, and the first
arm that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N_PRIME = 5


def child_gen(root, top_k, top_p, videos, reps):
    sys.path[:0] = [root, os.path.join(root, "tests", "golden")]
    import torch
    import seeded
    from lvt_amd.config import get_cfg
    from lvt_amd.modeling import build_model
    torch.cuda.set_device(0)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(root, "configs/vt/DSFVT.yaml"))
    cfg.MODEL.DEVICE = "cuda:0"
    cfg.OUTPUT_DIR = "/tmp/lvt_truncated_sampling"
    model = build_model(cfg)
    model.model.load_state_dict(seeded.seeded_params(seeded.dsfvt_shapes(), 4321), strict=False)
    model.eval()
    kw = {} if (top_k == 0 and top_p == 1.0) else {"top_k": top_k, "top_p": top_p}      # (the parent has no such arguments)
    video = torch.randint(0, 512, (videos, 4, 16, 16, 16), generator=torch.Generator().manual_seed(3)).to("cuda:0")
    torch.manual_seed(9)
    with torch.no_grad():
        model.sample_video(video, n_prime=15, **kw)              # builds the samplers, captures the graphs
        torch.cuda.synchronize()
        fps = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = model.sample_video(video, n_prime=N_PRIME, **kw)
            torch.cuda.synchronize()
            fps.append(videos * (16 - N_PRIME) / (time.perf_counter() - t0))
    print(json.dumps({"frames_per_s": round(statistics.median(fps), 2), "frames_per_s_all": [round(f, 2) for f in fps],
                      "videos": videos, "n_prime": N_PRIME, "checksum": int(out.sum()), "device": torch.cuda.get_device_name(0)}))


def child_kernels(rounds, calls=200):
    sys.path.insert(0, HERE)
    import torch
    from lvt_amd.hip import binding as L
    from lvt_amd.hip import tx
    torch.cuda.set_device(0)
    rows = 256
    g = torch.Generator().manual_seed(11)
    for V in (512, 2048):
        logits = (torch.randn(rows, V, generator=g) * 3).to("cuda:0")
        u = torch.rand(rows, generator=g).to("cuda:0")
        out = torch.empty(rows, dtype=torch.int64, device="cuda:0")
        forms = [("lvt_sample_categorical", 0, 1.0, lambda: tx.sample_categorical(logits, 0.9, u, out)),
                 ("lvt_sample_truncated", 0, 1.0, lambda: tx.sample_truncated(logits, 0.9, 0, 1.0, u, out)),
                 ("lvt_sample_truncated", 8, 1.0, lambda: tx.sample_truncated(logits, 0.9, 8, 1.0, u, out)),
                 ("lvt_sample_truncated", 0, 0.9, lambda: tx.sample_truncated(logits, 0.9, 0, 0.9, u, out)),
                 ("lvt_sample_truncated", 8, 0.9, lambda: tx.sample_truncated(logits, 0.9, 8, 0.9, u, out))]
        for _, _, _, fn in forms:
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        us = [[] for _ in forms]
        for _ in range(rounds):
            for i, (_, _, _, fn) in enumerate(forms):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    fn()
                b.record(); torch.cuda.synchronize()
                us[i].append(a.elapsed_time(b) * 1e3 / calls)
        for (name, k, p, _), t in zip(forms, us):
            print(json.dumps({"kind": "kernel", "op": name, "rows": rows, "V": V, "top_k": k, "top_p": p, "calls": calls,
                              "rounds": rounds, "us_per_call_median": round(statistics.median(t), 2), "us_min": round(min(t), 2),
                              "us_max": round(max(t), 2), "note": "back-to-back launches on one stream: launch rate included",
                              "device": torch.cuda.get_device_name(0), "abi": L.ABI_VERSION}))


def run_child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit("truncated_sampling: %s ended with status %d; nothing more is started" % (" ".join(args), r.returncode))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--videos", type=int, default=256)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "truncated_sampling.jsonl"))
    ap.add_argument("--child", nargs="*", default=None)
    a = ap.parse_args()
    if a.child is not None:
        if a.child[0] == "kernels":
            return child_kernels(int(a.child[1]))
        return child_gen(a.child[1], int(a.child[2]), float(a.child[3]), int(a.child[4]), int(a.child[5]))
    arms = [("b_off", HERE, 0, 1.0), ("c_top_k_8_top_p_0.9", HERE, 8, 0.9)]
    if a.parent:
        arms.insert(0, ("a_parent", os.path.abspath(a.parent), 0, 1.0))
    rows = run_child(["--child", "kernels", str(max(a.rounds, 5))], 300)
    for r in rows:
        print(r, flush=True)
    for rnd in range(a.rounds):
        for name, root, k, p in arms:
            for row in run_child(["--child", "gen", root, str(k), str(p), str(a.videos), str(a.reps)], 600):
                rows.append(dict({"kind": "generation", "arm": name, "round": rnd, "top_k": k, "top_p": p}, **row))
                print(rows[-1], flush=True)
    fps = {name: [r["frames_per_s"] for r in rows if r.get("arm") == name] for name, _, _, _ in arms}
    mean = {k: sum(v) / len(v) for k, v in fps.items()}
    verdict = {"kind": "verdict", "frames_per_s_mean": {k: round(v, 2) for k, v in mean.items()},
               "c_over_b": round(mean["c_top_k_8_top_p_0.9"] / mean["b_off"], 4)}
    if a.parent:
        spread = max(fps["a_parent"]) - min(fps["a_parent"])
        verdict.update({"a_spread_frames_per_s": round(spread, 2), "b_minus_a_frames_per_s": round(mean["b_off"] - mean["a_parent"], 2),
                        "off_path_within_spread": abs(mean["b_off"] - mean["a_parent"]) <= spread})
    rows.append(verdict)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print(verdict)


if __name__ == "__main__":
    main()
