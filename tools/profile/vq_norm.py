"""Time batch-normalised VQ-VAE conv stacks (csrc/norm.hip, hip/convnet.py) on PR-DVQVAE2.

One JSON line per measurement:
  * "kernel": each norm kernel at the shapes of the normalised layers of a 512-frame batch (32 clips x 16 frames), HIP
    events around each call, median of --reps; bytes are what the kernel must move, from the shapes (stats: y read once;
    apply: y and res read, out written; bwd_reduce: g and y read; bwd_apply: g and y read, dy written);
  * "step": the train step (supervised forward + backward + optimizer step) at 32 clips x 16 frames with NORM "", "BN"
    and "SyncBN" (world size 1) in encoder and generator;
  * "eval": no-grad eval encode and decode of the same batch with NORM "" and "BN" (the BN pass runs the eval fold).

    python tools/profile/vq_norm.py [--clips 32] [--reps 20] [--warmup 5] [--out profiles/vq_norm_bn.jsonl]

The event times above include the host side of each wrapper call (allocation, ctypes, launch gaps).  Kernel-only figures
come from a trace, one shape per run:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o norm -- python tools/profile/vq_norm.py --only kernel --shape I
    python tools/profile/vq_norm.py --trace DIR/norm_kernel_trace.csv --shape I      # -> "kernel_trace" JSON lines

(profiles/vq_norm_bn_trace.jsonl: median duration of each launch, the entry point's time as the sum of its launches, and
bytes/s from the shapes).  Math mode: f16x2 (the default of the Python side).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from lvt_amd.hip import binding as L, norm as BN  # noqa: E402

DEV = "cuda:0"
# (rows per frame, channels) of the normalised layers of PR-DVQVAE2 at 64x64 frames: encoder 32x32x128, 16x16x256 (x2),
# ResBlock 16x16x128 / 16x16x256; decoder 16x16x256, ResBlock 16x16x128 / 16x16x256, ConvT 32x32x128
SHAPES = [(32 * 32, 128), (16 * 16, 256), (16 * 16, 128)]


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def kernels(frames, reps, warmup, shapes=SHAPES):
    out = []
    for hw, C in shapes:
        M = frames * hw
        g = torch.Generator(device=DEV).manual_seed(M + C)
        y = torch.randn(M, C, device=DEV, generator=g)
        res = torch.randn(M, C, device=DEV, generator=g)
        gr = torch.randn(M, C, device=DEV, generator=g)
        one = torch.ones(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        st = BN.stats(y)
        sc, sh, sv = BN.finalize(C, C, one, one, rm, rv, stats=st, count=M, flags=0)
        sums = BN.bwd_reduce(gr, y, sv)
        act = 4 * M * C
        rows = {
            "stats": (lambda: BN.stats(y), act),
            "finalize": (lambda: BN.finalize(C, C, one, one, rm, rv, stats=st, count=M, flags=L.BN_UPDATE), 4 * 8 * C),
            "apply_res_relu": (lambda: BN.apply(y, sc, sh, res=res, act=L.EPI_RELU), 3 * act),
            "bwd_reduce": (lambda: BN.bwd_reduce(gr, y, sv), 2 * act),
            "bwd_apply": (lambda: BN.bwd_apply(gr, y, sc, sv, sums, n=M), 3 * act),
        }
        for name, (fn, nbytes) in rows.items():
            us = _time(fn, reps, warmup)
            out.append({"kind": "kernel", "kernel": name, "rows": M, "C": C, "us": round(us, 1), "bytes": nbytes,
                        "tb_per_s": round(nbytes / (us * 1e-6) / 1e12, 2)})
    return out


# launches of each entry point (csrc/norm.hip) and the bytes the entry must move per (M, C) activation
ENTRIES = {"stats": (("lvt_bn_stats_partial_kernel", "lvt_bn_stats_combine_kernel"), 1),
           "finalize": (("lvt_bn_finalize_kernel",), 0),
           "apply_res_relu": (("lvt_bn_apply_kernel",), 3),
           "bwd_reduce": (("lvt_bn_bwd_partial_kernel", "lvt_bn_bwd_combine_kernel"), 2),
           "bwd_apply": (("lvt_bn_bwd_apply_kernel",), 3)}


def trace_rows(path, frames, shape):
    """Per-launch median durations of a rocprofv3 kernel trace of `--only kernel --shape I` -> one row per entry point."""
    import csv
    import re
    hw, C = shape
    M = frames * hw
    dur = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r"lvt_bn_\w+_kernel", r["Kernel_Name"])
            if m is None:
                continue
            dur.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for entry, (launches, per_act) in ENTRIES.items():
        us = {k: round(statistics.median(dur[k]), 1) for k in launches}
        total = sum(us.values())
        row = {"kind": "kernel_trace", "kernel": entry, "rows": M, "C": C, "us": round(total, 1), "launch_us": us}
        if per_act:
            row["bytes"] = per_act * 4 * M * C
            row["tb_per_s"] = round(row["bytes"] / (total * 1e-6) / 1e12, 2)
        out.append(row)
    return out


def _model(norm):
    from lvt_amd.modeling import build_model
    from util_models import vqvae_cfg
    cfg = vqvae_cfg(DEV)
    cfg.MODEL.ENCODER.NORM = cfg.MODEL.GENERATOR.NORM = norm
    torch.manual_seed(11)
    return build_model(cfg)


def step_and_eval(clips, reps, warmup, norms):
    from lvt_amd.utils.events import EventStorage
    out = []
    g = torch.Generator().manual_seed(5)
    x = torch.rand(clips, 16, 3, 64, 64, generator=g).to(DEV)
    data = [{"image_sequence": x[j]} for j in range(clips)]
    for norm in norms:
        model = _model(norm)
        model.train()
        opts, _ = model.configure_optimizers_and_checkpointers()

        def step():
            with EventStorage(0):
                ls = model(data, mode="supervised")
            sum(ls.values()).backward()
            for o in opts:
                o["optimizer"].step()
            for o in opts:
                o["optimizer"].zero_grad()
        ms = _time(step, reps, warmup) / 1e3
        out.append({"kind": "step", "norm": norm, "clips": clips, "frames": clips * 16, "ms": round(ms, 2)})
        if norm == "SyncBN":
            continue
        model.eval()
        frames = x.view(-1, 3, 64, 64)
        with torch.no_grad():
            z = model.encode(frames)
            enc_ms = _time(lambda: model.encode(frames), reps, warmup) / 1e3
            dec_ms = _time(lambda: model.decode(z), reps, warmup) / 1e3
        out.append({"kind": "eval", "norm": norm, "frames": clips * 16, "encode_ms": round(enc_ms, 2),
                    "decode_ms": round(dec_ms, 2)})
        del model, opts
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["kernel", "model"], default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: time / summarise that shape only")
    ap.add_argument("--trace", default=None, help="summarise a rocprofv3 kernel_trace.csv of `--only kernel --shape I`")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    shapes = SHAPES if a.shape is None else [SHAPES[a.shape]]
    if a.trace:
        rows += trace_rows(a.trace, a.clips * 16, shapes[0])
    elif a.only in (None, "kernel"):
        rows += kernels(a.clips * 16, a.reps, a.warmup, shapes)
    if not a.trace and a.only in (None, "model"):
        rows += step_and_eval(a.clips, a.reps, a.warmup, ["", "BN", "SyncBN"])
    for r in rows:
        r["math"] = L.get_math_mode()
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
