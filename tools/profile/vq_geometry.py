"""Time the quantiser kernels per codebook geometry: search, gather, EMA accumulate and EMA finalize at 131,072 rows
(512 frames x 16 x 16), HIP events around each call, warm-up then the median of --reps calls.  One JSON line per geometry:
microseconds, algorithmic TFLOP/s of the search (2 rows NUM K Dg / t) and the bytes each kernel moves (algorithmic: z read
once, indices written / read once, codebooks read once, outputs written once).

    python tools/profile/vq_geometry.py [--rows 131072] [--reps 20] [--warmup 5]

The (4, 64, 512) geometry is timed twice: on its specialised kernels and with the search forced onto the generic kernel
(LVT_VQ_GENERIC).  Math mode: f16x2 (the default of the Python side).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lvt_amd.hip import binding as L, vq  # noqa: E402

GEOMETRIES = [(4, 64, 512, False), (4, 64, 512, True), (8, 32, 1024, False), (2, 128, 256, False), (4, 64, 2048, False),
              (1, 256, 1024, False)]


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


def run(num, dg, K, generic, rows, reps, warmup):
    """num == 1: SingleVQEmbedding's route (search = engine GEMM + lvt_vq_argmax_scores; gather / EMA on Dg / 64 groups of 64)."""
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(num * dg * K)
    D = num * dg
    P = 256
    z = torch.randn(rows, D, device=dev, generator=g)
    if num == 1:
        w = torch.randn(K, dg, device=dev, generator=g)
        groups = dg // 64
        wg = w.view(K, groups, 64).permute(1, 0, 2).contiguous()
        search = lambda: vq.nearest_single(z, w)                                        # noqa: E731
        idx = search()
        idx_g = idx.view(-1, 1, P).expand(-1, groups, P).contiguous()
        cbs, kgroups, kdg = wg, groups, 64
    else:
        cbs = torch.randn(num, K, dg, device=dev, generator=g)
        search = lambda: vq.nearest(z, cbs, P, generic=generic)                          # noqa: E731
        idx_g = search()
        kgroups, kdg = num, dg
    t_search = _time(search, reps, warmup)
    t_gather = _time(lambda: vq.gather(idx_g, cbs), reps, warmup)
    t_acc = _time(lambda: vq.ema_accumulate(idx_g, z, K), reps, warmup)
    stats = vq.ema_accumulate(idx_g, z, K)
    rs = torch.rand(kgroups, K, device=dev, generator=g) + 0.5
    rsum = cbs.clone()
    w2 = cbs.clone()
    t_fin = _time(lambda: vq.ema_finalize(stats, rs, rsum, w2), reps, warmup)
    flops = 2.0 * rows * num * K * dg
    cb_bytes = 4 * num * K * dg
    return {
        "geometry": {"NUM": num, "Dg": dg, "K": K, "rows": rows, "forced_generic": generic},
        "search": {"us": round(t_search, 1), "tflops": round(flops / (t_search * 1e-6) / 1e12, 1),
                   "bytes": 4 * rows * D + 8 * rows * (1 if num == 1 else num) + cb_bytes},
        "gather": {"us": round(t_gather, 1), "bytes": 8 * rows * kgroups + 4 * rows * D + cb_bytes},
        "ema_accumulate": {"us": round(t_acc, 1), "bytes": 8 * rows * kgroups + 4 * rows * D + 4 * kgroups * K * (kdg + 1)},
        "ema_finalize": {"us": round(t_fin, 1), "bytes": 4 * kgroups * K * (kdg + 1) + 4 * kgroups * K * 2 + 4 * 3 * kgroups * K * kdg},
        "math": L.get_math_mode(),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512 * 16 * 16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for num, dg, K, generic in GEOMETRIES:
        print(json.dumps(run(num, dg, K, generic, a.rows, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
