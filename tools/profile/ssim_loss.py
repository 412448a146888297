"""What the SSIM loss term costs and how accurate its kernel is (csrc/ssim_loss.hip, LOSS.SSIM.LAMBDA).
  kind "time":     microseconds per `ew.ssim_loss_fwd` call (both launches), with and without the gradient buffer, and per merged
                   backward launch (`ew.mse_bwd` with and without the second operand pair) at (512, 3, 64, 64) and (16, 3, 64, 64)
                   (median of `rounds` rounds of `calls` back-to-back calls between two events, after a warm-up).
  kind "step":     the PR-DVQVAE2 train step of bench.py (32 clips x 16 frames) with LAMBDA 0 and 0.5 on one box, the method of
                   tools/profile/leg_time.py: per-step synchronised median and free-running mean, in ms.
  kind "accuracy": per input class of tests/test_gpu_ssim_loss.py at (2, 3, 64, 64): the kernel's gradient and loss errors against
                   fp64 autograd of the plain-torch rule, next to those of fp32 torch autograd (err_t, the suite's yardstick).  Input
                   classes and references are the test file's own, imported from it.
python tools/profile/ssim_loss.py [calls] [rounds] [steps] [out.jsonl]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch
import bench
import test_gpu_ssim_loss as T
from lvt_amd.hip import binding as L, ew
from lvt_amd.modeling.loss import ReconstructionLoss

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "ssim_loss.jsonl")
torch.cuda.set_device(0)
base = {"device": torch.cuda.get_device_name(0), "abi": L.lib().lvt_version(), "math": L.get_math_mode()}
rows = []


def emit(row):
    rows.append(dict(row, **base))
    print(rows[-1], flush=True)


def us_per_call(fn):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls): fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls * 1e3)
    return round(statistics.median(ts), 2), round(min(ts), 2), round(max(ts), 2)


mean, std = torch.tensor([0.5] * 3, device="cuda"), torch.tensor([0.5] * 3, device="cuda")
one = torch.ones(1, device="cuda")
for shape in ((512, 3, 64, 64), (16, 3, 64, 64)):
    g = torch.Generator().manual_seed(0)
    x = T.to_cl(torch.rand(shape, generator=g) * 2 - 1)
    xt = T.to_cl(torch.rand(shape, generator=g) * 2 - 1)
    G = ew.ssim_loss_fwd(xt, x, mean, std, 1.0, 0.5, want_grad=True)[1]
    denom = float(x.numel() // 4 * 3)
    for name, fn in (("ew.ssim_loss_fwd with gradient", lambda: ew.ssim_loss_fwd(xt, x, mean, std, 1.0, 0.5, want_grad=True)),
                     ("ew.ssim_loss_fwd forward only", lambda: ew.ssim_loss_fwd(xt, x, mean, std, 1.0, 0.5)),
                     ("ew.mse_fwd", lambda: ew.mse_fwd(xt, x, denom)),
                     ("ew.mse_bwd", lambda: ew.mse_bwd(xt, x, denom, gout=one)),
                     ("ew.mse_bwd plus", lambda: ew.mse_bwd(xt, x, denom, gout=one, g_plus=one, plus=G))):
        med, lo, hi = us_per_call(fn)
        emit({"kind": "time", "op": name, "shape": list(shape), "calls": calls, "rounds": rounds, "us_median": med, "us_min": lo,
              "us_max": hi, "workgroups": L.lib().lvt_ssim_loss_partials(shape[0], 64, 64, 4) if "ssim" in name else None})
    del x, xt, G

for lam in (0.0, 0.5):
    leg = bench.VqvaeLeg("cuda:0", 1, 0, 0, 32, 4)
    cfg = leg.cfg.clone()
    cfg.defrost()
    cfg.LOSS.SSIM.LAMBDA = lam
    leg.model.reconstruction_loss = ReconstructionLoss(cfg)
    leg.model.pixel_loss = leg.model.reconstruction_loss.pixel_loss
    for i in range(5): leg.step(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); losses = leg.step(5 + i); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(steps): leg.step(5 + steps + i)
    torch.cuda.synchronize(); free = (time.perf_counter() - t0) / steps * 1e3
    emit({"kind": "step", "leg": "PR-DVQVAE2 32 x 16 frames", "LOSS.SSIM.LAMBDA": lam, "steps": steps, "ms_median_synchronised": round(statistics.median(ts), 3),
          "ms_free_running": round(free, 3), "losses": sorted(losses)})
    del leg

for cls in T.CLASSES:
    ref = T.reference(cls, T.SHAPES[-1])
    loss, G = T.run_kernel(ref)
    g64 = ref["g64"]
    scale = float(g64.abs().max())
    if cls == "equal":
        emit({"kind": "accuracy", "class": cls, "shape": list(T.SHAPES[-1]), "loss": float(loss), "max_abs_G": float(G.abs().max()),
              "max_abs_g_fp32_torch": float(ref["g32"].abs().max()), "max_abs_g_fp64": scale})
        continue
    emit({"kind": "accuracy", "class": cls, "shape": list(T.SHAPES[-1]), "loss_fp64": ref["l64"], "max_abs_g_fp64": scale,
          "err_kernel": float((T.from_cl(G, 3).double() - g64).abs().max()) / scale,
          "err_t": float((ref["g32"].double() - g64).abs().max()) / scale,
          "loss_err_kernel": abs(float(loss) - ref["l64"]), "loss_err_t": abs(ref["l32"] - ref["l64"])})

with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
