"""ConvEncoder / ConvDecoder (config (a) of fixture G28: NF 32, N_LAYERS 2, 256 latent channels, tanh head) inside PR-DVQVAE2 at
32 clips x 16 frames: train step (per-step synchronised median and free-running mean, the method of leg_time.py), the no-grad
`inference` pass, and the two resample kernels at the decoder's tensors set beside lvt_bn_apply on a tensor of the same bytes
(read once / write once, same box, same process, kernels alternating over `rounds`).  Bytes are the algorithm's: every input and
output element once.
python tools/profile/conv_coders.py [steps] [rounds] [out.jsonl]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch, bench
from lvt_amd.hip import binding as L, ew, norm as BN
from lvt_amd.modeling import build_model

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "conv_coders.jsonl")
dev = "cuda:0"; torch.cuda.set_device(0)
base = {"math": L.get_math_mode(), "device": torch.cuda.get_device_name(0)}
rows = []


def emit(row):
    rows.append(dict(row, **base))
    print(rows[-1], flush=True)


# ---- the model ------------------------------------------------------------------------------------------------------------
leg = bench.VqvaeLeg(dev, 1, 0, 0, 32, 2)
e, g = leg.cfg.MODEL.ENCODER, leg.cfg.MODEL.GENERATOR
e.NAME, e.NF, e.N_LAYERS, e.OUT_CHANNELS = "ConvEncoder", 32, 2, 256
g.NAME, g.IN_CHANNELS, g.NF, g.N_LAYERS = "ConvDecoder", 256, 32, 2
torch.manual_seed(bench.SEED)
leg.model = build_model(leg.cfg)
leg.model.train()
leg.optimizers, _ = leg.model.configure_optimizers_and_checkpointers()
for i in range(5): leg.step(i)
torch.cuda.synchronize()
for r in range(rounds):
    ts = []
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); leg.step(5 + i); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(steps): leg.step(5 + steps + i)
    torch.cuda.synchronize()
    emit({"kind": "train_step", "config": "PR-DVQVAE2 + ConvEncoder/ConvDecoder (a)", "clips": 32, "frames": bench.CLIP_FRAMES, "round": r,
          "steps": steps, "median_ms": round(statistics.median(ts), 3), "free_running_ms": round((time.perf_counter() - t0) / steps * 1e3, 3)})
leg.model.eval()
with torch.no_grad():
    for i in range(3): leg.model(leg.batches[0], mode="inference")
    torch.cuda.synchronize()
    for r in range(rounds):
        ts = []
        for i in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); leg.model(leg.batches[i % 2], mode="inference"); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        emit({"kind": "eval_inference", "config": "PR-DVQVAE2 + ConvEncoder/ConvDecoder (a)", "clips": 32, "frames": bench.CLIP_FRAMES,
              "round": r, "steps": steps, "median_ms": round(statistics.median(ts), 3)})
del leg
torch.cuda.empty_cache()


# ---- the resample kernels beside lvt_bn_apply -----------------------------------------------------------------------------
def timed(fn, reps=50):
    for _ in range(5): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for shape in ((512, 32, 32, 32), (512, 16, 16, 64)):
    n, h, w, c = shape
    small = torch.randn(n, h, w, c, device=dev)
    big = torch.randn(n, 2 * h, 2 * w, c, device=dev)
    nb = small.numel() * 4
    # lvt_bn_apply reads M x C and writes M x C: M so that its bytes equal the unmasked resample kernels' (1 + 4 small tensors)
    m_bn = small.numel() * 5 // 2 // c
    y_bn = torch.randn(m_bn, c, device=dev)
    sc, sh = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
    cases = {
        "upsample2x2": (lambda: ew.upsample2x2(small), 5 * nb),
        "pool2x2": (lambda: ew.pool2x2(big), 5 * nb),
        "upsample2x2 masked (pool backward)": (lambda: ew.upsample2x2(small, 0.25, mask=big, leaky=True), 9 * nb),
        "pool2x2 masked (upsample backward)": (lambda: ew.pool2x2(big, 1.0, mask=small, leaky=True), 6 * nb),
        "bn_apply (same bytes as the unmasked kernels)": (lambda: BN.apply(y_bn, sc, sh, act=L.EPI_RELU), 2 * y_bn.numel() * 4),
    }
    for r in range(rounds):
        for name, (fn, nbytes) in cases.items():
            ms = timed(fn)
            emit({"kind": "kernel", "kernel": name, "small_tensor": list(shape), "round": r, "bytes": nbytes, "us": round(ms * 1e3, 2),
                  "GBps": round(nbytes / ms / 1e6, 1)})
with open(out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
