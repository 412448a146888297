"""Time 16-frame generation with DSSVT (slices of (16,8,8) tokens, attention inside (4,8,8) blocks), TEST.VT_SAMPLER.N_PRIME = 5,
the seeded test weights, --videos videos per call.  Three runs, one JSON line each, appended to --out
(profiles/gen_blocksplit.jsonl) and printed:

    dssvt16_kv_cache     sample_video(...)                      K/V-cache path: 4 slices x 1024 single-token steps
    dssvt16_full_passes  sample_video(..., incremental=False)   the reference's schedule: 4 x 704 full decoder passes
    dsfvt_kv_cache       DSFVT, same video count                11 slices x 256 single-token steps, for scale

    python tools/profile/gen_blocksplit.py [--videos 16] [--reps 3] [--out FILE]

A run is one whole sample_video call: host clock from the call to a device synchronise after it.  Each configuration is
warmed up first (K/V-cache runs: one whole call, which also captures the decode graphs; the full-pass run: a call with 15
priming frames, the same launches at the same shapes), then timed --reps times (the full-pass run once: it is the slow
one); median and fastest are reported as generated frames per second = videos x 11 / seconds.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import seeded  # noqa: E402
from lvt_amd.config import get_cfg  # noqa: E402
from lvt_amd.modeling import build_model  # noqa: E402

N_PRIME, FRAMES, SEED = 5, 16, 4321


def build(config, **shape_args):
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, config))
    cfg.MODEL.DEVICE = "cuda"
    cfg.OUTPUT_DIR = "/tmp/lvt_gen_blocksplit"
    cfg.TEST.EVALUATORS = "VTSampler"
    model = build_model(cfg)
    model.model.load_state_dict(seeded.seeded_params(seeded.dsfvt_shapes(**shape_args), SEED), strict=False)
    return model.eval()


def timed(model, video, reps, warm_prime, **kw):
    with torch.no_grad():
        model.sample_video(video, n_prime=warm_prime, **kw)
        torch.cuda.synchronize()
        secs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = model.sample_video(video, n_prime=N_PRIME, **kw)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
    assert 0 <= int(out.min()) and int(out.max()) < 512 and torch.equal(out[:, :, :N_PRIME], video[:, :, :N_PRIME])
    frames = video.shape[0] * (FRAMES - N_PRIME)
    return {"videos": video.shape[0], "generated_frames": frames, "runs": reps, "seconds": [round(s, 3) for s in secs],
            "frames_per_s_median": round(frames / statistics.median(secs), 2), "frames_per_s_best": round(frames / min(secs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_blocksplit.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gen_blocksplit.py times generation on a GPU; none is visible")
    codes = torch.stack([seeded.seeded_codes("gen%d" % i, (FRAMES, 4, 16, 16), SEED) for i in range(a.videos)])
    video = codes.transpose(1, 2).contiguous().cuda()
    video[:, :, N_PRIME:] = 0
    dssvt = build("configs/vt/DSSVT.yaml", block=(4, 8, 8), kernel=(1, 3, 3), n_slices=4)
    runs = [("dssvt16_kv_cache", dssvt, a.reps, N_PRIME, {}),
            ("dssvt16_full_passes", dssvt, 1, FRAMES - 1, {"incremental": False}),
            ("dsfvt_kv_cache", None, a.reps, N_PRIME, {})]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name, model, reps, warm_prime, kw in runs:
        if model is None:
            dssvt._samplers = {}                                   # free the 1024-token caches
            model = build("configs/vt/DSFVT.yaml")
        rec = dict(run=name, n_prime=N_PRIME, **timed(model, video, reps, warm_prime, **kw), device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
