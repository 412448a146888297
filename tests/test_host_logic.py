"""CPU-only checks of the host side: config surface, registries, model construction / state_dict
keys, C-ABI symbol export, the slice/context builder against the reference's mapper goldens, and the
explicit absence of a CPU compute path."""
import ctypes
import os
import random
import re
import sys

import pytest
import torch

import seeded
from conftest import ROOT


def _cfg(path, device="cpu"):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, path))
    cfg.MODEL.DEVICE = device
    cfg.OUTPUT_DIR = "/tmp/lvt_test_out"
    return cfg


def test_config_surface():
    from lvt_amd.config import get_cfg
    cfg = _cfg("configs/vqvae/PR-DVQVAE2.yaml")
    assert cfg.MODEL.META_ARCHITECTURE == "VQVAEModel" and cfg.MODEL.CODEBOOK.NUM == 4      # _BASE_ + override
    assert cfg.SOLVER.IMS_PER_BATCH == 32 and cfg.MODEL.PIXEL_MEAN == [0.5, 0.5, 0.5]
    assert cfg.DATASETS.TRAIN == ("bair_train",)
    cfg = _cfg("configs/vt/DSFVT.yaml")
    vt = cfg.MODEL.AUTOREGRESSIVE.VT
    assert vt.KERNEL == (7, 1, 1) and vt.STRIDE == (16, 1, 1) and len(vt.BLOCKS_E) == 8 and vt.BLOCKS_D[3] == (1, 16, 16)
    assert cfg.SOLVER.RMSPROP.ALPHA_G == 0.95 and cfg.SOLVER.ADAM.BETA2_G == 0.9
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", "8", "MODEL.AUTOREGRESSIVE.VT.N_PRIME", 2, "OUTPUT_DIR", "/tmp/x"])
    assert cfg.SOLVER.IMS_PER_BATCH == 8 and vt.N_PRIME == 2 and cfg.OUTPUT_DIR == "/tmp/x"
    with pytest.raises(AssertionError):
        cfg.merge_from_list(["NO.SUCH.KEY", 1])
    c2 = cfg.clone()
    cfg.freeze()
    with pytest.raises(AttributeError):
        cfg.SEED = 1
    c2.SEED = 5                                   # the clone taken before freezing stays mutable
    assert "META_ARCHITECTURE" in cfg.dump()
    assert get_cfg().MODEL.DEVICE == "cuda"


def test_registries_and_errors():
    from lvt_amd.modeling import (AUTOREGRESSIVE_REGISTRY, ENCODER_REGISTRY, GENERATOR_REGISTRY, META_ARCH_REGISTRY,
                                  build_model)
    assert META_ARCH_REGISTRY.get("VQVAEModel").__name__ == "VQVAEModel"
    assert META_ARCH_REGISTRY.get("VideoTransformerModel") and META_ARCH_REGISTRY.get("AutoEncoderModel")
    assert ENCODER_REGISTRY.get("ResEncoder") and GENERATOR_REGISTRY.get("ResDecoder")
    build_model(_cfg("configs/vt/DSFVT.yaml"))
    assert AUTOREGRESSIVE_REGISTRY.get("VideoTransformer")
    with pytest.raises(KeyError):
        META_ARCH_REGISTRY.get("NoSuchModel")
    cfg = _cfg("configs/vqvae/PR-DVQVAE2.yaml")
    cfg.MODEL.META_ARCHITECTURE = "Bogus"
    with pytest.raises(KeyError):
        build_model(cfg)


def test_vqvae_construction_state_dict_and_contract():
    from lvt_amd.hip import LvtError
    from lvt_amd.modeling import build_model
    model = build_model(_cfg("configs/vqvae/PR-DVQVAE2.yaml"))
    assert set(model.encoder.state_dict()) == set(seeded.VQVAE_ENCODER_SHAPES)
    assert set(model.generator.state_dict()) == set(seeded.VQVAE_DECODER_SHAPES)
    for k, s in seeded.VQVAE_ENCODER_SHAPES.items():
        assert tuple(model.encoder.state_dict()[k].shape) == s
    cb = model.codebook.state_dict()
    assert set(cb) == {"ve.%d.%s" % (i, n) for i in range(4) for n in ("embedding.weight", "running_size", "running_sum")}
    assert tuple(cb["ve.3.embedding.weight"].shape) == (512, 64)
    assert all(not p.requires_grad for p in model.codebook.parameters())          # EMA codebooks take no gradient
    w = cb["ve.0.embedding.weight"]
    assert float(w.abs().max()) <= 1.0 / 512 and torch.equal(cb["ve.0.running_sum"], w)
    assert cb["ve.0.running_sum"].data_ptr() != w.data_ptr()                       # de-aliased (GPU semantics)
    # weights load (and survive a round trip) through the reference key names
    model.encoder.load_state_dict(seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, 3, "enc."))
    o, c = model.configure_optimizers_and_checkpointers()
    assert [x["type"] for x in o] == ["generator", "generator"] and len(c) == 3
    assert all(len(g["params"]) == 1 for g in o[0]["optimizer"].param_groups)     # one group per parameter
    assert o[0]["optimizer"].defaults["betas"] == (0.9, 0.9)
    # no CPU compute path
    with pytest.raises(LvtError):
        model([{"image": torch.rand(3, 64, 64).numpy()}], mode="inference")
    with pytest.raises(LvtError):
        model.encoder(torch.rand(1, 3, 64, 64))


def test_dsfvt_construction_state_dict():
    from lvt_amd.hip import LvtError
    from lvt_amd.modeling import build_model
    model = build_model(_cfg("configs/vt/DSFVT.yaml"))
    sd = model.model.state_dict()
    shapes = seeded.dsfvt_shapes()
    assert sum(p.numel() for p in model.model.parameters()) == 49872384
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    buffers = set(sd) - set(shapes)
    assert "decoder.block_local_attention.0.mask" in buffers and "encoder.block_local_attention.0.mask" not in buffers
    assert tuple(sd["encoder.block_local_attention.7.dw"].shape) == (65536,) and sd["decoder.block_local_attention.2.dh"].dtype == torch.int64
    assert tuple(sd["decoder.positional_encoder.inv_timescales"].shape) == (85,)
    assert tuple(sd["encoder.positional_encoder.inv_timescales"].shape) == (21,)
    lay = model.model.encoder.block_local_attention[0]
    assert float(lay.dh_bank.abs().max()) == 0.0                                   # banks start at zero
    o, _ = model.configure_optimizers_and_checkpointers()
    opt = o[0]["optimizer"]
    assert type(opt).__name__ == "RMSprop" and opt.defaults["alpha"] == 0.95 and opt.defaults["momentum"] == 0.9
    with pytest.raises(LvtError):
        model([{"image_sequence": torch.zeros(16, 4, 16, 16, dtype=torch.long)}], mode="inference")


def test_c_abi_exports_every_declared_symbol():
    """Every function declared in include/lvt_hip.h is exported by liblvt_hip.so and bound by ctypes."""
    from lvt_amd.hip import binding as L
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    declared = set(re.findall(r"\b(lvt_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in declared:
        assert getattr(lib, name) is not None, name
    assert declared == set(L.declared_symbols()), declared ^ set(L.declared_symbols())
    assert lib.lvt_version() >= 100
    # argument validation happens before any device work: usable without a GPU
    d = L.GemmDesc()
    assert lib.lvt_gemm_f32(ctypes.byref(d), None, 0, None) == -1
    assert b"null pointer" in lib.lvt_last_error()


def test_mapper_matches_reference_goldens(golden):
    from lvt_amd.data import DatasetMapper, prepare_slices
    from lvt_amd.data.dataset_mapper import prepare_slices_batch
    g = golden("g8_mapper")
    for a in (1, 2, 5, 9, 15):
        d = prepare_slices(g["codes"], (a, 0, 0), (16, 1, 1), (7, 1, 1), n_prime=1)
        for k in ("context", "slice", "slice_idx", "ignore_mask"):
            assert d[k].dtype == g["a%d_%s" % (a, k)].dtype and torch.equal(d[k], g["a%d_%s" % (a, k)]), (a, k)
    # batched device-side builder == per-sample builder
    vids = torch.stack([g["codes"], g["codes"].flip(0), g["codes"].roll(3, 0)])
    abcs = [(5, 0, 0), (9, 0, 0), (5, 0, 0)]
    ctx, sl, sidx, ig = prepare_slices_batch(vids, abcs, (16, 1, 1), (7, 1, 1), 1)
    for i, abc in enumerate(abcs):
        d = prepare_slices(vids[i], abc, (16, 1, 1), (7, 1, 1), 1)
        assert torch.equal(ctx[i], d["context"]) and torch.equal(sl[i], d["slice"])
        assert int(sidx[i]) == int(d["slice_idx"]) and torch.equal(ig[i], d["ignore_mask"])
    # the callable mapper: same random protocol as the reference (window start, then a, b, c)
    mapper = DatasetMapper(_cfg("configs/vt/DSFVT.yaml"), True)
    real = random.randint
    seq = iter([0, 9, 0, 0])
    random.randint = lambda lo, hi: next(seq)
    try:
        out = mapper({"image_sequence": g["codes"].numpy()})
    finally:
        random.randint = real
    assert torch.equal(out["context"], g["a9_context"]) and "image_sequence" not in out
    # the first N_PRIME frames are never drawn as a slice
    for _ in range(50):
        a = mapper({"image_sequence": g["codes"].numpy()})["slice_idx"]
        assert 1 <= int(a) <= 15


def test_subscale_helpers_match_goldens(golden):
    from lvt_amd.modeling.autoregressive import vt_utils as U
    g = golden("g7_subscale")
    vid = g["video"]
    for a in range(16):
        vm = U.visible_abc_mask(a, 0, 0, 16, 1, 1, 16, 16, 16, dtype=torch.bool)
        ctx = U.ss_shift(vid.masked_fill(~vm, -1), a, 0, 0, 16, 1, 1, 16, 16, 16, 7, 1, 1, pad_value=-1)
        assert torch.equal(ctx, g["dsfvt_ctx_%d" % a])
    for (a, b, c) in ((0, 0, 0), (1, 0, 1), (3, 1, 1), (2, 1, 0)):
        assert torch.equal(U.slice_mask(a, b, c, 4, 2, 2, 8, 8, 8, dtype=torch.bool), g["g422_smask_%d%d%d" % (a, b, c)])
        vm = U.visible_abc_mask(a, b, c, 4, 2, 2, 8, 8, 8, dtype=torch.bool)
        assert torch.equal(vm, g["g422_vmask_%d%d%d" % (a, b, c)])
        ctx = U.ss_shift(g["video2"].masked_fill(~vm, -1), a, b, c, 4, 2, 2, 8, 8, 8, 3, 3, 3, pad_value=-1)
        assert torch.equal(ctx, g["g422_ctx_%d%d%d" % (a, b, c)])


def test_checkpointer_roundtrip(tmp_path):
    from lvt_amd.modeling import build_model
    from lvt_amd.utils.checkpoint import Checkpointer, PeriodicCheckpointer
    model = build_model(_cfg("configs/vqvae/PR-DVQVAE2.yaml"))
    ck = Checkpointer(model.codebook, str(tmp_path))
    PeriodicCheckpointer(ck, 2, max_iter=4).step(3)
    assert os.path.exists(tmp_path / "model_0000003.pth") and os.path.exists(tmp_path / "model_final.pth")
    saved = torch.load(tmp_path / "model_final.pth")
    assert set(saved["model"]) == set(model.codebook.state_dict())
    other = build_model(_cfg("configs/vqvae/PR-DVQVAE2.yaml"))
    Checkpointer(other.codebook, str(tmp_path)).resume_or_load("", resume=True)
    assert torch.equal(other.codebook.state_dict()["ve.2.embedding.weight"], model.codebook.state_dict()["ve.2.embedding.weight"])


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: no module under lvt_amd/ may reference it."""
    for root, _, files in os.walk(os.path.join(ROOT, "lvt_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "oracle" not in src.replace("lvt_oracle_unused", ""), os.path.join(root, f)


@pytest.mark.parametrize("tag,stride,kernel", [("g15_dssvt", (1, 2, 2), (1, 3, 3)), ("g16_dstsvt", (4, 2, 2), (5, 3, 3))])
def test_mapper_general_strides_match_reference_contexts(golden, tag, stride, kernel):
    """The product's slice / context builder on the spatial and spatio-temporal subscale geometries against the
    contexts the reference's DatasetMapper produced (fixtures G15 / G16)."""
    from lvt_amd.data.dataset_mapper import prepare_slices, prepare_slices_batch
    g = golden(tag)
    abcs = [tuple(int(x) for x in g["abc"][i]) for i in range(g["codes"].shape[0])]
    ds = [prepare_slices(g["codes"][i].numpy(), abcs[i], stride, kernel, 1, -1) for i in range(len(abcs))]
    assert torch.equal(torch.stack([torch.as_tensor(d["context"]) for d in ds]), g["context"])
    assert torch.equal(torch.stack([torch.as_tensor(d["slice_idx"]) for d in ds]), g["slice_idx"])
    ctx, sl, sidx, ign = prepare_slices_batch(g["codes"], abcs, stride, kernel, 1, -1)
    assert torch.equal(ctx, g["context"]) and torch.equal(sidx, g["slice_idx"])
    assert torch.equal(sl, torch.stack([torch.as_tensor(d["slice"]) for d in ds]))
    assert torch.equal(ign, torch.stack([torch.as_tensor(d["ignore_mask"]) for d in ds]))


def test_frame_resident_kernel_routing_of_the_vqvae_layers():
    """Host-side queries of the C ABI (no GPU needed): which kernel family serves the layers of PR-DVQVAE2 / K-DVQVAE.
    A refactor that silently drops a layer back to the implicit-GEMM engine would cost 20-30 % on it without failing
    any numerics test."""
    import ctypes
    from lvt_amd.hip import binding as L, gemm as G
    lib, F32 = L.lib(), L.MATH_F32

    def geom(ci, co, k, s, p, h):
        return G.conv_geom(512, 1, h, h, ci, co, (1, k, k), (1, s, s), (0, p, p))

    k3, k4a = geom(256, 256, 3, 1, 1, 16), geom(256, 128, 3, 1, 1, 16)
    for g in (k3, k4a):
        assert lib.lvt_conv3d_uses_patch_kernel(ctypes.byref(g), 0) == 1                    # forward
        assert lib.lvt_conv3d_uses_patch_kernel(ctypes.byref(G.swapped_geom(g)), 0) == 1    # backward-data as a forward conv
        assert lib.lvt_conv3d_uses_patch_kernel(ctypes.byref(g), F32) == 0                  # f32 mode: implicit GEMM
        assert lib.lvt_conv3d_bwd_weight_fuses_bias(ctypes.byref(g), 0) == 1                # every route sums dy itself
        assert lib.lvt_conv3d_bwd_weight_fuses_bias(ctypes.byref(g), F32) == 1
    sg = G.swapped_geom(k4a)
    assert (sg.Ci, sg.Co, sg.ph, sg.pw, sg.Ho, sg.Wo) == (128, 256, 1, 1, 16, 16)
    k2 = geom(128, 256, 4, 2, 1, 32)                    # Conv 128->256 k4 s2 and, mirrored, ConvTranspose 256->128
    assert lib.lvt_conv3d_fwd_uses_parity_kernel(ctypes.byref(k2), 0) == 1
    assert lib.lvt_conv3d_bwd_data_uses_phase_kernel(ctypes.byref(k2), 0) == 1
    assert lib.lvt_conv3d_bwd_weight_fuses_bias(ctypes.byref(k2), 0) == 1
    assert lib.lvt_conv3d_fwd_uses_parity_kernel(ctypes.byref(k2), F32) == 0
    # layers that stay on the engine: 1x1, the image-side 4 -> 128 layer, other frame sizes
    for g in (geom(128, 256, 1, 1, 0, 16), geom(4, 128, 4, 2, 1, 64), geom(256, 256, 3, 1, 1, 32)):
        assert lib.lvt_conv3d_uses_patch_kernel(ctypes.byref(g), 0) == 0
        assert lib.lvt_conv3d_fwd_uses_parity_kernel(ctypes.byref(g), 0) == 0
        assert lib.lvt_conv3d_bwd_data_uses_phase_kernel(ctypes.byref(g), 0) == 0
        assert lib.lvt_conv3d_bwd_weight_fuses_bias(ctypes.byref(g), 0) == 1
    # workspace of the weight gradient covers both routes
    assert lib.lvt_conv3d_bwd_weight_workspace_bytes(ctypes.byref(k3)) >= 32 * 9 * 256 * 256 * 4


def test_vq_ema_statistics_plan_is_the_recorded_one():
    """lvt_vq_ema_workspace_bytes (launches nothing: no GPU needed) = num x row chunks x KC x (D + 1) floats, so it shows the
    row chunking of the EMA statistics.  The chunk partials are summed in chunk order: a planner that returns another chunk
    count changes the bits of the codebook update.  Constants recorded from the library before the whole-codebook and the
    ranged planner were merged: (rows, num, D, KC) on the whole-codebook family (one workgroup per CU), on the ranged one
    (two per CU over groups and code ranges), below the 256-row chunk floor and below one 64-row tile."""
    from lvt_amd.hip import binding as L
    lib = L.lib()
    recorded = {(131072, 4, 64, 512): 34078720, (240, 3, 64, 128): 99840, (6144, 3, 64, 1024): 19169280,
                (6144, 3, 256, 64): 4737024, (48, 1, 16, 2048): 139264}
    for args, nbytes in recorded.items():
        assert lib.lvt_vq_ema_workspace_bytes(*args) == nbytes, args


def test_bench_generation_roofline_arithmetic_is_integer():
    """Rounds 2 and 3 lost five GPU boxes to one line of bench.py: `hd = v.N_HEAD_D * v.DA` with N_HEAD_D a per-layer
    tuple made the K/V byte count an `int * tuple` -- a request for a 4.5e12-element tuple (36 TB) that exhausted the host.
    The byte count is a function now; this pins its type and value on the shipped config."""
    import bench
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vt/DSFVT.yaml"))
    v = cfg.MODEL.AUTOREGRESSIVE.VT
    assert isinstance(v.N_HEAD_D, (tuple, list))                      # the trap
    n = bench.generation_kv_bytes(v, 768, 5)
    assert type(n) is int
    assert n == 768 * 11 * 8 * (256 * 257 // 2) * 2 * 1024 * 4 == 18212808818688


def test_bench_self_launches_one_rank_per_gpu():
    """`python bench.py --gpus 2` without a launcher spawns its own ranks (reference: vidgen/engine/launch.py:25-67):
    dry run on CPU -- both ranks rendezvous on 127.0.0.1 and all-reduce."""
    import json
    import subprocess
    env = dict(os.environ, LVT_BENCH_DRYRUN="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    assert json.loads(line) == {"dry_run": True, "world": 2, "rank_sum": 1.0}
    # under an external launcher with a mismatching --gpus the error is explicit
    env.update(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", LVT_BENCH_DRYRUN="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2 but --gpus 1" in (r.stderr + r.stdout)


def test_bench_dump_outputs_on_toy_models(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR` (bench.dump_outputs) on two toy models on CPU: the returned losses and every floating
    state entry in key order as float32 .npy files; above the sample size a seeded sample that is the same from call to
    call; `--steps` below 1 is refused."""
    import types
    import numpy as np
    import bench
    torch.manual_seed(0)
    vq = types.SimpleNamespace(model=torch.nn.Linear(3, 2))
    ds = types.SimpleNamespace(model=torch.nn.Sequential(torch.nn.Linear(40, 50), torch.nn.Linear(50, 4)))
    vq.model.register_buffer("steps", torch.tensor(7))                             # integer entries are not state samples
    losses = {"loss_reconstruction": torch.tensor(0.25, requires_grad=True), "loss_commitment": torch.tensor(0.5)}
    monkeypatch.setattr(bench, "DUMP_STATE_SAMPLE", 1000)
    shapes = bench.dump_outputs(str(tmp_path / "a"), losses, torch.tensor(6.5), vq, ds)
    assert shapes == {"vqvae_loss_reconstruction": [], "vqvae_loss_commitment": [], "dsfvt_loss_cross_entropy": [],
                      "vqvae_state_sample": [8], "dsfvt_state_sample": [1000]}
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in shapes}
    assert all(x.dtype == np.float32 for x in a.values())
    assert float(a["vqvae_loss_reconstruction"]) == 0.25 and float(a["dsfvt_loss_cross_entropy"]) == 6.5
    sd = vq.model.state_dict()
    assert np.array_equal(a["vqvae_state_sample"], torch.cat([sd["bias"], sd["weight"].reshape(-1)]).numpy())
    full = torch.cat([v.reshape(-1) for _, v in sorted(ds.model.state_dict().items())]).numpy()
    assert np.isin(a["dsfvt_state_sample"], full).all() and len(np.unique(a["dsfvt_state_sample"])) > 990
    bench.dump_outputs(str(tmp_path / "b"), losses, torch.tensor(6.5), vq, ds)
    for n in shapes:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / (n + ".npy"))), n
    assert bench.parse(["--steps", "3", "--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_relu_decision_matching_helper_on_a_toy_network():
    """tests/util_relu.py (the gradient comparison that is exact about ReLU units sitting on their threshold) on a two-layer
    network with one planted undecided unit: a gradient that differs from fp64 only through that unit's decision is accepted
    and the unit is named; the same gradient with a genuine error is rejected; reported decisions are matched exactly."""
    from util_relu import ReluProbe, assert_grads_match, assert_grads_match_decisions, relu_probe
    torch.manual_seed(0)
    W1, W2, x = torch.randn(64, 32), torch.randn(8, 64), torch.randn(200, 32)
    pre = x @ W1.t()
    i, j = 5, 7
    x[i] += (-pre[i, j] + 1e-8 * float(pre.abs().max())) * W1[j] / W1[j].dot(W1[j])        # pre-activation (i, j) ~ 1e-8 of the max

    def run(dtype):
        w1, w2 = W1.clone().to(dtype).requires_grad_(True), W2.clone().to(dtype).requires_grad_(True)
        (torch.relu(x.to(dtype) @ w1.t()) @ w2.t()).pow(2).sum().backward()
        return {"w1": w1.grad, "w2": w2.grad}

    with relu_probe(ReluProbe(force={(0, (i, j)): False}, record=True)) as pr:
        flipped = {k: v.float() for k, v in run(torch.float64).items()}
    n, units = assert_grads_match(flipped, run, ["w1", "w2"])
    assert n >= 1 and [(u[0], u[1]) for u in units] == [(0, (i, j))]
    assert assert_grads_match({k: v.float() for k, v in run(torch.float64).items()}, run, ["w1", "w2"]) == (0, [])
    masks = [m.clone() for m in pr.masks]
    masks[0][i, j] = False                                             # what the path under test reports: unit (i, j) blocked
    assert assert_grads_match_decisions(flipped, masks, run, ["w1", "w2"]) == (1, 0)
    wrong = {k: v.clone() for k, v in flipped.items()}
    wrong["w1"][0, 0] += 1.0
    with pytest.raises(AssertionError):
        assert_grads_match(wrong, run, ["w1", "w2"])
    with pytest.raises(AssertionError):
        assert_grads_match_decisions(wrong, masks, run, ["w1", "w2"])


def test_channel_predictor_share_p_is_the_config_default_and_constructs():
    """SHARE_P defaults to True in the reference's config (vidgen/config/defaults.py:50): a config that does not set it must
    build, with ONE output layer whose state_dict keys are the reference's (`P.weight`, `P.bias`); SHARE_EMBEDDINGS (one layer d -> de, the decoder's tables as
    output matrices) constructs with the reference's keys."""
    from lvt_amd.config import get_cfg
    from lvt_amd.modeling.autoregressive.videotransformer import ChannelPredictor
    assert get_cfg().MODEL.AUTOREGRESSIVE.VT.SHARE_P is True
    cp = ChannelPredictor(64, 3, 16, 8, share_p=True)
    keys = set(cp.state_dict().keys())
    assert {"P.weight", "P.bias", "U.2.weight", "layer_norm.bias"} <= keys and not any(k.startswith("P.0") for k in keys)
    assert tuple(cp.P.weight.shape) == (16, 64)
    assert len(ChannelPredictor(64, 3, 16, 8, share_p=False).P) == 3
    se = ChannelPredictor(64, 3, 16, 8, share_p=False, share_embeddings=True)       # (videotransformer.py:124-125): P maps d -> de
    assert tuple(se.P.weight.shape) == (8, 64) and set(se.state_dict()) == {k for k in keys if not k.startswith("P.")} | {"P.weight", "P.bias"}
    with pytest.raises(AssertionError):
        ChannelPredictor(64, 3, 16, 8, share_p=True, share_embeddings=True)


def test_single_codebook_is_the_config_default_and_constructs():
    """CODEBOOK.NUM defaults to 1 (vidgen/config/defaults.py:79): a VQVAEModel config that does not set it builds `VQEmbedding`
    as its quantiser (vqvae.py:25-27) with the reference's state_dict keys."""
    from lvt_amd.config import get_cfg
    from lvt_amd.modeling.vq import SingleVQEmbedding
    assert get_cfg().MODEL.CODEBOOK.NUM == 1
    cb = SingleVQEmbedding(512, 256, True)
    assert sorted(cb.state_dict()) == ["embedding.weight", "running_size", "running_sum"]
    assert tuple(cb.embedding.weight.shape) == (512, 256) and cb.groups == 4
    assert sorted(SingleVQEmbedding(128, 64, False).state_dict()) == ["embedding.weight"]
    with pytest.raises(NotImplementedError):
        SingleVQEmbedding(512, 100, True)


def test_device_prefetcher_keeps_the_input_contract():
    """data/prefetch.py on CPU (the staging logic; the pinned buffers and the side stream need a GPU): batches come out in order as
    list[dict] whose array values are per-sample views of ONE batched tensor, which stack_to_device takes as it is."""
    import numpy as np
    from lvt_amd.data.prefetch import DevicePrefetcher
    from lvt_amd.modeling.meta_arch.common import stack_to_device
    loader = [[{"image": np.full((3, 4, 4), 10 * b + i, dtype=np.float32), "video_idx": i} for i in range(3)] for b in range(5)]
    seen = []
    for data in DevicePrefetcher(loader, "cpu"):
        assert isinstance(data, list) and data[2]["video_idx"] == 2
        x = stack_to_device([d["image"] for d in data], "cpu")
        assert x.shape == (3, 3, 4, 4) and x.data_ptr() == data[0]["image"].data_ptr()         # no second copy
        seen.append(float(x[:, 0, 0, 0].sum()))
    assert seen == [3.0 + 30 * b for b in range(5)]
    assert list(DevicePrefetcher([], "cpu")) == []
