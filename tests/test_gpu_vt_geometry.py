"""The DSFVT-shaped latent transformer at the codebook geometries the quantiser now supports: NC = 8 code channels and
NV = 1024 / 2048 codes (a 2 + 2-layer model, DSFVT blocks).  Training loss and gradients against the CPU oracle, logits of an
entire video against the oracle, and incremental sampling with graph replay equal to the eager steps (which at NV = 2048 runs
the wide lvt_sample_categorical kernel).  Tolerances as in test_gpu_vt.py."""
import pytest
import torch

import seeded
from conftest import rel_err
from oracle import lvt_oracle as O
from util_models import dsfvt_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC = 8
BLOCKS = ((1, 16, 16),) * 2
DS = dict(blocks_e=BLOCKS, blocks_d=BLOCKS, stride=(16, 1, 1))
SEED = 77


def _model(nv, evaluator=None):
    from lvt_amd.modeling import build_model
    cfg = dsfvt_cfg()
    vt = cfg.MODEL.AUTOREGRESSIVE.VT
    vt.NC, vt.NV = NC, nv
    vt.N_HEAD_E, vt.BLOCKS_E, vt.N_HEAD_D, vt.BLOCKS_D = (8, 8), BLOCKS, (8, 8), BLOCKS
    if evaluator:
        cfg.TEST.EVALUATORS = evaluator
    model = build_model(cfg)
    params = seeded.seeded_params(seeded.dsfvt_shapes(nc=NC, nv=nv, n_enc=2, n_dec=2), SEED)
    missing, unexpected = model.model.load_state_dict(params, strict=False)
    assert not unexpected
    return model, params


@pytest.mark.parametrize("nv", [1024, 2048])
def test_training_loss_and_grads_nc8(nv):
    """Three slices: the cross-entropy loss and gradients against O.vt_supervised_loss(..., nv)."""
    from lvt_amd.utils.events import EventStorage
    model, params = _model(nv)
    data = []
    for i, a in enumerate((2, 9, 15)):
        codes = seeded.seeded_codes("geo.vt%d" % i, (16, NC, 16, 16), SEED, nv=nv)
        data.append(O.prepare_slices(codes, (a, 0, 0), (16, 1, 1), (7, 1, 1), 1))
    model.train()
    model.model.zero_grad()
    with EventStorage(0):
        loss = model(data, mode="supervised")["loss_cross_entropy"]
    loss.backward()
    ctx = torch.stack([d["context"] for d in data]); sl = torch.stack([d["slice"] for d in data])
    si = torch.stack([d["slice_idx"] for d in data]); ig = torch.stack([d["ignore_mask"] for d in data])

    def oracle(dtype):
        p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
        lo, _ = O.vt_supervised_loss(p, ctx, sl, si, ig, nv=nv, **DS)
        lo.backward()
        return float(lo.detach()), {k: v.grad.double() for k, v in p.items()}
    ref, g32 = oracle(torch.float32)
    _, g64 = oracle(torch.float64)
    assert abs(float(loss.detach()) - ref) < 2e-5 * ref
    named = dict(model.model.named_parameters())
    # every channel's embedding table and predictor head, plus the deep and shallow ends of the stack
    names = ["encoder.conv.weight", "encoder.conv.bias", "encoder.linear_projector.weight", "decoder.linear_projector.weight",
             "decoder.block_local_attention.1.mha.w_k", "encoder.block_local_attention.0.ffn.1.weight"]
    names += ["decoder.ch_embedder.%d.weight" % k for k in range(NC)]
    names += [n for n in g64 if n.startswith("ch_predictor.")]
    for n in names:
        a, r32, r64 = named[n].grad.double().cpu(), g32[n], g64[n]
        e_mine, e_cpu = float((a - r64).norm() / r64.norm()), float((r32 - r64).norm() / r64.norm())
        assert e_mine < max(4 * e_cpu, 2e-5) or e_mine < 3e-3, (n, e_mine, e_cpu)


def test_entire_video_logits_nc8_nv1024():
    """calculate_logits_for_entire_video (mode "inference", BitsEvaluator) against O.vt_logits_for_entire_video."""
    nv = 1024
    model, params = _model(nv, "BitsEvaluator")
    codes = seeded.seeded_codes("geo.video", (16, NC, 16, 16), SEED, nv=nv)
    model.eval()
    with torch.no_grad():
        out = model([{"image_sequence": codes}], mode="inference")[0]
    lg = out["logits"].cpu()
    assert tuple(lg.shape) == (NC, nv, 16, 16, 16)
    p = {k: v.detach().clone() for k, v in params.items()}
    with torch.no_grad():
        ref = O.vt_logits_for_entire_video(p, codes[None], DS["blocks_e"], DS["blocks_d"], DS["stride"], (7, 1, 1), nv=nv)[0]
    assert rel_err(lg, ref) < 1e-4


@pytest.mark.parametrize("nv", [1024, 2048])
def test_graph_replay_equals_eager_nc8(nv, monkeypatch):
    """One captured hipGraph replayed for every position == the same steps launched eagerly, bit for bit (two generated
    frames); every code in range, primed frames untouched."""
    model, _ = _model(nv, "VTSampler")
    model.eval()
    codes = torch.stack([seeded.seeded_codes("geo.e%d" % i, (16, NC, 16, 16), SEED, nv=nv) for i in range(3)])
    with torch.no_grad():
        video = codes.transpose(1, 2).contiguous().to(DEV)
        video[:, :, 14:] = 0
        model._samplers = {}
        torch.manual_seed(5)
        graphed = model.sample_video(video, n_prime=14, temp=1.0)
        assert len(model._samplers) == 1
        (_, _, smp, _), = list(model._samplers.values())[0]
        assert set(smp.graphs) == {True}
        monkeypatch.setenv("LVT_DECODE_GRAPHS", "0")
        model._samplers = {}
        torch.manual_seed(5)
        eager = model.sample_video(video, n_prime=14, temp=1.0)
        (_, _, smp, _), = list(model._samplers.values())[0]
        assert not smp.graphs
        model._samplers = {}
    assert torch.equal(graphed, eager)
    g = graphed.cpu()
    assert torch.equal(g[:, :, :14], codes.transpose(1, 2)[:, :, :14])
    assert int(g.min()) >= 0 and int(g.max()) < nv
    # temp 1 over NV codes: the drawn codes spread over the upper half of the code range too
    assert int((g[:, :, 14:] >= nv // 2).sum()) > 0
