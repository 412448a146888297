"""K/V-cache decoding of slices larger than the attention block (block-split attention: DSSVT sampled at 16 frames,
slices of (16,8,8) tokens attending inside (4,8,8) blocks), checked teacher-forced against the full pass and against
the reference's whole-video likelihood (fixture G15).  Every test asserts the host-side capability check first: a tree
without the block-local decode attention fails there, before any launch with a geometry its kernels were not written
for.  No test compares free-running samples of two paths (one differing arg-max cascades through every later position)."""
import ctypes as C
import math

import pytest
import torch

import seeded
from conftest import rel_err
from test_gpu_variants import _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLICE = (16, 8, 8)


def _supports(decoder, thw):
    from lvt_amd.modeling.autoregressive.incremental import IncrementalDecoder
    assert IncrementalDecoder.supports(decoder, thw), "no K/V-cache decoding for slice %s" % (thw,)
    return IncrementalDecoder


@pytest.fixture(scope="module")
def g15(golden):
    g = golden("g15_dssvt")
    model, _, v = _build("g15_dssvt", g, evaluators="VTSampler")
    model.eval()
    return g, model, v


def _slices(model, v, video):
    """(slice, encoder output, (a, b, c)) of every subscale slice of video (B, nc, T, H, W), teacher-forced."""
    from lvt_amd.modeling.autoregressive.vt_utils import slice_and_context, subscale_order
    vt = model._vt
    B = video.shape[0]
    for si, (a, b, c) in enumerate(subscale_order(*vt.STRIDE)[0]):
        sl, ctx = slice_and_context(video, a, b, c, vt.STRIDE, vt.KERNEL, vt.PAD_VALUE)
        sidx = torch.full((B,), si, dtype=torch.long, device=video.device)
        yield sl, model.model.encoder.forward_tokens(ctx.contiguous(), sidx, None), (a, b, c)


def test_dssvt16_step_rows_equal_full_pass_rows(g15):
    """step(i) == row i of decoder.forward_tokens on a (16,8,8) slice with (4,8,8) blocks: both sides of every block
    boundary (255|256, 511|512, 767|768), the ends, and positions inside blocks."""
    g, model, v = g15
    Dec = _supports(model.model.decoder, SLICE)
    video = g["eval_video"].transpose(0, 1)[None].contiguous().to(DEV)
    check = {0, 1, 63, 64, 200, 255, 256, 257, 300, 511, 512, 513, 700, 767, 768, 769, 1000, 1022, 1023}
    with torch.no_grad():
        sl, zl, _ = next(_slices(model, v, video))
        assert tuple(sl.shape[2:]) == SLICE
        full = model.model.decoder.forward_tokens(sl, zl).view(1, 1024, -1)
        dec = Dec(model.model.decoder, zl, 1, SLICE)
        worst = 0.0
        for i in range(1024):
            y = dec.step(sl, i)
            if i in check:
                e = rel_err(y, full[:, i])
                print("position %4d: rel_err %.3g" % (i, e))
                worst = max(worst, e)
    assert worst < 2e-5, worst


def _seeded_decoder(blocks, seed):
    """A directly constructed VTDecoder (shipped widths, one layer per entry of `blocks`) with seeded weights."""
    from lvt_amd.modeling.autoregressive.videotransformer import VTDecoder
    shapes = {k[len("decoder."):]: s for k, s in seeded.dsfvt_shapes(n_dec=len(blocks)).items() if k.startswith("decoder.")}
    for i, blk in enumerate(blocks):
        for n, k in zip(("dt_bank", "dh_bank", "dw_bank"), blk):
            shapes["block_local_attention.%d.%s" % (i, n)] = (8, 2 * k - 1)
    params = seeded.seeded_params(shapes, seed, "bs.")
    dec_mod = VTDecoder(4, 512, 128, 128, 512, blocks, [8] * len(blocks))
    missing, unexpected = dec_mod.load_state_dict(params, strict=False)
    assert not unexpected and not (set(missing) & {n for n, _ in dec_mod.named_parameters()})
    return dec_mod.to(DEV).eval(), params


def _step_rows_vs_full(dec_mod, thw, b, full, sl, zl, check):
    Dec = _supports(dec_mod, thw)
    dec = Dec(dec_mod, zl, b, thw)
    worst = 0.0
    for i in range(thw[0] * thw[1] * thw[2]):
        y = dec.step(sl, i)
        if i in check:
            e = rel_err(y, full[:, i])
            print("position %4d: rel_err %.3g" % (i, e))
            worst = max(worst, e)
    return worst


def test_blocks_along_every_axis_step_rows():
    """(2,4,4) blocks on a (4,8,8) slice: 8 blocks whose keys are not contiguous cache rows (a block row is 4 tokens, the
    next one 8 rows on; the next block plane 64 rows on), mixed with one layer whose block is the slice.  The training
    kernels take blocks of a multiple of 256 tokens only, so the full pass is the oracle's decoder (fp64, same weights)."""
    from oracle import lvt_oracle as O
    thw, blocks = (4, 8, 8), [(2, 4, 4), (4, 8, 8), (2, 4, 4)]
    dec_mod, params = _seeded_decoder(blocks, 77)
    _supports(dec_mod, thw)
    b = 2
    sl = torch.stack([seeded.seeded_codes("bs%d" % i, (4,) + thw, 5) for i in range(b)])
    zl = 0.5 * seeded.seeded_input("bs.zl", (b * 256, 512), 5, -1.0, 1.0)
    with torch.no_grad():
        full = O.vt_decoder({"decoder." + k: v.double() for k, v in params.items()}, sl,
                            zl.double().view(b, *thw, 512).permute(0, 4, 1, 2, 3), blocks)
        full = full.permute(0, 2, 3, 4, 1).reshape(b, 256, 512)
        # 35 = (0,4,3): last of block (0,1,0)'s first row, its block-mates are rows 32..35; 36 opens block (0,1,1);
        # 91 = (1,3,3): the last key of block (0,0,0), rows {0..3, 8..11, 16..19, 24..27} + 64; 100 / 255: inner / last block
        check = {0, 1, 3, 4, 7, 8, 27, 28, 35, 36, 63, 64, 91, 92, 100, 127, 128, 129, 191, 219, 220, 255}
        worst = _step_rows_vs_full(dec_mod, thw, b, full, sl.to(DEV), zl.to(DEV), check)
    assert worst < 2e-5, worst


def test_2048_token_slice_blocks_along_every_axis_step_rows():
    """(4,8,8) blocks on an (8,16,16) slice, against the training path's own block-split full pass: every axis split
    with 256-token blocks, and a slice (2048 tokens) longer than any block may be."""
    thw, blocks = (8, 16, 16), [(4, 8, 8), (4, 8, 8)]
    dec_mod, _ = _seeded_decoder(blocks, 78)
    _supports(dec_mod, thw)
    sl = seeded.seeded_codes("bs.long", (1, 4) + thw, 6).to(DEV)
    zl = (0.5 * seeded.seeded_input("bs.zl.long", (2048, 512), 6, -1.0, 1.0)).to(DEV)
    # (t,h,w) -> (t*16 + h)*16 + w.  7 | 8: a block edge along w; 127 | 128: along h ((0,7,15) | (0,8,0)); 1023 | 1024: along t;
    # 1911 = (7,7,7): the last key of block (1,0,0); 2047: the last key of the last block
    check = {0, 1, 7, 8, 15, 16, 127, 128, 136, 255, 256, 775, 776, 1023, 1024, 1025, 1500, 1911, 1912, 2046, 2047}
    with torch.no_grad():
        full = dec_mod.forward_tokens(sl, zl).view(1, 2048, -1)
        worst = _step_rows_vs_full(dec_mod, thw, 1, full, sl, zl, check)
    assert worst < 2e-5, worst


def test_dssvt16_teacher_forced_nll_matches_reference(g15):
    """-log p[target] of EVERY position of EVERY slice of the 16-frame evaluation video through the incremental path
    == the reference's calculate_logits_for_entire_video (g["eval_nll"]), at the bound of the full-pass test."""
    g, model, v = g15
    Dec = _supports(model.model.decoder, SLICE)
    video = g["eval_video"].transpose(0, 1)[None].contiguous().to(DEV)         # (1, nc, 16, 16, 16)
    ref = g["eval_nll"]                                                         # (nc, 16, 16, 16)
    st, sh, sw = v["stride"]
    nll = torch.zeros_like(ref)
    pred = model.model.ch_predictor
    with torch.no_grad():
        dec = None
        for sl, zl, (a, b, c) in _slices(model, v, video):
            if dec is None:
                dec = Dec(model.model.decoder, zl, 1, SLICE)
            else:
                dec.begin_slice(zl)
            codes = sl.reshape(1, 4, 1024)
            rows = []
            for i in range(1024):
                y = dec.step(sl, i)
                _, probs = pred.sample_from_rows(y, 1.0, forced_codes=codes[:, :, i], return_probs=True)     # (1, nc, nv)
                rows.append(-torch.log(probs[0].gather(1, codes[0, :, i:i + 1]))[:, 0])
            part = torch.stack(rows, 1).view(4, *SLICE).cpu()
            print("slice (%d,%d,%d): rel_err %.3g" % (a, b, c, rel_err(part, ref[:, a::st, b::sh, c::sw])))
            nll[:, a::st, b::sh, c::sw] = part
    assert rel_err(nll, ref) < 1e-4, rel_err(nll, ref)


def test_dssvt16_sample_video_takes_the_cache_path(g15, monkeypatch):
    """sample_video on 16 frames never runs a full decoder pass, and keeps the sampler contract."""
    g, model, v = g15
    _supports(model.model.decoder, SLICE)

    def no_full_pass(*a, **k):
        raise AssertionError("sample_video ran a full decoder pass")
    monkeypatch.setattr(model.model.decoder, "forward_tokens", no_full_pass)
    codes = torch.stack([g["eval_video"], seeded.seeded_codes("bs.v1", (16, 4, 16, 16), 9)])     # (2, T, nc, H, W)
    n_prime = 15
    with torch.no_grad():
        video = codes.transpose(1, 2).contiguous().to(DEV)
        video[:, :, n_prime:] = 0
        model._samplers = {}
        torch.manual_seed(0)
        out = model.sample_video(video, n_prime=n_prime)
    groups = model._samplers[(2,) + SLICE + (1.0,)]
    assert len(groups) == 1 and groups[0][2].dec is not None and groups[0][2].dec.thw == SLICE
    assert tuple(out.shape) == (2, 4, 16, 16, 16) and out.dtype == torch.int64
    assert torch.equal(out[:, :, :n_prime].cpu(), codes.transpose(1, 2)[:, :, :n_prime])          # primed frames untouched
    assert 0 <= int(out.min()) and int(out.max()) < 512
    assert int((out[:, :, n_prime:] != 0).sum()) > 0.9 * out[:, :, n_prime:].numel()
    # the inference-mode contract used by scripts/generate_videos.py / VTSampler with this config
    monkeypatch.setattr(model.cfg.TEST.VT_SAMPLER, "N_PRIME", 15)
    monkeypatch.setattr(model.cfg.TEST.VT_SAMPLER, "NUM_SAMPLES", 1)
    with torch.no_grad():
        res = model([{"image_sequence": codes[1]}], mode="inference")
    assert len(res[0]["samples"]) == 1 and tuple(res[0]["samples"][0].shape) == (4, 16, 16, 16)
    model._samplers = {}


def test_dssvt16_graph_replay_equals_eager_and_repeats(g15, monkeypatch):
    """One captured graph replayed over the 1024 positions of each slice == the same steps launched eagerly, and the
    same call twice gives the same codes: bit for bit (same kernels, same uniforms, fixed summation order)."""
    g, model, v = g15
    _supports(model.model.decoder, SLICE)
    codes = torch.stack([seeded.seeded_codes("bs.e%d" % i, (16, 4, 16, 16), 21) for i in range(3)])
    key = (3,) + SLICE + (1e-4,)
    with torch.no_grad():
        video = codes.transpose(1, 2).contiguous().to(DEV)
        video[:, :, 15:] = 0
        outs = []
        for _ in range(2):
            model._samplers = {}
            torch.manual_seed(5)
            outs.append(model.sample_video(video, n_prime=15, temp=1e-4))
            (_, _, smp, _), = model._samplers[key]
            assert set(smp.graphs) == {True, False} and smp._next == 1024      # primed and generated positions: 2 graphs
        monkeypatch.setenv("LVT_DECODE_GRAPHS", "0")
        model._samplers = {}
        torch.manual_seed(5)
        eager = model.sample_video(video, n_prime=15, temp=1e-4)
        (_, _, smp, _), = model._samplers[key]
        assert not smp.graphs
        model._samplers = {}
    print("graph vs graph: %d codes differ; graph vs eager: %d" % (int((outs[0] != outs[1]).sum()), int((outs[0] != eager).sum())))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], eager)


def test_attn_decode_blocks_equals_attn_decode_on_the_gathered_block():
    """Kernel level: the block-local entry on slice-ordered caches == lvt_attn_decode on the block's rows gathered into
    a cache of their own, bit for bit (same arithmetic in the same order), for a leading-axis split and a full split."""
    from lvt_amd.hip import tx
    from lvt_amd.modeling.autoregressive.incremental import IncrementalDecoder
    from lvt_amd.modeling.autoregressive.vt_attention import _block_permutation
    assert hasattr(IncrementalDecoder, "supports") and hasattr(tx, "attn_decode_blocks")
    B, H, da = 3, 2, 128
    gen = torch.Generator().manual_seed(3)
    for thw, blk in (((8, 4, 4), (2, 4, 4)), ((4, 8, 8), (2, 4, 4)), ((2, 4, 6), (1, 2, 3))):
        S, vol = thw[0] * thw[1] * thw[2], blk[0] * blk[1] * blk[2]
        q = torch.randn(B, S, H * da, generator=gen).to(DEV)
        Kc, Vc = torch.randn(B, S, H * da, generator=gen).to(DEV), torch.randn(B, S, H * da, generator=gen).to(DEV)
        banks = [(0.5 * torch.randn(H, 2 * k - 1, generator=gen)).to(DEV) for k in blk]
        perm, inv = _block_permutation(thw, blk, torch.device(DEV))
        pos = torch.zeros(1, dtype=torch.int32, device=DEV)
        for qi in sorted({0, 1, vol - 1, vol, vol + 1, S // 2 + 3, S - vol, S - 1}):
            li, nb = int(inv[qi]) % vol, int(inv[qi]) // vol
            rows = perm[nb * vol:(nb + 1) * vol]
            want = tx.attn_decode(q[:, qi].contiguous(), Kc[:, rows].contiguous(), Vc[:, rows].contiguous(), H, li,
                                  math.sqrt(da), *banks, blk)
            got = tx.attn_decode_blocks(q[:, qi].contiguous(), Kc, Vc, H, qi, math.sqrt(da), *banks, thw, blk)
            assert torch.equal(got, want), (thw, blk, qi)
            pos.fill_(qi)                                   # device cursor + query rows addressed by it
            got = tx.attn_decode_blocks(q, Kc, Vc, H, 0, math.sqrt(da), *banks, thw, blk, ldq=S * H * da, pos=pos, q_pos=H * da)
            assert torch.equal(got, want), (thw, blk, qi, "cursor")


def test_argument_checks(g15):
    from lvt_amd.hip import binding as L
    g, model, v = g15
    Dec = _supports(model.model.decoder, SLICE)
    assert not Dec.supports(model.model.decoder, (6, 8, 8)) and not Dec.supports(model.model.decoder, (16, 8, 12))
    zl = torch.zeros(6 * 8 * 8, 512, device=DEV)
    with pytest.raises(L.LvtError, match="multiple"):
        Dec(model.model.decoder, zl, 1, (6, 8, 8))
    # the C entry refuses before launching: the output keeps its fill
    B, H, da = 1, 2, 128
    buf = torch.zeros(B, 2048, H * da, device=DEV)
    banks = torch.zeros(H, 64, device=DEV)
    o = torch.full((B, H * da), 7.0, device=DEV)

    def call(da_, thw, blk):
        return L.lib().lvt_attn_decode_blocks(L.ptr(buf), H * da, L.ptr(buf), L.ptr(buf), B, H, da_, 0, 1.0, L.ptr(banks),
                                              L.ptr(banks), L.ptr(banks), *thw, *blk, L.ptr(o), C.c_void_p(0), 0, L.stream_ptr())
    assert call(da, (8, 16, 16), (8, 16, 16)) != 0                     # 2048 keys per block
    assert call(64, (8, 8, 8), (4, 8, 8)) != 0                         # da != 128
    assert call(da, (6, 8, 8), (4, 8, 8)) != 0                         # 4 does not divide 6
    assert call(da, (8, 8, 8), (4, 8, 3)) != 0
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    assert call(da, (8, 8, 8), (4, 8, 8)) == 0
    torch.cuda.synchronize()
    assert bool((o != 7.0).all())


def test_memory_rule_lowers_rows_and_samples_in_passes(g15, monkeypatch):
    """With little free memory the rows per group drop and a batch beyond one wave of groups is sampled in passes
    (4 videos at one video per group: three concurrent groups, then the fourth video)."""
    import lvt_amd.modeling.meta_arch.vt as vtmod
    g, model, v = g15
    Dec = _supports(model.model.decoder, SLICE)
    per = Dec.bytes_per_video(model.model.decoder, SLICE)
    assert per == 4 * 1024 * (8 * 3 * 1024 + 512)
    assert vtmod.decode_group_rows(per, 1 << 40) == vtmod.DECODE_GROUP_ROWS
    assert vtmod.decode_group_rows(per, 0) == 1
    free = int(vtmod.MAX_CONCURRENT_GROUPS * per / vtmod.DECODE_MEMORY_FRACTION) + 1024          # one video per group
    assert vtmod.decode_group_rows(per, free) == 1
    monkeypatch.setattr(vtmod, "_free_device_bytes", lambda device: free)
    codes = torch.stack([seeded.seeded_codes("bs.m%d" % i, (16, 4, 16, 16), 4) for i in range(4)])
    with torch.no_grad():
        video = codes.transpose(1, 2).contiguous().to(DEV)
        video[:, :, 15:] = 0
        model._samplers = {}
        out = model.sample_video(video, n_prime=15, temp=1e-4)
        (key, groups), = model._samplers.items()
        assert key[0] == 1 and len(groups) == 1                       # last pass: the fourth video alone
        model._samplers = {}
    assert tuple(out.shape) == (4, 4, 16, 16, 16) and torch.equal(out[:, :, :15].cpu(), codes.transpose(1, 2)[:, :, :15])
    assert 0 <= int(out.min()) and int(out.max()) < 512
    assert int((out[:, :, 15:] != 0).sum()) > 0.9 * out[:, :, 15:].numel()
