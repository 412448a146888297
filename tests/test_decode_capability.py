"""Host-side rules of K/V-cache sampling: which slice geometries decode incrementally, and how many videos a decode
group holds for a given amount of free device memory."""
from types import SimpleNamespace

import torch


def _decoder(blocks, da=128, na=8, d=512):
    layers = [SimpleNamespace(block_size=b, mha=SimpleNamespace(na=na, da=da)) for b in blocks]
    return SimpleNamespace(block_local_attention=layers, linear_projector=SimpleNamespace(weight=torch.empty(d, d, 1, 1, 1)))


def test_supported_slice_geometries():
    from lvt_amd.modeling.autoregressive.incremental import IncrementalDecoder as D
    assert D.supports(_decoder([(4, 8, 8)] * 8), (4, 8, 8))                       # slice == block
    assert D.supports(_decoder([(4, 8, 8)] * 8), (16, 8, 8))                      # DSSVT at 16 frames
    assert D.supports(_decoder([(2, 4, 4), (4, 8, 8)]), (4, 8, 8))                # per-layer blocks, every axis split
    assert not D.supports(_decoder([(4, 8, 8)] * 8), (6, 8, 8))
    assert not D.supports(_decoder([(4, 8, 8), (4, 8, 3)]), (16, 8, 8))
    assert not D.supports(_decoder([(8, 16, 16)]), (8, 16, 16))                   # 2048 keys per query
    assert not D.supports(_decoder([(4, 8, 8)], da=64), (4, 8, 8))
    assert D.bytes_per_video(_decoder([(4, 8, 8)] * 8), (16, 8, 8)) == 4 * 1024 * (8 * 3 * 1024 + 512)


def test_decode_group_rows_follow_free_memory():
    import lvt_amd.modeling.meta_arch.vt as vtmod
    per = 100 << 20
    full = vtmod.MAX_CONCURRENT_GROUPS * vtmod.DECODE_GROUP_ROWS * per / vtmod.DECODE_MEMORY_FRACTION
    assert vtmod.decode_group_rows(per, int(full)) == vtmod.DECODE_GROUP_ROWS
    assert vtmod.decode_group_rows(per, 1 << 50) == vtmod.DECODE_GROUP_ROWS
    assert vtmod.decode_group_rows(per, int(full) // 2) == vtmod.DECODE_GROUP_ROWS // 2
    assert vtmod.decode_group_rows(per, 0) == 1
    # the shipped 256-token slices keep full groups on a device with 40 GB free
    assert vtmod.decode_group_rows(26 << 20, 40 << 30) == vtmod.DECODE_GROUP_ROWS
