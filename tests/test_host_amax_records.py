"""The max-|.| records of the f16x2 arithmetic (lvt_amd/hip/binding.py) on CPU tensors: the bookkeeping alone, no library.

Rule: after a wrapper writes a tensor through its raw pointer (new_amax for a launch that reports max |C|, drop_amax for one
that does not), no view of that storage -- its base included -- may keep a record older than the write.  Values are written
here through numpy, which (like a kernel) does not bump torch's `_version`."""
import ctypes as C

import pytest
import torch

from lvt_amd.hip import binding as L, gemm as G


@pytest.fixture(autouse=True)
def f16x2_mode():
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    yield
    L.set_math_mode(before)


def _launch(t, value):
    """What an engine launch into `t` does to the bookkeeping: a fresh record, then the kernel writes and reports."""
    slot = L.new_amax(t)
    t.numpy()[...] = value
    slot.fill_(value)
    return slot


def test_write_into_a_view_makes_the_base_record_stale():
    out = torch.zeros(128, 64)
    _launch(out, 1.0)
    assert float(L.amax_of(out)) == 1.0
    v = out[0:96]
    s = _launch(v, 1000.0)
    assert L._valid_amax(out) is None
    assert L.amax_of(v) is s
    with pytest.raises(L.LvtError):          # no valid record: amax_of would scan the tensor anew (a device pass)
        L.amax_of(out)


def test_write_into_the_base_makes_a_view_record_stale():
    out = torch.zeros(128, 64)
    v = out[32:64]
    _launch(v, 1.0)
    s = _launch(out, 1000.0)
    assert L._valid_amax(v) is None
    assert L.amax_of(v) is s                  # the base's fresh record bounds the part


def test_drop_amax_reaches_base_and_overlapping_views():
    buf = torch.zeros(4, 256)
    sb = _launch(buf, 1.0)
    a, b = buf[1], buf[1, 128:]
    sa = L.new_amax(a)
    L.drop_amax(b)                            # an in-place kernel rewrote the second half of row 1
    assert getattr(b, "_lvt_amax", None) is None
    assert L._valid_amax(a) is None and L._valid_amax(buf) is None
    assert sb is not sa


def test_disjoint_views_keep_their_records():
    """Slices of one buffer written one after the other (q / k / v of a packed projection): each keeps its own record, and
    a record made after the writes stays valid -- the bookkeeping still spares the device passes it spared before."""
    buf = torch.zeros(3, 64, 64)
    q, k = buf[0], buf[1]
    s0 = _launch(q, 1.0)
    s1 = _launch(k, 2.0)
    s2 = _launch(buf[2], 3.0)
    assert L.amax_of(q) is s0 and L.amax_of(k) is s1
    whole = L.amax_slot(buf.device).fill_(3.0)
    L.set_amax(buf, whole)
    assert L.amax_of(buf) is whole and L.amax_of(buf[2, 5:9]) is whole
    assert s2 is not whole


def test_records_survive_reads_and_many_unrelated_writes():
    w = torch.zeros(256, 256)
    s = _launch(w, 0.5)
    for _ in range(200):
        _launch(torch.zeros(64), 1.0)         # other storages
    assert L.amax_of(w) is s


def test_set_math_mode_forgets_every_record():
    x = torch.zeros(64, 64)
    _launch(x, 1.0)
    L.set_math_mode("bf16x3")
    L.set_math_mode("f16x2")
    assert L._valid_amax(x) is None


class _FakeLib:
    """Stands in for liblvt_hip.so: records the descriptor of each lvt_gemm_f32 call."""

    def __init__(self):
        self.descs = []

    def lvt_gemm_f32(self, d, ws, nws, stream):
        self.descs.append(C.cast(d, C.POINTER(L.GemmDesc)).contents)
        return 0

    def lvt_gemm_workspace_bytes(self, d):
        return 0


@pytest.fixture
def fake_engine(monkeypatch):
    lib = _FakeLib()
    monkeypatch.setattr(L, "lib", lambda: lib)
    monkeypatch.setattr(L, "require", lambda *t: None)
    monkeypatch.setattr(L, "stream_ptr", lambda: C.c_void_p(0))
    monkeypatch.setattr(L, "workspace", lambda n, dev, tag="default": None)
    return lib


@pytest.mark.parametrize("mode,splits", [("f16x2", 7), ("bf16x3", 1), ("f32", 1)])
def test_gemm_without_a_record_drops_the_old_one(fake_engine, mode, splits):
    """Split-K launches and launches outside f16x2 report no max |C|: they must still forget C's old record, and the
    base's (and a view's) when C is a part of another tensor."""
    L.set_math_mode(mode)
    a, b = torch.zeros(64, 32), torch.zeros(32, 32)
    L.set_amax(a, L.amax_slot(a.device).fill_(1.0))
    L.set_amax(b, L.amax_slot(b.device).fill_(1.0))
    out = torch.zeros(128, 32)
    top = out[:64]
    _launch(out, 1.0)
    L.set_amax(top, L.amax_slot(top.device).fill_(1.0))
    G.gemm(a, b, top, 64, 32, 32, splits=splits)
    assert not fake_engine.descs[-1].c_amax
    assert L._valid_amax(top) is None and L._valid_amax(out) is None


def test_gemm_with_a_record_replaces_it(fake_engine):
    a, b = torch.zeros(64, 32), torch.zeros(32, 32)
    L.set_amax(a, L.amax_slot(a.device).fill_(1.0))
    L.set_amax(b, L.amax_slot(b.device).fill_(1.0))
    out = torch.zeros(128, 32)
    old = _launch(out, 1.0)
    part = out[64:]
    G.gemm(a, b, part, 64, 32, 32)
    d = fake_engine.descs[-1]
    new = L._valid_amax(part)
    assert new is not None and new is not old and d.c_amax == new.data_ptr()
    assert d.a_amax == L.amax_of(a).data_ptr() and d.b_amax == L.amax_of(b).data_ptr()   # operand records reused
    assert L._valid_amax(out) is None
