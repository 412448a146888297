"""The quantiser's kernels (csrc/vq.hip, csrc/vq_single.hip) through their C entry points, each against a plain fp64 (or, for the
gather, a bit-exact) reference, in NaN-payload guard buffers (tests/util_guard.py) with a row pitch the Python wrappers never
pass: lvt_vq_nearest on every search route, lvt_vq_argmax_scores / vq.nearest_single, lvt_vq_gather, lvt_vq_ema_accumulate,
lvt_vq_ema_finalize.

Search routes (flags of lvt_vq_nearest -> kernel), on the specialised geometry D 64, K in {128, 256, 512} unless stated:
  f16x2          LVT_MATH_F16X2                      lvt_vq_nearest_f16x2_kernel<K>
  f32            LVT_MATH_F32                        lvt_vq_nearest_kernel<K>
  bf16x3         neither, with its workspace         lvt_vq_nearest_half_kernel + lvt_vq_nearest_merge_kernel: one 256-code part at
                                                     K 256, two at K 512; K 128 is no multiple of a part: lvt_vq_nearest_kernel<128>
  bf16x3_nows    neither, workspace NULL             lvt_vq_nearest_kernel<K> (the fall-back without the merge scratch)
  coarse         LVT_VQ_COARSE                       lvt_vq_nearest_coarse_kernel<K>
  coarse_f16x2   LVT_VQ_COARSE | LVT_MATH_F16X2      the same kernel: LVT_VQ_COARSE is tested first
  generic_f16x2  LVT_VQ_GENERIC | LVT_MATH_F16X2     lvt_vq_gen_norms_kernel, lvt_vq_gen_planes_kernel, lvt_vq_nearest_gen_f16x2_kernel<D>
  generic_f32    LVT_VQ_GENERIC | LVT_MATH_F32       lvt_vq_gen_norms_kernel, lvt_vq_nearest_gen_f32_kernel<D>
  the two generic routes also at (D 16, K 2048) and (D 256, K 64), there WITHOUT LVT_VQ_GENERIC: the geometry decides.

Index checks (tests/util_vq_ref.py): equal to the fp64 argmin on clear-margin rows (util_models.margin_ok), inside the margin
band on the others, and the share of excluded rows of every case under its cap (1 %; 35 % for the near-tie scale class).
[guard]: everything outside the logical output keeps its payload bits, pitch padding of the inputs holds the NaN payload;
[repeat]: a second launch into fresh buffers gives the same bits."""
import ctypes as C
import functools

import pytest
import torch

from lvt_amd.hip import binding as L, vq
from util_guard import DEV, IPAYLOAD, PAD, PAYLOAD, Buf, IBuf, dense, fbuf, obuf, rows_idx
import util_vq_ref as R

pytestmark = pytest.mark.gpu
F16X2, F32, COARSE, GENERIC = L.MATH_F16X2, L.MATH_F32, vq.VQ_COARSE, vq.VQ_GENERIC
SPECIAL = [(64, 128), (64, 256), (64, 512)]
OTHER = [(16, 2048), (256, 64)]
# route -> (flags on the specialised geometry, flags elsewhere (None: not run there), workspace given)
ROUTES = {
    "f16x2": (F16X2, None, True),
    "f32": (F32, None, True),
    "bf16x3": (0, None, True),
    "bf16x3_nows": (0, None, False),
    "coarse": (COARSE, None, True),
    "coarse_f16x2": (COARSE | F16X2, None, True),
    "generic_f16x2": (GENERIC | F16X2, F16X2, True),
    "generic_f32": (GENERIC | F32, F32, True),
}
ROUTE_IDS = list(ROUTES)


def _geometries(route):
    return SPECIAL + (OTHER if ROUTES[route][1] is not None else [])


def _flags(route, D, K):
    return ROUTES[route][0] if (D, K) in SPECIAL else ROUTES[route][1]


def _call(fn, *args):
    rc = fn(*args, L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg


def _p(b):
    return L.ptr(b.view) if b is not None else C.c_void_p(0)


def _untouched(b):
    bits = b.bits()
    return bool((bits == (PAYLOAD if bits.dtype == torch.int32 else IPAYLOAD)).all())


# ---- A1 lvt_vq_nearest ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _zbuf_cached(key, ldz):
    z, _ = R.search_case(*key)
    return Buf(rows_idx(z.size(0), z.size(1), ldz), z)


@functools.lru_cache(maxsize=8)
def _cbbuf_cached(key):
    return fbuf(R.search_case(*key)[1])


def _nearest(zb, cbb, rows, ldz, num, D, K, P, flags, with_ws=True, ws_view=None, ws_bytes=None):
    """One lvt_vq_nearest launch into a fresh all-payload index buffer -> (rc, message, IBuf)."""
    lib = L.lib()
    idx = IBuf(dense(max(rows // P, 1), num, P))
    need = max(lib.lvt_vq_nearest_workspace_bytes(rows, num, K), lib.lvt_vq_nearest_generic_workspace_bytes(num, D, K), 256)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    wp, nws = (L.ptr(ws), need) if with_ws else (C.c_void_p(0), 0)
    if ws_view is not None:
        wp = L.ptr(ws_view(ws))
    if ws_bytes is not None:
        nws = ws_bytes(need)
    rc, msg = _call(lib.lvt_vq_nearest, _p(zb), rows, ldz, num, D, K, _p(cbb), _p(idx), P, flags, wp, nws)
    return rc, msg, idx


def _search_and_check(route, key, P, ldz, cap):
    """A seeded case (util_vq_ref.search_case) on `route`: the banded index check per group, the case's excluded share under
    `cap`, [guard], [repeat].  -> indices (rows / P, num, P)."""
    D, K, num, rows = key[:4]
    zb, cbb = _zbuf_cached(key, ldz), _cbbuf_cached(key)
    flags, with_ws = _flags(route, D, K), ROUTES[route][2]
    rc, msg, idx = _nearest(zb, cbb, rows, ldz, num, D, K, P, flags, with_ws)
    assert rc == 0, msg
    got = idx.logical()
    what = "%s D %d K %d rows %d P %d ldz %d scales %s" % (route, D, K, rows, P, ldz, key[4:6])
    share = R.excluded_share(*key)
    assert share <= cap, "%s: %.2f %% of the rows are sub-margin (cap %.0f %%)" % (what, 100 * share, 100 * cap)
    z, cb = R.search_case(*key)
    for g, ref in enumerate(R.search_case_ref(*key)):
        R.check_indices(got[:, g].reshape(-1), z[:, D * g:D * (g + 1)], cb[g], 1.0, "%s group %d" % (what, g), ref=ref)
    assert idx.outside_untouched(), what + ": wrote outside the index layout"
    rc, msg, idx2 = _nearest(zb, cbb, rows, ldz, num, D, K, P, flags, with_ws)
    assert rc == 0 and torch.equal(idx.bits(), idx2.bits()), what + ": a second launch gave other bits"
    return got


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_nearest_pitch_groups_and_layout(route):
    """Three groups with a codebook each, ldz = num D + 4 and + 20 (payload padding), rows in {1, 31, 33, 112}: less than one
    32-row tile, one row into a second tile, 3.5 tiles; P in {1, 16, rows}: the index layout (rows / P, num, P).  Every wave has at
    most one tile.  Kernel per route: the table in the module docstring."""
    for D, K in _geometries(route):
        for rows, P in R.PITCH_ROWS_P:
            for pad in (4, 20):
                _search_and_check(route, (D, K, 3, rows, 1.0, 1.0, -1), P, 3 * D + pad, R.CAP_CLEAR)


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_nearest_scale_classes_and_zero_row(route):
    """The five scale classes of test_gpu_vq_geometry.py (operands 1e-20 .. 1e12; the last one near ties: at most 35 % of the
    rows excluded, 1 % in the others) on 112 rows x 3 groups, ldz = num D + 4.  Row 5 is all zero: it takes the code of smallest
    norm, on every route."""
    for D, K in _geometries(route):
        for zs, es in R.SCALES:
            key = (D, K, 3, 112, zs, es, 5)
            got = _search_and_check(route, key, 16, 3 * D + 4, R.share_cap(zs, es))
            cb = R.search_case(*key)[1]
            for g in range(3):
                assert int(got[0, g, 5]) == int((cb[g].double() ** 2).sum(-1).argmin()), (route, D, K, zs, es, g)


@pytest.mark.parametrize("K", [128, 256, 512])
@pytest.mark.parametrize("route", ROUTE_IDS)
def test_nearest_second_tile_per_wave(route, K):
    """num 32, rows 2160, P 16, D 64, ldz = num D + 4: min(256 / 32, ceil(68 / 8)) = 8 workgroups per group, 64 waves for 67.5
    tiles -- waves 0 .. 3 of workgroup 0 take a second tile (`tile += stride`; the f16x2 kernel prefetches it with
    load_rows(tile + tstride) and clamps the 16 rows past the end to row 2159; the coarse kernel reuses its per-wave candidate
    lists), and the last tile is half full.  The half kernel (bf16x3) gets 256 / (32 groups x parts) workgroups per (group, part):
    8 at K 256, 4 at K 512, where 32 waves share the 68 tiles -- up to three tiles per wave.  The generic kernels hold one tile per wave by construction (9 workgroups
    of 256 rows per group).  randn operands at scale 1."""
    _search_and_check(route, (64, K, R.TILE2["num"], R.TILE2["rows"], 1.0, 1.0, -1), R.TILE2["P"], 32 * 64 + 4, R.CAP_CLEAR)


def _exact_search(route, D, K, cb, z, P):
    """z (rows, D) against ONE codebook used by two groups -> indices (rows, 2)."""
    rows, ldz = z.size(0), 2 * D + 4
    zb = Buf(rows_idx(rows, 2 * D, ldz), z.repeat(1, 2))
    cbb = fbuf(torch.stack([cb, cb]))
    rc, msg, idx = _nearest(zb, cbb, rows, ldz, 2, D, K, P, _flags(route, D, K), ROUTES[route][2])
    assert rc == 0, msg
    assert idx.outside_untouched()
    return idx.logical().permute(0, 2, 1).reshape(rows, 2)


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_nearest_exact_ties(route):
    """Exact duplicates of code 5 at 28 and (K 512) 260, 300, 511 -- both half-waves of a 32-code tile and both 256-code parts,
    positions scaled with K -- queried with codes 5, 260, 9, 511 over 256 rows: the lowest index wins (5, 5, 9, 5).  This is the
    fp32 kernel's cross-lane `ob == best && oi < bidx` reduction, the merge kernel's strict `<` between the parts, the coarse
    kernel's candidate walk, and the generic kernels' order across code tiles.  Then a codebook whose K codes are all equal
    (the coarse kernel's overflow path: every code is a candidate): index 0 on every row."""
    for D, K in _geometries(route):
        cb, z, want = R.tie_case(D, K)
        got = _exact_search(route, D, K, cb, z, 64)
        assert torch.equal(got[:, 0], want) and torch.equal(got[:, 1], want), (route, D, K, got[:8].tolist())
        g = R.search_gen(D, K, 78)
        same = torch.randn(1, D, generator=g).repeat(K, 1)
        zz = torch.randn(64, D, generator=g)
        zz[3], zz[40] = same[0], 0
        got = _exact_search(route, D, K, same, zz, 16)
        assert bool((got == 0).all()), (route, D, K, got.reshape(-1)[:16].tolist())


@pytest.mark.parametrize("route", ["f16x2", "f32", "bf16x3", "coarse", "generic_f16x2", "generic_f32"])
def test_nearest_refusals(route):
    """LVT_EINVAL for rows % P, ldz % 4, ldz < num D, z off 16-byte alignment, D 24, K 96; LVT_EWORKSPACE for the generic
    route's workspace (null, one byte short, 16 bytes off its 256-byte alignment).  The index buffer stays all payload."""
    D, K, num, rows = 64, 128, 3, 32
    flags = ROUTES[route][0]
    z = torch.zeros(rows + 1, num * D + 8)
    cbb = fbuf(torch.zeros(num, K, D))
    zb = Buf(rows_idx(rows + 1, num * D + 8, num * D + 8), z)
    zoff = Buf(rows_idx(rows + 1, num * D + 8, num * D + 8), z, start=PAD + 1)
    cases = [dict(P=5), dict(ldz=num * D + 2), dict(ldz=num * D - 4), dict(z=zoff), dict(D=24), dict(K=96)]
    for kw in cases:
        rc, msg, idx = _nearest(kw.get("z", zb), cbb, rows, kw.get("ldz", num * D + 4), num, kw.get("D", D), kw.get("K", K),
                                kw.get("P", 16), flags)
        assert rc == -1 and "vq_nearest" in msg, (kw, rc, msg)
        assert _untouched(idx), kw
    if flags & GENERIC:
        for kw in (dict(with_ws=False), dict(ws_bytes=lambda n: L.lib().lvt_vq_nearest_generic_workspace_bytes(num, D, K) - 1),
                   dict(ws_view=lambda ws: ws[16:])):
            rc, msg, idx = _nearest(zb, cbb, rows, num * D + 4, num, D, K, 16, flags, **kw)
            assert rc == -2 and "workspace" in msg, (sorted(kw), rc, msg)
            assert _untouched(idx), sorted(kw)


# ---- A2 lvt_vq_argmax_scores, vq.nearest_single ----------------------------------------------------------------------
def _argmax_scores(s, ld, e):
    rows, K = s.shape
    sb, eb, idx = Buf(rows_idx(rows, K, ld), s), fbuf(e), IBuf(dense(rows))
    rc, msg = _call(L.lib().lvt_vq_argmax_scores, _p(sb), rows, K, ld, _p(eb), e.size(1), _p(idx))
    return rc, msg, idx


def _check_argmax_scores(rows, K, D, pad):
    g = R.search_gen(rows, K, D, 5)
    s, e = torch.randn(rows, K, generator=g) * 3, torch.randn(K, D, generator=g)
    dup = [K // 2 + 1, K - 1] + ([71] if K >= 128 else [])   # another lane, the last lane's last code, the same lane (7 + 64)
    if K >= 64:                                            # exact ties on the even rows: duplicated codes with duplicated scores
        s[::2, 7] = 400.0                                  # (far above every other score minus half norm)
        for j in dup:
            e[j], s[::2, j] = e[7], s[::2, 7]
    rc, msg, idx = _argmax_scores(s, K + pad, e)
    assert rc == 0, msg
    got = idx.logical()
    ref, clear = R.argmax_scores_ref(s, e)
    if K >= 64:                                            # the tied rows: equal maxima by construction, the lowest index is 7
        ref[::2], clear[::2] = 7, True
    assert float(clear.float().mean()) >= 0.99, (rows, K, D)
    assert torch.equal(got[clear], ref[clear]), (rows, K, D, pad)
    assert bool(((got >= 0) & (got < K)).all()) and idx.outside_untouched()
    rc, msg, idx2 = _argmax_scores(s, K + pad, e)
    assert rc == 0 and torch.equal(idx.bits(), idx2.bits())


@pytest.mark.parametrize("K", [1, 63, 64, 65, 1000, 2048])
def test_argmax_scores(K):
    """lvt_vq_argmax_scores_kernel, one wave per row: K below, at and above the 64 lanes (K 1: 63 lanes hold no candidate),
    D in {1, 64, 256} (the half norms' FMA chain), ld = K and K + 3 (payload padding), rows in {1, 5}; exact ties between
    duplicated codes resolve to the lowest index."""
    for D in (1, 64, 256):
        for rows in (1, 5):
            for pad in (0, 3):
                _check_argmax_scores(rows, K, D, pad)


def test_argmax_scores_grid_stride():
    """16387 rows, K 64: more than 4096 workgroups x 4 rows, the rows 16384 .. 16386 come on the loop's second trip."""
    _check_argmax_scores(16387, 64, 16, 3)


def test_argmax_scores_three_way_tie():
    """Three equal scores over equal codes in lanes 7, 33 and 63: index 7."""
    s = torch.zeros(2, 64)
    s[:, 7] = s[:, 33] = s[:, 63] = 40.0
    e = torch.ones(64, 1)
    rc, msg, idx = _argmax_scores(s, 64, e)
    assert rc == 0 and idx.logical().tolist() == [7, 7]


def test_nearest_single_chunks():
    """vq.nearest_single on 300 rows with chunk_rows = 128 (chunks of 128, 128, 44 rows into one reused score buffer) equals the
    unchunked call bit for bit, and the fp64 search on clear-margin rows."""
    g = R.search_gen(300, 3)
    z, w = torch.randn(300, 256, generator=g), torch.randn(1024, 256, generator=g)
    zd, wd = z.to(DEV), w.to(DEV)
    whole = vq.nearest_single(zd, wd).cpu()
    parts = vq.nearest_single(zd, wd, chunk_rows=128).cpu()
    assert torch.equal(whole, parts), "%d rows differ" % int((whole != parts).sum())
    R.check_indices(whole, z, w, R.CAP_CLEAR, "nearest_single")


# ---- A3 lvt_vq_gather ----------------------------------------------------------------------------------------------
def _gather(idx, cbb, rows, num, D, K, P, ldo):
    out = Buf(rows_idx(rows, num * D, ldo))
    rc, msg = _call(L.lib().lvt_vq_gather, L.ptr(idx), _p(cbb), rows, num, D, K, P, _p(out), ldo)
    return rc, msg, out


@pytest.mark.parametrize("D", [4, 20, 64, 256])
def test_gather(D):
    """lvt_vq_gather_kernel<64> (D 64) and <0> (run-time width), K in {1, 100, 512, 2048}, ldo = num D and + 8: 35 rows x 3 groups
    x D / 4 float4 items, never a multiple of the 1024 items a workgroup moves per trip (the unroll's tail), indices 0 and K - 1
    included.  Bit-equal to codebooks[g][idx]."""
    n, num, P = 5, 3, 7
    for K in (1, 100, 512, 2048):
        g = R.search_gen(D, K, 31)
        cb = torch.randn(num, K, D, generator=g)
        idx = torch.randint(0, K, (n, num, P), generator=g)
        idx[0, :, 0], idx[-1, :, -1] = 0, K - 1
        ref = torch.stack([cb[q][idx[:, q]] for q in range(num)], 2).reshape(n * P, num * D)
        cbb, idd = fbuf(cb), idx.to(DEV)
        for ldo in (num * D, num * D + 8):
            rc, msg, out = _gather(idd, cbb, n * P, num, D, K, P, ldo)
            assert rc == 0, msg
            assert torch.equal(out.logical().view(torch.int32), ref.view(torch.int32)), (D, K, ldo)
            assert out.outside_untouched(), (D, K, ldo)


def test_gather_grid_stride():
    """rows 32832, num 4, D 256 (134 MB of output): 8404992 float4 items, more than 8192 workgroups x 1024 -- the 16384 items
    past the first trip of the grid-stride loop.  Compared on the device; the guard is the payload behind the last element."""
    rows, num, D, K, P = 32832, 4, 256, 64, 16
    g = R.search_gen(rows, 32)
    cb = torch.randn(num, K, D, generator=g)
    idx = torch.randint(0, K, (rows // P, num, P), generator=g)
    cbd, idd = cb.to(DEV), idx.to(DEV)
    n = rows * num * D
    out = torch.full((n + PAD,), PAYLOAD, dtype=torch.int32, device=DEV)
    rc, msg = _call(L.lib().lvt_vq_gather, L.ptr(idd), L.ptr(cbd), rows, num, D, K, P, L.ptr(out), num * D)
    assert rc == 0, msg
    ref = torch.stack([cbd[q][idd[:, q]] for q in range(num)], 2).reshape(-1)
    assert torch.equal(out[:n], ref.view(torch.int32))
    assert bool((out[n:] == PAYLOAD).all())


# ---- A4 lvt_vq_ema_accumulate --------------------------------------------------------------------------------------
EMA_D, EMA_K, EMA_CLASSES = [4, 20, 64, 100, 256], [1, 100, 128, 512, 2048], [1, 3, 8, 11, 24]


def _ema_rows(cls):
    """With 256-row chunks (the floor of the plan): cls chunks, the last one 40 rows -- no multiple of the 64-row tile."""
    return 256 * cls - 216


def _ema_cases(D):
    """(K, class) pairs whose plan gives exactly `class` chunks at _ema_rows(class): the whole-codebook route (D 64, K 128 | 512)
    reaches all five; a ranged plan with many code ranges has fewer row chunks (2 x 256 / (3 groups x ranges))."""
    return [(K, c) for K in EMA_K for c in EMA_CLASSES if R.ema_nchunks(_ema_rows(c), 3, D, K) == c]


def _ema_accumulate(idd, zb, rows, ldz, num, D, K, P, ws_bytes=None):
    lib = L.lib()
    stats = obuf(num, K, D + 1)
    need = lib.lvt_vq_ema_workspace_bytes(rows, num, D, K)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    nws = need if ws_bytes is None else ws_bytes
    rc, msg = _call(lib.lvt_vq_ema_accumulate, L.ptr(idd), _p(zb), rows, ldz, num, D, K, P, _p(stats), L.ptr(ws) if nws else C.c_void_p(0), nws)
    return rc, msg, stats


def _check_ema_accumulate(D, K, cls):
    num, rows = 3, _ema_rows(cls)
    P = 8 if rows % 8 == 0 else 1
    need = L.lib().lvt_vq_ema_workspace_bytes(rows, num, D, K)
    assert need == 4 * num * K * (D + 1) * cls, "D %d K %d rows %d: %d chunks, meant for %d" % (D, K, rows, need // (4 * num * K * (D + 1)), cls)
    g = R.search_gen(D, K, cls, 41)
    z = torch.randn(rows, num * D, generator=g)
    idx = torch.randint(0, K, (rows // P, num, P), generator=g)                  # group 0: uniform
    third = idx[:, 1].reshape(-1)
    third[::3] = K - 1                                                         # group 1: one code takes a third of the rows
    idx[:, 1] = third.view(-1, P)
    idx[:, 2] = K // 2                                                          # group 2: one code takes all rows
    ldz = num * D + 4
    zb, idd = Buf(rows_idx(rows, num * D, ldz), z), idx.to(DEV)
    rc, msg, stats = _ema_accumulate(idd, zb, rows, ldz, num, D, K, P)
    assert rc == 0, msg
    got = stats.logical()
    for q in range(num):
        flat, zr = idx[:, q].reshape(-1), z[:, D * q:D * (q + 1)]
        tot64, cnt64, mag64 = R.ema_sums(flat, zr, K)
        tot32, _, _ = R.ema_sums(flat, zr, K, torch.float32)
        assert torch.equal(got[q, :, D].double(), cnt64), "D %d K %d class %d group %d: counts" % (D, K, cls, q)
        R.sum_ok(got[q, :, :D], tot64, tot32, mag64, "D %d K %d class %d group %d: sums" % (D, K, cls, q))
        empty = cnt64 == 0
        assert bool((got[q][empty].view(torch.int32) == 0).all()), "a code without rows is not exactly zero"
    assert stats.outside_untouched()
    rc, msg, stats2 = _ema_accumulate(idd, zb, rows, ldz, num, D, K, P)
    assert rc == 0 and torch.equal(stats.bits(), stats2.bits()), "a second launch gave other bits"


@pytest.mark.parametrize("D", EMA_D)
def test_ema_accumulate(D):
    """lvt_vq_ema_partial_kernel<64, K> (D 64, K 128 | 512: the whole codebook in LDS) and <0, 0> (code ranges), then
    lvt_vq_ema_reduce_kernel over 1, 3, 8, 11 or 24 chunk partials: the tail loop alone (1, 3), one group of eight alone (8),
    a group and a tail of three in one call (11), three groups (24) -- wherever the geometry's plan reaches the class
    (_ema_cases).  Three groups, ldz = num D + 4 with payload padding, the last chunk 40 rows; a uniform, a skewed and a
    one-code histogram; codes without rows give exact zeros.  Counts exact, every sum element under the reduction bound."""
    cases = _ema_cases(D)
    assert {c for _, c in cases} >= ({1, 3, 8, 11, 24} if D <= 64 else {1, 3}), cases
    for K, cls in cases:
        _check_ema_accumulate(D, K, cls)


def test_ema_accumulate_reduce_group_and_tail_on_the_whole_codebook_route():
    """2600 rows, D 64, K 512: 11 chunks on lvt_vq_ema_partial_kernel<64, 512> -- both loops of the reduce kernel in one call."""
    assert _ema_rows(11) == 2600 and (512, 11) in _ema_cases(64) and (128, 24) in _ema_cases(64)
    _check_ema_accumulate(64, 512, 11)


def test_ema_accumulate_short_workspace():
    """One byte short, or none: LVT_EWORKSPACE, `stats` untouched."""
    rows, num, D, K = 600, 3, 64, 128
    zb, idd = fbuf(torch.zeros(rows, num * D)), torch.zeros(rows, num, 1, dtype=torch.int64, device=DEV)
    need = L.lib().lvt_vq_ema_workspace_bytes(rows, num, D, K)
    for nws in (need - 1, 0):
        rc, msg, stats = _ema_accumulate(idd, zb, rows, num * D, num, D, K, 1, ws_bytes=nws)
        assert rc == -2 and "workspace" in msg, (nws, rc, msg)
        assert _untouched(stats)


# ---- A5 lvt_vq_ema_finalize ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("num,K,D", [(1, 1, 4), (2, 100, 20), (3, 128, 64), (1, 2048, 256), (2, 64, 1)])
def test_ema_finalize(num, K, D):
    """lvt_vq_ema_finalize_kernel<64> (D 64) and <0>: running_size, running_sum and the new codebook pointwise per row against
    the fp64 update of vq_embedding.py:48-59.  The last group's counts are all zero (its sizes only decay); code 0 of group 0
    has a running size of 1e-12 (the Laplace smoothing keeps its divisor at eps n / (n + K eps))."""
    decay, eps = 0.99, 1e-5
    g = R.search_gen(num, K, D, 51)
    rs = torch.rand(num, K, generator=g) * 4 + 0.1
    rs[0, 0] = 1e-12
    rsum = torch.randn(num, K, D, generator=g)
    stats = torch.randn(num, K, D + 1, generator=g)
    stats[:, :, D] = torch.randint(0, 40, (num, K), generator=g).float()
    stats[num - 1, :, D] = 0
    stats[0, 0, D] = 0
    decay32 = float(torch.tensor(decay, dtype=torch.float32))                   # the entry point takes floats
    eps32 = float(torch.tensor(eps, dtype=torch.float32))

    def run():
        sb, rsb, rsumb, wb = fbuf(stats), fbuf(rs), fbuf(rsum), obuf(num, K, D)
        rc, msg = _call(L.lib().lvt_vq_ema_finalize, _p(sb), num, D, K, decay, eps, _p(rsb), _p(rsumb), _p(wb))
        assert rc == 0, msg
        return rsb, rsumb, wb

    rsb, rsumb, wb = run()
    r64 = R.ema_finalize_ref(stats, rs, rsum, decay32, eps32)
    r32 = R.ema_finalize_ref(stats, rs, rsum, decay32, eps32, torch.float32)
    R.rows_ok(rsb.logical(), r64[0], r32[0], "running_size")
    R.rows_ok(rsumb.logical(), r64[1], r32[1], "running_sum")
    R.rows_ok(wb.logical(), r64[2], r32[2], "weight")
    assert all(b.outside_untouched() for b in (rsb, rsumb, wb))
    again = run()
    assert all(torch.equal(a.bits(), b.bits()) for a, b in zip((rsb, rsumb, wb), again)), "a second launch gave other bits"
