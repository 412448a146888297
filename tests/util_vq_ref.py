"""fp64 references, bounds and seeded inputs shared by test_gpu_vq_kernels.py, test_gpu_frame_kernels.py and (on the CPU)
test_host_vq_kernel_refs.py.  Nothing here touches a GPU.

Bounds (tests/test_gpu_row_kernels.py).  The reference is the same formula in fp64 on the CPU; err32 is the distance of torch's
fp32 CPU evaluation of it from that (a property of the reference, never of the kernel).
  pointwise outputs, per row:   |got - ref64| <= max(4 err32_row, 2^-21 max |ref64_row|)
  reductions:                   |got - ref64| <= max(4 err32, 2^-21 sum |terms|), the terms summed in fp64
Index outputs of the searches: equal to the fp64 argmin on every row whose fp64 top-2 gap is clear (util_models.margin_ok); on
the other rows the chosen code's fp64 distance lies within the same margin band of the best."""
import functools

import torch

from oracle import lvt_oracle as O
from util_models import margin_ok

EPS = 2.0 ** -21
REL = 1e-5                                        # the margin of util_models.margin_ok
# (activation scale, codebook scale) -> the share of rows a search case may exclude as sub-margin
SCALES = ((1.0, 1.0), (1e-20, 1e10), (1e12, 1e12), (1e-15, 1e-15), (3.0, 1.0 / 512))
CAP_CLEAR, CAP_NEAR_TIE = 0.01, 0.35


def share_cap(zs, es):
    return CAP_NEAR_TIE if (zs, es) == SCALES[4] else CAP_CLEAR


# ---- bounds ---------------------------------------------------------------------------------------------------------
def rows_bad(got, ref64, ref32):
    """Pointwise bound per row (last dim) -> (bool mask of the elements out of bound, err / bound)."""
    err = (got.double() - ref64).abs()
    err32 = (ref32.double() - ref64).abs().amax(-1, keepdim=True)
    tol = torch.maximum(4 * err32, EPS * ref64.abs().amax(-1, keepdim=True))
    return ~(err <= tol), err / tol.clamp_min(1e-300)


def rows_ok(got, ref64, ref32, what):
    bad, ratio = rows_bad(got, ref64, ref32)
    assert not bool(bad.any()), "%s: %d elements out of bound (worst err / bound %.3g, first at %s)" % (
        what, int(bad.sum()), float(ratio[bad].max()), tuple(bad.nonzero()[0].tolist()))


def each_ok(got, ref64, ref32, what):
    """The pointwise bound with every element its own row."""
    rows_ok(got.reshape(-1, 1), ref64.reshape(-1, 1), ref32.reshape(-1, 1), what)


def sum_bad(got, ref64, ref32, terms, floor=EPS):
    """Reduction bound; `terms` = sum |terms| in fp64, elementwise; `floor`: the relative floor (2^-21 unless a test derives
    another from the kernel's summation depth)."""
    err = (got.double() - ref64).abs()
    tol = torch.maximum(4 * (ref32.double() - ref64).abs(), floor * terms)
    return ~(err <= tol), err / tol.clamp_min(1e-300)


def sum_ok(got, ref64, ref32, terms, what, floor=EPS):
    bad, ratio = sum_bad(got, ref64, ref32, terms, floor)
    assert not bool(bad.any()), "%s: %d sums out of bound (worst err / bound %.3g, first at %s)" % (
        what, int(bad.sum()), float(ratio[bad].max()), tuple(bad.nonzero()[0].tolist()))


# ---- the search -----------------------------------------------------------------------------------------------------
def search_ref(rows, cb):
    """(fp64 distances (rows, K), fp64 argmin, clear-margin mask, margin band rel * scale per row)."""
    flat, e = rows.double(), cb.double()
    d64 = (e ** 2).sum(1)[None, :] + (flat ** 2).sum(1, keepdim=True) - 2.0 * flat @ e.t()      # O.vq_margin_fp64's form
    ref = O.vq_margin_fp64(rows, cb)[2] if cb.size(0) > 1 else torch.zeros(rows.size(0), dtype=torch.int64)
    clear = margin_ok(rows, cb, rel=REL) if cb.size(0) > 1 else torch.ones(rows.size(0), dtype=torch.bool)
    band = REL * ((flat ** 2).sum(-1) + (e ** 2).sum(-1).max())
    return d64, ref, clear, band


def banded_index_errors(got, d64, ref, clear, band):
    """-> (rows with a clear margin whose index is not the fp64 argmin, rows whose index is no code or whose code lies
    outside the margin band of the best), as row lists."""
    K = d64.size(1)
    got = got.reshape(-1)
    valid = (got >= 0) & (got < K)
    dg = d64.gather(1, got.clamp(0, K - 1)[:, None])[:, 0]
    inside = valid & ((dg - d64.gather(1, ref[:, None])[:, 0]) <= band)
    wrong = clear & (got != ref)
    return wrong.nonzero().reshape(-1).tolist(), (~inside).nonzero().reshape(-1).tolist()


def check_indices(got, rows, cb, cap, what, ref=None):
    """The banded index check of one group: `got` (n,) int64 against the fp64 search of `rows` in `cb`.  Asserts the share of
    excluded (sub-margin) rows against `cap` as well: the check is no weaker than the cap says."""
    d64, r, clear, band = ref if ref is not None else search_ref(rows, cb)
    excluded = 1.0 - float(clear.float().mean())
    assert excluded <= cap, "%s: %.2f %% of the rows are sub-margin (cap %.0f %%)" % (what, 100 * excluded, 100 * cap)
    wrong, outside = banded_index_errors(got, d64, r, clear, band)
    assert not wrong, "%s: %d clear-margin rows differ from the fp64 argmin, first row %d: got %d, want %d" % (
        what, len(wrong), wrong[0], int(got.reshape(-1)[wrong[0]]), int(r[wrong[0]]))
    assert not outside, "%s: %d rows chose a code outside the margin band, first row %d: got %d" % (
        what, len(outside), outside[0], int(got.reshape(-1)[outside[0]]))


def search_gen(*key):
    return torch.Generator().manual_seed(7000 + sum(int(k) * (11 + 4 * i) for i, k in enumerate(key)))


@functools.lru_cache(maxsize=None)
def search_case(D, K, num, rows, zs, es, zero_row=-1):
    """Seeded operands of one search case: z (rows, num D) and num different codebooks (num, K, D), a zero row on request."""
    g = search_gen(D, K, num, rows, SCALES.index((zs, es)) if (zs, es) in SCALES else 9)
    z = torch.randn(rows, num * D, generator=g) * zs
    cb = torch.randn(num, K, D, generator=g) * es
    if zero_row >= 0:
        z[zero_row] = 0
    return z, cb


@functools.lru_cache(maxsize=None)
def search_case_ref(D, K, num, rows, zs, es, zero_row=-1):
    """search_ref of every group of search_case, computed once and shared by the routes."""
    z, cb = search_case(D, K, num, rows, zs, es, zero_row)
    return [search_ref(z[:, D * g:D * (g + 1)], cb[g]) for g in range(num)]


def excluded_share(D, K, num, rows, zs, es, zero_row=-1):
    refs = search_case_ref(D, K, num, rows, zs, es, zero_row)
    return 1.0 - float(torch.cat([r[2] for r in refs]).float().mean())


def tie_positions(K):
    """Exact duplicates of code 5: both half-waves of a 32-code tile (28: register 12 of half 1; code 5: half 1 as well, 260 /
    300: half 0 and half 1) and, at K = 512, both 256-code parts."""
    return [28, K // 2 + K // 128, 300 * K // 512, K - 1]


def tie_case(D, K, seed=0):
    """-> (codebook (K, D) with the duplicates, queries (256, D), expected indices (256,))."""
    g = search_gen(D, K, 77, seed)
    cb = torch.randn(K, D, generator=g)
    pos = tie_positions(K)
    for j in pos:
        cb[j] = cb[5]
    pick = [5, pos[1], 9, pos[3]]
    return cb, cb[pick].repeat(64, 1).contiguous(), torch.tensor([5, 5, 9, 5]).repeat(64)


# search cases of test_gpu_vq_kernels.py; test_host_vq_kernel_refs.py holds their sub-margin shares to the caps
GEOMETRIES = [(64, 128), (64, 256), (64, 512), (16, 2048), (256, 64)]
PITCH_ROWS_P = [(1, 1), (31, 1), (31, 31), (33, 1), (33, 33), (112, 1), (112, 16), (112, 112)]
TILE2 = dict(num=32, rows=2160, P=16)


def gpu_search_cases():
    """(D, K, num, rows, zs, es, zero_row) of every seeded search case the GPU tests run."""
    out = []
    for D, K in GEOMETRIES:
        for rows in sorted({r for r, _ in PITCH_ROWS_P}):
            out.append((D, K, 3, rows, 1.0, 1.0, -1))
        for zs, es in SCALES:
            out.append((D, K, 3, 112, zs, es, 5))
        if D == 64:
            out.append((D, K, TILE2["num"], TILE2["rows"], 1.0, 1.0, -1))
    return out


# ---- argmax over a score matrix (csrc/vq_single.hip) ------------------------------------------------------------------
def argmax_scores_ref(s, e):
    """fp64 argmax_k (s[r][k] - |e_k|^2 / 2) and the rows whose top-2 gap exceeds 2^-21 (max |s| + max |e|^2 / 2)."""
    hn = 0.5 * (e.double() ** 2).sum(1)
    v = s.double() - hn[None, :]
    if v.size(1) == 1:
        return torch.zeros(v.size(0), dtype=torch.int64), torch.ones(v.size(0), dtype=torch.bool)
    top = torch.topk(v, 2, dim=1)
    clear = (top.values[:, 0] - top.values[:, 1]) > EPS * (s.double().abs().amax(1) + hn.max())
    return top.indices[:, 0], clear


# ---- EMA statistics and update ---------------------------------------------------------------------------------------
def ema_nchunks(rows, num, D, K, num_cu=256):
    """Row chunks of lvt_vq_ema_accumulate (ema_plan in csrc/vq.hip, restated): the workspace holds num * nchunks * K * (D + 1)
    floats, and the reduce kernel sums the chunk partials eight at a time, then a tail."""
    whole = D == 64 and K in (128, 256, 512)
    kt = K if whole else min(K, 73728 // (4 * (D + 1)) // 64 * 64)
    nr = (K + kt - 1) // kt
    target = max(1, (1 if whole else 2) * num_cu // (num * nr))
    rpc = max(256, -(-(-(-rows // target)) // 64) * 64)
    return -(-rows // rpc)


def ema_sums(idx_flat, rows, K, dtype=torch.float64):
    """(sums (K, D), counts (K,), sum of |terms| (K, D)) of the rows assigned to each code, by index_add_ in `dtype`."""
    D = rows.size(1)
    r = rows.to(dtype)
    tot = torch.zeros(K, D, dtype=dtype).index_add_(0, idx_flat, r)
    cnt = torch.zeros(K, dtype=dtype).index_add_(0, idx_flat, torch.ones(rows.size(0), dtype=dtype))
    mag = torch.zeros(K, D, dtype=dtype).index_add_(0, idx_flat, r.abs())
    return tot, cnt, mag


def ema_finalize_ref(stats, rs, rsum, decay, eps, dtype=torch.float64):
    """The reference's update (vq_embedding.py:48-59) in `dtype`: stats (num, K, D + 1) -> (running_size, running_sum, weight).
    (1 - decay) is a double-precision python number there, and a group whose sizes sum to 0 divides 0 by 0."""
    K, D = rs.size(1), rsum.size(2)
    stats, rs, rsum = stats.to(dtype), rs.to(dtype), rsum.to(dtype)
    omd = 1.0 - decay
    if dtype == torch.float32:
        omd = float(torch.tensor(omd, dtype=torch.float32))
    rs = rs * decay + omd * stats[:, :, D]
    rsum = rsum * decay + omd * stats[:, :, :D]
    n = rs.sum(1, keepdim=True)
    size_ = (rs + eps) / (n + K * eps) * n
    return rs, rsum, rsum / size_.unsqueeze(2)
