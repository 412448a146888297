"""Typed wrappers over the vector-quantiser kernels (csrc/vq.hip)."""
import os

import torch

from . import binding as L


VQ_COARSE = 1 << 17          # include/lvt_hip.h: LVT_VQ_COARSE
VQ_GENERIC = 1 << 22         # include/lvt_hip.h: LVT_VQ_GENERIC (tests / A-B only)
_COARSE_DEFAULT = bool(os.environ.get("LVT_VQ_COARSE"))


def nearest(z, codebooks, P, coarse=None, generic=False):
    """z (rows, ldz) channels-last, codebooks (num, K, D) -> idx int64 (rows/P, num, P).
    coarse=True: the coarse-then-exact search (same exact argmin; opt-in, see csrc/vq.hip for when it pays).
    generic=True: the generic-geometry search even where a specialised kernel exists (tests and A/B measurements; every
    geometry other than D == 64, K in {128, 256, 512} takes it anyway)."""
    L.require(z, codebooks)
    rows, ldz = z.shape
    num, K, D = codebooks.shape
    idx = torch.empty(rows // P, num, P, dtype=torch.int64, device=z.device)
    lib = L.lib()
    nws = max(lib.lvt_vq_nearest_workspace_bytes(rows, num, K), lib.lvt_vq_nearest_generic_workspace_bytes(num, D, K))
    ws = L.workspace(nws, z.device, "vq_nearest")
    flags = L.math_flag() | (VQ_COARSE if (coarse if coarse is not None else _COARSE_DEFAULT) else 0) | (VQ_GENERIC if generic else 0)
    L.check(lib.lvt_vq_nearest(L.ptr(z), rows, ldz, num, D, K, L.ptr(codebooks), L.ptr(idx), P, flags,
                               L.ptr(ws), nws, L.stream_ptr()), "lvt_vq_nearest")
    return idx


def nearest_single(z, weight, chunk_rows=1 << 16):
    """z (rows, D) channels-last rows, weight (K, D): ONE codebook as wide as the rows (CODEBOOK.NUM == 1) -> idx int64 (rows,).
    Scores x E^T on the GEMM engine (rows are walked in chunks: the score matrix of a chunk is rows x K floats), then
    lvt_vq_argmax_scores; see csrc/vq_single.hip."""
    from . import gemm as G
    L.require(z, weight)
    rows, D = z.shape
    K = weight.shape[0]
    idx = torch.empty(rows, dtype=torch.int64, device=z.device)
    w = weight.detach()
    scores = torch.empty(min(rows, chunk_rows), K, dtype=torch.float32, device=z.device)
    for r0 in range(0, rows, chunk_rows):
        r1 = min(rows, r0 + chunk_rows)
        G.gemm(z[r0:r1], w, scores, r1 - r0, K, D)
        L.check(L.lib().lvt_vq_argmax_scores(L.ptr(scores), r1 - r0, K, K, L.ptr(w), D, L.ptr(idx[r0:r1]), L.stream_ptr()),
                "lvt_vq_argmax_scores")
    return idx


def gather(idx, codebooks):
    """idx (n, num, P) int64 -> (n*P, num*D) channels-last rows of selected code vectors."""
    L.require(idx, codebooks)
    n, num, P = idx.shape
    _, K, D = codebooks.shape
    out = torch.empty(n * P, num * D, dtype=torch.float32, device=idx.device)
    L.check(L.lib().lvt_vq_gather(L.ptr(idx), L.ptr(codebooks), n * P, num, D, K, P, L.ptr(out), num * D,
                                  L.stream_ptr()), "lvt_vq_gather")
    if L.f16x2():
        L.set_amax(out, L.amax_of(codebooks))        # rows of the codebooks: their max |.| bounds the selection
    return out


def ema_accumulate(idx, z, K, out=None):
    """-> stats (num, K, D+1): per-code sums and counts of the rows assigned to each code.
    out: a contiguous (num, K, D+1) float32 tensor to write them into (a view of the buffer that one collective sums:
    restart_buffer) instead of a fresh one."""
    L.require(idx, z)
    n, num, P = idx.shape
    rows, ldz = z.shape
    D = ldz // num
    if out is None:
        stats = torch.empty(num, K, D + 1, dtype=torch.float32, device=z.device)
    else:
        L.require(out)
        if out.shape != (num, K, D + 1) or out.dtype != torch.float32 or out.device != z.device:
            raise L.LvtError("ema_accumulate: out must be a float32 (%d, %d, %d) tensor on %s" % (num, K, D + 1, z.device))
        stats = out
    lib = L.lib()
    nws = lib.lvt_vq_ema_workspace_bytes(rows, num, D, K)
    ws = L.workspace(nws, z.device, "ema")
    L.check(lib.lvt_vq_ema_accumulate(L.ptr(idx), L.ptr(z), rows, ldz, num, D, K, P, L.ptr(stats), L.ptr(ws), nws,
                                      L.stream_ptr()), "lvt_vq_ema_accumulate")
    return stats


def ema_finalize(stats, running_size, running_sum, weight, decay=0.99, eps=1e-5):
    L.require(stats, running_size, running_sum, weight)
    num, K, D = weight.shape
    L.check(L.lib().lvt_vq_ema_finalize(L.ptr(stats), num, D, K, decay, eps, L.ptr(running_size),
                                        L.ptr(running_sum), L.ptr(weight), L.stream_ptr()), "lvt_vq_ema_finalize")
    L.drop_amax(weight)         # rewritten in place behind torch's back


# ---- codebook restart (MODEL.CODEBOOK.RESTART; csrc/vq_restart.hip) --------------------------------------------------------
_M64 = (1 << 64) - 1


def _mix64(z):
    """splitmix64's finaliser."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def restart_row(seed, pass_, i, k, R, K):
    """Global row (0 <= r < R) whose sub-vector code k of codebook i takes if it is restarted in pass `pass_`: the plain-Python
    statement of rst_row in csrc/vq_restart.hip.  Code k draws from its own stratum [k R // K, (k + 1) R // K) of the R rows,
    so distinct codes get distinct rows whenever R >= K; an empty stratum (R < K) yields its lower end."""
    h = _mix64((seed ^ (pass_ * 0x9E3779B97F4A7C15) ^ (i << 32 | k)) & _M64)
    lo, hi = k * R // K, (k + 1) * R // K
    return lo + (h % (hi - lo) if hi > lo else 0)


def restart_buffer(num, K, D, device):
    """One flat float32 buffer [stats (num, K, D+1) | cand (num, K, D)] -> (flat, stats view, cand view): a data-parallel pass
    sums it with ONE collective, which completes the statistics and gathers the candidates (all ranks but a row's owner
    contribute zeros)."""
    ns = num * K * (D + 1)
    flat = torch.empty(ns + num * K * D, dtype=torch.float32, device=device)
    return flat, flat[:ns].view(num, K, D + 1), flat[ns:].view(num, K, D)


def restart_candidates(z, cand, P, rank, world, seed, pass_counter, shared_index=False):
    """cand (num, K, D) <- for every code the sub-vector of the row it would be re-seeded from (restart_row), where this rank
    owns that row, zeros elsewhere.  z (rows_local, ldz) channels-last; pass_counter: int64 device scalar (read only)."""
    L.require(z, cand, pass_counter)
    rows, ldz = z.shape
    num, K, D = cand.shape
    L.check(L.lib().lvt_vq_restart_candidates(L.ptr(z), rows, ldz, num, D, K, P, rank, world, seed, L.ptr(pass_counter),
                                              int(bool(shared_index)), L.ptr(cand), L.stream_ptr()),
            "lvt_vq_restart_candidates")


def ema_finalize_restart(stats, cand, running_size, running_sum, weight, threshold, health, restarts_total, pass_counter,
                         decay=0.99, eps=1e-5):
    """ema_finalize, then the restart rule; writes health (num, 3) float32 = (perplexity, dead, restarted), adds `restarted` to
    restarts_total (num,) int64 and advances pass_counter (int64 scalar)."""
    L.require(stats, cand, running_size, running_sum, weight, health, restarts_total, pass_counter)
    num, K, D = weight.shape
    L.check(L.lib().lvt_vq_ema_finalize_restart(L.ptr(stats), L.ptr(cand), num, D, K, decay, eps, threshold,
                                                L.ptr(running_size), L.ptr(running_sum), L.ptr(weight), L.ptr(health),
                                                L.ptr(restarts_total), L.ptr(pass_counter), L.stream_ptr()),
            "lvt_vq_ema_finalize_restart")
    L.drop_amax(weight)         # rewritten in place behind torch's back
