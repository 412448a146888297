"""CPU checks of the references and bounds that test_gpu_vq_kernels.py and test_gpu_frame_kernels.py rely on
(tests/util_vq_ref.py): a check that cannot fail proves nothing about a kernel."""
import pytest
import torch

import util_vq_ref as R


def test_banded_check_accepts_the_fp64_argmin_and_rejects_a_far_code():
    z, cb = R.search_case(64, 128, 3, 112, 1.0, 1.0, -1)
    rows, e = z[:, :64], cb[0]
    ref = R.search_ref(rows, e)
    d64, best, clear, band = ref
    R.check_indices(best.clone(), rows, e, R.CAP_CLEAR, "fp64 argmin", ref=ref)
    # the farthest code of row 3: outside the band, and (the row's margin is clear) not the argmin either
    bad = best.clone()
    bad[3] = d64[3].argmax()
    wrong, outside = R.banded_index_errors(bad, *ref)
    assert wrong == [3] and outside == [3]
    with pytest.raises(AssertionError):
        R.check_indices(bad, rows, e, R.CAP_CLEAR, "far code", ref=ref)
    # an index that is no code at all
    bad = best.clone()
    bad[7] = 128
    assert R.banded_index_errors(bad, *ref)[1] == [7]
    bad[7] = -1
    assert R.banded_index_errors(bad, *ref)[1] == [7]


def test_banded_check_on_a_sub_margin_row():
    """Two codes at almost the same distance: either is accepted, a third one is not."""
    g = R.search_gen(1)
    e = torch.randn(64, 16, generator=g)
    e[9] = e[4] * (1 + 2.0 ** -22)
    rows = e[4:5].clone()
    ref = R.search_ref(rows, e)
    assert not bool(ref[2][0])
    for pick, ok in ((4, True), (9, True), (5, False)):
        wrong, outside = R.banded_index_errors(torch.tensor([pick]), *ref)
        assert not wrong and (not outside) == ok, pick
    with pytest.raises(AssertionError):                       # and the cap on excluded rows bites
        R.check_indices(torch.tensor([4]), rows, e, R.CAP_CLEAR, "share", ref=ref)


def test_share_caps_hold_for_the_gpu_seeds():
    """Every seeded search case of test_gpu_vq_kernels.py: at most 1 % of its rows sub-margin, 35 % in the near-tie class."""
    for key in R.gpu_search_cases():
        share = R.excluded_share(*key)
        assert share <= R.share_cap(key[4], key[5]), (key, share)
    near = [R.excluded_share(D, K, 3, 112, 3.0, 1.0 / 512, 5) for D, K in R.GEOMETRIES]
    assert max(near) > R.CAP_CLEAR                            # (the near-tie class does exclude rows: its cap is the other one)


def test_tie_case_and_zero_row():
    for D, K in R.GEOMETRIES:
        cb, z, want = R.tie_case(D, K)
        pos = R.tie_positions(K)
        assert len(set(pos + [5, 9])) == 6 and max(pos) == K - 1 and all(torch.equal(cb[j], cb[5]) for j in pos)
        d = ((z.double()[:, None, :] - cb.double()[None]) ** 2).sum(-1)
        assert torch.equal(d.argmin(1), want) and bool((d.min(1).values == 0).all())
        zz, cbs = R.search_case(D, K, 3, 112, 1.0, 1.0, 5)
        assert bool((zz[5] == 0).all()) and bool(zz[4].abs().sum() > 0)
        assert R.search_case_ref(D, K, 3, 112, 1.0, 1.0, 5)[1][1][5] == (cbs[1].double() ** 2).sum(-1).argmin()


def test_pointwise_bound_bites():
    g = R.search_gen(2)
    x, a, s = torch.rand(37, 12, generator=g) * 4 - 2, torch.rand(12, generator=g) + 0.5, torch.rand(12, generator=g) + 0.5
    ref64, ref32 = (x.double() - a.double()) / s.double(), (x - a) / s
    R.rows_ok(ref32, ref64, ref32, "torch's own fp32 evaluation")
    ulp = 2.0 ** -23 * ref64.abs().amax(-1)
    for r, c in ((0, 0), (17, 5), (36, 11)):
        for sign in (1, -1):
            bad = ref32.clone()
            bad[r, c] += sign * 8 * float(ulp[r])
            mask, _ = R.rows_bad(bad, ref64, ref32)
            assert mask.nonzero().tolist() == [[r, c]]
    nan = ref32.clone()
    nan[2, 3] = float("nan")
    assert R.rows_bad(nan, ref64, ref32)[0].nonzero().tolist() == [[2, 3]]


def test_reduction_bound_bites():
    g = R.search_gen(3)
    x = torch.rand(4097, 12, generator=g) * 2 - 1
    ref64, ref32, terms = x.double().sum(0), x.sum(0), x.double().abs().sum(0)
    R.sum_ok(ref32, ref64, ref32, terms, "torch's own fp32 evaluation")
    bad = ref32.clone()
    bad[5] += 8 * 2.0 ** -23 * float(terms[5])
    assert R.sum_bad(bad, ref64, ref32, terms)[0].nonzero().tolist() == [[5]]
    # one row of 4097 left out of a column sum
    short = x[1:].sum(0)
    assert int(R.sum_bad(short, ref64, ref32, terms)[0].sum()) >= 11


def test_ema_references():
    g = R.search_gen(4)
    rows, K, D = 600, 100, 20
    z, idx = torch.randn(rows, D, generator=g), torch.randint(0, K - 1, (rows,), generator=g)
    tot64, cnt, mag = R.ema_sums(idx, z, K)
    tot32, _, _ = R.ema_sums(idx, z, K, torch.float32)
    assert float(cnt.sum()) == rows and float(cnt[K - 1]) == 0 and bool((tot64[K - 1] == 0).all())
    for k in (0, 57):
        assert torch.allclose(tot64[k], z[idx == k].double().sum(0), rtol=0, atol=1e-12)
    R.sum_ok(tot32, tot64, tot32, mag, "fp32 index_add_")
    # the plan: 256-row chunks while the row count is small; the whole-codebook route reaches every class of the reduce kernel
    assert [R.ema_nchunks(256 * c - 216, 3, 64, 512) for c in (1, 3, 8, 11, 24)] == [1, 3, 8, 11, 24]
    assert R.ema_nchunks(2600, 3, 64, 512) == 11 and R.ema_nchunks(24 * 256, 4, 64, 512) == 24
    assert R.ema_nchunks(2600, 3, 256, 2048) == 5             # 32 code ranges x 3 groups: 5 row chunks at the most
    # finalize: fp32 against fp64 under the pointwise bound; a group without counts only decays
    rs, rsum = torch.rand(2, K, generator=g) + 0.5, torch.randn(2, K, D, generator=g)
    stats = torch.randn(2, K, D + 1, generator=g)
    stats[0, :, D], stats[1, :, D] = torch.randint(0, 9, (K,), generator=g).float(), 0
    r64, r32 = R.ema_finalize_ref(stats, rs, rsum, 0.99, 1e-5), R.ema_finalize_ref(stats, rs, rsum, 0.99, 1e-5, torch.float32)
    for a, b, what in zip(r32, r64, ("running_size", "running_sum", "weight")):
        R.rows_ok(a, b, a, what)
    assert torch.allclose(r64[0][1], rs[1].double() * 0.99)
    n = r64[0][0].sum()
    assert torch.allclose(r64[2][0, 3], r64[1][0, 3] / ((r64[0][0, 3] + 1e-5) / (n + K * 1e-5) * n))


def test_argmax_scores_reference():
    s = torch.tensor([[1.0, 5.0, 2.0], [3.0, 3.0 + 2.0 ** -20, 0.0]])
    e = torch.tensor([[0.0], [2.0], [0.0]])
    ref, clear = R.argmax_scores_ref(s, e)                   # row 0: 1, 3, 2 -> 1; row 1: 3, 1 + 2^-20, 0 -> 0
    assert ref.tolist() == [1, 0] and clear.tolist() == [True, True]
    s[1, 1] = 5.0 + 2.0 ** -22                                # 3 against 3 + 2^-22: inside 2^-21 (5 + 2)
    assert R.argmax_scores_ref(s, e)[1].tolist() == [True, False]
