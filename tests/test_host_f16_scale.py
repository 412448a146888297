"""The f16x2 operand split against its specification, for EVERY exponent of the max-|.| scalar (CPU, fp32 arithmetic).

An operand is scaled by a power of two s taken from a scalar >= max |a| (lvt_f16_scale, lvt_amd/csrc/lvt_common.h), then split
into hi = RN16(a s) and lo = RN16(2048 (a s - hi)), the second product formed as a * (s * 2048) in fp32 (f16_split_pair,
gemm_engine.hip).  tests/util_f16_scale.py restates both in the same fp32 operations; tests/test_gpu_p2.py holds the kernels
to that restatement byte for byte, and this file holds the restatement to the specification:

  * s, s * 2048, hi and lo are finite for every biased exponent eb in 0..254 of the scalar (0: a zero or subnormal max);
  * (hi + lo / 2048) / s reproduces a within 2^-22 max wherever a s is a normal fp16 number;
  * a zero element gives hi == lo == +0 bit for bit.

This is the test of the clamp constant: with the upper clamp of the scale's exponent at 252 (s up to 2^125) it FAILS for every
eb <= 24, i.e. every operand with max |a| < 2^-102 -- s * 2048 is +inf there, a zero element gives lo = 0 * inf = NaN and a
non-zero one lo = inf -- and passes with 243 (s * 2048 <= 2^127).  test_clamp_252_breaks_exactly_eb_le_24 pins that finding."""
import pytest
import torch

from util_f16_scale import LOSCALE, SE_MAX, _scale_of, _split

F16_MIN_NORMAL = 2.0 ** -14


def _maxima(eb):
    """max-|.| scalars with biased exponent eb: the bottom and the top of the binade (eb = 0: zero and two subnormals)."""
    if eb == 0:
        return [0.0, 2.0 ** -149, 2.0 ** -127 + 2.0 ** -130]
    return [2.0 ** (eb - 127), float(torch.tensor(2.0 ** (eb - 127), dtype=torch.float32) * (2.0 - 2.0 ** -23))]


def _violations(amax, se_max):
    """The specification's clauses that the split under `se_max` breaks for an operand of max `amax` (empty: it holds)."""
    bad = []
    s = _scale_of(amax, se_max)
    s2k = torch.tensor(s, dtype=torch.float32) * torch.tensor(LOSCALE, dtype=torch.float32)
    if not (torch.isfinite(torch.tensor(s)) and bool(torch.isfinite(s2k))):
        bad.append("s or s * 2048 is not finite")
    a = torch.tensor([0.0, amax, -amax, amax * 0.5, amax * 2.0 ** -12, amax * 2.0 ** -20], dtype=torch.float32)
    hi, lo = _split(a, s)
    if not (bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())):
        bad.append("hi or lo is not finite")
    if int(hi.view(torch.int16)[0]) != 0 or int(lo.view(torch.int16)[0]) != 0:
        bad.append("a zero element is not (+0, +0)")
    a64 = a.double()
    normal = (a64 * s).abs() >= F16_MIN_NORMAL
    back = (hi.double() + lo.double() / LOSCALE) / s
    err = (back - a64).abs()
    if not bool((err[normal] <= 2.0 ** -22 * amax).all()):                   # (a NaN compares false: counted)
        bad.append("reconstruction error above 2^-22 max")
    return bad


@pytest.mark.parametrize("eb", range(255))
def test_split_specification(eb):
    for amax in _maxima(eb):
        assert _violations(amax, SE_MAX) == [], (eb, amax)


def test_scale_is_unchanged_above_2_pow_minus_102():
    """The clamp binds only below 2^-102: every larger max gets max * s in [2^14, 2^15), as before (bit-identical planes)."""
    for eb in range(25, 255):
        for amax in _maxima(eb):
            assert _scale_of(amax) == 2.0 ** (141 - eb) and 2.0 ** 14 <= amax * _scale_of(amax) < 2.0 ** 15


def test_clamp_252_breaks_exactly_eb_le_24():
    """The finding this file exists for: under the former clamp the specification fails for eb <= 24 and only there."""
    for eb in range(255):
        broken = any(_violations(amax, 252) for amax in _maxima(eb))
        assert broken == (eb <= 24), eb
