"""Python restatement of the f16x2 operand split (lvt_amd/csrc/lvt_common.h: lvt_f16_scale; gemm_engine.hip: f16_split_pair).

a * s = hi + lo / 2048 with s a power of two taken from a scalar >= max |a|, hi = RN16(a s), lo = RN16(2048 (a s - hi)).  The
clamp constant and the split live here once on the Python side: tests/test_host_f16_scale.py holds _scale_of / _split to the
split's specification, and tests/test_gpu_p2.py holds the kernels byte for byte to _image_ref, which is _split laid out as an
image -- one restatement, checked from both sides."""
import torch

SE_MIN, SE_MAX = 2, 243          # clamp of the scale's biased exponent: s * 2048 <= 2^127 stays finite (254 - 11 = 243)
LOSCALE = 2048.0


def _biased_exponent(amax):
    bits = int(torch.tensor([float(amax)], dtype=torch.float32).view(torch.int32))
    return (bits >> 23) & 0xff


def _scale_of(amax, se_max=SE_MAX):
    """lvt_f16_scale: the power of two s with amax * s in [2^14, 2^15) wherever the clamp does not bind."""
    se = min(max(268 - _biased_exponent(amax), SE_MIN), se_max)
    return float(torch.tensor([se << 23], dtype=torch.int32).view(torch.float32))


def _split(x, s):
    """fp32 tensor, scale -> (hi, lo) fp16 in the kernels' own fp32 arithmetic: t = x s, hi = RN16(t), t2 = x (s 2048) (the
    product s * 2048 is formed in fp32 FIRST, as f16_split_pair does), lo = RN16(t2 - 2048 hi)."""
    x = x.float()
    s32 = torch.tensor(s, dtype=torch.float32)
    hi = (x * s32).to(torch.float16)
    s2k = s32 * torch.tensor(LOSCALE, dtype=torch.float32)
    # t2 - 2048 hi is one fused operation on the device; the difference is exact in fp32 whenever t2 is finite, so fp64
    # arithmetic rounded once gives the same bits and propagates inf / nan the same way
    lo = ((x * s2k).double() - LOSCALE * hi.double()).float().to(torch.float16)
    return hi, lo


def _image_ref(x, amax):
    """(rows, K) fp32 -> (rows, K / 32, 2, 32) fp16: the P2 image, the planes of _split under the scale of `amax`."""
    hi, lo = _split(x, _scale_of(amax))
    r, k = x.shape
    return torch.stack([hi.view(r, k // 32, 32), lo.view(r, k // 32, 32)], dim=2)
