"""NaN-payload guard buffers shared by the kernel conformance tests (test_gpu_gemm_matrix.py, test_gpu_attention_fallback.py,
test_gpu_row_kernels.py, test_gpu_plane_attention.py, test_gpu_flash_matrix.py).

A `Buf` holds its logical elements inside a buffer that is otherwise filled with one recognisable quiet-NaN bit pattern, PAD
elements before and after: a kernel that writes outside its logical output changes payload bits (`outside_untouched`), and one
that reads padding of an input carries a NaN into its output.  PAD = 64 elements keeps the view 16-byte aligned (256 bytes for
float32, 512 for int64), which the float4 entry points need.  `IBuf` is the same for int64 buffers (index outputs, code
tables).  The tests hand `view.data_ptr()` straight to the C entry points (`binding.lib()`) wherever the Python wrapper would
allocate the output itself."""
import torch

DEV = "cuda:0"
PAD = 64                                   # elements of payload before and after every buffer
PAYLOAD = 0x7FC0DEAD                       # a quiet NaN with a recognisable mantissa
IPAYLOAD = 0x7FC0DEAD7FC0DEAD              # the int64 buffers repeat it (read as two floats: the same NaN twice)


def float_bits(x):
    """The int32 bit pattern of the fp32 value x (a `payload` for Buf)."""
    return int(torch.tensor([x], dtype=torch.float32).view(torch.int32))


class Buf:
    """A NaN-payload buffer (PAD floats before and after) holding `values` at element offsets `idx` (same shape).  `payload`:
    another int32 bit pattern for everything that is not a logical element.  A row maximum built with fmaxf drops a NaN, so
    padding that leaked into one shows only with a finite payload (float_bits(3.0e38): the row's scale swallows it)."""

    def __init__(self, idx, values=None, dtype=torch.float32, start=PAD, payload=PAYLOAD):
        self.idx, self.start, self.payload = idx, start, payload
        n = (int(idx.max()) + 1) if idx.numel() else 0
        host = torch.full((start + n + PAD,), payload, dtype=torch.int32).view(torch.float32)
        if values is not None:
            host[start + idx.reshape(-1)] = values.reshape(-1).float()
        self.dev = host.to(DEV)
        self.view = self.dev[start:]
        if dtype != torch.float32:
            self.view = self.view.view(dtype)

    def logical(self):
        return self.dev.cpu()[self.start + self.idx]

    def outside_untouched(self):
        bits = self.dev.cpu().view(torch.int32)
        keep = torch.ones(bits.numel(), dtype=torch.bool)
        keep[self.start + self.idx.reshape(-1)] = False
        return bool((bits[keep] == self.payload).all())

    def bits(self):
        return self.dev.cpu().view(torch.int32)


class IBuf:
    """The int64 variant of `Buf`: PAD int64 of payload before and after, `values` at element offsets `idx`."""

    def __init__(self, idx, values=None, start=PAD):
        self.idx, self.start = idx, start
        n = (int(idx.max()) + 1) if idx.numel() else 0
        host = torch.full((start + n + PAD,), IPAYLOAD, dtype=torch.int64)
        if values is not None:
            host[start + idx.reshape(-1)] = values.reshape(-1).to(torch.int64)
        self.dev = host.to(DEV)
        self.view = self.dev[start:]

    def logical(self):
        return self.dev.cpu()[self.start + self.idx]

    def outside_untouched(self):
        bits = self.dev.cpu()
        keep = torch.ones(bits.numel(), dtype=torch.bool)
        keep[self.start + self.idx.reshape(-1)] = False
        return bool((bits[keep] == IPAYLOAD).all())

    def bits(self):
        return self.dev.cpu()


def dense(*shape):
    """Element offsets of a contiguous tensor of `shape`."""
    n = 1
    for s in shape:
        n *= s
    return torch.arange(n).view(*shape)


def rows_idx(rows, cols, ld):
    """Element offsets of a (rows, cols) matrix with row pitch ld >= cols."""
    return torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]


def fbuf(t):
    """Contiguous float tensor -> Buf holding it."""
    return Buf(dense(*t.shape), t)


def obuf(*shape):
    """An all-payload output Buf of a contiguous `shape`."""
    return Buf(dense(*shape))
