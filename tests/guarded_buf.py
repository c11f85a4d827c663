"""Device buffers between guard rows for the GPU tests that call kernels' C entry points directly
(tests/test_gpu_gru_recurrence.py, tests/test_gpu_decoder_kernels.py).  An output starts filled with a sentinel, so that an
element the kernel never wrote and a guard element it did write both show; an input lies between NaN guards and remembers
its bits."""
import numpy as np
import torch

F32 = np.float32
SENT = 0x7FC0DEAD                    # a quiet-NaN bit pattern no kernel produces
SENT64 = 0x7FC0DEAD7FC0DEAD          # the int64 sentinel: far outside any token range
G = 64                               # guard elements on each side of a buffer (256 bytes of float32: the data stays 16-byte aligned)


class Buf:
    """n float32 between two guard rows of G floats; off = 1 starts the data 4 bytes past a 16-byte boundary."""

    def __init__(self, n, fill_bits=None, data=None, off=0):
        self.n, self.lo = int(n), G + off
        total = self.lo + self.n + G
        if data is None:
            self.buf = torch.full((total,), SENT if fill_bits is None else fill_bits, dtype=torch.int32, device='cuda').view(torch.float32)
        else:
            self.buf = torch.full((total,), float('nan'), dtype=torch.float32, device='cuda')
            self.buf[self.lo:self.lo + self.n] = torch.from_numpy(np.array(data, F32).ravel()).cuda()
            self.before = self.bits().clone()
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == 4 * off

    def bits(self):
        return self.buf.view(torch.int32)

    def view(self):
        return self.buf[self.lo:self.lo + self.n]

    def numpy(self, shape):
        return self.view().cpu().numpy().reshape(shape)

    def guards_intact(self):
        b = self.bits()
        return bool((b[:self.lo] == SENT).all()) and bool((b[self.lo + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.bits() == SENT).all())

    def unchanged(self):
        return torch.equal(self.bits(), self.before)


class Buf64:
    """The int64 form: n int64 between two guard rows of G elements.  An output starts as SENT64 everywhere; an input
    (data given) lies between SENT64 guards and remembers its values."""

    def __init__(self, n, data=None):
        self.n, self.lo = int(n), G
        self.buf = torch.full((self.lo + self.n + G,), SENT64, dtype=torch.int64, device='cuda')
        if data is not None:
            self.buf[self.lo:self.lo + self.n] = torch.from_numpy(np.array(data, np.int64).ravel()).cuda()
            self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 8 * self.lo
        assert self.ptr % 16 == 0

    def bits(self):
        return self.buf

    def view(self):
        return self.buf[self.lo:self.lo + self.n]

    def numpy(self, shape):
        return self.view().cpu().numpy().reshape(shape)

    def guards_intact(self):
        return bool((self.buf[:self.lo] == SENT64).all()) and bool((self.buf[self.lo + self.n:] == SENT64).all())

    def untouched(self):
        return bool((self.buf == SENT64).all())

    def unchanged(self):
        return torch.equal(self.buf, self.before)
