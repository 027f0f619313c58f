"""Guarded operands for the GPU edge tests (tests/test_gpu_edges*.py): B and C as views into the
middle of one larger allocation, so that what a kernel touches outside its operands is seen.

    flat = [ low band: G elements | payload: rows x cols | high band: G elements ]

G is 128 rows' worth of elements rounded up to a multiple of 128 elements (at least 256 bytes at
every plan dtype), so the payload keeps the 256-byte alignment of the allocation -- the vector
paths assume 16 bytes -- and one whole k-step (32 rows of B) or row block (up to 128 rows of C)
past either end still lies inside the allocation: a stray access is caught, not a fault.

- guarded_B: both bands NaN.  A B row read past row K - 1 (or before row 0) that is not zeroed
  turns the result NaN instead of reading whatever finite data the allocator left there.
- guarded_C: both bands a fixed non-zero bit pattern, the payload NaN.  A store outside C changes
  a band word (assert_guards_intact compares them as integers, bit for bit); an element of C that
  is never written stays NaN and fails the bit-exact comparison.

Nothing here touches the GPU when device is "cpu" (tests/test_guarded.py runs without one).
int_values and assert_bit_exact are those of tests/test_gpu_exact.py; assert_bits adds the 32-bit
case (assert_bit_exact compares 16-bit words)."""
import torch

from test_gpu_exact import assert_bit_exact, int_values  # noqa: F401  (re-exported)

GUARD_ROWS = 128
BAND_BITS = {2: 0x5A5A, 4: 0x5A5A5A5A}  # C's bands: finite, non-zero, the same in every byte pair


def _int_dtype(t):
    return {2: torch.int16, 4: torch.int32}[t.element_size()]


def guard_elems(cols):
    """elements per band: 128 rows of `cols` elements, rounded up to a multiple of 128 elements"""
    return (GUARD_ROWS * int(cols) + 127) // 128 * 128


class Holder:
    """the whole allocation of one guarded operand and what its bands must still hold"""

    def __init__(self, flat, rows, cols):
        self.flat, self.rows, self.cols = flat, int(rows), int(cols)
        self.G = guard_elems(cols)
        iv = flat.view(_int_dtype(flat))
        self.want_lo = iv[:self.G].clone()
        self.want_hi = iv[self.G + self.rows * self.cols:].clone()

    @property
    def payload(self):
        return self.flat[self.G:self.G + self.rows * self.cols].view(self.rows, self.cols)

    def refill(self, value=float("nan")):
        """the payload back to `value` (NaN), the bands as they are"""
        self.payload.fill_(value)


def _flat(rows, cols, dtype, device):
    G = guard_elems(cols)
    return torch.empty(G + int(rows) * int(cols) + G, dtype=dtype, device=device), G


def guarded_B(B_cpu, device):
    """(B, holder): B_cpu (K x N, any device) copied between two NaN bands on `device`"""
    K, N = B_cpu.shape
    flat, G = _flat(K, N, B_cpu.dtype, device)
    flat.fill_(float("nan"))
    flat[G:G + K * N].copy_(B_cpu.reshape(-1))
    h = Holder(flat, K, N)
    return h.payload, h


def guarded_C(M, N, dtype, device):
    """(C, holder): an M x N NaN payload between two bands of BAND_BITS"""
    flat, G = _flat(M, N, dtype, device)
    flat.view(_int_dtype(flat)).fill_(BAND_BITS[flat.element_size()])
    h = Holder(flat, M, N)
    h.refill()
    return h.payload, h


def assert_guards_intact(holder, what=""):
    """both bands bit for bit as they were made; names the first altered word by its row and
    column relative to the payload (row -1 is the row just before it, row `rows` the one after)"""
    iv = holder.flat.view(_int_dtype(holder.flat))
    G, n = holder.G, holder.rows * holder.cols
    for name, got, want, base in (("low", iv[:G], holder.want_lo, -G), ("high", iv[G + n:], holder.want_hi, n)):
        bad = got != want
        n_bad = int(bad.sum().item())
        if n_bad:
            off = base + int(bad.nonzero()[0].item())
            r, c = off // holder.cols, off % holder.cols
            raise AssertionError(f"{what}: {n_bad} words of the {name} guard band altered, first at element offset "
                                 f"{off} = row {r}, column {c} relative to the operand ({holder.rows} x {holder.cols})")


def assert_bits(C, ref, what):
    """C == ref bit for bit: assert_bit_exact for the 16-bit types, the same on 32-bit words"""
    assert C.dtype == ref.dtype and C.shape == ref.shape, (what, C.dtype, ref.dtype, C.shape, ref.shape)
    if C.element_size() == 2:
        return assert_bit_exact(C, ref, what)
    bad = C.view(torch.int32) != ref.view(torch.int32)
    n_bad = int(bad.sum().item())
    if n_bad:
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n_bad} elements differ, first at {i}: {C[i[0], i[1]].item()} vs "
                             f"{ref[i[0], i[1]].item()}")
