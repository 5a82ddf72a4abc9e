"""Memory-behaviour helpers for the kernel tests: guard-banded device buffers and self-describing bit-identity checks.

`Guarded` puts a payload between two guard bands inside ONE allocation the test owns, fills the whole of it with a
byte pattern, and reports afterwards which guard bytes changed. A kernel that stores past either end of its output (or
its workspace) then shows as a changed guard instead of as a silent write into somebody else's allocation; a kernel that
reads a workspace slot nobody wrote in this call reads the pattern, and the pattern is chosen to make that visible:

  nan   0x7FC07FC0  a quiet NaN in fp32, and both bf16 halves are NaN as well
  ones  0xFFFFFFFF  NaN in fp32 and bf16, -1 as an integer
  zero  0x00000000
  big   0x7F7F7F7F  finite in fp32 (3.4e38) and bf16 (3.4e38): any sum that takes it in overflows
  unit  0x3F803F80  finite and plausible (1.0019 in fp32, 1.0 in both bf16 halves): a read of it changes results
                    quietly instead of producing NaN, so only a comparison across patterns sees it

Limits: a guard band is 64 KiB on each side. A stray store that lands farther away than that from the payload is not
seen by `check()`; nor is a stray store into the payload of the same buffer (the output checks see those as values).

`assert_same_bits(a, b, what, axes)` passes exactly when `torch.equal(a, b)` does (NaN is unequal to NaN). On failure
its message says how many elements differ, by how much, how many NaNs each side holds, the index extents of the
differing elements on each named axis and the first eight differing indices, so that a rare failure leaves evidence.
"""
import torch

GUARD_BYTES = 64 * 1024
ALIGN = 256

PATTERNS = {
    "nan": 0x7FC07FC0,
    "ones": 0xFFFFFFFF,
    "zero": 0x00000000,
    "big": 0x7F7F7F7F,
    "unit": 0x3F803F80,
}


def _as_int32(word):
    """A 32-bit pattern as the signed value torch.int32 stores."""
    return word - (1 << 32) if word >= 1 << 31 else word


class Guarded:
    """One device allocation: [front guard >= 64 KiB][payload: exactly `nbytes`, 256-byte aligned][back guard >= 64 KiB].

    The whole allocation (guards and payload) holds `pattern` after construction and after `fill()`; `check()` compares
    both guards with the pattern of the last fill."""

    def __init__(self, nbytes, device, pattern="nan", guard=GUARD_BYTES):
        if nbytes < 0:
            raise ValueError(f"nbytes must be >= 0, got {nbytes}")
        if guard < GUARD_BYTES or guard % 4:
            raise ValueError(f"guard must be a multiple of 4 of at least {GUARD_BYTES} bytes, got {guard}")
        self.nbytes = int(nbytes)
        words = (guard + (ALIGN - 4) + self.nbytes + 3 + guard) // 4  # room to shift the payload onto a 256-byte boundary
        self._buf = torch.empty(words, dtype=torch.int32, device=device)
        base = self._buf.data_ptr()
        self.start = guard + (-(base + guard)) % ALIGN  # payload offset in bytes from the allocation start (multiple of 4)
        self.end = self.start + self.nbytes
        self.total = words * 4
        self.pattern = None
        self.fill(pattern)

    @property
    def ptr(self):
        """Device address of the payload's first byte."""
        return self._buf.data_ptr() + self.start

    def _bytes(self):
        return self._buf.view(torch.uint8)

    def fill(self, pattern):
        """Write `pattern` (a PATTERNS key) over the guards and the payload."""
        self._buf.fill_(_as_int32(PATTERNS[pattern]))
        self.pattern = pattern
        return self

    def fill_payload(self, pattern):
        """Write `pattern` over the payload only (the guards keep the pattern `check()` compares with)."""
        word = torch.tensor([_as_int32(PATTERNS[pattern])], dtype=torch.int32, device=self._buf.device)
        rep = word.view(torch.uint8).repeat((self.nbytes + 3) // 4)[: self.nbytes]
        self._bytes()[self.start:self.end].copy_(rep)
        return self

    def payload(self, dtype=torch.uint8, shape=None):
        """The payload as a typed view (`nbytes` must be a multiple of the element size)."""
        esz = torch.empty((), dtype=dtype).element_size()
        if self.nbytes % esz:
            raise ValueError(f"payload of {self.nbytes} bytes is not a whole number of {dtype} elements")
        v = self._bytes()[self.start:self.end].view(dtype)
        return v.view(shape) if shape is not None else v

    def check(self):
        """None when both guards still hold the pattern, else a description of the changed bytes: side, first and last
        offset (front: bytes before the payload start, as negative offsets; back: bytes after the payload end) and count."""
        word = torch.tensor([_as_int32(PATTERNS[self.pattern])], dtype=torch.int32, device=self._buf.device)
        want = word.view(torch.uint8)
        b = self._bytes()
        problems = []
        for side, lo, hi, origin in (("front", 0, self.start, self.start), ("back", self.end, self.total, self.end)):
            g = b[lo:hi]
            ref = want.repeat((hi - lo + 3) // 4 + 1)[(lo % 4):(lo % 4) + (hi - lo)]
            bad = torch.nonzero(g != ref).flatten()
            if bad.numel():
                first, last = int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin
                problems.append(f"{side} guard: {bad.numel()} byte(s) changed at offsets {first} .. {last} "
                                f"(pattern {self.pattern})")
        return "; ".join(problems) if problems else None


def describe_difference(a, b, what, axes=None):
    """Text describing where and how two tensors of one shape differ (see assert_same_bits)."""
    if a.shape != b.shape:
        return f"{what}: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}"
    if a.device != b.device:
        b = b.to(a.device)
    ne = a != b  # True where either side is NaN, as torch.equal counts it
    idx = torch.nonzero(ne)
    n = idx.shape[0]
    lines = [f"{what}: {n} of {a.numel()} elements differ"]
    if a.dtype != b.dtype:
        lines.append(f"dtypes {a.dtype} vs {b.dtype}")
    if n:
        da, db = a[ne].double(), b[ne].double()
        both = torch.isfinite(da) & torch.isfinite(db)
        dmax = float((da[both] - db[both]).abs().max()) if bool(both.any()) else float("nan")
        lines.append(f"max |delta| {dmax:.6g} over {int(both.sum())} finite pairs")
        nan_a = int(torch.isnan(a).sum()) if a.is_floating_point() else 0
        nan_b = int(torch.isnan(b).sum()) if b.is_floating_point() else 0
        lines.append(f"NaN count: {nan_a} (first) vs {nan_b} (second)")
        names = list(axes) if axes is not None else [f"dim{i}" for i in range(a.dim())]
        names += [f"dim{i}" for i in range(len(names), a.dim())]
        if a.dim():
            lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
            lines.append("extents: " + ", ".join(f"{names[i]} {lo[i]}..{hi[i]}" for i in range(a.dim())))
        first = []
        for row in idx[:8].tolist():
            t = tuple(row)
            first.append(f"{t}: {a[t].item()!r} vs {b[t].item()!r}")
        lines.append("first differing: " + "; ".join(first))
    return "\n  ".join(lines)


def assert_same_bits(a, b, what="tensors", axes=None):
    """assert torch.equal(a, b), with a failure message that locates the difference (describe_difference)."""
    if torch.equal(a, b):
        return
    raise AssertionError(describe_difference(a, b, what, axes))


__all__ = ["GUARD_BYTES", "PATTERNS", "Guarded", "assert_same_bits", "describe_difference"]
