"""Guard bands and poisoned padding for kernels that take a leading dimension.

A `Guarded` is a strided [batch][rows][cols] view (row stride ld >= cols, batch stride bstride)
carved out of ONE larger buffer that the test allocates itself: at least `GUARD_ROWS` rows of ld
elements lie before the first and after the last row, so a kernel that overruns by a whole
256-row tile still lands in memory the test owns, and everything that is not a declared element
(guard rows, the gap columns cols .. ld-1, the rows between two batches, and for attention the
columns of a row that belong to no head slice) is `outside`.

Outputs: `fill_pattern()` writes a fixed, position-dependent bit pattern over the whole buffer,
`snapshot()` keeps a copy and `check_untouched()` compares everything outside with it as
integers, bit for bit (the pattern holds NaN payloads: never compare it as float).

Inputs: `poison_check(run, inputs)` runs the call twice, with 0 and with NaN in everything outside
the inputs' declared extents; every output must be finite and bit-equal between the two runs. A
kernel that masks a ragged tail on one operand only computes 0 * finite = 0 next to ordinary
data and 0 * NaN = NaN here.
"""
import torch

GUARD_ROWS = 256       # one full tile of the largest kernel under test (256 x 256 GEMM)
MIN_GUARD_ELEMS = 4096  # for 1-D buffers (ld = a few elements): still several tiles of rows

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Guarded:
    def __init__(self, rows, cols, ld=None, dtype=torch.float32, device="cpu", batch=1,
                 bstride=None, col_ranges=None):
        """col_ranges: [(first column, width), ...] of the declared columns of a row when they are
        not 0 .. cols-1 (attention head slices); cols is then the row's extent."""
        ld = cols if ld is None else ld
        assert ld >= cols and rows >= 1 and batch >= 1
        if bstride is None:
            bstride = rows * ld
        assert batch == 1 or bstride >= rows * ld
        self.rows, self.cols, self.ld, self.batch, self.bstride = rows, cols, ld, batch, bstride
        self.dtype = dtype
        esz = torch.empty(0, dtype=dtype).element_size()
        guard = max(GUARD_ROWS * ld, MIN_GUARD_ELEMS)
        guard = (guard + 63) // 64 * 64  # keeps the first row 16-byte aligned for every dtype
        self.offset = guard
        span = (batch - 1) * bstride + (rows - 1) * ld + cols
        self.total = guard + span + (ld - cols) + guard
        self.buf = torch.zeros(self.total, dtype=dtype, device=device)
        self.ibuf = self.buf.view(_INT[esz])
        self.view = self._strided(self.buf)
        inside = torch.zeros(self.total, dtype=torch.bool, device=device)
        iv = self._strided(inside)
        for c0, w in (col_ranges or [(0, cols)]):
            assert 0 <= c0 and c0 + w <= cols
            iv[:, :, c0:c0 + w] = True
        self.inside = inside
        self._snap = None

    def _strided(self, flat):
        return flat.as_strided((self.batch, self.rows, self.cols), (self.bstride, self.ld, 1),
                               self.offset)

    @property
    def t(self):
        """The tensor to hand to a kernel: data_ptr() is element (0, 0, 0) of the view."""
        return self.view

    @property
    def v2(self):
        """[rows][cols] view of a single-batch buffer."""
        assert self.batch == 1
        return self.view[0]

    def fill_pattern(self):
        """A fixed bit pattern that differs from element to element (so that a copy of a
        neighbouring element shows too) over the WHOLE buffer, declared elements included."""
        n = self.total
        i = torch.arange(n, dtype=torch.int64, device=self.buf.device)
        bits = 8 * self.ibuf.element_size()
        p = (i * 2654435761 + 0x5bd1e995) ^ (i >> 3)
        if bits < 64:
            p = p & ((1 << bits) - 1)
            if bits > 8:
                p = p - ((p >> (bits - 1)) << bits)  # to the signed range of the integer view
        self.ibuf.copy_(p.to(self.ibuf.dtype))
        return self

    def set(self, data):
        self.view.copy_(data.reshape(self.view.shape))
        return self

    def fill_outside(self, value):
        """value (0 or NaN) into every element outside the declared extents."""
        self.buf[~self.inside] = value
        return self

    def snapshot(self):
        self._snap = self.ibuf.clone()
        return self

    def check_untouched(self, what, also=None):
        """Everything outside the declared extents (and the declared elements `also`, a bool
        tensor shaped like the view, that the header says the call leaves alone) still holds the
        bits of the snapshot."""
        assert self._snap is not None, "snapshot() first"
        mask = ~self.inside
        if also is not None:
            extra = torch.zeros_like(self.inside)
            self._strided(extra).copy_(also.reshape(self.view.shape))
            mask = mask | (extra & self.inside)
        bad = (self.ibuf != self._snap) & mask
        if bool(bad.any()):
            idx = int(bad.nonzero()[0])
            rel = idx - self.offset
            n = int(bad.sum())
            if rel < 0:
                where = f"{-rel} elements before the first row"
            else:
                b = min(rel // self.bstride, self.batch - 1) if self.batch > 1 else 0
                r, c = divmod(rel - b * self.bstride, self.ld)
                where = f"batch {b} row {r} col {c} (rows {self.rows}, cols {self.cols}, ld {self.ld})"
            raise AssertionError(f"{what}: {n} elements outside the declared extents were "
                                 f"written, the first at {where}")


def poison_check(run, inputs, what=""):
    """run() -> list of output tensors (it copies them: the buffers are reused). Called with 0 and
    with NaN outside every input's declared extents; the outputs must be finite and bit-equal.
    Returns the outputs of the NaN run."""
    outs = []
    for fill in (0.0, float("nan")):
        for g in inputs:
            g.fill_outside(fill)
        outs.append([o.clone(memory_format=torch.contiguous_format) for o in run()])
    for k, (a, b) in enumerate(zip(*outs)):
        if a.is_floating_point():
            assert bool(torch.isfinite(b.float()).all()), \
                f"{what}: output {k} is not finite with NaN in the inputs' padding"
        assert torch.equal(a, b), f"{what}: output {k} depends on what the inputs' padding holds"
    return outs[1]
