"""The guard-band helper (tests/guard_util.py) against deliberately wrong torch "kernels": each of
the three mistakes it exists for must be rejected, and a correct kernel accepted. CPU only."""
import pytest
import torch

from guard_util import GUARD_ROWS, Guarded, poison_check


def _rowscale_kernel(x, y, rows, cols, overrun=None):
    """y[r][c] = 2 x[r][c] through flat pointers and leading dimensions, as a HIP kernel sees
    them. overrun: 'row' stores one element past the last row, 'gap' one into a gap column."""
    xb, yb = x.buf, y.buf
    for b in range(x.batch):
        for r in range(rows):
            xo = x.offset + b * x.bstride + r * x.ld
            yo = y.offset + b * y.bstride + r * y.ld
            yb[yo:yo + cols] = 2 * xb[xo:xo + cols]
    last = y.offset + (y.batch - 1) * y.bstride + (rows - 1) * y.ld
    if overrun == "row":
        yb[last + y.ld] = 1.0
    elif overrun == "gap":
        yb[last + cols] = 1.0
    elif overrun == "tile":  # a whole 256-row tile past the end: still inside the test's buffer
        yb[last + y.ld:last + y.ld + (GUARD_ROWS - 1) * y.ld] = 1.0
    elif overrun == "batch":  # a row between two batches
        yb[y.offset + rows * y.ld] = 1.0


def _io(dtype=torch.float32, batch=1):
    rows, cols = 5, 12
    x = Guarded(rows, cols, ld=16, dtype=dtype, batch=batch, bstride=(rows + 3) * 16)
    y = Guarded(rows, cols, ld=20, dtype=dtype, batch=batch, bstride=(rows + 2) * 20)
    x.set(torch.randn(batch, rows, cols, generator=torch.Generator().manual_seed(1)).to(dtype))
    return rows, cols, x, y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_correct_kernel_is_accepted(dtype):
    rows, cols, x, y = _io(dtype, batch=3)
    y.fill_pattern().snapshot()
    _rowscale_kernel(x, y, rows, cols)
    y.check_untouched("y")
    assert torch.equal(y.view, 2 * x.view)
    # the pattern is compared as integers: it holds NaN payloads, which never equal themselves
    assert bool(torch.isnan(y.buf.float()).any())


@pytest.mark.parametrize("overrun", ["row", "gap", "tile", "batch"])
def test_stores_outside_the_extents_are_rejected(overrun):
    rows, cols, x, y = _io(batch=3)
    y.fill_pattern().snapshot()
    _rowscale_kernel(x, y, rows, cols, overrun=overrun)
    with pytest.raises(AssertionError, match="outside the declared extents"):
        y.check_untouched("y")


def test_rows_the_header_leaves_alone():
    rows, cols, x, y = _io()
    y.fill_pattern().snapshot()
    _rowscale_kernel(x, y, rows, cols)
    also = torch.zeros(1, rows, cols, dtype=torch.bool)
    also[:, 3:] = True  # "rows >= 3 are not written": this kernel writes them
    with pytest.raises(AssertionError, match="outside the declared extents"):
        y.check_untouched("y", also=also)


def _rowsum_kernel(x, rows, cols, mask_both):
    """Row sums over whole 16-wide chunks of the row, the tail masked: on the data (right) or by
    a 0 / 1 factor only (wrong: 0 * NaN)."""
    out = torch.empty(rows)
    keep = (torch.arange(x.ld) < cols).to(x.dtype)
    for r in range(rows):
        row = x.buf[x.offset + r * x.ld:x.offset + (r + 1) * x.ld]
        if mask_both:
            row = torch.where(keep.bool(), row, torch.zeros_like(row))
        out[r] = (row * keep).sum()
    return out


def test_padding_that_leaks_as_zero_times_x_is_rejected():
    rows, cols, x, _ = _io()
    poison_check(lambda: [_rowsum_kernel(x, rows, cols, True)], [x], "rowsum")
    with pytest.raises(AssertionError, match="not finite"):
        poison_check(lambda: [_rowsum_kernel(x, rows, cols, False)], [x], "rowsum")


def test_column_ranges_and_alignment():
    g = Guarded(7, 448, ld=448, dtype=torch.bfloat16, col_ranges=[(8, 128), (152, 128), (304, 128)])
    assert g.t.data_ptr() % 16 == 0 and g.offset >= GUARD_ROWS * 448
    assert int(g.inside.sum()) == 7 * 384
    g.fill_pattern().snapshot()
    g.view[0, 2, 140] = 1.0  # a column between two head slices
    with pytest.raises(AssertionError, match="row 2 col 140"):
        g.check_untouched("qkv")
