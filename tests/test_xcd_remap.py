"""The XCD-major workgroup remap every LDS-DMA kernel applies to its block id (csrc/gfx950_prims.h xcd_major),
checked on the host through hiseg_xcd_major / hiseg_xcd_major_fill (no GPU): if it were not a bijection for some
grid size, a tile would silently be computed twice and another never."""
import numpy as np

LARGE = (65535, 1048583)
HUGE = 2 ** 31 - 1
EDGE = 4096   # blocks sampled at each end of the HUGE grid


def restated(b, n):
    """The formula, restated: XCD x = b % 8 owns a run of n // 8 ids, one more for the first n % 8 XCDs."""
    q, r = n >> 3, n & 7          # (shifts: numpy's integer division is several times slower)
    x, loc = b & 7, b >> 3
    return np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + loc


def fill(n, out, first=0):
    """out[:] = xcd_major(first .. first + len(out) - 1, n), from the library."""
    from hiseg import _lib as L
    L.check(L.lib().hiseg_xcd_major_fill(n, first, len(out), out.ctypes.data), "xcd_major_fill")


def check(got, b, n, g=None):
    """got = the remapped ids of blocks b of a grid of n blocks (or, n an array of grid sizes, of grid n[g] per
    block): the restated formula; every id inside the run of its class x = b % 8, where the runs are contiguous,
    ascend with x and have the classes' own sizes (which differ by at most one).  With distinct ids, each class
    then maps ONTO its run."""
    assert np.array_equal(got, restated(b, n if g is None else n[g]))
    cls = np.arange(8).reshape((8,) + (1,) * np.ndim(n))
    sizes = (n - cls + 7) // 8                   # blocks of the grid with b % 8 == x, per x
    assert (sizes.max(0) - sizes.min(0) <= 1).all() and (sizes.sum(0) == n).all()
    starts = np.cumsum(sizes, 0) - sizes         # run x begins where run x - 1 ends
    at = (b & 7,) if g is None else (b & 7, g)
    lo = starts[at]
    assert ((got >= lo) & (got < lo + sizes[at])).all()


def test_bijection_and_runs_for_every_grid_up_to_4096():
    ns = np.arange(1, 4097, dtype=np.int32)
    base = (np.cumsum(ns) - ns).astype(np.int32)   # grid n's blocks sit at [base, base + n) of the flat arrays
    total = int(ns.sum())
    got = np.empty(total, np.int32)
    for n, o in zip(ns.tolist(), base.tolist()):
        fill(n, got[o:o + n])
    g = np.repeat(np.arange(len(ns), dtype=np.int32), ns)            # the grid each flat element belongs to
    b = np.arange(total, dtype=np.int32) - base[g]
    assert ((got >= 0) & (got < ns[g])).all()
    assert (np.bincount(got + base[g], minlength=total) == 1).all()  # a bijection on [0, n) for every n
    check(got, b, ns, g)


def test_large_grids():
    for n in LARGE:
        got = np.empty(n, np.int32)
        fill(n, got)
        assert got.min() == 0 and got.max() == n - 1 and (np.bincount(got, minlength=n) == 1).all(), n
        check(got.astype(np.int64), np.arange(n, dtype=np.int64), n)


def test_largest_grid_sampled_at_both_ends():
    n = HUGE
    for first in (0, n - EDGE):
        got = np.empty(EDGE, np.int32)
        fill(n, got, first)
        assert got.min() >= 0 and got.max() < n and len(np.unique(got)) == EDGE
        check(got.astype(np.int64), np.arange(first, first + EDGE, dtype=np.int64), n)


def test_scalar_entry_point_agrees():
    from hiseg import _lib as L
    lib = L.lib()
    for n in (1, 7, 8, 9, 61, 4096, 65535, HUGE):
        for b in sorted(b for b in {0, 1, 7, 8, n // 2, n - 9, n - 8, n - 1} if 0 <= b < n):
            assert lib.hiseg_xcd_major(b, n) == int(restated(np.int64(b), n)), (b, n)
    assert lib.hiseg_xcd_major_fill(8, 4, 5, np.empty(8, np.int32).ctypes.data) == -1   # past the grid: refused
