"""scan_top_rounds<C, ITEMS> with coalesced accesses (wave_inl.h): a wave takes 64 * ITEMS consecutive tile sums as ITEMS rows
of 64 and scans the rows one behind the other, so a wrong carry can hide between two lanes, two rows, two waves or two rounds.
ITEMS 8 is what the product instantiates (k_scan_top, k_scan3_top, k_scan5_top); ITEMS 32 is the widest form the probe has
(k_scan5_top's before it was measured against 8).  Both with one and with three arrays, through the probe of
libbramble_selftest.so, exact against tests/scan_ref.py, at the tile counts around a wave, a row, a block's 256 sums and a
round."""
import functools

import numpy as np
import pytest

from tests import scan_ref as R
from tests.scan_probe import Buf, call, lib

pytestmark = pytest.mark.gpu

PRODUCT_ITEMS = (8, 32)


def sizes_for(items):
    rnd = 256 * items
    return sorted({1, 63, 64, 65, 255, 256, 257, rnd - 1, rnd, rnd + 1, 2 * rnd + 3})


CASES = [(c, items, n) for c in (1, 3) for items in PRODUCT_ITEMS for n in sizes_for(items)]


@functools.lru_cache(maxsize=None)
def _inputs(kind, n_tiles, channels):
    """small: values below 1 000.  carry: 2^28 ... 2^29 each, so that the running sum passes 2^32 after ten or so sums -- inside
    the first row of the first wave -- and many times more in every row, wave and round after it: a carry kept in 32 bits
    anywhere is a wrong result.  (A size too small to reach 2^32 gets one sum of 2^32 - 1 up front.)"""
    r = np.random.default_rng([7, n_tiles, channels, kind == "carry"])
    if kind == "small":
        t = r.integers(0, 1000, n_tiles * channels, dtype=np.uint64)
    else:
        t = r.integers(1 << 28, 1 << 29, n_tiles * channels, dtype=np.uint64)
        t.reshape(channels, -1)[:, 0] = np.uint64((1 << 32) - 1)
    want, tots = R.top_rounds_ref(t, channels)
    t.setflags(write=False), want.setflags(write=False), tots.setflags(write=False)
    return t, want, tots


@pytest.mark.parametrize("kind", ["small", "carry"])
@pytest.mark.parametrize("channels,items,n_tiles", CASES)
def test_scan_top_rounds_coalesced(channels, items, n_tiles, kind):
    t, want, want_tot = _inputs(kind, n_tiles, channels)
    if kind == "carry" and n_tiles > 1:
        assert int(want_tot.min()) > 1 << 32
    what = "scan_top_rounds<%d, %d>, %d tiles, %s values" % (channels, items, n_tiles, kind)
    sums, tot = Buf(np.uint64, t.size, values=t), Buf(np.uint64, channels)
    call(lib().brst_top_rounds, None, channels, items, sums.ptr, n_tiles, tot.ptr)
    got = sums.read(what)   # (and nothing written before or behind the sums)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: sum %d = %d, not %d (%d wrong)" % (what, bad[0], got[bad[0]], want[bad[0]], bad.size)
    assert np.array_equal(tot.read(what + ": totals"), want_tot), what + ": totals"
