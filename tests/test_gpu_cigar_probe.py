"""cigar_inl.h and wave_turns (wave_inl.h), each called directly through libbramble_selftest.so and compared exactly with the
references of tests/cigar_ref.py.  Every test is one launch of one block of 256 threads; every output sits between guard words
(tests/scan_probe.py).  test_cigar_ref_cpu.py shows that these inputs fail wrong tables."""
import numpy as np
import pytest

from tests import cigar_ref as R
from tests.scan_probe import OUT_FILL, Buf, call, lib

pytestmark = pytest.mark.gpu

FILL32 = OUT_FILL & 0xffffffff


@pytest.mark.parametrize("name", list(R.turn_cases()))
def test_wave_turns_calls_the_set_lanes_lowest_first(name):
    """per wave: the list is the set lanes in ascending order with their values fetched by shuffle, all 64 lanes are in every
    call, the count is the mask's population count, and nothing is written behind the list or into another wave's"""
    masks = R.turn_cases()[name]
    assert len(set(masks)) == 4
    flag, val = R.turn_inputs(masks)
    d_flag, d_val = Buf(np.uint32, 256, values=flag), Buf(np.uint32, 256, values=val)
    lists, counts = Buf(np.uint32, 4 * 64 * 3), Buf(np.uint32, 4)
    call(lib().brst_wave_turns, None, d_flag.ptr, d_val.ptr, lists.ptr, counts.ptr)
    want_lists, want_counts = R.turn_ref(masks, val, FILL32)
    got_lists, got_counts = lists.read("lists"), counts.read("counts")
    assert got_counts.tolist() == want_counts.tolist() == [bin(m).count("1") for m in masks]
    for w in range(4):
        assert np.array_equal(got_lists[192 * w:192 * (w + 1)], want_lists[192 * w:192 * (w + 1)]), "wave %d" % w
    d_flag.assert_untouched("flag"); d_val.assert_untouched("val")


def test_wave_cigar_ref_len_and_the_op_tables():
    pool, offs, ns = R.pool_case()
    ops = R.table_ops()
    k = len(offs)
    d_pool, d_offs, d_ns, d_ops = (Buf(np.uint32, pool.size, off=1, values=pool), Buf(np.uint64, k, values=offs), Buf(np.uint32, k, values=ns),
                                   Buf(np.uint32, 16, values=ops))
    sums, same, tab, tab_len, inl = Buf(np.uint64, k), Buf(np.uint32, k), Buf(np.uint32, 16), Buf(np.uint64, 16), Buf(np.uint64, 48)
    call(lib().brst_cigar, None, d_pool.ptr, d_offs.ptr, d_ns.ptr, k, sums.ptr, same.ptr, d_ops.ptr, tab.ptr, tab_len.ptr, inl.ptr)
    want = R.ref_len_sums(pool, offs, ns)
    assert sums.read("sums").tolist() == want.tolist() and int(want.max()) >= 1 << 32
    assert same.read("same").tolist() == [64] * k                                  # every lane holds the sum
    want_tab, want_len, want_inl = R.table_ref(ops)
    got_tab = tab.read("tab")
    assert {t for t in range(16) if got_tab[t] & 1} == {0, 7, 8} and {t for t in range(16) if got_tab[t] & 2} == {2, 3}
    assert got_tab.tolist() == want_tab.tolist()
    assert tab_len.read("tab_len").tolist() == want_len.tolist() and inl.read("inl").tolist() == want_inl.tolist()
    for b, what in ((d_pool, "pool"), (d_offs, "offs"), (d_ns, "ns"), (d_ops, "ops")):
        b.assert_untouched(what)


def test_pool_holds_refuses_what_leaves_the_pool():
    n_pool_words = 5000
    cases = R.pool_holds_cases(n_pool_words)
    offs, ns = np.array([c[0] for c in cases], dtype=np.uint64), np.array([c[1] for c in cases], dtype=np.uint32)
    d_offs, d_ns, out = Buf(np.uint64, len(cases), values=offs), Buf(np.uint32, len(cases), values=ns), Buf(np.uint32, len(cases))
    call(lib().brst_pool_holds, None, n_pool_words, d_offs.ptr, d_ns.ptr, len(cases), out.ptr)
    got = out.read("out").tolist()
    assert got == [int(c[2]) for c in cases], [c for c, g in zip(cases, got) if int(c[2]) != g]
