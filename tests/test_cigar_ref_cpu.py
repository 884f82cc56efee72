"""The references and inputs of test_gpu_cigar_probe.py can tell right from wrong: the references agree with naive loops, and
the chosen pool, op words and masks give other results for a wrong op table, a 32-bit sum, a shifted offset or another order of
the turns.  No GPU."""
import numpy as np
import pytest

from tests import cigar_ref as R


def test_the_pool_is_what_the_probe_is_meant_to_meet():
    pool, offs, ns = R.pool_case()
    assert ns.tolist() == [0, 1, 63, 64, 65, 128, 300] and all(int(o) % 2 == 1 for o in offs)
    ends = [int(o) + int(n) for o, n in zip(offs, ns)]
    assert all(e < int(o) for e, o in zip(ends, offs[1:])) and ends[-1] < pool.size      # apart, words between and behind them
    big = pool[int(offs[-1]):ends[-1]]
    assert set((big & 15).tolist()) == set(range(16)) and int(big[150]) == (R.MAX_LEN << 4)
    assert pool.dtype == np.uint32 and offs.dtype == np.uint64 and ns.dtype == np.uint32


def test_reference_sums_are_the_naive_loop():
    pool, offs, ns = R.pool_case()
    want = []
    for o, n in zip(offs.tolist(), ns.tolist()):
        acc = 0
        for w in pool[o:o + n].tolist():
            if w & 15 in (0, 2, 3, 7, 8):
                acc += w >> 4
        want.append(acc)
    got = R.ref_len_sums(pool, offs, ns)
    assert got.dtype == np.uint64 and got.tolist() == want and want[0] == 0
    assert sum(w >= 1 << 32 for w in want) >= 3 and max(want) < 1 << 63


@pytest.mark.parametrize("codes,what", [((0, 1, 2, 3, 7, 8), "I counted"), ((0, 2, 3, 4, 7, 8), "S counted"), ((0, 2, 7, 8), "N left out"),
                                        ((0, 2, 3, 8), "= left out"), ((0, 2, 3, 7), "X left out"), ((0, 7, 8), "the covering ops only"),
                                        ((0, 2, 3, 5, 6, 7, 8), "H and P counted"), (tuple(range(16)), "every code counted"),
                                        ((0, 2, 3, 7, 8, 9), "a code past X counted")])
def test_the_pool_fails_a_wrong_table(codes, what):
    pool, offs, ns = R.pool_case()
    right, wrong = R.ref_len_sums(pool, offs, ns), R.ref_len_sums(pool, offs, ns, codes)
    assert wrong[-1] != right[-1], what                       # the 300 ops hold every code with a positive length
    assert int((wrong != right).sum()) >= 3, what
    ops = R.table_ops()
    assert not np.array_equal(R.table_ref(ops, codes)[1], R.table_ref(ops)[1]), what
    assert not np.array_equal(R.table_ref(ops, codes)[2], R.table_ref(ops)[2]), what


def test_the_pool_fails_a_narrow_sum_and_a_shifted_walk():
    pool, offs, ns = R.pool_case()
    right = R.ref_len_sums(pool, offs, ns)
    assert int(((right & np.uint64(0xffffffff)) != right).sum()) >= 3                  # a 32-bit accumulator
    for d_off, d_n in ((1, 0), (-1, 0), (0, -1), (0, 1)):                              # an op more or less at either end
        moved = R.ref_len_sums(pool, (offs.astype(np.int64) + d_off).astype(np.uint64), (ns.astype(np.int64) + d_n).clip(0).astype(np.uint32))
        assert int((moved != right).sum()) >= 5, (d_off, d_n)                   # the CIGARs of 63 ops and more
    for lanes in (63, 65):                                                             # a stride that is not the wave
        part = R.ref_len_sums(pool, offs, np.minimum(ns, lanes).astype(np.uint32))
        assert part[-1] != right[-1] and part[-2] != right[-2]


def test_table_reference_is_the_naive_loop():
    ops = R.table_ops()
    tab, tab_len, inl = R.table_ref(ops)
    assert [int(w) & 15 for w in ops] == list(range(16)) and all(int(w) >> 12 for w in ops)
    for t, w in enumerate(ops.tolist()):
        nxt = int(ops[(t + 1) % 16])
        a = (w >> 4) if t in (0, 2, 3, 7, 8) else 0
        b = (nxt >> 4) if (t + 1) % 16 in (0, 2, 3, 7, 8) else 0
        assert int(tab[t]) == (1 if t in (0, 7, 8) else 0) + (2 if t in (2, 3) else 0)
        assert int(tab_len[t]) == a and inl[3 * t:3 * t + 3].tolist() == [0, a, a + b]
    assert len({int(x) for x in tab_len if x}) == 5                                    # no two lengths alike: a swapped entry shows


def test_pool_holds_cases_are_the_plain_comparison():
    P = 5000
    cases = R.pool_holds_cases(P)
    for off, n, want in cases:
        assert 0 <= off < 1 << 64 and 0 <= n < 1 << 32 and want == (off + n <= P)        # in unbounded integers
    wrapped = [((off + n) % (1 << 64) <= P) for off, n, _ in cases]                     # the sum in 64 bits
    assert wrapped != [c[2] for c in cases]
    assert {(P + 1, 300, False), (2 ** 64 - 100, 300, False), (P - 299, 300, False), (P - 300, 300, True)} <= set(cases)
    assert [off <= P for off, n, _ in cases] != [c[2] for c in cases] and [n <= P for off, n, _ in cases] != [c[2] for c in cases]


def test_turn_cases_fail_other_orders():
    cases = R.turn_cases()
    seen = set()
    for name, masks in cases.items():
        assert len(set(masks)) == 4, name
        seen |= set(masks)
        flag, val = R.turn_inputs(masks)
        assert [int(f != 0) for f in flag] == [(m >> l) & 1 for m in masks for l in range(64)]
        assert len(set(val.tolist())) == 256                                           # a value names its lane and wave
        lists, counts = R.turn_ref(masks, val, 0xa5a5a5a5)
        assert counts.tolist() == [bin(m).count("1") for m in masks]
        rows = lists.reshape(4, 64, 3)
        for w, m in enumerate(masks):
            k = int(counts[w])
            assert rows[w, :k, 0].tolist() == [l for l in range(64) if (m >> l) & 1] and (rows[w, k:] == 0xa5a5a5a5).all()
            if k > 1:                                                                  # highest first, or another wave's values
                assert rows[w, :k, 0].tolist() != rows[w, :k, 0][::-1].tolist()
                assert rows[w, :k, 1].tolist() != [int(val[64 * ((w + 1) % 4) + l]) for l in rows[w, :k, 0]]
    assert {R.NONE, R.ALL, R.LANE0, R.LANE63, R.EVEN, R.ODD} <= seen
    assert all(m not in (R.NONE, R.ALL, R.LANE0, R.LANE63, R.EVEN, R.ODD) for m in cases["random"])
