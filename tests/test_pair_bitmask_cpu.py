"""k_pair_mask's mask path restated in numpy on the oracle's match lists (no GPU): the span rule, the tid masks relative to the
pair's smallest tid, their AND and the 1 + 1 rule give what the intersection of the two sets gives; and the inputs of
tests/test_gpu_pair_bitmask.py really hold every case that test is about, so that a change of the generator cannot empty one
silently."""
import numpy as np
import pytest

from tests import pair_bitmask_cases as pc

SHIFTS = (0, 1)


@pytest.mark.parametrize("shift", SHIFTS)
def test_survivors_are_the_slots_members(shift):
    """the construction holds: a read's survivors are its slot's members, and the batch has at least four windows"""
    _, matches = pc.oracle(shift)
    lists = pc.survivor_lists(matches)
    recs = pc.records(shift)
    assert len(recs) == len(lists) and len(recs) >= 4 * pc.WINDOW
    by_start = {}
    for locus, (_, slots) in pc.LOCI.items():
        for s in slots:
            by_start[pc._slot_start(locus, s)] = (locus, s)
    for i, r in enumerate(recs):
        where = next((w for st, w in by_start.items() if st <= r["ref_start"] < st + pc.SLOT_LEN), None)
        assert sorted(int(t) for t in lists[i]) == sorted(pc.members(where)), (i, where)


@pytest.mark.parametrize("shift", SHIFTS)
def test_mask_rule_equals_set_intersection(shift):
    orc, matches = pc.oracle(shift)
    lists = pc.survivor_lists(matches)
    rows_of = np.bincount(np.asarray(orc["input_index"], dtype=np.int64), minlength=len(lists))
    n_mask = 0
    for i, m in pc.pairs_of(matches):
        for x, y, a in ((lists[i], lists[m], i), (lists[m], lists[i], m)):
            by_sets = pc.kept_by_sets(x, y)
            if pc.span_of(x, y) <= 63:
                n_mask += 1
                assert pc.kept_by_mask(x, y) == by_sets, (a, x, y)
            # the oracle's rows agree with the rule: an alignment of a PAIR emits its kept survivors
            assert rows_of[a] == len(by_sets[0]), (a, rows_of[a], by_sets)
    assert n_mask > 100


def _census(shift):
    _, matches = pc.oracle(shift)
    lists = pc.survivor_lists(matches)
    pred = pc.predict(matches)
    c = dict.fromkeys(["span63", "span64", "base_leader", "base_mate", "one_one", "one_two", "two_two", "strict_subset",
                       "all_common", "outside", "outside_quad", "mixed_windows", "deferred", "beside_deferred",
                       "list_long", "second_round_subset"], 0)
    lengths = set()
    edges = set()
    for i, m in pc.pairs_of(matches):
        x, y = lists[i], lists[m]
        big = pred["path"][i] == "big"
        if big:
            c["deferred"] += 1
            continue
        span = pc.span_of(x, y)
        common = set(x.tolist()) & set(y.tolist())
        two = len(x) == 2 and len(y) == 2
        c["span63"] += int(span == 63 and two)
        c["span64"] += int(span == 64 and two)
        if span <= 63 and x.min() != y.min():
            c["base_leader" if x.min() < y.min() else "base_mate"] += 1
        if not common:
            c["one_one"] += int(len(x) == 1 and len(y) == 1)
            c["one_two"] += int(sorted((len(x), len(y))) == [1, 2])
            c["two_two"] += int(two)
        elif len(common) < len(x) and len(common) < len(y):
            c["strict_subset"] += 1
            c["second_round_subset"] += int(span <= 63 and min(len(x), len(y)) > 8)
        elif len(common) == len(x) == len(y):
            c["all_common"] += 1
        if common and span <= 63:
            lengths.update((len(x), len(y)))
        c["list_long"] += int(span > 63 and max(len(x), len(y)) > 16)
        for a, b in ((i, m), (m, i)):
            if not pc.in_window(a, b):
                c["outside"] += 1
                c["outside_quad"] += int(abs(a - b) == 2)
        if m == i + 1 and i % pc.WINDOW in (pc.WINDOW - 1, 0):
            edges.add((i % pc.WINDOW, pred["path"][i]))
    # a window that holds owners of both paths
    by_window = {}
    for a, p in pred["path"].items():
        by_window.setdefault(a // pc.WINDOW, set()).add(p)
    c["mixed_windows"] = sum(1 for s in by_window.values() if {"mask", "list"} <= s)
    c["beside_deferred"] = sum(1 for s in by_window.values() if "big" in s and "mask" in s)
    return c, lengths, edges, pred


@pytest.mark.parametrize("shift", SHIFTS)
def test_every_case_is_present(shift):
    c, lengths, edges, pred = _census(shift)
    for k, v in c.items():
        assert v >= 1, (k, c)
    assert set(pc.LIST_LENGTHS) <= lengths, lengths                 # every list length, with a common subset, on the mask path
    assert pred["n_big"] >= 4 and pred["list_path"] >= 2 * pc.N_FAR
    # a pair of neighbours whose leader is a window's last alignment (shift 1: (61, 62), ...) or its first (shift 0: (62, 63), ...)
    assert {e[0] for e in edges} == ({pc.WINDOW - 1} if shift else {0}), edges
    _, matches = pc.oracle(shift)
    mate = np.asarray(matches["mate_idx"])
    assert (mate[61], mate[62]) == (62, 61) if shift else (mate[62], mate[63]) == (63, 62)


def test_window_edges_meet_both_paths():
    """over the two batches, pairs that straddle a window edge take the mask path and the list path"""
    paths = set()
    for shift in SHIFTS:
        paths |= {e[1] for e in _census(shift)[2]}
    assert {"mask", "list"} <= paths, paths
