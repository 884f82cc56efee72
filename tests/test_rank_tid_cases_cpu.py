"""The inputs of tests/test_gpu_emit_rank.py really hold every case that test is about (no GPU): survivors are the slots' members,
candidate order (slab rows, ordered by exon start) is the reverse of tid order for lists of 2, 9 and 17, kept sets are strict
subsets with dropped transcripts on every side, kept tids sit on bit 0 and bit 63 of the word, survivors lie on both strands,
the mates of a pair fall into different emit classes, and the fallbacks are there -- so that a change of the generator cannot
empty a case silently."""
import numpy as np
import pytest

from tests import pair_bitmask_cases as pc
from tests import rank_tid_cases as rc

SHIFTS = (0, 1)


def _where(rec):
    for locus, (_, _, slots) in rc.LOCI.items():
        for s in slots:
            s0 = rc._slot_start(locus, s)
            if s0 <= rec["ref_start"] < s0 + 1000:
                return (locus, s)
    return None


def _shape(rec):
    c = rec["cigar"]
    return "I" if "I" in c else "3" if c.count("N") == 2 else "L" if c.count("N") == 1 else "M"


def _candidate_order(where):
    """the slot's members as the index lists them for a read whose first exon lies in E1: '+' rows, then '-' rows, each by
    exon start -- and E1 of transcript i starts N - 1 - i behind the slot's start"""
    n, strands, slots = rc.LOCI[where[0]]
    key = lambda i: (strands[i % len(strands)] == "-", n - 1 - i)
    return [rc.tid_of(where[0], i) for i in sorted(slots[where[1]], key=key)]


@pytest.mark.parametrize("shift", SHIFTS)
def test_survivors_are_the_slots_members(shift):
    orc, matches = rc.oracle(shift)
    lists = pc.survivor_lists(matches)
    recs = rc.records(shift)
    assert len(recs) == len(lists) and len(recs) >= 6 * pc.WINDOW   # more than one block of k_pair_mask (4 windows)
    assert orc["n_rows"] > 8 * 256                                  # ... and of the emit kernels
    assert pc.predict(matches)["n_big"] == 0
    for i, r in enumerate(recs):
        assert sorted(int(t) for t in lists[i]) == sorted(rc.members(_where(r))), (i, _where(r))


def _census(shift):
    orc, matches = rc.oracle(shift)
    lists = pc.survivor_lists(matches)
    recs = rc.records(shift)
    want = rc.expected_words(orc, matches)
    pred = pc.predict(matches)
    mate = np.asarray(matches["mate_idx"], dtype=np.int64)
    off = np.asarray(matches["aln_off"], dtype=np.int64)
    strand = np.asarray(matches["strand"])
    rows_a, rows_t = np.asarray(orc["input_index"], dtype=np.int64), np.asarray(orc["tid"], dtype=np.int64)
    c = dict.fromkeys(["order2", "order9", "order17", "subset_all_sides", "subset_both_mates", "bit0", "bit63", "base_not_kept",
                       "both_strands", "simple_general_I", "simple_general_3", "light", "light_general", "word_general",
                       "solo_reversed", "span64_list", "straddle_word", "outside_list"], 0)
    for a, w in want.items():
        kept = rows_t[rows_a == a]
        assert np.array_equal(kept, np.sort(kept))   # the oracle's records of an alignment are in tid order: the rank IS the record
        cand = [t for t in _candidate_order(_where(recs[a])) if t in set(kept.tolist())]
        # candidate order is the exact reverse of tid order: the rank of every kept survivor but an odd list's middle one
        # differs from its place among the candidates
        reversed_ = len(kept) > 1 and cand == sorted(cand, reverse=True)
        sh = _shape(recs[a])
        if w is None:
            if mate[a] < 0 or len(lists[int(mate[a])]) == 0:
                c["solo_reversed"] += int(reversed_)
            elif pred["path"].get(a) == "list":
                m = int(mate[a])
                c["span64_list"] += int(pc.span_of(lists[a], lists[m]) == 64 and len(kept) > 0)
                c["outside_list"] += int(not pc.in_window(a, m))
            continue
        base, bits = w
        m = int(mate[a])
        if reversed_ and _where(recs[a])[0] == "R":
            for n in (2, 9, 17):
                c["order%d" % n] += int(len(kept) == n)
        full = [int(t) for t in lists[a]]
        lo, hi = int(kept.min()), int(kept.max())
        sides = any(t < lo for t in full) and any(t > hi for t in full) and any(lo < t < hi and t not in kept for t in full)
        c["subset_all_sides"] += int(sides)
        if sides:
            fm = [int(t) for t in lists[m]]
            c["subset_both_mates"] += int(any(t < lo for t in fm) and any(t > hi for t in fm) and any(lo < t < hi and t not in kept for t in fm))
        c["bit0"] += int(0 in bits)
        c["bit63"] += int(63 in bits)
        c["base_not_kept"] += int(0 not in bits)
        st = strand[off[a]:off[a + 1]][np.isin(lists[a], kept)]
        c["both_strands"] += int(len(set(st.tolist())) == 2)
        shm = _shape(recs[m])
        c["simple_general_I"] += int(sh == "M" and shm == "I")
        c["simple_general_3"] += int(sh == "M" and shm == "3")
        c["light"] += int(sh == "L")
        c["light_general"] += int(sh == "L" and shm == "3")
        c["word_general"] += int(sh in "I3")
        c["straddle_word"] += int(abs(a - m) == 1 and min(a, m) % pc.WINDOW == pc.WINDOW - 1)
    return c


def test_every_case_is_present():
    total = {}
    for shift in SHIFTS:
        c = _census(shift)
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
        # everything but the straddling pair (odd offsets only) is in each batch
        for k, v in c.items():
            assert v >= 1 or k == "straddle_word", (shift, k, c)
    assert total["straddle_word"] >= 1, total


@pytest.mark.parametrize("shift", SHIFTS)
def test_words_follow_from_the_lists(shift):
    """the restatement of the word agrees with pair_bitmask_cases' restatement of the mask path"""
    orc, matches = rc.oracle(shift)
    lists = pc.survivor_lists(matches)
    mate = np.asarray(matches["mate_idx"], dtype=np.int64)
    want = rc.expected_words(orc, matches)
    n_word = 0
    for a, w in want.items():
        if w is None:
            continue
        kept, same = pc.kept_by_mask(lists[a], lists[int(mate[a])])
        assert same and sorted(kept) == [w[0] + b for b in w[1]], (a, kept, w)
        assert max(w[1]) <= 63
        n_word += 1
    assert n_word > 200
    assert sum(1 for w in want.values() if w is None) > 40
