"""k_emit_rows<1|2> with "emit_rank_tids" 1 (a kept survivor's record index is the number of bits below its tid in the word
k_pair_mask leaves per alignment) and 0 (the loop over the kept survivors' tids only), each with "pair_bitmask" 1 and 0, on the
direct-rows route: the rows of all four settings equal the oracle's and each other's, and the downloaded words
(br_ctx_direct_tidwords) are the ones the CPU restatement predicts -- {common tids, the pair's smallest tid} for both mates of
every pair on the mask path with a transcript in common, the marker for every other alignment that keeps a survivor -- which
proves that the popcount path ran and where.  Inputs: tests/rank_tid_cases.py (what they hold is asserted by
tests/test_rank_tid_cases_cpu.py) and tests/pair_bitmask_cases.py (long lists, pairs deferred to k_pair_big)."""
import numpy as np
import pytest

from bramble_amd import lib
from tests import pair_bitmask_cases as pc
from tests import rank_tid_cases as rc
from tests.parity import _EXACT, assert_rows_equal
from tests.route_cases import new_context, prefix_on_a_name_boundary, route_of, slice_batch

pytestmark = pytest.mark.gpu

SETTINGS = [(1, 1), (1, 0), (0, 1), (0, 0)]   # (emit_rank_tids, pair_bitmask)
INPUTS = {"rank-even": (rc, 0), "rank-odd": (rc, 1), "bitmask-even": (pc, 0), "bitmask-odd": (pc, 1)}


@pytest.fixture(scope="module")
def indexes():
    idx = {rc: lib.Index(rc.annotation(), device=0), pc: lib.Index(pc.annotation(), device=0)}
    yield idx
    for i in idx.values():
        i.close()


def _project(index, b, rank_tids, bitmask):
    """(rows, words, emit launches) of batch b on the direct-rows route, which the kernel timers confirm"""
    ctx = new_context(index, "direct", emit_rank_tids=rank_tids, pair_bitmask=bitmask)
    try:
        rows = ctx.project_batch(lib.make_config(), b)
        assert route_of(ctx, b["n_aln"]) == "direct"
        ms = ctx.kernel_ms()
        launched = (ms[lib.KERNEL_NAMES[lib.K_EMIT_ROWS_SIMPLE]][1], ms[lib.KERNEL_NAMES[lib.K_EMIT_ROWS]][1])
        return rows, ctx.direct_tidwords(b["n_aln"]), launched, ctx.direct_diag()
    finally:
        ctx.close()


def _assert_same_rows(x, y):
    for k, _ in _EXACT:   # (HI among them)
        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
    assert np.array_equal(x["cigar_off"], y["cigar_off"]) and np.array_equal(x["cigar"], y["cigar"])
    assert np.array_equal(x["is_primary"], y["is_primary"])


@pytest.mark.parametrize("name", list(INPUTS))
def test_both_ranks_give_the_oracles_rows_and_the_predicted_words(indexes, name):
    mod, shift = INPUTS[name]
    b = mod.batch(shift)
    orc, matches = mod.oracle(shift)
    want = rc.expected_words(orc, matches)
    n = b["n_aln"]
    first = None
    for rank_tids, bitmask in SETTINGS:
        rows, (common, base), launched, diag = _project(indexes[mod], b, rank_tids, bitmask)
        assert_rows_equal(rows, orc)
        if first is None:
            first = rows
        else:
            _assert_same_rows(rows, first)
        if rank_tids and bitmask:
            n_word, n_none = rc.check_words(want, common, base, n)
            print(name, "alignments", n, "words", n_word, "markers", n_none, "light entries", diag["light"], "emit launches", launched)
            assert n_word >= 100 and n_none >= 40
            if mod is rc:   # both emit kernels ranked from words (the CPU test: word alignments of every class)
                assert launched[0] >= 1 and launched[1] >= 1 and diag["light"] > 0
        else:   # no mask path, or no words at all: every alignment that keeps a survivor carries the marker
            for a in want:
                assert int(base[a]) == lib.KT_NONE, (rank_tids, bitmask, a, int(base[a]))


def test_the_switch_is_read_at_every_launch(indexes):
    """one context, 1 -> 0 -> 1: the same rows, words only where the switch is on"""
    b = rc.batch(1)
    orc, matches = rc.oracle(1)
    want = rc.expected_words(orc, matches)
    ctx = new_context(indexes[rc], "direct")
    try:
        for rank_tids in (1, 0, 1):
            ctx.set_param("emit_rank_tids", rank_tids)
            assert_rows_equal(ctx.project_batch(lib.make_config(), b), orc)
            common, base = ctx.direct_tidwords(b["n_aln"])
            if rank_tids:
                assert rc.check_words(want, common, base, b["n_aln"])[0] >= 100
            else:
                assert np.all(base == lib.KT_NONE)
        for bad in (2, -1):
            with pytest.raises(lib.BrambleError):
                ctx.set_param("emit_rank_tids", bad)
    finally:
        ctx.close()


def test_a_smaller_batch_after_a_larger_one_reads_no_stale_word(indexes):
    """the second call's batch is a shorter piece of the first one's that starts 36 alignments in (the kinds repeat every 40),
    so its alignments sit at other indices: a word the first call left would rank wrongly or show in the download"""
    big = rc.batch(0)
    lo = prefix_on_a_name_boundary(big, 37)
    hi = prefix_on_a_name_boundary(big, lo + 200)
    assert 0 < lo < hi < big["n_aln"] and lo % (2 * len(rc.KINDS)) != 0
    small = slice_batch(big, lo, hi)
    orc_b, _ = rc.oracle(0)
    orc_s, matches_s = rc.run_oracle(small)
    want_s = rc.expected_words(orc_s, matches_s)
    assert sum(1 for w in want_s.values() if w is None) >= 10 and sum(1 for w in want_s.values() if w) >= 50
    ctx = new_context(indexes[rc], "direct")
    try:
        assert_rows_equal(ctx.project_batch(lib.make_config(), big), orc_b)
        assert_rows_equal(ctx.project_batch(lib.make_config(), small), orc_s)
        common, base = ctx.direct_tidwords(small["n_aln"])
        rc.check_words(want_s, common, base, small["n_aln"])
    finally:
        ctx.close()
