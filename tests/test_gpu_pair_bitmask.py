"""k_pair_mask with "pair_bitmask" 1 (mates' survivor sets intersected as 64-bit tid masks where they span at most 64 tids) and 0
(tid lists always) on the inputs of tests/pair_bitmask_cases.py, on the direct-rows route: the rows of both settings equal the
oracle's and each other's, the pairing flags are the same, and the number of alignments that the list path resolved is the
one predicted from the oracle's match lists by the span rule and the window rule.  What the inputs hold -- spans of exactly 63
and 64, the smallest tid on either side, 1 + 1 / 1 + 2 / 2 + 2 without a common transcript, common transcripts a strict subset
of both lists, lists of 1, 8, 9, 16, 17 and 64, pairs across window edges at even and odd offsets, partners outside the window,
windows with both paths, pairs deferred to k_pair_big beside ordinary ones -- is asserted by tests/test_pair_bitmask_cpu.py."""
import numpy as np
import pytest

from bramble_amd import lib
from tests import pair_bitmask_cases as pc
from tests.parity import _EXACT, assert_rows_equal
from tests.route_cases import new_context, route_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def index():
    idx = lib.Index(pc.annotation(), device=0)
    yield idx
    idx.close()


def _project(index, shift, bitmask):
    """(rows, direct_diag) of batch(shift) on the direct-rows route, which the kernel timers confirm"""
    b = pc.batch(shift)
    ctx = new_context(index, "direct", pair_bitmask=bitmask)
    try:
        rows = ctx.project_batch(lib.make_config(), b)
        assert route_of(ctx, b["n_aln"]) == "direct"
        return rows, ctx.direct_diag(b["n_aln"])
    finally:
        ctx.close()


@pytest.mark.parametrize("shift", [0, 1], ids=["even", "odd"])
def test_masks_and_lists_give_the_oracles_rows(index, shift):
    orc, matches = pc.oracle(shift)
    pred = pc.predict(matches)
    (rows1, d1), (rows0, d0) = _project(index, shift, 1), _project(index, shift, 0)
    print("pair_bitmask 1:", {k: v for k, v in d1.items() if k != "pflags"}, "0:", {k: v for k, v in d0.items() if k != "pflags"},
          "predicted list path:", pred["list_path"], "big:", pred["n_big"])
    assert_rows_equal(rows1, orc)
    assert_rows_equal(rows0, orc)
    for k, _ in _EXACT:
        assert np.array_equal(np.asarray(rows1[k]), np.asarray(rows0[k])), k
    assert np.array_equal(rows1["cigar"], rows0["cigar"]) and np.array_equal(rows1["is_primary"], rows0["is_primary"])
    assert np.array_equal(d1["pflags"], d0["pflags"])
    # more than 64 candidate rows exactly where the inputs were built to have them: the prediction's deferred pairs are the device's
    assert d1["n_big"] == pred["n_big"] and d0["n_big"] == pred["n_big"]
    assert d1["pm_list"] == pred["list_path"], (d1["pm_list"], pred["list_path"])
    assert d0["pm_list"] == 0   # (counted with pair_bitmask 1 only)
    # the flags of every PAIR, from the sets: paired iff something is kept, PF_SAME iff a transcript is common
    lists = pc.survivor_lists(matches)
    pf = d1["pflags"]
    for i, m in pc.pairs_of(matches):
        for a, b in ((i, m), (m, i)):
            kept, same = pc.kept_by_sets(lists[a], lists[b])
            want = (lib.PF_PAIRED if kept else 0) | (lib.PF_SAME if kept and same else 0) | (lib.PF_MATE if kept and a > b else 0)
            assert int(pf[a]) & (lib.PF_PAIRED | lib.PF_SAME | lib.PF_MATE) == want, (a, b, int(pf[a]), want, pred["path"][a])


def test_second_call_on_one_context_switches_paths(index):
    """the switch is read at every launch: one context, 1 -> 0 -> 1, the same rows and the count of each setting"""
    orc, matches = pc.oracle(0)
    pred = pc.predict(matches)
    ctx = new_context(index, "direct")
    try:
        for bitmask, want in ((1, pred["list_path"]), (0, 0), (1, pred["list_path"])):
            ctx.set_param("pair_bitmask", bitmask)
            assert_rows_equal(ctx.project_batch(lib.make_config(), pc.batch(0)), orc)
            assert ctx.direct_diag()["pm_list"] == want
        with pytest.raises(lib.BrambleError):
            ctx.set_param("pair_bitmask", 2)
    finally:
        ctx.close()
