"""tests/route_cases.py without a GPU: yardstick_rows and its helpers against cases worked out by hand and against oracle_tables,
and -- from the oracle's rows alone -- what tests/test_gpu_consumers_routes.py and tests/test_gpu_cli_routes.py rely on in their
inputs: CIGARs of more than 2, 8 and 64 ops and all nine op codes, rescued clips, paired fragments, more than 64 rows of one
alignment at the dense locus, a command-line input of more than 65 536 alignments, and an EM whose restatement spreads over the
class orders (the rule the device's EM is held to needs a spread above 0)."""
import numpy as np
import pytest

from tests import route_cases as rc
from tests.test_quant_fld_cpu import ROW_FIRST, ROW_MINUS, ROW_PAIRED, ROW_PRIMARY, ROW_SAME_TX


def _orc(rows):
    """rows: (input_index, group, tid, pos, strand, paired, same, first, primary, CIGAR words) -> the oracle's columns"""
    cig = [list(r[9]) for r in rows]
    col = lambda k, dt: np.asarray([r[k] for r in rows], dtype=dt)   # noqa: E731
    return {"n_rows": len(rows), "input_index": col(0, np.int32), "group": col(1, np.uint32), "tid": col(2, np.uint32), "pos": col(3, np.uint32),
            "strand": np.asarray([ord(r[4]) for r in rows], dtype=np.int8), "is_paired": col(5, np.uint8), "same_transcript": col(6, np.uint8),
            "is_first": col(7, np.uint8), "primary": col(8, np.uint8),
            "cigar_off": np.concatenate([[0], np.cumsum([len(c) for c in cig])]).astype(np.uint64),
            "cigar": np.asarray([w for c in cig for w in c], dtype=np.uint32)}


def test_yardstick_rows_by_hand():
    # five alignments in three read names (2, 1, 2); name 0: a pair on transcript 4 and a row of its second alignment on 9;
    # name 1: nothing; name 2: one row of its second alignment
    orc = _orc([(0, 0, 4, 10, "+", 1, 1, 1, 1, [0x30]), (1, 0, 4, 50, "-", 1, 1, 0, 0, [0x20, 0x13, 0x20]), (1, 0, 9, 7, "+", 0, 0, 1, 0, []),
                (4, 2, 5, 0, "-", 0, 0, 1, 1, [0x10, 0x11, 0x10, 0x12])])
    rows, row_off, group_off = rc.yardstick_rows(orc, [0, 2, 3, 5])
    assert rows["meta"].tolist() == [1 | ROW_PAIRED | ROW_SAME_TX | ROW_FIRST | ROW_PRIMARY, 3 | ROW_MINUS | ROW_PAIRED | ROW_SAME_TX,
                                     0 | ROW_FIRST, 4 | ROW_MINUS | ROW_FIRST | ROW_PRIMARY]
    assert rows["tid"].tolist() == [4, 4, 9, 5] and rows["pos"].tolist() == [10, 50, 7, 0] and rows["cigar_off"].tolist() == [0, 1, 4, 4, 8]
    assert row_off.tolist() == [0, 3, 3, 3, 4, 4] and group_off.tolist() == [0, 2, 3, 5]
    assert row_off.dtype == np.uint64 and group_off.dtype == np.uint32
    # without the batch's groups: one alignment a name, up to the last name with rows
    _, row_off1, group_off1 = rc.yardstick_rows(orc)
    assert row_off1.tolist() == [0, 3, 3, 4] and group_off1.tolist() == [0, 1, 2, 3]
    # a row of an alignment outside its read name is refused
    with pytest.raises(AssertionError):
        rc.yardstick_rows(orc, [0, 1, 3, 5])
    # no rows at all
    rows0, row_off0, group_off0 = rc.yardstick_rows(_orc([]), [0, 2])
    assert len(rows0["tid"]) == 0 and row_off0.tolist() == [0, 0, 0] and group_off0.tolist() == [0, 2]
    # two calls one after the other
    rows2, row_off2, group_off2 = rc.concat_tables([(rows, row_off, group_off), (rows0, row_off0, group_off0), (rows, row_off, group_off)])
    assert rows2["cigar_off"].tolist() == [0, 1, 4, 4, 8, 9, 12, 12, 16] and rows2["tid"].tolist() == [4, 4, 9, 5] * 2
    assert row_off2.tolist() == [0, 3, 3, 3, 4, 4, 4, 4, 7, 7, 7, 8, 8] and group_off2.tolist() == [0, 2, 3, 5, 7, 9, 10, 12]


def test_batch_helpers_by_hand():
    from bramble_amd import lib
    from bramble_amd.batch import make_batch
    recs = [{"name": n, "ref_id": 0, "ref_start": 10 * (i + 1), "cigar": c} for i, (n, c) in
            enumerate([("a", "5M"), ("a", "2S3M"), ("ab", "4M1D2M"), ("a", "7M"), ("b", "1M"), ("b", "2M")])]
    b = make_batch(recs)
    g = rc.group_starts(b)
    assert g.tolist() == [0, 2, 3, 4, 6] and np.array_equal(g, lib.prepare_batch(b)[1])
    assert rc.group_starts(make_batch([])).tolist() == [0]
    assert [rc.prefix_on_a_name_boundary(b, n) for n in (0, 1, 2, 3, 5, 6, 99)] == [0, 0, 2, 3, 4, 6, 6]
    s = rc.slice_batch(b, 2, 4)
    assert s["n_aln"] == 2 and s["ref_start"].tolist() == [30, 40] and s["cigar_off"].tolist() == [0, 3, 4]
    assert s["cigar"].tolist() == [0x40, 0x12, 0x20, 0x70] and bytes(s["names"]) == b"aba" and s["name_off"].tolist() == [0, 2, 3]
    assert s["seq_off"] is None and rc.slice_batch(b, 0, 0)["cigar_off"].tolist() == [0]


def test_yardstick_rows_are_oracle_tables():
    """on the input of the three features' own tests: the tables oracle_tables frames from the records' names"""
    from tests.test_quant_fld_cpu import wide_rows
    for mode in ("pe", "ont"):
        tb, rows = wide_rows(mode)   # (built on yardstick_rows, which it holds to tb's row_off and group_off)
        assert len(rows["meta"]) == len(tb["tids"]) > 1000


def _nops(rows):
    return np.diff(rows["cigar_off"].astype(np.int64))


def test_plain_pairs_hold_fragments_and_both_emit_classes():
    for name in ("plain-default", "plain-strict", "plain-fr"):
        inp = rc.BY_ID[name]
        rows, row_off, group_off = inp.tables()
        want = inp.want()
        nops = _nops(rows)
        print("%s: %d alignments, %d rows, %d fragments observed, %d rows of one op, %d of more than two"
              % (name, inp.data()[1]["n_aln"], len(nops), want["fld"]["n_obs"], int((nops == 1).sum()), int((nops > 2).sum())))
        assert inp.data()[1]["n_aln"] >= 6000 and len(group_off) - 1 == 3000 and len(nops) > 3000
        assert want["fld"]["n_obs"] > 100                                  # paired fragments (fr keeps half of the pairs)
        assert int((nops == 1).sum()) > 500 and int((nops > 2).sum()) > 100   # inline CIGARs and pooled ones


def test_dense_locus_holds_more_than_64_rows_of_one_alignment():
    inp = rc.BY_ID["dense"]
    orc, _ = inp.oracle()
    per_aln = np.bincount(orc["input_index"], minlength=inp.data()[1]["n_aln"])
    print("dense: %d alignments, %d rows, at most %d rows of one alignment, %d alignments with more than 64"
          % (len(per_aln), orc["n_rows"], int(per_aln.max()), int((per_aln > 64).sum())))
    assert int((per_aln > 64).sum()) > 50            # (every row is a candidate row that survived: k_big's alignments)
    assert inp.want()["fld"]["n_obs"] + inp.want()["fld"]["n_no_fragment"] > 0


def test_alphabet_inputs_hold_long_cigars_and_every_op():
    assert len(rc.ALPHABET) == 24 and sum(1 for i in rc.ALPHABET if "dense" in i.id) == 3 and sum(1 for i in rc.ALPHABET if "near" in i.id) == 5
    ops, longest = set(), {}
    for inp in rc.ALPHABET:
        rows, _, _ = inp.tables()
        nops = _nops(rows)
        ops_here = set((rows["cigar"] & 15).tolist())
        longest[inp.id] = int(nops.max())
        ops |= ops_here
        assert ops_here >= set(range(9)), inp.id                    # all nine op codes, in every input
        assert int((nops > 2).sum()) > 100, inp.id                 # pooled CIGARs
        assert int((nops > 8).sum()) > 20 or "near" in inp.id or "dense" in inp.id, inp.id
    print("the longest rewritten CIGAR per input:", longest)
    assert ops == set(range(9))
    assert sum(1 for v in longest.values() if v > 8) >= 20
    assert max(longest.values()) > 64 and longest["alphabet-adv-long-lr-26"] > 64


def test_long_reads_and_rescue():
    for name in ("long-ont-lr", "long-hifi-lr_hq"):
        inp = rc.BY_ID[name]
        rows, _, _ = inp.tables()
        assert 400 <= inp.data()[1]["n_aln"] <= 800 and len(rows["tid"]) > 400 and int(_nops(rows).max()) > 8, name
        assert inp.want()["fld"]["n_obs"] == 0
    inp = rc.BY_ID["rescue-ont-lr-S"]
    orc, _ = inp.oracle()
    rescued = int((orc["clip_score"] != 0).sum())
    print("rescue: %d rows, %d of them with a rescued clip" % (orc["n_rows"], rescued))
    assert rescued > 100


@pytest.mark.parametrize("inp", rc.INPUTS, ids=[i.id for i in rc.INPUTS])
def test_em_rule_applies(inp):
    """the restatement's EM spreads over the class orders: the bound the device's EM is held to is neither 0 nor loose"""
    ref, s = inp.want()["em"]
    cl = inp.want()["classes"]
    print("%s: %d names in %d classes, %d without rows; spread %.3e" % (inp.id, cl["n_names"], len(cl["labels"]), cl["n_unassigned"], s))
    assert 0 < s < 1e-9
    assert cl["n_names"] == len(inp.tables()[2]) - 1 and len(cl["labels"]) > 10


def test_cli_input_leaves_the_small_route():
    _, b = rc.cli_pairs()
    assert b["n_aln"] > rc.SMALL_N and len(rc.group_starts(b)) - 1 == 40000
