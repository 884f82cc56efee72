"""The full CIGAR alphabet through every emit path: reads of tests/adversarial.py (= X H P ops, several indels per exon,
an I beside an N, CIGARs of more than 8 and more than 64 ops, starts and junctions on the exon edge and 1-2 bases off it,
light-class spellings beside their general twins) against the oracle, bit for bit.

The batches are the fixed ones of tests/alphabet_cases.py; tests/test_cigar_alphabet_cpu.py shows on the CPU that they
give rows for enough reads and reach every merge_ops cell the generator can reach.  Every batch is projected on each
route that holds a merge_cigars call site -- the small-batch path, direct rows (k_emit_rows, and k_big at the dense
locus), the match table (k_emit_dense; the only route of the similarity-filter presets), and with -S the rescue's emit
pass -- with 8 and with 64 lanes per group; a share of them goes in as BAM records and comes out as BAM records (the
encoder recomputes reference length and bin from the rewritten CIGAR), and one batch goes through br_project_group /
br_project_groups name by name."""
import numpy as np
import pytest

from bramble_amd import lib
from oracle import oracle_binding as ob
from tests import adversarial as adv
from tests import alphabet_cases as ac
from tests.parity import assert_rows_equal
from tests.test_gpu_bam_bundle import assert_streams_equal, run_both_bam
from tests.test_gpu_group import _group_alignments

pytestmark = pytest.mark.gpu

# (route, context parameters): direct_rows is the default of the ordinary pipeline for the short-read presets; the presets
# with a similarity filter and -S take the match table whatever it says
ROUTES = [("small", {"small_batch": 1}), ("direct", {"small_batch": 0, "direct_rows": 1}),
          ("match_table", {"small_batch": 0, "direct_rows": 0})]
_ORC = {}


def _oracle(case):
    if case.id not in _ORC:
        b = case.batch()
        orc, _, _ = ob.run(ob.OracleIndex(case.annotation()), ob.make_flags(**case.flags), b, want_matches=False)
        ac.conditions(case, orc, b)
        _ORC[case.id] = (b, orc)
    return _ORC[case.id]


@pytest.mark.parametrize("case", ac.CASES, ids=[c.id for c in ac.CASES])
def test_full_alphabet_rows_equal_oracle(case):
    batch, orc = _oracle(case)
    idx = lib.Index(case.annotation(), device=0)
    cfg = lib.make_config(**case.flags)
    for route, params in ROUTES:
        for lanes in (8, 64):
            ctx = lib.Context(idx)
            ctx.set_param("group_lanes", lanes)
            for k, v in params.items():
                ctx.set_param(k, v)
            try:
                assert_rows_equal(ctx.project_batch(cfg, batch), orc)
            except AssertionError as e:
                raise AssertionError("%s, route %s, %d lanes: %s" % (case.id, route, lanes, e))
            if route == "direct" and case.family == "short":
                d = ctx.direct_diag()
                if case.kind == "dense":
                    assert d["n_big"] > 50, d          # alignments with more than 64 candidate rows: k_big
                if case.mode == "near":
                    assert d["light"] > 20, d          # the M N M spellings took the light two-exon class
            ctx.close()
    idx.close()


@pytest.mark.parametrize("case", ac.BAM_CASES, ids=[c.id for c in ac.BAM_CASES])
def test_full_alphabet_bam_records_equal_oracle(case):
    ann = case.annotation()
    stream = adv.bam_stream(case.records())
    ref_map = np.arange(len(ann["refnames"]), dtype=np.int32)
    got, counters, orc, _ = run_both_bam(ann, stream, ref_map, **case.flags)
    # the records carry what the flat batch carries: the oracle fed with either gives the same rows
    batch, flat = _oracle(case)
    assert orc["n_rows"] == flat["n_rows"] and np.array_equal(orc["cigar"], flat["cigar"])
    assert counters["n_rows"] == orc["n_rows"]
    for k in ("total_complete", "total_unique", "dropped_reads", "total_processed"):
        assert counters[k] == orc[k], k
    assert_streams_equal(got, orc["bam_stream"])


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.id in ("adv-mm-default-23", "adv-near-default-24")],
                         ids=["multimappers", "near_misses"])
def test_full_alphabet_name_groups_equal_oracle(case):
    """br_project_group name by name, then br_project_groups over the same names in one call: the oracle's rows of each
    name group, CIGAR words included."""
    batch, orc = _oracle(case)
    idx = lib.Index(case.annotation(), device=0)
    ctx = lib.Context(idx)
    cfg = lib.make_config(**case.flags)
    _, goff = lib.prepare_batch(batch)
    sizes = np.diff(goff.astype(np.int64))
    order = np.argsort(-sizes, kind="stable")[:60].tolist() + list(range(0, len(sizes), max(1, len(sizes) // 140)))
    order = sorted(set(order))
    ogroup = np.asarray(orc["group"])
    many, expect, rows_seen, ops = [], [], 0, set()
    for g in order:
        lo, hi = int(goff[g]), int(goff[g + 1])
        alns = _group_alignments(batch, lo, hi)
        res = ctx.project_group(cfg, alns)
        sel = np.nonzero(ogroup == g)[0]
        assert len(res) == len(sel), (g, len(res), len(sel))
        for p, r in zip(res, sel):
            c0, c1 = int(orc["cigar_off"][r]), int(orc["cigar_off"][r + 1])
            assert np.array_equal(p["cigar"], orc["cigar"][c0:c1]), (g, ob.format_cigar(p["cigar"]), ob.format_cigar(orc["cigar"][c0:c1]))
            assert p["transcript_id"] == orc["tid"][r] and p["transcript_start"] == orc["pos"][r]
            assert (p["nh"], p["hi"], p["mapq"]) == (orc["nh"][r], orc["hi"][r], orc["mapq"][r])
            assert p["is_primary"] == orc["primary"][r] and p["is_paired_out"] == orc["is_paired"][r]
            assert p["input_index"] == orc["input_index"][r] - lo
            assert p["aligned_len"] == max(int(orc["ref_consumed"][r]), 0)
            ops |= set(int(w) & 0xF for w in p["cigar"])
            expect.append((len(many) + p["input_index"], p))
        many.extend(alns)
        rows_seen += len(res)
    assert rows_seen > 300 and ops >= set(range(9)), (rows_seen, ops)
    res = ctx.project_groups(cfg, many)
    assert len(res) == len(expect)
    for p, (ii, q) in zip(res, expect):
        assert p["input_index"] == ii and p["transcript_id"] == q["transcript_id"] and np.array_equal(p["cigar"], q["cigar"])
        assert (p["nh"], p["hi"], p["is_primary"]) == (q["nh"], q["hi"], q["is_primary"])
    ctx.close()
    idx.close()
