"""The hand-built -S rescue cases (tests/rescue_cases.py) on the device: each case alone, the mixed batch and its reversal
through every route of RESCUE_ROUTES and through the BAM-record entry.  Rows against the frozen expectations of the
independent restatement (tests/golden/rescue_expect.json) and against the oracle; the numbers of rescue problems and of
accepted rescues against the restatement's counts -- what catches a wrong gating decision that happens not to change a row."""
import functools
import json
import os

import numpy as np
import pytest

from bramble_amd import lib
from bramble_amd.batch import format_cigar, parse_cigar
from oracle import oracle_binding as ob
from tests import bamio, cigar_ref
from tests import rescue_cases as rc
from tests import route_cases
from tests.parity import assert_rows_equal
from tests.test_gpu_bam_bundle import assert_streams_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"lr": 1, "use_fasta": 1}
QUERY_CODES = np.asarray([0, 1, 4, 7, 8], dtype=np.uint32)     # M I S = X
REF_MAP = np.array([0], dtype=np.int32)


@pytest.fixture(scope="module")
def idx():
    i = lib.Index(rc.annotation(), device=0)
    yield i
    i.close()


@functools.lru_cache(maxsize=None)
def frozen():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "rescue_expect.json")))["cases"]


@functools.lru_cache(maxsize=None)
def oracle_index():
    return ob.OracleIndex(rc.annotation())


class Input:
    """a record list with everything the device's answer is held to"""

    def __init__(self, name, records, frozen_rows=None):
        self.name, self.records = name, records
        self.batch = rc.batch_of(records)
        self.orc, _, _ = ob.run(oracle_index(), ob.make_flags(**FLAGS), self.batch, want_matches=False)
        self.rows, self.problems, self.rescued = rc.expected(records)
        if frozen_rows is not None:
            assert self.rows == frozen_rows["rows"] and (self.problems, self.rescued) == (frozen_rows["problems"], frozen_rows["rescued"])
        sides = [a[s] for per in rc.answers_of(records) for _, a in per for s in ("left", "right") if a[s]["exists"]]
        self.leftover = sum(1 for s in sides if s["t_has_n"] or len(s["target"]) > 384)
        self.n_target_n = sum(1 for s in sides if s["t_has_n"])


@functools.lru_cache(maxsize=None)
def inputs():
    out = [Input(c.id, c.records, frozen()[c.id]) for c in rc.cases()]
    return out + [Input("mixed", rc.mixed()), Input("mixed reversed", rc.mixed(True))]


@functools.lru_cache(maxsize=None)
def crowded():
    return Input("crowded", rc.crowded())


def rows_of(prod):
    ids = [t["id"] for t in rc.annotation()["transcripts"]]
    out = []
    for k in range(prod["n_rows"]):
        c0, c1 = int(prod["cigar_off"][k]), int(prod["cigar_off"][k + 1])
        out.append([int(prod["input_index"][k]), ids[int(prod["transcript_id"][k])], int(prod["pos"][k]), chr(prod["strand"][k]),
                    format_cigar(prod["cigar"][c0:c1]), int(prod["clip_score"][k])])
    return sorted(out)


def check_call(ctx, inp, tag):
    """one host-batch call on `ctx` against everything `inp` holds"""
    prod = ctx.project_batch(lib.make_config(**FLAGS), inp.batch)
    where = "%s, %s" % (inp.name, tag)
    assert rows_of(prod) == inp.rows, where
    try:
        assert_rows_equal(prod, inp.orc)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (where, e))
    # every output CIGAR spells its read's length
    n = prod["n_rows"]
    offs = np.asarray(prod["cigar_off"], dtype=np.int64)
    qlen = cigar_ref.ref_len_sums(np.asarray(prod["cigar"], dtype=np.uint32), offs[:-1], np.diff(offs), QUERY_CODES)
    assert np.array_equal(qlen.astype(np.int64), np.asarray(inp.batch["l_qseq"], dtype=np.int64)[np.asarray(prod["input_index"][:n], dtype=np.int64)]), where
    st = ctx.rescue_stats()
    assert (st["problems"], st["rescued"]) == (inp.problems, inp.rescued), (where, st, inp.problems, inp.rescued)
    return prod


@pytest.mark.parametrize("asked,expect", route_cases.RESCUE_ROUTES, ids=[a for a, _ in route_cases.RESCUE_ROUTES])
def test_cases_on_every_route(idx, asked, expect):
    ctx = route_cases.new_context(idx, asked)
    try:
        for inp in inputs():
            check_call(ctx, inp, asked)
            if inp.problems:
                assert route_cases.route_of(ctx, inp.batch["n_aln"]) == expect, (inp.name, asked)
        # the device-batch entry (run_route), on the batches that hold every case: the route it takes and the counts it leaves
        for inp in inputs()[-2:]:
            route, db = route_cases.run_route(ctx, asked, lib.make_config(**FLAGS), inp.batch)
            st = ctx.rescue_stats()
            assert route == expect and (st["problems"], st["rescued"]) == (inp.problems, inp.rescued), (inp.name, asked, route, st)
            del db
    finally:
        ctx.close()


def test_general_kernel_alone_small_tape_and_the_leftovers(idx):
    """ksw_fast = 0 (k_ksw alone) and a tape of 1 MiB (the register arrays in pieces) give the same rows and counts; by default
    the problems with an N in the target and those beyond 384 target columns, and no others, are left to the general kernel"""
    mixed = inputs()[-2]
    with_n = [i for i in inputs() if i.name.split(".")[0] in ("tN10", "tN9", "longN", "long", "past_end")]
    assert len(with_n) == 18 and mixed.n_target_n >= 14 and mixed.leftover > mixed.n_target_n
    ctx = lib.Context(idx)
    try:
        for inp in with_n + [mixed, inputs()[-1]]:
            check_call(ctx, inp, "default")
            d = ctx.ksw_diag()
            assert d["leftover_before"] == inp.leftover and sum(d["per_shape"]) == inp.problems - inp.leftover, (inp.name, d, inp.leftover)
            assert d["leftover_after"] == d["leftover_before"], (inp.name, d)
        check_call(ctx, crowded(), "default")
        assert ctx.ksw_diag()["pieces"] == 1 and crowded().problems > 2048
        ctx.set_param("ksw_tape_mb", 1)
        check_call(ctx, crowded(), "ksw_tape_mb 1")
        assert ctx.ksw_diag()["pieces"] > 1, ctx.ksw_diag()
        for inp in inputs():
            check_call(ctx, inp, "ksw_tape_mb 1")
        ctx.set_param("ksw_fast", 0)
        for inp in inputs():
            check_call(ctx, inp, "ksw_fast 0")
        assert ctx.ksw_diag()["pieces"] == 0
    finally:
        ctx.close()


# ---- the BAM-record entry ------------------------------------------------------------------------------------------------------
NT16 = "=ACMGRSVTWYHKDBN"


def bam_records(records):
    """the records as BAM records (tests/bamio.py): the sequence in 4-bit codes, none for a record without one"""
    out = []
    for r in records:
        seq = (r.get("seq") or "").upper()
        codes = [NT16.index(ch) for ch in seq] + [0] * (len(seq) & 1)
        packed = bytes((codes[k] << 4) | codes[k + 1] for k in range(0, len(codes), 2))
        out.append(bamio.bam_record(r["name"].encode(), 0, r["ref_start"] - 1, parse_cigar(r["cigar"]), len(seq), seq=packed,
                                    qual=bytes([30] * len(seq))))
    return out


def split3(recs):
    sizes = np.asarray([len(r) + 4 for r in recs], dtype=np.uint64)
    return bamio.frame(recs), (np.cumsum(sizes, dtype=np.uint64) - sizes + np.uint64(4)), (sizes - np.uint64(4)).astype(np.uint32)


def projected_rows(stream):
    """[read name, transcript id, pos, CIGAR] of a projected record stream: a projected record's reference is its transcript
    and its position the row's"""
    ids = [t["id"] for t in rc.annotation()["transcripts"]]
    out = []
    for rec in bamio.split_stream(stream):
        f = bamio.record_fields(rec)
        out.append([f["name"].decode(), ids[f["ref_id"]], f["pos"], format_cigar(f["cigar"])])
    return sorted(out)


def record_cigar(text, strand):
    """a record on a '-' transcript carries its CIGAR in the transcript's direction: the row's ops in reversed order"""
    ops = parse_cigar(text)
    return format_cigar(ops[::-1] if strand == "-" else ops)


def test_cases_through_the_bam_record_entry(idx):
    """project_bam_bundle on the same reads as BAM records: reads of odd length, 4-bit codes other than A C G T N in a clip,
    records without a sequence.  The stream against the oracle's, its records against the restatement's rows, the counts."""
    assert any(len(r["seq"]) & 1 for i in inputs() for r in i.records) and any(ch in "RY" for r in rc.mixed() for ch in r["seq"].upper())
    ctx = lib.Context(idx)
    cfg = lib.make_config(**FLAGS)
    try:
        for inp in inputs():
            stream, roff, rlen = split3(bam_records(inp.records))
            orc, _, _, _ = ob.run_bam(oracle_index(), ob.make_flags(**FLAGS), stream, roff, rlen, REF_MAP)
            got, counters = ctx.project_bam_bundle(cfg, stream, roff, rlen, REF_MAP)
            assert counters["n_rows"] == orc["n_rows"] == len(inp.rows), inp.name
            assert_streams_equal(got, orc["bam_stream"])
            want = sorted([inp.records[k]["name"], t, pos, record_cigar(cig, strand)] for k, t, pos, strand, cig, _ in inp.rows)
            assert projected_rows(got) == want, inp.name
            st = ctx.rescue_stats()
            assert (st["problems"], st["rescued"]) == (inp.problems, inp.rescued), (inp.name, st, inp.problems, inp.rescued)
    finally:
        ctx.close()
