"""--quant, --quant-eff-length and --coverage on the rows of every projection route.  The three features read the device row table
a projection call leaves behind (br_quant_add_last, br_coverage_add_last: br_row_a, the CIGAR reference column, the sparse CIGAR
arena with n_pool_words, row_off / group_off), and four routes write that table: the small-batch path, the predicted launch of a
large batch, direct rows (k_emit_rows<1>, <2>, k_big, the side arena's retry) and the match table (with the -S rescue's DP in the
middle).  The features' own tests feed them from the small-batch path only; a production run feeds them from the other three.

Here every input of tests/route_cases.py -- plain pairs under three presets, the dense paired locus, the full CIGAR alphabet, long
reads, -S -- goes down every route it can take (the route is asserted from the kernel timers), and the call's table goes through
rc.check_consumers: classes, fragment histogram, effective lengths and coverage exactly as the yardsticks on the oracle's rows say,
the EM under the rule of test_gpu_quant._assert_em, and theta / tpm equal in bits among the routes of one input (the class table is
the EM's only input).  Then production-shaped sequences of calls on one context with one set of accumulators, and add_last after
the two diagnostics that touch a direct-rows call's tables."""
import numpy as np
import pytest

from bramble_amd import device, lib, synth
from oracle import oracle_binding as ob
from tests import route_cases as rc

pytestmark = pytest.mark.gpu

_EM = {}    # input -> (route, theta / tpm) of the first route that ran


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64).view(np.uint64), np.asarray(y, dtype=np.float64).view(np.uint64))


def _assert_direct_diag(ctx, inp, asked):
    d = ctx.direct_diag()
    if inp.id.startswith("plain-"):
        # both emit classes held rows: exact two-exon matches on the light one, and rows of more than two ops, which only the
        # general one writes
        nops = np.diff(inp.tables()[0]["cigar_off"].astype(np.int64))
        assert d["light"] > 0 and int((nops > 2).sum()) > 100, d
    if "dense" in inp.id:
        assert d["n_big"] > 50, d                       # k_big, k_pair_big and the side arena
    if asked == "direct_side64":
        assert d["side_attempts"] >= 2 and d["side_cap"] > 64, d     # the arena was regrown and the attempt repeated


CASES = [(inp, asked, expect) for inp in rc.INPUTS for asked, expect in inp.routes]


@pytest.mark.parametrize("inp,asked,expect", CASES, ids=["%s-%s" % (i.id, a) for i, a, _ in CASES])
def test_consumers_on_every_route(inp, asked, expect):
    annd, batch = inp.data()
    _, lens = inp.oracle()
    want = inp.want()
    idx = lib.Index(annd, device=0)
    ctx = rc.new_context(idx, asked)
    try:
        route, db = rc.run_route(ctx, asked, lib.make_config(**inp.flags), batch)
        assert route == expect, (inp.id, asked, route)
        if route == "direct":
            _assert_direct_diag(ctx, inp, asked)
        res = rc.check_consumers(ctx, want, lens, len(lens), em=True, tag="%s on %s" % (inp.id, asked))
        del db
    finally:
        ctx.close()
        idx.close()
    first_route, first = _EM.setdefault(inp.id, (asked, res))
    for key in ("theta", "tpm"):
        assert _same_bits(first[key], res[key]), (inp.id, key, first_route, asked)


# ---- production-shaped sequences of calls ---------------------------------------------------------------------------------------
class _Run:
    """one context, one Quant and two Coverages (primary_only 0 and 1) with add_last after every call"""

    def __init__(self, annd, flags, **params):
        self.oi = ob.OracleIndex(annd)
        self.lens = rc.oracle_lens(self.oi)
        self.flags = flags
        self.idx = lib.Index(annd, device=0)
        self.ctx = lib.Context(self.idx)
        for k, v in params.items():
            self.ctx.set_param(k, v)
        self.ctx.set_profiling(True)
        self.q = rc.new_quant(len(self.lens), self.lens, em=True)
        self.cov = [rc.new_coverage(self.lens, p) for p in (0, 1)]
        self.tables, self.keep = [], []

    def call(self, batch, small_n, expect):
        db = device.upload_batch(batch)
        self.keep.append(db)
        self.ctx.project_batch_device(lib.make_config(**self.flags), db)
        if batch["n_aln"]:
            route = rc.route_of(self.ctx, batch["n_aln"], small_n)
            assert route == expect, (len(self.tables), route, expect)
        for acc in [self.q] + self.cov:
            acc.add_last(self.ctx)
        if batch["n_aln"]:   # (an empty batch has no read names and no rows: it adds nothing to the yardsticks either)
            orc, _, _ = ob.run(self.oi, ob.make_flags(**self.flags), batch, want_matches=False)
            self.tables.append(rc.yardstick_rows(orc, rc.group_starts(batch)))
        return db

    def finish(self, tag):
        """the accumulators against the yardsticks over the concatenation of all batches' oracle rows"""
        want = rc.yardsticks(*rc.concat_tables(self.tables), self.lens, em=True)
        assert want["classes"]["n_names"] == sum(len(t[2]) - 1 for t in self.tables)
        rc.assert_quant(self.q, want, len(self.lens), em=True, tag=tag)
        for p in (0, 1):
            rc.assert_coverage(self.cov[p], want, self.lens, p, tag)
        return want

    def close(self):
        for acc in [self.q] + self.cov:
            acc.close()
        self.ctx.close()
        self.idx.close()


def test_a_run_of_short_read_calls():
    """small, predicted, direct rows twice (the second call starts from the first one's tables), an empty batch -- it resets the
    context's last table, so the adds after it add nothing --, and small again"""
    ann = synth.Annotation("S")
    small_n = 2000
    b = [ann.reads(n, "pe", seed=s) for n, s in ((800, 101), (2500, 102), (2000, 103), (1500, 104), (700, 105))]
    assert b[0]["n_aln"] <= small_n < b[1]["n_aln"] and b[4]["n_aln"] <= small_n < min(b[2]["n_aln"], b[3]["n_aln"])
    run = _Run(ann.as_dict(), {}, small_n=small_n)
    try:
        run.call(b[0], small_n, "small")
        run.call(b[1], small_n, "predicted")
        run.ctx.set_param("small_batch", 0)
        run.call(b[2], small_n, "direct")
        run.call(b[3], small_n, "direct")
        run.call(rc.slice_batch(b[3], 0, 0), small_n, None)
        run.ctx.set_param("small_batch", 1)
        run.call(b[4], small_n, "small")
        want = run.finish("short reads")
        assert want["fld"]["n_obs"] > 500 and want["classes"]["n_names"] == 7500
    finally:
        run.close()


def test_a_run_of_long_read_calls():
    """a similarity-filter preset: the ordinary match table (nothing to predict from), a predicted launch, and a predicted launch
    of a batch with far fewer matches per alignment than predicted (nine in ten alignments unmapped).  The first batch is twice
    the others: a predicted launch needs the tables the ordinary call left (its counts and a quarter) to hold 1.15 times the
    scaled counts and 4 096 entries more, which at these sizes only a smaller batch leaves room for."""
    ann = synth.Annotation("G", n_genes=300, n_refs=2)
    small_n = 1000
    h = [ann.reads(n, "hifi", seed=s) for n, s in ((4000, 79), (2000, 80), (2000, 81))]
    few = dict(h[2])
    few["ref_id"] = np.where(np.arange(few["n_aln"]) % 10 == 0, few["ref_id"], -1).astype(np.int32)
    assert min(x["n_aln"] for x in h) > small_n
    run = _Run(ann.as_dict(), {"lr_hq": 1}, small_n=small_n)
    try:
        run.call(h[0], small_n, "match_table")
        run.call(h[1], small_n, "predicted")
        run.call(few, small_n, "predicted")
        want = run.finish("long reads")
        assert len(run.tables[2][0]["tid"]) * 5 < len(run.tables[1][0]["tid"]) and want["fld"]["n_obs"] == 0
    finally:
        run.close()


def test_add_last_after_the_diagnostics_of_a_direct_rows_call():
    """br_device_rows_detail runs the emit kernels once more over a direct-rows call's tables; br_ctx_collect_counters projects the
    batch once more through the match table and replaces what the context calls its last table.  add_last after either reads
    what the yardsticks say."""
    inp = rc.BY_ID["plain-default"]
    annd, batch = inp.data()
    _, lens = inp.oracle()
    want = inp.want()
    idx = lib.Index(annd, device=0)
    ctx = rc.new_context(idx, "direct")
    try:
        route, db = rc.run_route(ctx, "direct", lib.make_config(**inp.flags), batch)
        assert route == "direct"
        assert ctx.rows_detail()
        rc.check_consumers(ctx, want, lens, len(lens), tag="after br_device_rows_detail")
        counters = ctx.collect_counters(db)
        assert counters["matches"] >= len(inp.tables()[0]["tid"])
        rc.check_consumers(ctx, want, lens, len(lens), tag="after br_ctx_collect_counters")
    finally:
        ctx.close()
        idx.close()
