"""Helpers of the tests that hold --quant, --quant-eff-length and --coverage to their yardsticks on the rows of EVERY projection
route.  Those features read the device row table a projection call leaves behind (br_quant_add_last, br_coverage_add_last); four
routes write that table (pipeline.cpp, run_device_paths): the small-batch path, the predicted launch of a large batch, direct rows
and the match table.  Here are

  * ROUTES / run_route / route_of: context parameters that force a route at small shapes, and the route a call took, read from
    the kernel timers;
  * yardstick_rows / group_starts / concat_tables / yardsticks: the oracle's rows in the form the yardsticks of
    test_quant_cpu.py, test_quant_fld_cpu.py and test_coverage_cpu.py take, and those yardsticks over them;
  * check_consumers: a Quant and two Coverages fed from a context's last call, against the yardsticks;
  * INPUTS: the inputs of tests/test_gpu_consumers_routes.py, with the oracle's rows and the yardsticks cached per input so that
    the routes share them.  tests/test_route_cases_cpu.py checks on the CPU, from the oracle's rows alone, that the inputs hold
    what the GPU tests rely on.

Nothing here is derived from a device run: every expectation comes from the oracle's rows through classes_of, fragments_of,
eff_lengths, coverage_of and em_reference."""
import functools

import numpy as np

from tests.test_quant_fld_cpu import ROW_FIRST, ROW_MINUS, ROW_PAIRED, ROW_PRIMARY, ROW_SAME_TX

SMALL_N = 65536     # br_ctx's default "small_n": batches up to this many alignments take the small-batch path
FLD_MAX = 1000      # br_quant's default "fld_max"
EM_ITERS = 100

# route -> context parameters.  "predicted" is a sequence, not a parameter set: run_route lowers "small_n", makes a priming call
# of at most that many alignments and then projects the batch
ROUTES = {"small": {}, "direct": {"small_batch": 0}, "match_table": {"small_batch": 0, "direct_rows": 0}, "predicted": {},
          # direct rows from a side arena of 64 entries: the consumers read the table a regrown arena and a retried attempt left
          "direct_side64": {"small_batch": 0, "side_cap": 64}}


# ---- batches -------------------------------------------------------------------------------------------------------------------
_PER_ALN = ("ref_id", "ref_start", "flags", "xs", "ts", "mate_ref_id", "mate_start", "l_qseq")


def slice_batch(b, lo, hi):
    """the alignments [lo, hi) of a flat batch as a batch of their own (lo and hi on read-name boundaries)"""
    out = {"n_aln": hi - lo}
    for k in _PER_ALN:
        out[k] = np.asarray(b[k])[lo:hi].copy()
    for off, data in (("cigar_off", "cigar"), ("name_off", "names"), ("seq_off", "seqs")):
        if b.get(off) is None:
            out[off] = out[data] = None
            continue
        o = np.asarray(b[off], dtype=np.uint64)
        out[off] = (o[lo:hi + 1] - o[lo]).astype(np.uint64)
        out[data] = np.asarray(b[data])[int(o[lo]):int(o[hi])].copy()
    return out


def group_starts(batch):
    """uint32 [n_groups + 1]: where the runs of equal read names of a flat batch begin, and n_aln (the input contract of
    br_batch_prepare, restated: yardstick_rows checks it against the oracle's group column)"""
    n = int(batch["n_aln"])
    off = np.asarray(batch["name_off"], dtype=np.int64)
    names = np.asarray(batch["names"], dtype=np.uint8).tobytes()
    starts, prev = [], None
    for i in range(n):
        cur = names[off[i]:off[i + 1]]
        if cur != prev:
            starts.append(i)
            prev = cur
    return np.asarray(starts + [n], dtype=np.uint32)


def prefix_on_a_name_boundary(batch, n_max):
    """the largest number of leading alignments <= n_max that ends with a whole read name"""
    g = group_starts(batch)
    return int(g[g <= n_max][-1])


# ---- the oracle's rows in the yardsticks' form ----------------------------------------------------------------------------------
def yardstick_rows(orc, group_off=None):
    """orc: the oracle's rows (ob.run or ob.run_bam).  -> (rows, row_off, group_off): rows in the form
    tests.test_quant_fld_cpu.rows_of defines (tid, pos, meta = NCIGAR | the strand / is_paired / same_transcript / is_first /
    primary bits, cigar_off, cigar), and the tables tests.test_quant_cpu.oracle_tables derives from the oracle's group column: a
    row_off (uint64 [n_aln + 1]) that gives every read name's rows to its first alignment -- only row_off[group_off[g]] is ever
    read -- and group_off (uint32 [n_groups + 1]).
    group_off: the read names' first alignments (group_starts of the batch).  Without it every read name up to the last one with
    rows stands as one alignment: the same classes, fragments and coverage, but read names without rows behind the last row are
    not counted."""
    n_rows = int(orc["n_rows"])
    grp = np.asarray(orc["group"], dtype=np.int64)
    if group_off is None:
        group_off = np.arange((int(grp[-1]) + 1 if n_rows else 0) + 1, dtype=np.uint32)
    else:
        group_off = np.asarray(group_off, dtype=np.uint32)
        n_groups = len(group_off) - 1
        aln_group = np.repeat(np.arange(n_groups), np.diff(group_off.astype(np.int64)))
        assert np.array_equal(aln_group[np.asarray(orc["input_index"], dtype=np.int64)], grp)   # a row belongs to its alignment's read name
    n_groups, n_aln = len(group_off) - 1, int(group_off[-1])
    assert np.all(np.diff(grp) >= 0) and (n_rows == 0 or grp[-1] < n_groups)
    per_aln = np.zeros(n_aln, dtype=np.int64)
    per_aln[group_off[:-1]] = np.bincount(grp, minlength=n_groups)
    row_off = np.zeros(n_aln + 1, dtype=np.uint64)
    row_off[1:] = np.cumsum(per_aln)
    ncig = np.diff(np.asarray(orc["cigar_off"], dtype=np.int64)).astype(np.uint32)
    assert n_rows == 0 or int(ncig.max()) < (1 << 24)
    meta = (ncig | np.where(orc["strand"] == ord("-"), ROW_MINUS, 0) | np.where(orc["is_paired"] != 0, ROW_PAIRED, 0)
            | np.where(orc["same_transcript"] != 0, ROW_SAME_TX, 0) | np.where(orc["is_first"] != 0, ROW_FIRST, 0)
            | np.where(orc["primary"] != 0, ROW_PRIMARY, 0)).astype(np.uint32)
    rows = {"tid": np.asarray(orc["tid"], dtype=np.uint32), "pos": np.asarray(orc["pos"], dtype=np.uint32), "meta": meta,
            "cigar_off": np.asarray(orc["cigar_off"], dtype=np.uint64), "cigar": np.asarray(orc["cigar"], dtype=np.uint32)}
    return rows, row_off, group_off


def concat_tables(tables):
    """[(rows, row_off, group_off)] of several calls -> the tables of one call that holds their read names one after the other"""
    rows = {k: np.concatenate([t[0][k] for t in tables]) for k in ("tid", "pos", "meta", "cigar")}
    cig, ro, go = [np.zeros(1, dtype=np.uint64)], [np.zeros(1, dtype=np.uint64)], [np.zeros(1, dtype=np.uint32)]
    n_words = n_rows = n_aln = 0
    for r, row_off, group_off in tables:
        cig.append(r["cigar_off"][1:] + np.uint64(n_words))
        ro.append(np.asarray(row_off, dtype=np.uint64)[1:] + np.uint64(n_rows))
        go.append(np.asarray(group_off, dtype=np.uint32)[1:] + np.uint32(n_aln))
        n_words, n_rows, n_aln = n_words + int(r["cigar_off"][-1]), n_rows + int(row_off[-1]), n_aln + int(group_off[-1])
    rows["cigar_off"] = np.concatenate(cig)
    return rows, np.concatenate(ro), np.concatenate(go)


def _depth_of(cov, lens):
    """the transcripts whose depth arrays are compared: the deepest, the busiest, the first, the last and the longest"""
    if not len(lens):
        return []
    return sorted({int(np.argmax(cov["max_depth"])), int(np.argmax(cov["records"])), 0, len(lens) - 1, int(np.argmax(lens))})


def yardsticks(rows, row_off, group_off, lens, em=False):
    """every expectation check_consumers holds a call to: the classes, the fragment histogram with its counters, the effective
    lengths, the coverage without and with primary_only; em: also the restatement's EM over 1 / effective length after EM_ITERS
    iterations and its own spread over three class orders (the rule of tests.test_gpu_quant._assert_em)"""
    from tests.test_coverage_cpu import coverage_of
    from tests.test_quant_cpu import classes_of
    from tests.test_quant_fld_cpu import eff_lengths, fragments_of
    lens = np.asarray(lens, dtype=np.int64)
    want = {"classes": classes_of(rows["tid"], row_off, group_off), "fld": fragments_of(rows, row_off, group_off, FLD_MAX)}
    want["eff"] = eff_lengths(want["fld"]["hist"], lens, FLD_MAX)
    want["cov"] = (coverage_of(rows, lens, False), coverage_of(rows, lens, True))
    want["depth_of"] = tuple(_depth_of(c, lens) for c in want["cov"])
    if em:
        from tests.test_gpu_quant import _spread
        want["em"] = _spread(want["classes"], len(lens), want["eff"], True, EM_ITERS)
    return want


# ---- routes --------------------------------------------------------------------------------------------------------------------
def route_of(ctx, n_aln=None, small_n=SMALL_N):
    """The route of the last call on `ctx` (profiling on), from the kernel timers: direct rows launch k_pair_mask, the ordinary
    match-table path k_group_ids, the small-batch path and the predicted launch neither (k_segment labels the groups there);
    those two differ in the batch's size: a batch of at most small_n alignments is a small one."""
    from bramble_amd import lib
    launches = ctx.kernel_ms()
    if launches[lib.KERNEL_NAMES[lib.K_PAIR_MASK]][1]:
        return "direct"
    if launches[lib.KERNEL_NAMES[lib.K_GROUP_IDS]][1]:
        return "match_table"
    assert n_aln is not None
    return "small" if n_aln <= small_n else "predicted"


def new_context(idx, route, **more):
    from bramble_amd import lib
    ctx = lib.Context(idx)
    for k, v in dict(ROUTES[route], **more).items():
        ctx.set_param(k, v)
    ctx.set_profiling(True)
    return ctx


def run_route(ctx, route, cfg, batch, dev_batch=None):
    """Projects `batch` on a context new_context made for `route` and returns (the route the call took, the uploaded batch -- it
    holds the group table the context's last call points at, so it has to live until the consumers have read it).  "predicted":
    the first read names of the batch, at most half of its alignments, go first as a small call; "small_n" is that call's size,
    so the batch itself is a large one that is launched from the counts the small call left."""
    from bramble_amd import device
    small_n = SMALL_N
    if route == "predicted":
        small_n = prefix_on_a_name_boundary(batch, int(batch["n_aln"]) // 2)
        assert 0 < small_n < int(batch["n_aln"])
        ctx.set_param("small_n", small_n)
        prime = device.upload_batch(slice_batch(batch, 0, small_n))
        ctx.project_batch_device(cfg, prime)
        assert route_of(ctx, small_n, small_n) == "small"
    db = dev_batch if dev_batch is not None else device.upload_batch(batch)
    ctx.project_batch_device(cfg, db)
    return route_of(ctx, int(batch["n_aln"]), small_n), db


# ---- the consumers of a context's last call ---------------------------------------------------------------------------------------
def assert_quant(q, want, n_tx, em=False, tag=""):
    """a Quant ("eff_len" = 1) that holds every add, not finished yet, against the yardsticks; -> the EM's result with em"""
    from tests.test_gpu_quant import _assert_classes, _assert_em_to
    from tests.test_gpu_quant_fld import _assert_fld, _same_bits
    _assert_fld(q.fld(), want["fld"], tag)
    q.finish()
    _assert_classes(q, want["classes"], n_tx)
    _assert_fld(q.fld(), want["fld"], tag)
    assert _same_bits(q.eff_lengths(), want["eff"]), tag
    if not em:
        return None
    assert q.em()[0] == EM_ITERS
    res = q.result()
    _assert_em_to(res, want["em"][0], want["em"][1], EM_ITERS, tag)
    return res


def assert_coverage(c, want, lens, primary_only, tag=""):
    """a Coverage that holds every add, not finished yet, against the yardstick"""
    from tests.test_gpu_coverage import _assert_coverage
    c.finish()
    _assert_coverage(c, want["cov"][primary_only], lens, want["depth_of"][primary_only], "%s primary_only=%d" % (tag, primary_only))


def new_quant(n_tx, lens, em=False):
    from bramble_amd import lib
    q = lib.Quant(n_tx, lens)
    q.set_param("eff_len", 1)
    if em:
        q.set_param("max_iters", EM_ITERS)
        q.set_param("tolerance", 0)
    return q


def new_coverage(lens, primary_only):
    from bramble_amd import lib
    c = lib.Coverage(lens)
    c.set_param("primary_only", primary_only)
    return c


def check_consumers(ctx, want, lens, n_tx, em=False, tag=""):
    """The row table the last call on `ctx` left, through its device consumers, against `want` (yardsticks): quant with
    "eff_len" = 1 (labels, counts, first, unique, ambig, n_unassigned; the fragment histogram and its three counters exactly, the
    effective lengths in bits), coverage with "primary_only" 0 and 1 (runs, summary columns and counters exactly, the depth
    arrays of the deepest, busiest, first, last and longest transcripts).  em: EM_ITERS iterations at tolerance 0 as well, under
    the rule of tests.test_gpu_quant._assert_em; -> its theta / tpm (else None)."""
    lens = np.asarray(lens, dtype=np.int64)
    q = new_quant(n_tx, lens, em)
    try:
        q.add_last(ctx)
        res = assert_quant(q, want, n_tx, em, tag)
    finally:
        q.close()
    for primary_only in (0, 1):
        c = new_coverage(lens, primary_only)
        try:
            c.add_last(ctx)
            assert_coverage(c, want, lens, primary_only, tag)
        finally:
            c.close()
    return res


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
def oracle_lens(oi):
    return np.asarray([oi.transcript_len(t) for t in range(oi.num_transcripts())], dtype=np.int64)


class Input:
    """One batch under one preset.  routes: (route asked for, route the call takes) -- a preset that cannot take a route is held
    to the route it falls to: the similarity-filter presets and -S never take direct rows, -S takes neither the small-batch
    path nor a predicted launch, and the dense locus outgrows the small-batch path's tables."""

    def __init__(self, name, make, flags, routes):
        self.id, self._make, self.flags, self.routes = name, make, dict(flags), routes

    @functools.lru_cache(maxsize=None)
    def data(self):
        """(annotation dict, flat batch)"""
        return self._make()

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        """(the oracle's rows, transcript lengths)"""
        from oracle import oracle_binding as ob
        annd, batch = self.data()
        oi = ob.OracleIndex(annd)
        orc, _, _ = ob.run(oi, ob.make_flags(**self.flags), batch, want_matches=False)
        return orc, oracle_lens(oi)

    @functools.lru_cache(maxsize=None)
    def tables(self):
        orc, _ = self.oracle()
        return yardstick_rows(orc, group_starts(self.data()[1]))

    @functools.lru_cache(maxsize=None)
    def want(self):
        return yardsticks(*self.tables(), self.oracle()[1], em=True)


SHORT_ROUTES = (("small", "small"), ("predicted", "predicted"), ("direct", "direct"), ("match_table", "match_table"))
# the similarity-filter presets: direct rows are not for them
LONG_ROUTES = (("small", "small"), ("predicted", "predicted"), ("direct", "match_table"), ("match_table", "match_table"))
# -S: the match table with the DP in the middle, whatever the context is told
RESCUE_ROUTES = (("small", "match_table"), ("direct", "match_table"), ("match_table", "match_table"))
# the dense locus: 300 candidate rows an alignment are beyond the small-batch path's bounds (32 matches an alignment), with or
# without a priming call; the call is redone on direct rows
DENSE_ROUTES = (("small", "direct"), ("direct", "direct"), ("direct_side64", "direct"), ("match_table", "match_table"))


def _plain():
    from bramble_amd import synth
    ann = synth.Annotation("S")
    return ann.as_dict(), ann.reads(3000, "pe")


def _dense():
    from bramble_amd.batch import make_batch
    from tests.test_gpu_pairing_dense import annotation, paired_dense_records
    return annotation(), make_batch(paired_dense_records())


def _alphabet(case):
    return lambda: (case.annotation(), case.batch())


def _long(mode, n):
    def make():
        from bramble_amd import synth
        ann = synth.Annotation("G", n_genes=300, n_refs=2)
        return ann.as_dict(), ann.reads(n, mode)
    return make


def _rescue():
    from bramble_amd import synth
    ann = synth.Annotation("G", n_genes=300, n_refs=2, with_genome=True)   # (the input of test_soft_clip_rescue_with_genome, a third of it)
    return ann.as_dict(), ann.reads(1000, "ont", with_seq=1)


def _inputs():
    from tests import alphabet_cases as ac
    _plain_cached = functools.lru_cache(maxsize=None)(_plain)
    out = [Input("plain-" + name, _plain_cached, flags, SHORT_ROUTES)
           for name, flags in (("default", {}), ("strict", {"strict": 1}), ("fr", {"fr": 1}))]
    out.append(Input("dense", _dense, {}, DENSE_ROUTES))
    out += [Input("alphabet-" + c.id, _alphabet(c), c.flags, DENSE_ROUTES if c.kind == "dense" else SHORT_ROUTES)
            for c in ac.CASES if c.family == "short"]
    long_case = next(c for c in ac.CASES if c.id == "adv-long-lr-26")
    out.append(Input("alphabet-" + long_case.id, _alphabet(long_case), long_case.flags, LONG_ROUTES))
    out.append(Input("long-ont-lr", _long("ont", 600), {"lr": 1}, LONG_ROUTES))
    out.append(Input("long-hifi-lr_hq", _long("hifi", 600), {"lr_hq": 1}, LONG_ROUTES))
    out.append(Input("rescue-ont-lr-S", _rescue, {"lr": 1, "use_fasta": 1}, RESCUE_ROUTES))
    return out


INPUTS = _inputs()
BY_ID = {i.id: i for i in INPUTS}
ALPHABET = [i for i in INPUTS if i.id.startswith("alphabet-")]


# ---- the command line's input ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cli_pairs():
    """(Annotation, batch with its records): 40 000 synthetic pairs -- one default bundle of the command line (1 000 000 records)
    holds more than SMALL_N alignments of them, the smallest shape at which the program itself leaves the small-batch path"""
    from bramble_amd import synth
    ann = synth.Annotation("G", n_genes=1500)
    return ann, ann.reads(40000, "pe", with_records=1)
