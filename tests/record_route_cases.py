"""Helpers of the tests that hold --dedup, --cells, --quant-bam and --coverage-weight to their restatements on the rows AND records
of every projection route.  br_dedup_add_last, br_cells_add_last and br_assign_add_last read three things a bundle call leaves in
HBM -- the row table, the read-name groups and the projected record stream (ctx->last_bam) -- and four routes write the first two
(tests/route_cases.py).  A flat batch leaves no records, so the inputs here are raw BAM records, decorated so that every consumer
has work: UMIs by dedup_cases.with_umis_records (its plan of exact copies, one-mismatch copies, names without a UMI, a UMI of 33
bytes) on the even read names, barcodes and UMIs by cells_cases.with_cells_records (<name>_<CB>_<UMI>, the layout BC_NAME_PREV
reads, every seventh name without a barcode) on the odd ones.

  * decorate / decorate_lightly / prefixed / cut / records_of_batch: the inputs' builders;
  * Run, short_run, long_run, staged_run: production-shaped runs of bundle calls on one context;
  * run_route: a bundle call down a forced route (route_cases.ROUTES), through br_project_bam_bundle or br_project_bam_resident;
  * Expect: every expectation over one or several calls, from the oracle's bam_stream and rows alone, through the restatements of
    dedup_cases, cells_cases, quant_bam_cases, test_coverage_weight_cpu and test_quant_cpu;
  * Consumers: one object of each kind fed with add_last, and their results against an Expect;
  * INPUTS: the inputs of tests/test_gpu_record_consumers_routes.py; tests/test_record_route_cases_cpu.py checks on the CPU, from
    the oracle alone, that each holds what the GPU tests rely on.

What the inputs hold (test_record_route_cases_cpu.py asserts the conditions and prints these counts):

  input         records  names  with records  rows    molecules unique / directional  duplicates  no UMI  no barcode  cells (ambiguous)  unequal names  big alignments
  pairs-default 3036     1464   1414          13569   802 / 743                       671         190     882         12 (12)            992            0
  pairs-strict  3036     1464   1414          13551   802 / 743                       671         190     882         12 (12)            992            0
  dense         958      452    393           32359   221 / 203                       190         50      254         12 (12)            300            83
  long-ont-lr   1353     1353   1352          5990    767 / 711                       641         185     838         12 (12)            952            0
  rescue-ont-S  2252     2252   2252          10185   1280 / 1187                     1065        310     1397        12 (12)            1547           0

(records: in the input, after the decoration; rows: the oracle's rows = projected records; duplicates under the directional method;
unequal names: read names whose placements lie on two or more transcripts and do not all weigh the same under the restatement's own
EM; big alignments: those with more than 64 rows.  The runs: short_run 7 728 records in five bundles and an empty one, 35 977 rows;
long_run 4 433 records, 11 306 rows, 336 of them in the bundle with nine in ten records off the annotation; staged_run 6 700
records, 35 511 rows; the command line's input 88 674 records, 466 026 rows.)

No expectation is derived from a device run.  The quantifier's theta is held to the restatement's own EM over the exact classes
under the rule of tests.test_gpu_quant._assert_em (a bound from the restatement's spread over three class orders); what is a
function of theta -- posteriors, ZW, the sampled pick, the weight words of the EM-weighted depth -- is then restated from the theta
that passed that check, one IEEE operation after the other, and compared bit for bit, as the features' own tests do."""
import functools
import struct

import numpy as np

from tests import cells_cases as cc
from tests import dedup_cases as dc
from tests import quant_bam_cases as qb
from tests import route_cases as rc
from tests import unprojected_cases as uc

BIG = 1 << 30
INVALID = -1
CELLS_ITERS = 40     # tests/test_gpu_cells.py's EM_ITERS
SEED = 5             # the sampled placement's seed
N_FEATURES = 37


# ---- records -------------------------------------------------------------------------------------------------------------------
def cat(recs):
    return np.frombuffer(b"".join(recs), dtype=np.uint8) if recs else np.zeros(0, np.uint8)


def records_of_batch(b):
    """a synthetic batch made with with_records=1 -> its framed records"""
    from bramble_amd import synth
    return uc.split(synth.Annotation.frame_records(b)[0])


def decorate(recs, seed=0):
    """the read names of `recs` (framed, collated) alternately through with_umis_records and with_cells_records: names with a UMI
    alone (one separator: no barcode), names with a barcode and a UMI, and what the two plans hold of names with neither"""
    groups = uc.groups_of(recs)
    even = [r for a, e in groups[0::2] for r in recs[a:e]]
    odd = [r for a, e in groups[1::2] for r in recs[a:e]]
    return dc.with_umis_records(even, seed=seed) + cc.with_cells_records(odd, seed=seed)


def decorate_lightly(recs, n_copied=2000, seed=0):
    """the command line's input, 40 000 read names: the first n_copied of them through decorate (the copies that make duplicates),
    every other one once under <name>_<CB>_<UMI> with with_cells_records' cells -- every ninth without the barcode --, so that the
    bundle keeps its size and the Python restatements their seconds"""
    rng = np.random.default_rng(seed)
    cells = [cc._bc(rng, 8 + k % 3) for k in range(12)]     # (cells_cases.with_cells_records' and whitelist_cases.cli_whitelist's)
    groups = uc.groups_of(recs)
    cut_at = groups[n_copied][0]
    out = decorate(recs[:cut_at], seed=seed)
    for i, (a, e) in enumerate(groups[n_copied:]):
        nm = bytes(recs[a][36:36 + recs[a][12] - 1]).replace(b"_", b"-")
        name = nm + (b"_" + cells[int(rng.integers(12))] if i % 9 else b"") + b"_" + dc.random_umi(rng)
        out += [dc.renamed(bytes(r), name) for r in recs[a:e]]
    return out


def prefixed(recs, prefix):
    """the records under <prefix><name>: read names that never repeat across the bundles of a run"""
    return [dc.renamed(bytes(r), prefix + bytes(r[36:36 + r[12] - 1])) for r in recs]


def moved_off_the_annotation(recs, n_refs, keep_every=10):
    """all but every keep_every-th record on reference n_refs + its own: a reference the reference map sends to -1"""
    out = []
    for i, r in enumerate(recs):
        if i % keep_every:
            ref = struct.unpack_from("<i", r, 4)[0]
            r = r[:4] + struct.pack("<i", n_refs + ref) + r[8:]
        out.append(r)
    return out


def group_off_of(recs):
    return np.asarray([a for a, _ in uc.groups_of(recs)] + [len(recs)], dtype=np.uint32)


def cut(recs, sizes):
    """the records in consecutive pieces of about sizes[k] records, cut on read-name boundaries (the last piece takes the rest)"""
    go = group_off_of(recs).astype(np.int64)
    out, at = [], 0
    for k, n in enumerate(sizes):
        end = len(recs) if k == len(sizes) - 1 else int(go[go <= min(at + n, len(recs))][-1])
        assert end > at
        out.append(recs[at:end])
        at = end
    return out


def split3(recs):
    """-> (stream, rec_off, rec_len) as br_bam_bundle takes them"""
    sizes = np.asarray([len(r) for r in recs], dtype=np.uint64)      # (a framed record: its block_size word and block_size bytes)
    rec_off = np.cumsum(sizes, dtype=np.uint64) - sizes + np.uint64(4) if len(recs) else np.zeros(0, np.uint64)
    return cat(recs), rec_off, (sizes - np.uint64(4)).astype(np.uint32)


# ---- routes --------------------------------------------------------------------------------------------------------------------
def project(ctx, cfg, recs, ref_map, resident=False):
    """one bundle call -> (the projected stream, the tensors that must live until the consumers have read the call).  resident:
    the records are uploaded here and the result stays in HBM (br_project_bam_resident, BR_OUT_RESIDENT) and is fetched with
    br_device_bam_download, which leaves the context's last call as it is"""
    from bramble_amd import lib
    stream, roff, rlen = split3(recs)
    if not resident or not len(recs):
        return ctx.project_bam_bundle(cfg, stream, roff, rlen, ref_map)[0], None
    import torch
    held = (torch.from_numpy(stream.copy()).cuda(), torch.from_numpy(roff.astype(np.int64)).cuda(), torch.from_numpy(rlen.astype(np.int32)).cuda())
    r = lib.BrDeviceRecords()
    r.blob, r.rec_off, r.n_aln, r.rec_len = held[0].data_ptr(), held[1].data_ptr(), len(rlen), held[2].data_ptr()
    db, cnt = ctx.project_bam_resident_kept(cfg, r, ref_map)
    return db, held


def run_route(ctx, route, cfg, recs, ref_map, resident=False):
    """`recs` down `route` on a context route_cases.new_context made for it -> (the route the call took, the projected stream or,
    resident, the BrDeviceBam; what has to be kept alive).  "predicted": the first read names, at most half of the records, go
    first as a bundle of their own; "small_n" is that bundle's size, so the input itself is a large batch launched from the
    counts the small call left"""
    small_n = rc.SMALL_N
    if route == "predicted":
        go = group_off_of(recs).astype(np.int64)
        small_n = int(go[go <= len(recs) // 2][-1])
        assert 0 < small_n < len(recs)
        ctx.set_param("small_n", small_n)
        project(ctx, cfg, recs[:small_n], ref_map)
        assert rc.route_of(ctx, small_n, small_n) == "small"
    out, held = project(ctx, cfg, recs, ref_map, resident)
    return rc.route_of(ctx, len(recs), small_n), out, held


# ---- expectations -----------------------------------------------------------------------------------------------------------------
def _lazy(fn):
    return functools.lru_cache(maxsize=None)(fn)


class Expect:
    """Every expectation over the calls [(the oracle's rows of a bundle, the bundle's group_off)], the calls' read names one after
    the other as the accumulators number them; lens: the transcript lengths; long_reads: br_assign's "long_reads"."""

    def __init__(self, calls, lens, long_reads=False):
        self.lens, self.long_reads, self.n_tx = np.asarray(lens, dtype=np.int64), bool(long_reads), len(lens)
        self.stream = np.concatenate([np.asarray(o["bam_stream"], dtype=np.uint8) for o, _ in calls] + [np.zeros(0, np.uint8)])
        self.rows_per_alignment = np.concatenate([np.bincount(np.asarray(o["input_index"], dtype=np.int64), minlength=int(g[-1])) for o, g in calls])
        self.rows, self.row_off, self.group_off = rc.concat_tables([rc.yardstick_rows(o, g) for o, g in calls])
        self.projected = uc.split(self.stream)               # framed, record i = row i
        assert len(self.projected) == len(self.rows["tid"])
        ro, go = self.row_off.astype(np.int64), self.group_off.astype(np.int64)
        self.n_names = len(go) - 1
        self.groups = [[self.projected[r][4:] for r in range(int(ro[go[g]]), int(ro[go[g + 1]]))] for g in range(self.n_names)]
        for g in self.groups:                                # a name's records carry one read name
            assert len({r[32:32 + r[8]] for r in g}) <= 1
        # (transcript t is feature t mod N_FEATURES: the isoforms of a gene are features of their own, and distant genes share them)
        self.n_features = min(N_FEATURES, max(self.n_tx, 1))
        self.tx_feature = (np.arange(self.n_tx, dtype=np.uint32) % np.uint32(self.n_features)).astype(np.uint32)

    # -- dedup
    @_lazy
    def umis(self):
        return dc.umis_of(self.groups)

    @_lazy
    def signatures(self):
        return dc.signatures_of(self.groups)

    @_lazy
    def dedup(self, method, per_cell=False):
        umis, cnt = self.umis()
        sigs = self.signatures()
        if per_cell:
            rep, gf = cc.per_cell_molecules(method, self.groups, umis, self.barcodes()[0])
        else:
            rep, gf = dc.molecules_of(method, sigs, umis), dc.groups_of(sigs)
        dup = dc.dup_of(rep)
        return {"umis": dc.umi_matrix(umis), "cnt": cnt, "gf": gf, "rep": rep, "dup": dup, "hist": dc.hist_of(rep), "counts": dc.counts_of(rep),
                "stream": dc.expected_stream(self.groups, dup, True)}

    # -- cells
    @_lazy
    def barcodes(self):
        return cc.barcodes_of(self.groups)

    @_lazy
    def cells_model(self):
        name_cls, classes = cc.classes_of(self.groups)
        return cc.model_of(self.barcodes()[0], name_cls, classes, self.tx_feature)

    @_lazy
    def cells(self, mode):
        """-> (the restatement's matrix, its spread s over three summation orders; s is None in mode unique)"""
        if mode == "unique":
            return cc.matrix_of(self.cells_model(), "unique"), None
        return cc.spread_of(self.cells_model(), mode, 1 if mode == "uniform" else CELLS_ITERS)

    # -- the quantifier's tables
    @_lazy
    def classes(self):
        from tests.test_quant_cpu import classes_of
        return classes_of(self.rows["tid"], self.row_off, self.group_off)

    @_lazy
    def name_classes(self):
        from tests.test_coverage_weight_cpu import name_classes_of
        return name_classes_of(self.rows["tid"], self.row_off, self.group_off)

    @_lazy
    def row_names(self):
        from tests.test_coverage_weight_cpu import row_names_of
        return row_names_of(len(self.rows["tid"]), self.row_off, self.group_off)

    @_lazy
    def placements(self):
        return qb.placements_of(self.rows["meta"], self.row_off, self.group_off)

    def posteriors(self, theta):
        """the posteriors of `theta` under length normalisation (the quantifier's default w = 1 / length)"""
        from tests.test_coverage_weight_cpu import posteriors_of
        from tests.test_quant_cpu import weights
        return posteriors_of(self.classes(), theta, weights(self.lens, self.n_tx, 1))

    def assign(self, post, mode):
        """-> (w per record, kept per record, the rewritten stream)"""
        pl = self.placements()
        w, _ = qb.weights_of(post, self.classes(), self.name_classes(), self.row_names(), self.rows["tid"], pl)
        kept = qb.kept_of(w, pl, mode, SEED)
        return w, kept, qb.rewrite(self.projected, qb.zw_of(w), kept, mode, self.long_reads)

    # -- weighted coverage
    @_lazy
    def coverage_nh(self):
        from tests.test_coverage_weight_cpu import nh_of, weight_words_nh, weighted_coverage_of
        nh = nh_of(len(self.rows["tid"]), self.row_off, self.group_off)
        return weighted_coverage_of(self.rows, self.lens, weight_words_nh(nh), False)

    def coverage_em(self, post):
        from tests.test_coverage_weight_cpu import weight_words_em, weighted_coverage_of
        q = weight_words_em(self.classes(), post, self.name_classes(), self.row_names(), self.rows["tid"])
        return weighted_coverage_of(self.rows, self.lens, q, False)

    def depth_of(self, cov):
        return sorted({int(np.argmax(cov["max_depth"])), int(np.argmax(cov["records"])), 0, self.n_tx // 2, self.n_tx - 1, int(np.argmax(self.lens))})

    # -- what the inputs hold
    @_lazy
    def counts(self):
        with_records = [i for i, g in enumerate(self.groups) if g]
        uniq, direc = self.dedup("unique")["counts"], self.dedup("directional")["counts"]
        bcs, bcnt = self.barcodes()
        model = self.cells_model()
        ambiguous = sum(1 for es in model["entries"] if any(len(fs) != 1 for _, _, fs in es))
        tid, ro, go = self.rows["tid"], self.row_off.astype(np.int64), self.group_off.astype(np.int64)
        multi_tx = sum(1 for g in range(self.n_names) if len(set(tid[int(ro[go[g]]):int(ro[go[g + 1]])].tolist())) >= 2)
        return {"records_out": len(self.projected), "names": self.n_names, "names_with_records": len(with_records), "rows": len(tid),
                "molecules_unique": uniq[1], "molecules_directional": direc[1], "duplicates": direc[2], "no_umi": self.umis()[1]["no_umi"],
                "no_barcode": bcnt["no_barcode"], "cells": len(model["cells"]), "cells_ambiguous": ambiguous, "names_multi_tx": multi_tx,
                "big_alignments": int((self.rows_per_alignment > 64).sum())}

    @_lazy
    def em_spread(self):
        """(the restatement's own EM over the classes -- 1 / length, rc.EM_ITERS iterations, tolerance 0 --, its spread s over three
        class orders): what the device's theta and tpm are held to, under the rule of tests.test_gpu_quant._assert_em"""
        from tests.test_gpu_quant import _spread
        return _spread(self.classes(), self.n_tx, self.lens, True, rc.EM_ITERS)

    def em_restated(self):
        """the restatement's theta: the input of the conditions the CPU test checks"""
        return self.em_spread()[0]["theta"]

    def names_with_unequal_weights(self, post):
        """the read names whose placements lie on two or more transcripts and do not all weigh the same"""
        w, _ = qb.weights_of(post, self.classes(), self.name_classes(), self.row_names(), self.rows["tid"], self.placements())
        tid, out = self.rows["tid"], 0
        for mine in self.placements()[1]:
            out += len({int(tid[r]) for r in mine}) >= 2 and len({float(w[r]) for r in mine}) >= 2
        return out


# ---- the consumers of a context's last call ----------------------------------------------------------------------------------------
def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def drain(obj, max_bytes=BIG):
    parts = []
    for data, off in obj.pieces(max_bytes):
        assert off[0] == 0 and int(off[-1]) == data.size and np.all(np.diff(off) > 0)
        parts.append(data)
    assert obj.next_records(max_bytes).n_rows == 0
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


ALL = ("dedup:directional", "dedup:unique", "dedup:cell", "cells:unique", "cells:uniform", "cells:em", "assign:tag", "assign:sample", "cov:nh", "cov:em")


class Consumers:
    """A Quant ("keep_names") and the record consumers named in `kinds` (ALL), each fed with add_last after every call."""

    def __init__(self, lens, long_reads=False, kinds=ALL):
        from bramble_amd import lib
        lens = np.asarray(lens, dtype=np.int64)
        self.lens, self.n_tx = lens, len(lens)
        self.q = lib.Quant(self.n_tx, lens)
        self.q.set_param("keep_names", 1)
        self.q.set_param("max_iters", rc.EM_ITERS)
        self.q.set_param("tolerance", 0)
        self.objs = {}
        for kind in kinds:
            what, how = kind.split(":")
            if what == "dedup":
                o = lib.Dedup(method=dc.METHODS["directional" if how == "cell" else how], keep_records=1, mark=1, **({"cell_source": 1} if how == "cell" else {}))
            elif what == "cells":
                o = lib.Cells(mode=cc.MODES[how], max_iters=1 if how == "uniform" else CELLS_ITERS, tolerance=0.0, call_counts=1)
            elif what == "assign":
                o = lib.Assign(mode=qb.MODES[how], seed=SEED, long_reads=int(long_reads))
            else:
                o = lib.Coverage(lens)
                o.set_param("weight", 1 if how == "nh" else 2)
            self.objs[kind] = o

    def everything(self):
        return [self.q] + list(self.objs.values())

    def add_last(self, ctx):
        for o in self.everything():
            o.add_last(ctx)

    def close(self):
        for o in self.everything():
            o.close()

    def check(self, want, tag=""):
        """finishes every object and holds it to `want` (an Expect) -> the floating-point results, for comparisons in bits:
        theta, the cells' values, w (whose float32 is ZW), the EM-weighted runs"""
        from tests.test_gpu_coverage_weight import _assert_weighted
        from tests.test_gpu_quant import _assert_classes
        q, n, floats = self.q, want.n_names, {}
        q.finish()
        _assert_classes(q, want.classes(), self.n_tx)
        assert np.array_equal(q.name_classes(), want.name_classes()), tag
        assert q.em()[0] == rc.EM_ITERS
        from tests.test_gpu_quant import _assert_em_to
        res = q.result()
        ref, s = want.em_spread()
        _assert_em_to(res, ref, s, rc.EM_ITERS, tag)    # theta and tpm against the restatement's own EM over the exact classes
        floats["theta"], floats["tpm"] = res["theta"], res["tpm"]
        post = q.posteriors()
        assert same_bits(post, want.posteriors(floats["theta"])), tag
        for kind, o in self.objs.items():
            what, how = kind.split(":")
            t = "%s %s" % (tag, kind)
            if what == "dedup":
                self._check_dedup(o, want.dedup("directional" if how == "cell" else how, how == "cell"), n, t)
            elif what == "cells":
                floats[kind] = self._check_cells(o, want, how, n, t)
            elif what == "assign":
                w, kept, stream = want.assign(post, how)
                n_out, n_named = o.finish(q)
                assert (n_out, n_named) == (int(kept.sum()), sum(1 for mine in want.placements()[1] if mine)), t
                gw, gz, gk = o.values(0, len(w))
                assert same_bits(gw, w) and same_bits(gz, qb.zw_of(w)) and np.array_equal(gk, kept), t
                got = drain(o, 1 << 16)
                assert got.size == stream.size and np.array_equal(got, stream), t
                assert all(v == 0 for k, v in o.stats().items() if k.startswith("bad_")), t
                floats[kind] = gw
            elif how == "nh":
                o.finish()
                cov = want.coverage_nh()
                _assert_weighted(o, cov, self.lens, want.depth_of(cov), t)
            else:
                o.finish_em(q)
                cov = want.coverage_em(post)
                _assert_weighted(o, cov, self.lens, want.depth_of(cov), t)
                floats[kind] = o.runs64()[3]
        return floats

    @staticmethod
    def _check_dedup(d, exp, n, tag):
        assert d.finish() == exp["counts"], tag
        umi, ln = d.umis(0, n)
        assert np.array_equal(ln, exp["umis"][1]) and np.array_equal(umi, exp["umis"][0]), tag
        rep, gf, dup = d.result()
        for got, e, what in ((gf, exp["gf"], "group_first"), (rep, exp["rep"], "rep"), (dup, exp["dup"], "dup")):
            bad = np.flatnonzero(got != e)
            assert bad.size == 0, (tag, what, bad[:5], got[bad[:5]], e[bad[:5]])
        assert np.array_equal(d.hist(), exp["hist"]), tag
        st = d.stats()
        assert (st["names"], st["no_umi"], st["umi_too_long"], st["bad_aux"]) == (n, exp["cnt"]["no_umi"], exp["cnt"]["too_long"], exp["cnt"]["bad_aux"]), tag
        assert st["groups"] == len(set(exp["gf"].tolist()) - {dc.NONE}) and st["names_with_rows"] == int(np.count_nonzero(exp["rep"] != dc.NONE)), tag
        got = drain(d, 1 << 16)
        assert got.size == exp["stream"].size and np.array_equal(got, exp["stream"]), tag

    def _check_cells(self, c, want, mode, n, tag):
        from tests.test_gpu_cells import _assert_values
        model = want.cells_model()
        ref, s = want.cells(mode)
        bcs, cnt = want.barcodes()
        c.finish(self.q, want.tx_feature, want.n_features)
        cb, ln = c.barcodes(0, n)
        wcb, wln = cc.barcode_matrix(bcs)
        assert np.array_equal(ln, wln) and np.array_equal(cb, wcb), tag
        assert (c.n_cells, c.n_entries) == (len(model["cells"]), len(ref["feature"])) and c.cell_barcodes() == model["cells"], tag
        assert np.array_equal(c.name_cells(0, n), model["name_cell"]), tag
        off, feat, val = c.matrix()
        assert np.array_equal(off, ref["off"]) and np.array_equal(feat, ref["feature"]), tag
        cs = c.cell_stats()
        for k in ("names", "unique", "multi", "features", "iterations"):
            assert np.array_equal(cs[k], ref[k]), (tag, k)
        st = c.stats()
        assert (st["names"], st["no_barcode"], st["barcode_too_long"], st["bad_aux"]) == (n, cnt["no_barcode"], cnt["too_long"], cnt["bad_aux"]), tag
        assert st["counted"] == int(np.count_nonzero(model["name_cell"] != cc.NONE)) == int(ref["names"].sum()) and st["cells"] == len(model["cells"]), tag
        if mode == "unique":
            assert same_bits(val, ref["value"]), tag     # integers: exact
        else:
            _assert_values(val, ref["value"], s, tag)
        return val


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
class Input:
    """One decorated record stream under one preset.  routes: (route asked for, route the call takes), as route_cases.Input."""

    def __init__(self, name, make, flags, routes):
        self.id, self._make, self.flags, self.routes = name, make, dict(flags), routes
        self.long_reads = bool(flags.get("lr") or flags.get("lr_hq"))

    @_lazy
    def data(self):
        """(annotation dict, the framed records, the reference map)"""
        annd, recs = self._make()
        return annd, recs, np.arange(len(annd["refnames"]), dtype=np.int32)

    @_lazy
    def want(self):
        from oracle import oracle_binding as ob
        annd, recs, ref_map = self.data()
        oi = ob.OracleIndex(annd)
        orc, _, _, _ = ob.run_bam(oi, ob.make_flags(**self.flags), *split3(recs), ref_map)
        return Expect([(orc, group_off_of(recs))], rc.oracle_lens(oi), self.long_reads)


PAIR_ROUTES = rc.SHORT_ROUTES
DENSE_ROUTES = (("direct", "direct"), ("direct_side64", "direct"), ("match_table", "match_table"))
LONG_ROUTES = (("small", "small"), ("predicted", "predicted"), ("match_table", "match_table"))
RESCUE_ROUTES = rc.RESCUE_ROUTES
DENSE_NAMES = 200    # read names of dense-pe-default-25 before the decoration


@_lazy
def _pairs():
    from bramble_amd import synth
    ann = synth.Annotation("S")
    return ann.as_dict(), tuple(decorate(records_of_batch(ann.reads(650, "pe", with_records=1))))


@_lazy
def _dense():
    ann, _, _, _, _, _, recs = uc.case_input("dense-pe-default-25")
    return ann, tuple(decorate(recs[:int(group_off_of(recs)[DENSE_NAMES])]))


@_lazy
def _long():
    from bramble_amd import synth
    ann = synth.Annotation("G", n_genes=300, n_refs=2)
    return ann.as_dict(), tuple(decorate(records_of_batch(ann.reads(600, "ont", with_records=1))))


@_lazy
def _rescue():
    from bramble_amd import synth
    ann = synth.Annotation("G", n_genes=300, n_refs=2, with_genome=True)
    return ann.as_dict(), tuple(decorate(records_of_batch(ann.reads(1000, "ont", with_seq=1, with_records=1))))


INPUTS = [Input("pairs-default", _pairs, {}, PAIR_ROUTES), Input("pairs-strict", _pairs, {"strict": 1}, PAIR_ROUTES),
          Input("dense", _dense, {}, DENSE_ROUTES), Input("long-ont-lr", _long, {"lr": 1}, LONG_ROUTES),
          Input("rescue-ont-S", _rescue, {"lr": 1, "use_fasta": 1}, RESCUE_ROUTES)]
BY_ID = {i.id: i for i in INPUTS}


# ---- production-shaped runs -----------------------------------------------------------------------------------------------------------
class Run:
    """A run of bundle calls on one context: calls = [(the bundle's framed records, the route the call takes or None for an empty
    bundle, context parameters to set before it)]; the expectations are those over the concatenation of the calls' oracle
    streams and rows"""

    def __init__(self, annd, flags, small_n, ref_map, calls):
        self.annd, self.flags, self.small_n, self.ref_map, self.calls = annd, dict(flags), small_n, np.asarray(ref_map, dtype=np.int32), calls
        self.long_reads = bool(flags.get("lr") or flags.get("lr_hq"))

    @_lazy
    def oracle(self):
        """-> ([(the oracle's rows, group_off) per call with records], the transcript lengths)"""
        from oracle import oracle_binding as ob
        oi = ob.OracleIndex(self.annd)
        out = []
        for recs, _, _ in self.calls:
            if len(recs):
                out.append((ob.run_bam(oi, ob.make_flags(**self.flags), *split3(recs), self.ref_map)[0], group_off_of(recs)))
        return out, rc.oracle_lens(oi)

    @_lazy
    def want(self):
        calls, lens = self.oracle()
        return Expect(calls, lens, self.long_reads)


def _bundle(ann, n, mode, seed, k):
    """a decorated synthetic bundle whose read names carry the call's number in front"""
    return tuple(prefixed(decorate(records_of_batch(ann.reads(n, mode, seed=seed, with_records=1)), seed=k), b"c%d." % k))


@_lazy
def short_run():
    """small, predicted, direct rows twice (the second call starts from the first one's tables), an empty bundle -- it resets
    the context's last table, so the adds after it add nothing --, and small again"""
    from bramble_amd import synth
    ann = synth.Annotation("S")
    small_n = 1000
    b = [_bundle(ann, n, "pe", s, k) for k, (n, s) in enumerate(((190, 101), (500, 102), (450, 103), (350, 104), (150, 105)))]
    assert len(b[0]) <= small_n < len(b[1]) and len(b[4]) <= small_n < min(len(b[2]), len(b[3]))
    calls = [(b[0], "small", {}), (b[1], "predicted", {}), (b[2], "direct", {"small_batch": 0}), (b[3], "direct", {}), ((), None, {}),
             (b[4], "small", {"small_batch": 1})]
    return Run(ann.as_dict(), {}, small_n, np.arange(1, dtype=np.int32), calls)


@_lazy
def long_run():
    """a similarity-filter preset: the ordinary match table (nothing to predict from), a predicted launch, and a predicted launch
    of a bundle with far fewer matches per record than predicted: nine in ten records lie on references the reference map does
    not know.  The first bundle is more than twice the others, as in tests/test_gpu_consumers_routes.py"""
    from bramble_amd import synth
    ann = synth.Annotation("G", n_genes=300, n_refs=2)
    small_n = 600
    b = [_bundle(ann, n, "hifi", s, k) for k, (n, s) in enumerate(((1070, 79), (450, 80), (450, 81)))]
    b[2] = tuple(moved_off_the_annotation(b[2], 2))
    assert min(len(x) for x in b) > small_n and len(b[0]) > 2 * max(len(b[1]), len(b[2]))
    calls = [(b[0], "match_table", {}), (b[1], "predicted", {}), (b[2], "predicted", {})]
    return Run(ann.as_dict(), {"lr_hq": 1}, small_n, np.asarray([0, 1, -1, -1], dtype=np.int32), calls)


STAGED_SIZES = (1800, 300, 2500, 900, 1200)


@_lazy
def staged_run():
    """five bundles of about STAGED_SIZES records for the command line's call form (br_bam_bundle_stage +
    br_project_bam_staged_nowait over three slots)"""
    from bramble_amd import synth
    ann = synth.Annotation("G", n_genes=600, n_refs=3)
    recs = decorate(records_of_batch(ann.reads(1500, "pe", seed=501, with_records=1)))
    assert len(recs) > sum(STAGED_SIZES)
    calls = [(tuple(piece), "small", {}) for piece in cut(recs, STAGED_SIZES + (1,))[:len(STAGED_SIZES)]]   # (the rest is left out)
    return Run(ann.as_dict(), {}, rc.SMALL_N, np.arange(3, dtype=np.int32), calls)
