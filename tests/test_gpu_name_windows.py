"""The shared front end of the adds that take read names (name_window.h, names_inl.h) and the field sort (barcode_sort.h), through
every accumulator that uses them.  The features' own tests mostly add from row 0 of tables of their own; here ONE table
(tests/name_window_cases.py, about 200 names: UMIs, cell barcodes, names without rows, names of 17 to 200 rows, pooled CIGARs)
goes into Quant (with and without "eff_len"), Coverage (weight em), Assign (with and without records), Dedup (with and without
"keep_records", and per cell) and Cells, from host tables and from device tables, once as one add and once as three adds that
point into the same whole tables: the middle add starts at a non-zero alignment, row and record byte, and its first and last
names have no rows, so a bias that is dropped or applied twice moves what a name reads.

Every read-out of the three-add objects is held to the CPU restatements (record_route_cases.Expect / Consumers.check: the classes
and name classes, the depth, the kept stream, rep / dup / group_first and the record pieces, the barcodes, the matrix -- exact --
and theta under the rule of tests.test_gpu_quant._assert_em_to, the only restatement a sum of doubles has) and is equal in bits to
the one-add objects'.  Before its middle add a three-add object is offered the bad tables -- a descending group_off, a descending
row_off at a name's boundary inside the window, a record offset that leaves n_bytes, a record shorter than 36 bytes -- and must
refuse each with BR_ERR_INVALID_ARG and go on as if it had never seen them: that is the comparison with the one-add object.
What has no record stream is offered the first two.  br_assign keeps the records' bytes and reads none of them at the add, so it
checks that the offsets ascend and stay inside the stream, not the 36 bytes: the short record is offered to Dedup and Cells.  And
of DEVICE tables only the span's ends come to the host: the kernels of Quant, Dedup and Cells take every name's rows from its
two offsets and refuse a name whose offsets descend, but those of Assign and Coverage find a row's name by a search over the
offsets, and offsets that descend somewhere between the right ends still give every row an alignment and a name (the intervals
chain) -- so the two descending tables are offered to Assign and Coverage from host tables only, where the add checks every
entry."""
import numpy as np
import pytest

from bramble_amd import lib
from tests import cells_cases as cc
from tests import dedup_cases as dc
from tests import name_window_cases as nw
from tests import record_route_cases as rr
from tests import route_cases as rc

pytestmark = pytest.mark.gpu

INVALID = -1
KINDS = ("dedup:directional", "dedup:cell", "cells:unique", "cells:em", "assign:tag", "cov:em")
_SEEN = {}    # way in -> the one-add objects' read-outs


class _Tables:
    """the whole tables in host or device memory, and variants of single tables that an add must refuse"""

    def __init__(self, t, where):
        self.t, self.dev = t, where == "device"
        tb = t.tb
        self.n_rows, self.n_pool, self.n_bytes = len(tb["a"]), len(tb["pool"]), int(t.stream.size)
        self.keep = {}
        self.ptr = {k: self._put(k, v) for k, v in (("a", tb["a"]), ("cigar", tb["cigar"]), ("pool", tb["pool"]), ("row_off", tb["row_off"]),
                                                    ("group_off", tb["group_off"]), ("data", t.stream), ("rec_off", t.rec_off))}

    def _put(self, key, arr):
        arr = np.ascontiguousarray(arr)
        if self.dev:
            import torch
            held = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()
            self.keep[key] = held
            return held.data_ptr()
        self.keep[key] = arr
        return arr.ctypes.data

    def stream(self):
        if not self.dev:
            return None
        import torch
        return torch.cuda.current_stream().cuda_stream

    def recs(self, rec_off=None, n_bytes=None):
        return lib.BrDeviceBam(self.ptr["data"], self.n_bytes if n_bytes is None else n_bytes, self.ptr["rec_off"] if rec_off is None else rec_off, self.n_rows)

    def add(self, kind, o, g0, g1, **bad):
        """the names [g0, g1) into `o` through its add as it is, every table whole; bad: addresses (or n_bytes) that stand in -> the
        return code"""
        p = dict(self.ptr, **{k: v for k, v in bad.items() if k != "n_bytes"})
        go, n, st = p["group_off"] + 4 * g0, g1 - g0, self.stream()
        recs = self.recs(p["rec_off"], bad.get("n_bytes"))
        if kind.startswith("quant"):
            return o.add_rows_raw(p["a"], p["cigar"], p["pool"], p["row_off"], self.n_rows, self.n_pool, go, n, self.dev, st)
        if kind.startswith("cov"):
            return o.add_names_raw(p["a"], p["cigar"], p["pool"], p["row_off"], self.n_rows, self.n_pool, go, n, self.dev, st)
        if kind.startswith("assign"):
            return o.add_raw(None if kind == "assign:values" else recs, p["a"], p["row_off"], self.n_rows, go, n, self.dev, st)
        if kind.startswith("dedup"):
            return o.add_raw(recs, p["a"], p["cigar"], p["pool"], p["row_off"], self.n_rows, self.n_pool, go, n, self.dev, st)
        return o.add_raw(recs, p["row_off"], self.n_rows, go, n, self.dev, st)

    def bad_tables(self, kind, g0, g1):
        """[(what, the stand-ins)] for the window [g0, g1): each a copy of one table with one entry changed"""
        t = self.t
        go, ro, rec = t.tb["group_off"].astype(np.int64), t.tb["row_off"].copy(), t.rec_off.copy()
        k = next(g for g in range(g0 + 2, g1) if ro[go[g]] > ro[go[g - 1]] > ro[go[g0]])   # name k - 1 has rows, and the window rows in front of it
        bad_go = t.tb["group_off"].copy()
        bad_go[k] = bad_go[g0]                                                           # name k - 1 ends where the window begins
        assert bad_go[k] < bad_go[k - 1]
        bad_ro = ro.copy()
        bad_ro[go[k]] = ro[go[k - 1]] - 1                                                # name k - 1 ends in front of where it begins
        out = []
        if not self.dev or kind.split(":")[0] in ("quant", "dedup", "cells"):
            out = [("group_off descends", {"group_off": self._put("bad_go", bad_go)}), ("row_off descends", {"row_off": self._put("bad_ro", bad_ro)})]
        if kind.split(":")[0] in ("dedup", "cells") or kind == "assign:tag":
            r1 = int(ro[go[g1]])
            out.append(("a record offset leaves n_bytes", {"n_bytes": int(rec[r1]) - 1}))
        if kind.split(":")[0] in ("dedup", "cells"):
            r = int(ro[go[k - 1]])                                                        # the first record of name k - 1: its last 35 bytes
            short = rec.copy()                                                           # (the record in front of it, whose fields stay where
            short[r] = short[r + 1] - np.uint64(35)                                      # they are, takes the rest)
            out.append(("a record of 35 bytes", {"rec_off": self._put("short", short)}))
        return out


def _objects(t):
    """-> (the Consumers of KINDS, {kind: object} of what Consumers does not hold)"""
    cons = rr.Consumers(nw.LENS, False, KINDS)
    q2 = lib.Quant(nw.N_TX, nw.LENS)
    for k, v in (("eff_len", 1), ("max_iters", rc.EM_ITERS), ("tolerance", 0)):
        q2.set_param(k, v)
    extra = {"quant:eff_len": q2, "assign:values": lib.Assign(mode=0, seed=rr.SEED), "dedup:no_records": lib.Dedup(method=dc.METHODS["directional"])}
    return cons, extra


def _feed(tabs, pieces):
    t = tabs.t
    cons, extra = _objects(t)
    everything = [("quant", cons.q)] + list(cons.objs.items()) + list(extra.items())
    for i, (g0, g1) in enumerate(nw.windows(t, pieces)):
        for kind, o in everything:
            if pieces == 3 and i == 1:
                for what, bad in tabs.bad_tables(kind, g0, g1):
                    assert tabs.add(kind, o, g0, g1, **bad) == INVALID, (kind, what)
            assert tabs.add(kind, o, g0, g1) == 0, (kind, g0, g1)
    if tabs.dev:
        import torch
        torch.cuda.synchronize()
    return cons, extra


def _read_out(tabs, pieces):
    """feeds, finishes and checks every object against the restatements -> every read-out, for the comparison in bits"""
    t, want = tabs.t, tabs.t.want
    cons, extra = _feed(tabs, pieces)
    try:
        out = dict(cons.check(want, "%s, %d adds" % ("device" if tabs.dev else "host", pieces)))
        n, n_rows = want.n_names, len(want.projected)
        out["name_classes"] = cons.q.name_classes()
        for kind in ("dedup:directional", "dedup:cell"):
            out[kind] = cons.objs[kind].result() + (cons.objs[kind].umis(0, n)[0],)
        for kind in ("cells:unique", "cells:em"):
            out[kind + " matrix"] = cons.objs[kind].matrix() + cons.objs[kind].barcodes(0, n)
        out["kept"] = cons.objs["assign:tag"].values(0, n_rows)
        out["depth"] = tuple(cons.objs["cov:em"].depth64(tid) for tid in want.depth_of(want.coverage_em(cons.q.posteriors())))
        # what Consumers does not hold
        q2 = extra["quant:eff_len"]
        q2.finish()
        from tests.test_gpu_quant import _assert_classes
        _assert_classes(q2, want.classes(), nw.N_TX)
        assert q2.em()[0] == rc.EM_ITERS
        res = q2.result()
        out["eff_len"] = tuple(np.asarray(res[k]) for k in sorted(res) if isinstance(res[k], np.ndarray))
        a2 = extra["assign:values"]
        assert a2.finish(cons.q) == (int(out["kept"][2].sum()), sum(1 for mine in want.placements()[1] if mine))
        out["values"] = a2.values(0, n_rows)
        for x, y in zip(out["values"], out["kept"]):
            assert rr.same_bits(x, y)                                # the records change nothing in the values
        d2, exp = extra["dedup:no_records"], want.dedup("directional")
        assert d2.finish() == exp["counts"]
        out["dedup:no_records"] = d2.result()
        for got, e in zip(out["dedup:no_records"], (exp["rep"], exp["gf"], exp["dup"])):
            assert np.array_equal(got, e)
        return out
    finally:
        cons.close()
        for o in extra.values():
            o.close()


def _assert_same(a, b, tag):
    assert set(a) == set(b)
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], tuple) else ((a[k],), (b[k],))
        assert len(xs) == len(ys), (tag, k)
        for x, y in zip(xs, ys):
            assert rr.same_bits(np.asarray(x), np.asarray(y)), (tag, k)


@pytest.mark.parametrize("where", ["host", "device"])
def test_one_add_equals_the_restatements(where):
    _SEEN[where] = _read_out(_Tables(nw.table(), where), 1)


@pytest.mark.parametrize("where", ["host", "device"])
def test_three_adds_into_the_whole_tables_and_the_refusals_between_them(where):
    tabs = _Tables(nw.table(), where)
    one = _SEEN.get(where) or _read_out(tabs, 1)
    _assert_same(one, _read_out(tabs, 3), where)
    if "host" in _SEEN and "device" in _SEEN:
        _assert_same(_SEEN["host"], _SEEN["device"], "host against device")


# ---- the field sort ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["directional", "unique"])
def test_per_cell_groups_that_share_barcodes_and_umis(method):
    """the group id in the length key keeps two position groups with the same (barcode, UMI) pairs apart in the sorted order; "an
    empty field is a head" keeps the names without a UMI, neighbours in that order, a molecule each"""
    run = nw.field_sort_run()
    groups = dc.records_of(run)
    tb, stream = dc.tables_of(run), dc.stream_of(groups)
    umis, _ = dc.umis_of(groups)
    bcs, _ = cc.barcodes_of(groups)
    rep, gf = cc.per_cell_molecules(method, groups, umis, bcs)
    d = lib.Dedup(method=dc.METHODS[method], cell_source=1)
    try:
        d.add_host(tb["a"], tb["cigar"], tb["pool"], tb["row_off"], tb["group_off"], stream)
        assert d.finish() == dc.counts_of(rep)
        got_rep, got_gf, got_dup = d.result()
        assert np.array_equal(got_rep, rep) and np.array_equal(got_gf, gf) and np.array_equal(got_dup, dc.dup_of(rep))
        st = d.stats()
        nodes = len({(g, u) for g, u in zip(gf.tolist(), umis) if u is not None}) + sum(1 for u in umis if u is None)
        assert st["groups"] == len(set(gf.tolist()) - {dc.NONE}) == 6 and st["nodes"] == nodes
    finally:
        d.close()
