"""--dedup, --cells, --quant-bam and --coverage-weight on the rows and records of every projection route.  br_dedup_add_last,
br_cells_add_last and br_assign_add_last read what a bundle call leaves in HBM -- the row table, the read-name groups and the
projected record stream (ctx->last_bam) -- and the weighted br_coverage_add_last the first two; four routes write them: the
small-batch path, the predicted launch of a large batch, direct rows (k_big and the side arena's retry among them) and the match
table (with the -S rescue's DP in the middle).  The features' own tests feed them from hand-built tables or from the small-batch
path only; the command line calls add_last after every bundle of 1 000 000 records, so a production run feeds them from the
other three.

Here every input of tests/record_route_cases.py -- decorated pairs under two presets, the dense paired locus, long reads, -S --
goes down every route it can take, through br_project_bam_bundle or br_project_bam_resident (the route is asserted from the kernel
timers, the call's own stream is the oracle's byte for byte), and fresh objects take the call with add_last: Dedup in both
methods and per cell, Cells in three modes, Assign in both modes beside a Quant, Coverage with weight nh and em.  Every result is
held to the restatements over the oracle's stream and rows (rr.Expect / rr.Consumers.check), and every floating-point result --
theta, the cells' values, w (ZW), the EM-weighted depth -- is equal in bits among the routes of one input: the consumers run the
same code on the same logical table.  Then production-shaped runs of calls on one context with one set of accumulators; the
command line's own call form, br_bam_bundle_stage + br_project_bam_staged_nowait over three slots, where nobody waits for a
bundle's download before the next launch; and the refusals of a flat batch call on the other routes."""
import ctypes as C

import numpy as np
import pytest

from bramble_amd import lib
from tests import record_route_cases as rr
from tests import route_cases as rc

pytestmark = pytest.mark.gpu

_FLOATS = {}    # input -> (route, the floating-point results) of the first route that ran
RESIDENT = ("direct", "match_table")   # the routes asked for through br_project_bam_resident; the others go through br_project_bam_bundle


def _assert_same_floats(key, asked, floats):
    first_route, first = _FLOATS.setdefault(key, (asked, floats))
    assert set(first) == set(floats)
    for k in floats:
        assert rr.same_bits(first[k], floats[k]), (key, k, first_route, asked)


def _assert_direct_diag(ctx, inp, asked):
    d = ctx.direct_diag()
    if inp.id == "dense":
        assert d["n_big"] > 50, d                                    # k_big, k_pair_big and the side arena
    if asked == "direct_side64":
        assert d["side_attempts"] > 1 and d["side_cap"] > 64, d     # the arena was regrown and the attempt repeated


CASES = [(inp, asked, expect) for inp in rr.INPUTS for asked, expect in inp.routes]


# ---- (a) one call, every route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inp,asked,expect", CASES, ids=["%s-%s" % (i.id, a) for i, a, _ in CASES])
def test_record_consumers_on_every_route(inp, asked, expect):
    annd, recs, ref_map = inp.data()
    want = inp.want()
    idx = lib.Index(annd, device=0)
    ctx = rc.new_context(idx, asked)
    cons = rr.Consumers(want.lens, inp.long_reads)
    try:
        route, out, held = rr.run_route(ctx, asked, lib.make_config(**inp.flags), list(recs), ref_map, resident=asked in RESIDENT)
        assert route == expect, (inp.id, asked, route)
        if route == "direct":
            _assert_direct_diag(ctx, inp, asked)
        cons.add_last(ctx)
        stream = ctx.device_bam_download(out) if asked in RESIDENT else out
        assert stream.size == want.stream.size and np.array_equal(stream, want.stream)   # the call's own records are the oracle's
        floats = cons.check(want, "%s on %s" % (inp.id, asked))
        del held
    finally:
        cons.close()
        ctx.close()
        idx.close()
    _assert_same_floats(inp.id, asked, floats)


# ---- (b) production-shaped runs of calls ----------------------------------------------------------------------------------------------
RUN_KINDS = ("dedup:directional", "cells:em", "assign:tag", "cov:em")


def _play(run, kinds=RUN_KINDS):
    """the calls of `run` on one context, one object of each kind taking add_last after every call (the calls alternate between
    the two entry points); the accumulators against the restatements over the concatenation of the calls' oracle streams and rows"""
    want = run.want()
    idx = lib.Index(run.annd, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("small_n", run.small_n)
    ctx.set_profiling(True)
    cons = rr.Consumers(want.lens, run.long_reads, kinds)
    cfg = lib.make_config(**run.flags)
    streams, keep = [], []
    try:
        for k, (recs, route, params) in enumerate(run.calls):
            for name, v in params.items():
                ctx.set_param(name, v)
            resident = k % 2 == 1 and len(recs) > 0
            out, held = rr.project(ctx, cfg, list(recs), run.ref_map, resident)
            keep.append(held)
            if route is not None:
                got = rc.route_of(ctx, len(recs), run.small_n)
                assert got == route, (k, got, route)
            before = cons.q.stats()["held_bytes"]
            cons.add_last(ctx)
            if not len(recs):   # an empty bundle resets the context's last table: the adds after it add nothing
                assert out.size == 0 and cons.q.stats()["held_bytes"] == before
            streams.append(ctx.device_bam_download(out) if resident else out)
        got = np.concatenate(streams)
        assert got.size == want.stream.size and np.array_equal(got, want.stream)
        return cons.check(want, "run")
    finally:
        cons.close()
        ctx.close()
        idx.close()


def test_a_run_of_short_read_bundles():
    """small, predicted, direct rows twice (the second call starts from the first one's tables), an empty bundle, small again"""
    run = rr.short_run()
    assert [r for _, r, _ in run.calls] == ["small", "predicted", "direct", "direct", None, "small"]
    _play(run)


def test_a_run_of_long_read_bundles():
    """the ordinary match table, a predicted launch, a predicted launch with nine in ten records off the annotation"""
    run = rr.long_run()
    assert [r for _, r, _ in run.calls] == ["match_table", "predicted", "predicted"]
    _play(run)


# ---- (c) the command line's own call form ---------------------------------------------------------------------------------------------
STAGED_KINDS = ("dedup:directional", "cells:em", "assign:tag", "assign:sample")


def _staged(run, wait_every_bundle):
    """br_bam_bundle_stage + br_project_bam_staged_nowait, bundle k in slot k % 3, add_last on every object right after the
    launch; br_host_bam_wait after every bundle, or only after the last one -> (the consumers' floats, the dedup's and the two
    assigns' record streams, the last bundle's downloaded blocks)"""
    want = run.want()
    L = lib.lib()
    L.br_bam_bundle_stage.argtypes = [C.c_void_p, C.POINTER(lib.BrBamBundle), C.c_int]
    L.br_project_bam_staged_nowait.argtypes = [C.c_void_p, C.POINTER(lib.BrConfig), C.POINTER(lib.BrBamBundle), C.c_int, C.POINTER(lib.BrHostBam)]
    L.br_host_bam_wait.argtypes = [C.c_void_p, C.POINTER(lib.BrHostBam)]
    idx = lib.Index(run.annd, device=0)
    ctx = lib.Context(idx)
    cfg = lib.make_config(**run.flags)
    cons = rr.Consumers(want.lens, run.long_reads, STAGED_KINDS)
    ref_map = np.ascontiguousarray(run.ref_map, dtype=np.int32)
    keep, fields = [], ("n_bytes", "n_rows", "total_complete", "total_unique", "dropped_reads", "total_processed")
    try:
        outs = []
        for k, (recs, _, _) in enumerate(run.calls):
            stream, roff, rlen = rr.split3(list(recs))
            keep.append((stream, roff, rlen))
            bb = lib.BrBamBundle(stream.ctypes.data, stream.size, roff.ctypes.data, rlen.ctypes.data, len(rlen), ref_map.ctypes.data, len(ref_map), 1)
            out = lib.BrHostBam()
            assert L.br_bam_bundle_stage(ctx.h, C.byref(bb), k % 3) == 0
            assert L.br_project_bam_staged_nowait(ctx.h, C.byref(cfg), C.byref(bb), k % 3, C.byref(out)) == 0
            if wait_every_bundle:
                assert L.br_host_bam_wait(ctx.h, C.byref(out)) == 0
            cons.add_last(ctx)
            outs.append(out)
        assert L.br_host_bam_wait(ctx.h, C.byref(outs[-1])) == 0
        last = np.ctypeslib.as_array(C.cast(outs[-1].data, C.POINTER(C.c_uint8)), shape=(int(outs[-1].n_bytes),)).copy()
        counters = [tuple(int(getattr(o, f)) for f in fields) for o in outs]
        assert sum(c[1] for c in counters) == len(want.projected)
        # the streams are drained inside check and held to the restatement there; here they are read once more for the comparison
        floats = cons.check(want, "staged, wait_every_bundle=%d" % wait_every_bundle)
        tables = {"dedup": cons.objs["dedup:directional"].result(), "cells": cons.objs["cells:em"].matrix(),
                  "kept": [cons.objs[k].values(0, len(want.projected))[2] for k in ("assign:tag", "assign:sample")]}
        return floats, tables, last, counters
    finally:
        cons.close()
        ctx.close()
        idx.close()


def test_add_last_beside_downloads_nobody_waits_for():
    """Five bundles over the three slots.  The command line's writer waits for bundle k only after bundle k + 1 was launched, and
    its consumers take bundle k + 1 with add_last in between: their copies inside HBM run beside the download of bundle k and
    before the device buffers come round again.  Both runs are held to the restatement (the kept and the rewritten records
    byte for byte); their tables and the last bundle's blocks are the same."""
    run = rr.staged_run()
    assert len(run.calls) == 5
    late = _staged(run, False)
    each = _staged(run, True)
    for k in late[0]:
        assert rr.same_bits(late[0][k], each[0][k]), k
    for a, b in zip(late[1]["dedup"] + late[1]["cells"] + tuple(late[1]["kept"]), each[1]["dedup"] + each[1]["cells"] + tuple(each[1]["kept"])):
        assert rr.same_bits(a, b)
    assert np.array_equal(late[2], each[2]) and late[3] == each[3]


# ---- (d) refusals, and a diagnostic that runs kernels again -----------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["direct", "match_table"])
def test_add_last_refuses_a_flat_batch_call_on_every_route(route):
    """a flat batch call leaves rows and no records, whatever route made the rows: Dedup and Cells refuse it and stay empty, an
    Assign that holds records refuses it and stays as it was; all three take a bundle call afterwards.  An Assign without adds
    takes the flat call by design (assign.cpp, br_assign_add_last: it becomes an object of values only)"""
    inp = rr.BY_ID["pairs-default"]
    annd, recs, ref_map = inp.data()
    flat = rc.BY_ID["plain-default"]
    assert flat.data()[0] == annd           # the same annotation: one index serves both calls
    idx = lib.Index(annd, device=0)
    ctx_flat, ctx = rc.new_context(idx, route), lib.Context(idx)
    cfg = lib.make_config()
    few = rr.cut(list(recs), (300, 1))[0]
    d, c, a, fresh = lib.Dedup(keep_records=1), lib.Cells(), lib.Assign(), lib.Assign()
    empty = fresh.stats()["held_bytes"]
    try:
        took, db = rc.run_route(ctx_flat, route, cfg, flat.data()[1])
        assert took == route
        rr.project(ctx, cfg, few, ref_map)
        a.add_last(ctx)
        held = a.stats()["held_bytes"]
        assert d._raw("add_last", ctx_flat.h) == rr.INVALID and c._raw("add_last", ctx_flat.h) == rr.INVALID and a._raw("add_last", ctx_flat.h) == rr.INVALID
        assert d.stats()["names"] == 0 and c.stats()["names"] == 0 and a.stats()["held_bytes"] == held
        for o in (d, c, a):
            o.add_last(ctx)
        n = len(rr.group_off_of(few)) - 1
        assert d.stats()["names"] == n and c.stats()["names"] == n and a.stats()["held_bytes"] > held
        assert d.finish()[0] == n
        # the other side of it: an Assign without adds takes the flat call, as an object of values only, and from then on takes
        # the rows and names of a bundle call without its records
        assert fresh._raw("add_last", ctx_flat.h) == 0 and fresh.stats()["held_bytes"] > empty
        assert fresh._raw("set_param", b"mode", 1) == rr.INVALID      # (it holds an add now)
        rows_only = fresh.stats()["held_bytes"]
        fresh.add_last(ctx)
        assert fresh.stats()["held_bytes"] > rows_only
        del db
    finally:
        for o in (d, c, a, fresh, ctx_flat, ctx, idx):
            o.close()


@pytest.mark.parametrize("how", ["bundle", "resident"])
def test_an_empty_bundle_leaves_nothing_behind(how):
    """a bundle without records is a call like any other: after it the context has no last table and no last records, so add_last
    adds nothing and br_ctx_last_device_bam (what --sort takes every bundle from) is empty -- not the bundle before it once more"""
    inp = rr.BY_ID["pairs-default"]
    annd, recs, ref_map = inp.data()
    few = rr.cut(list(recs), (300, 1))[0]
    n = len(rr.group_off_of(few)) - 1
    idx = lib.Index(annd, device=0)
    ctx = lib.Context(idx)
    cfg = lib.make_config()
    d, c, a, q = lib.Dedup(keep_records=1), lib.Cells(), lib.Assign(), lib.Quant(idx.num_transcripts(), inp.want().lens)
    try:
        rr.project(ctx, cfg, few, ref_map)
        for o in (d, c, a, q):
            o.add_last(ctx)
        held = a.stats()["held_bytes"]
        assert d.stats()["names"] == c.stats()["names"] == n
        if how == "bundle":
            out, _ = rr.project(ctx, cfg, [], ref_map)
            assert out.size == 0
        else:
            db, cnt = ctx.project_bam_resident_kept(cfg, lib.BrDeviceRecords(), ref_map)
            assert cnt["n_rows"] == 0 and cnt["total_processed"] == 0
        last = lib.BrDeviceBam()
        L = lib.lib()
        L.br_ctx_last_device_bam.argtypes = [C.c_void_p, C.POINTER(lib.BrDeviceBam)]
        assert L.br_ctx_last_device_bam(ctx.h, C.byref(last)) == 0 and (int(last.n_rows), int(last.n_bytes)) == (0, 0)
        for o in (d, c, a, q):
            o.add_last(ctx)
        assert d.stats()["names"] == c.stats()["names"] == n and a.stats()["held_bytes"] == held
        assert d.finish()[0] == n and q.finish()[0] == n
    finally:
        for o in (d, c, a, q, ctx, idx):
            o.close()


def test_add_last_after_rows_detail_of_a_direct_rows_bundle():
    """br_device_rows_detail runs the emit kernels once more over a direct-rows call's tables; add_last after it reads the rows
    and records the call left"""
    inp = rr.BY_ID["pairs-default"]
    annd, recs, ref_map = inp.data()
    want = inp.want()
    idx = lib.Index(annd, device=0)
    ctx = rc.new_context(idx, "direct")
    cons = rr.Consumers(want.lens, inp.long_reads)
    try:
        route, out, _ = rr.run_route(ctx, "direct", lib.make_config(**inp.flags), list(recs), ref_map)
        assert route == "direct" and np.array_equal(out, want.stream)
        assert ctx.rows_detail()
        cons.add_last(ctx)
        floats = cons.check(want, "after br_device_rows_detail")
    finally:
        cons.close()
        ctx.close()
        idx.close()
    _assert_same_floats(inp.id, "direct after rows_detail", floats)
