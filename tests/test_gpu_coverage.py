"""--coverage on the GPU: br_coverage's runs, summary, counters and depth against the tests' restatement of the definitions
(test_coverage_cpu.py) on the oracle's rows of the synthetic inputs -- fed from the host, from HBM and from a context's last
projection call -- and on hand-built tables for what those inputs do not hold; paging; the errors; and the command line with the
switches against the run without them."""
import functools
import os

import numpy as np
import pytest

from bramble_amd import lib, synth
from tests import bamio
from tests.test_coverage_cpu import coverage_of
from tests.test_gpu_collate import _files, _inputs, _report, _run
from tests.test_gpu_quant import _body, _fill
from tests.test_quant_fld_cpu import ROW_FIRST, ROW_PRIMARY, packed_of, rows_of, wide_rows

pytestmark = pytest.mark.gpu

COUNTERS = ("rows_counted", "rows_skipped", "clipped_bases")
SUMMARY = ("records", "aligned_bases", "covered_bases", "max_depth")


@functools.lru_cache(maxsize=None)
def _tables(mode):
    """(oracle_tables, the oracle's rows as packed device rows, the yardstick without and with primary_only)"""
    tb, rows = wide_rows(mode)
    return tb, packed_of(rows), (coverage_of(rows, tb["lens"], False), coverage_of(rows, tb["lens"], True))


def _cuts(n_rows, calls):
    return [0, n_rows] if calls == 1 else [0, n_rows // 3, n_rows // 3 + 1, n_rows]   # (a call of one row among them)


def _fill_rows(c, pk, how):
    """the whole row table into `c`: from host memory or from HBM, in 1 or 3 calls"""
    import torch
    a, ref, pool = pk
    cuts = _cuts(len(a), 3 if how.endswith("3") else 1)
    if how.startswith("host"):
        for r0, r1 in zip(cuts, cuts[1:]):
            c.add_rows_host(a, ref, pool, r0, r1)
        return
    d_a = torch.from_numpy(a.view(np.int32)).cuda()
    d_ref = torch.from_numpy(ref.view(np.int64)).cuda()
    d_pool = torch.from_numpy(pool.view(np.int32)).cuda()
    for r0, r1 in zip(cuts, cuts[1:]):
        c.add_rows_device(d_a, d_ref, d_pool, r0, r1)


def _assert_coverage(c, want, lens, depth_of, tag=""):
    """a finished Coverage against the yardstick: runs, summary, counters, and the depth of the transcripts `depth_of`"""
    got = c.runs()
    assert c.n_runs == len(want["runs"][0]), tag
    for g, w, name in zip(got, want["runs"], ("tid", "start", "end", "depth")):
        assert g.dtype == np.uint32 and np.array_equal(g, w), (tag, name)
    s = c.summary()
    for k in SUMMARY:
        assert s[k].dtype == want[k].dtype and np.array_equal(s[k], want[k]), (tag, k)
    st = c.stats()
    assert {k: st[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}, tag
    assert st["peak_bytes"] >= st["held_bytes"] > 0
    for t in depth_of:
        d = c.depth(t)
        assert len(d) == max(int(lens[t]), 0) and np.array_equal(d, want["depth"][t]), (tag, t)
    return st


# ---- the synthetic inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("primary_only", [0, 1])
@pytest.mark.parametrize("how", ["host", "host3", "dev1", "dev3", "last_batch", "last_resident"])
def test_coverage_matches_the_yardstick(mode, how, primary_only):
    tb, pk, wants = _tables(mode)
    want = wants[primary_only]
    c = lib.Coverage(tb["lens"])
    if primary_only:
        c.set_param("primary_only", 1)
    if how.startswith("last"):
        _fill(c, tb, how)   # (br_coverage_add_last takes all rows of the context's last call)
    else:
        _fill_rows(c, pk, how)
    c.finish()
    deepest = int(np.argmax(want["max_depth"]))
    busiest = int(np.argmax(want["records"]))
    some = sorted({deepest, busiest, 0, tb["n_tx"] // 2, tb["n_tx"] - 1, int(np.argmax(tb["lens"])), int(np.argmin(tb["lens"]))})
    _assert_coverage(c, want, tb["lens"], some, "%s %s %d" % (mode, how, primary_only))
    assert want["max_depth"].max() >= (2 if primary_only else 8) and c.n_runs >= 1000
    c.close()


# ---- a hand-built table ------------------------------------------------------------------------------------------------------------
N_BULK = 100000
T_WIDE, T_INLINE, T_EDGE, T_NONE, T_NEG, T_FULL_A, T_FULL_B, T_LONG, T_BULK, T_GAP, T_LAST = range(11)
HAND_LENS = np.asarray([1000, 50, 100, 0, -1, 20, 20, 70000, 500, -5, 30], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _hand_built():
    """What the synthetic inputs do not hold: pooled CIGARs of 3, 64, 65 and 300 ops over all nine op codes; inline CIGARs of 0, 1
    and 2 ops; intervals that end exactly at L, start at L and straddle L, and a long M from a position near 2^32; transcripts
    without bases between covered ones; two neighbours covered end to end at depth 1; a 70 000-base transcript under one 70000M row
    with shorter rows on top (a carry through many scan tiles); N_BULK identical rows on one spot (a depth above 65 535); and a
    last transcript whose last base is covered (the word behind the last base).  About a third of the rows are primary.
    -> (rows, the yardstick without and with primary_only)"""
    rng = np.random.RandomState(5)

    def wide(n):   # n ops, every op code 0 .. 8 in turn, 1 .. 3 bases each
        return [((1 + int(rng.randint(3))) << 4) | (k % 9) for k in range(n)]
    items = []
    for n in (3, 64, 65, 300):
        items += [(T_WIDE, 5, wide(n)), (T_WIDE, 400 + n, wide(n)), (T_LONG, 4000 + n, wide(n))]
    items += [(T_WIDE, 990, wide(300)), (T_LAST, 0, wide(65))]                        # long CIGARs that run past the end
    items += [(T_INLINE, 5, []), (T_INLINE, 5, "10M"), (T_INLINE, 0, "5M3D"), (T_INLINE, 2, "4S6M"), (T_INLINE, 9, "7=8X"), (T_INLINE, 30, "2I"),
              (T_INLINE, 31, "3N4M"), (T_INLINE, 49, "1M"), (T_INLINE, 0, "50M")]
    items += [(T_EDGE, 90, "10M"), (T_EDGE, 100, "5M"), (T_EDGE, 95, "10M"), (T_EDGE, 2 ** 32 - 5, [((2 ** 28 - 1) << 4) | 0]),
              (T_EDGE, 2 ** 32 - 1, "3M200N5M"), (T_EDGE, 50, "20M100D20M"), (T_EDGE, 99, wide(65))]
    items += [(T_NONE, 0, "10M"), (T_NEG, 2, "3M"), (T_GAP, 0, wide(70)), (T_NONE, 7, "5M2D5M")]
    items += [(T_FULL_A, 0, "20M"), (T_FULL_B, 0, "20M")]
    items += [(T_LONG, 0, "70000M")]
    for _ in range(300):                                                              # short rows all along it, tile edges among them
        p = int(rng.choice([int(rng.randint(70000)), 4096 * int(rng.randint(1, 17)) - int(rng.randint(30))]))
        items.append((T_LONG, p, "%dM%dD%dM" % (1 + rng.randint(40), 1 + rng.randint(5), 1 + rng.randint(40))))
    items += [(T_LAST, 20, "10M"), (T_LAST, 25, "5M")]
    items = [(t, p, (ROW_PRIMARY if rng.randint(3) == 0 else 0) | ROW_FIRST, c) for t, p, c in items]
    order = rng.permutation(len(items))
    items = [items[i] for i in order[:len(items) // 2]] + [(T_BULK, 100, ROW_PRIMARY if j % 2 else 0, "12M") for j in range(N_BULK)] \
        + [items[i] for i in order[len(items) // 2:]]
    rows = rows_of(items)
    return rows, (coverage_of(rows, HAND_LENS, False), coverage_of(rows, HAND_LENS, True))


def test_hand_built_table_holds_its_cases():
    rows, (want, want_p) = _hand_built()
    runs = list(zip(*[v.tolist() for v in want["runs"]]))
    assert sorted(set(int(w) & 15 for w in rows["cigar"])) == list(range(9))
    assert {3, 64, 65, 300} <= set(np.diff(rows["cigar_off"].astype(np.int64)).tolist())
    assert want["clipped_bases"] > 2 ** 28 and want["records"][[T_NONE, T_NEG, T_GAP]].tolist() == [2, 1, 1]
    assert (T_FULL_A, 0, 20, 1) in runs and (T_FULL_B, 0, 20, 1) in runs
    assert int(want["max_depth"][T_BULK]) == N_BULK > 65535 and (T_BULK, 100, 112, N_BULK) in runs
    assert int(want["covered_bases"][T_LONG]) == 70000 and want["depth"][T_LONG].min() >= 1 and want["max_depth"][T_LONG] >= 3
    assert runs[-1][0] == T_LAST and runs[-1][2] == 30 and want["depth"][T_LAST][-1] >= 2
    assert want["depth"][T_EDGE][99] >= 2 and want["depth"][T_EDGE][89] < want["depth"][T_EDGE][90]
    assert 0 < want_p["rows_counted"] < want["rows_counted"] and want_p["rows_skipped"] > N_BULK // 2 - 1
    assert int(want_p["max_depth"][T_BULK]) == N_BULK // 2


@pytest.mark.parametrize("primary_only", [0, 1])
@pytest.mark.parametrize("how", ["host", "dev3"])
def test_hand_built_table(how, primary_only):
    rows, wants = _hand_built()
    c = lib.Coverage(HAND_LENS)
    c.set_param("primary_only", primary_only)
    _fill_rows(c, packed_of(rows), how)
    c.finish()
    _assert_coverage(c, wants[primary_only], HAND_LENS, range(len(HAND_LENS)), how)
    c.close()


def test_held_bytes_follow_the_device_memory_account():
    """coverage.cpp's "Device memory" account, to the byte: what new makes; a host add's uploads (24 bytes a row and 4 a pool word,
    one entry more each) are in the peak and gone from the held bytes when the add returns; what finish leaves"""
    rows, _ = _hand_built()
    a, ref, pool = packed_of(rows)
    T, B = len(HAND_LENS), int(np.maximum(HAND_LENS, 0).sum())
    from_new = 4 * (B + 1) + 16 * (T + 1) + 64
    c = lib.Coverage(HAND_LENS)
    assert c.stats()["held_bytes"] == from_new
    c.add_rows_host(a, ref, pool)
    st = c.stats()
    assert st["held_bytes"] == from_new and st["peak_bytes"] == from_new + 24 * (len(a) + 1) + 4 * (len(pool) + 1)
    n_runs = c.finish()
    assert n_runs > 300 and c.stats()["held_bytes"] == from_new + 20 * (T + 1) + 16 * (n_runs + 1)
    c.close()


def test_a_depth_carried_through_more_tiles_than_one_scan_block_takes():
    """4 300 000 bases are 1 050 tiles of 4 096: a depth carried from tile to tile of k_cov_tile_apply, through more tiles than one
    block has threads.  The 1 050 tile sums are one tile of launch_scan, scanned by one block in one launch; the tiled top
    level of the scan (more than 4 194 304 items) is test_gpu_scan_unit.py::test_launch_scan_from_u32's."""
    lens = np.asarray([4300000, 7], dtype=np.int64)
    rows = rows_of([(0, 0, 0, "4300000M"), (0, 4299000, 0, "1000M"), (0, 1, 0, "4194303M"), (1, 0, 0, "7M")])
    want = coverage_of(rows, lens)
    assert [tuple(int(v[k]) for v in want["runs"]) for k in range(len(want["runs"][0]))] == [
        (0, 0, 1, 1), (0, 1, 4194304, 2), (0, 4194304, 4299000, 1), (0, 4299000, 4300000, 2), (1, 0, 7, 1)]
    c = lib.Coverage(lens)
    _fill_rows(c, packed_of(rows), "host")
    c.finish()
    _assert_coverage(c, want, lens, [0, 1])
    c.close()


def test_no_rows_and_no_bases():
    empty = packed_of(rows_of([]))
    for fill in (False, True):   # nothing added at all; an add of no rows
        c = lib.Coverage(HAND_LENS)
        if fill:
            c.add_rows_host(*empty)
        assert c.finish() == 0
        _assert_coverage(c, coverage_of(rows_of([]), HAND_LENS), HAND_LENS, range(len(HAND_LENS)))
        c.close()
    # B = 0: every base of every row is clipped, the records count
    lens = np.asarray([0, -3, 0], dtype=np.int64)
    rows = rows_of([(0, 0, 0, "10M"), (2, 5, 0, "3M2D3M"), (2, 0, 0, []), (1, 0, 0, [(4 << 4) | (k % 9) for k in range(70)])])
    want = coverage_of(rows, lens)
    assert want["clipped_bases"] == 10 + 6 + 4 * 22 and want["records"].tolist() == [1, 1, 2]
    for how in ("host", "dev1"):
        c = lib.Coverage(lens)
        _fill_rows(c, packed_of(rows), how)
        assert c.finish() == 0
        _assert_coverage(c, want, lens, [0, 1, 2], how)
        c.close()
    # one base, and no transcript at all
    c = lib.Coverage([1])
    c.add_rows_host(*packed_of(rows_of([(0, 0, 0, "1M"), (0, 0, 0, "5M")])))
    assert c.finish() == 1
    assert [v.tolist() for v in c.runs()] == [[0], [0], [1], [2]] and c.stats()["clipped_bases"] == 4
    c.close()
    c = lib.Coverage([])
    assert c.finish() == 0 and c.summary()["records"].size == 0
    c.close()


# ---- paging ------------------------------------------------------------------------------------------------------------------------
def test_runs_in_pages():
    L = lib.lib()
    rows, wants = _hand_built()
    c = lib.Coverage(HAND_LENS)
    _fill_rows(c, packed_of(rows), "dev1")
    n = c.finish()
    assert n == len(wants[0]["runs"][0]) and n > 300
    whole = c.runs()
    for page in (1, 1000, 7):
        for g, w in zip(c.runs(page=page), whole):
            assert np.array_equal(g, w), page
    # a page may leave columns out; pages outside [0, n_runs] are refused
    end = np.zeros(3, dtype=np.uint32)
    assert L.br_coverage_runs(c.h, n - 3, 3, None, None, end.ctypes.data, None) == 0 and np.array_equal(end, whole[2][-3:])
    assert L.br_coverage_runs(c.h, n, 0, None, None, None, None) == 0
    for first, count in ((-1, 1), (0, n + 1), (n, 1), (n + 1, 0), (1, n), (0, -1), (2 ** 62, 2 ** 62)):
        assert L.br_coverage_runs(c.h, first, count, None, None, end.ctypes.data, None) == -1, (first, count)
    assert L.br_coverage_depth(c.h, -1, None) == -1 and L.br_coverage_depth(c.h, len(HAND_LENS), None) == -1
    assert L.br_coverage_depth(c.h, T_NONE, None) == 0
    c.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------
def _refuses_everything(c):
    L = lib.lib()
    out = np.zeros(4096, dtype=np.uint64)
    n = lib.C.c_int64()
    assert L.br_coverage_set_param(c.h, b"primary_only", 0) == -1
    assert c.add_rows_raw(None, None, None, 0, 0, 0, 0, False) == -1
    assert L.br_coverage_finish(c.h, lib.C.byref(n)) == -1
    assert L.br_coverage_runs(c.h, 0, 0, None, None, None, None) == -1
    assert L.br_coverage_depth(c.h, 0, out.ctypes.data) == -1
    assert L.br_coverage_summary(c.h, out.ctypes.data, None, None, None) == -1
    assert L.br_coverage_stats(c.h, None, None, None, None, None, None, None) == -1


def test_errors():
    import torch
    L = lib.lib()
    rows, wants = _hand_built()
    a, ref, pool = packed_of(rows)
    # a transcript id past the table: the row is skipped, nothing faults, finish refuses
    for how in ("host", "dev1"):
        c = lib.Coverage(HAND_LENS[:T_LAST])
        _fill_rows(c, (a, ref, pool), how)
        assert L.br_coverage_finish(c.h, None) == -1
        c.close()
    bad_a = a.copy()
    bad_a[5, 0] = 0xffffffff
    c = lib.Coverage(HAND_LENS)
    c.add_rows_host(bad_a, ref, pool)
    assert L.br_coverage_finish(c.h, None) == -1
    c.close()
    # a pooled reference that leaves the pool -- a lane's CIGAR and a wave's -- and a row range past n_rows: the add is refused,
    # and everything after it
    small = int(np.flatnonzero((a[:, 2] & 0xffffff) == 64)[0])
    big = int(np.flatnonzero((a[:, 2] & 0xffffff) == 300)[0])
    for row, off in ((small, len(pool) - 63), (small, 1 << 40), (big, len(pool) - 299), (big, len(pool) + 1), (big, 2 ** 64 - 100)):
        bad = ref.copy()
        bad[row] = off
        c = lib.Coverage(HAND_LENS)
        assert c.add_rows_raw(a.ctypes.data, bad.ctypes.data, pool.ctypes.data, len(a), len(pool), 0, len(a), False) == -1, (row, off)
        _refuses_everything(c)
        c.close()
        d = [torch.from_numpy(x).cuda() for x in (a.view(np.int32), bad.view(np.int64), pool.view(np.int32))]
        c = lib.Coverage(HAND_LENS)
        assert c.add_rows_raw(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(a), len(pool), 0, len(a), True,
                              torch.cuda.current_stream().cuda_stream) == -1, (row, off)
        _refuses_everything(c)
        c.close()
    for r0, r1 in ((0, len(a) + 1), (-1, 5), (7, 6)):
        c = lib.Coverage(HAND_LENS)
        assert c.add_rows_raw(a.ctypes.data, ref.ctypes.data, pool.ctypes.data, len(a), len(pool), r0, r1, False) == -1
        _refuses_everything(c)
        c.close()
    # the order of the calls
    c = lib.Coverage(HAND_LENS)
    out = np.zeros(len(HAND_LENS), dtype=np.uint64)
    assert L.br_coverage_set_param(c.h, b"primary_only", 2) == -1 and L.br_coverage_set_param(c.h, b"primary", 1) == -1
    assert L.br_coverage_set_param(c.h, b"primary_only", 1) == 0
    assert L.br_coverage_runs(c.h, 0, 0, None, None, None, None) == -1                       # before finish
    assert L.br_coverage_depth(c.h, 0, None) == -1 and L.br_coverage_summary(c.h, out.ctypes.data, None, None, None) == -1
    c.add_rows_host(a, ref, pool, 0, 10)
    assert L.br_coverage_set_param(c.h, b"primary_only", 0) == -1                            # after the first add
    c.add_rows_host(a, ref, pool, 10, len(a))
    c.finish()
    assert c.add_rows_raw(a.ctypes.data, ref.ctypes.data, pool.ctypes.data, len(a), len(pool), 0, 1, False) == -1   # after finish
    assert L.br_coverage_finish(c.h, None) == -1
    _assert_coverage(c, wants[1], HAND_LENS, [T_LONG])                                        # the refusals changed nothing
    c.close()


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _bedgraph(want, names):
    return "".join("%s\t%d\t%d\t%d\n" % (names[int(t)], s, e, d) for t, s, e, d in zip(*want["runs"]))


def _assert_summary(text, want, names, lens, tag):
    lines = text.split("\n")
    assert lines[0] == "Name\tLength\tRecords\tAlignedBases\tCoveredBases\tMaxDepth\tMeanDepth\tBreadth" and lines[-1] == "", tag
    fields = [l.split("\t") for l in lines[1:-1]]
    listed = [t for t in range(len(lens)) if lens[t] > 0]
    assert [f[0] for f in fields] == [names[t] for t in listed] and all(len(f) == 8 for f in fields), tag
    assert [int(f[1]) for f in fields] == [int(lens[t]) for t in listed], tag
    for col, key in ((2, "records"), (3, "aligned_bases"), (4, "covered_bases"), (5, "max_depth")):
        assert [int(f[col]) for f in fields] == [int(want[key][t]) for t in listed], (tag, key)
    for col, key in ((6, "aligned_bases"), (7, "covered_bases")):   # %.6f: the quotient to the print precision
        got = np.asarray([float(f[col]) for f in fields])
        assert all(len(f[col].split(".")[1]) == 6 for f in fields), tag
        assert np.all(np.abs(got - np.asarray([int(want[key][t]) / int(lens[t]) for t in listed])) <= 1e-6), (tag, key)


def test_cli_coverage(tmp_path):
    annd, _, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, hdr = _files(tmp_path, annd, stream, "in")
    sam_text = hdr.encode() + synth.records_to_sam(stream, annd["refnames"])
    tb, rows = wide_rows("pe", guide_order=True)   # (the command line numbers the transcripts in guide order)
    names = [t["id"] for t in tb["annd"]["transcripts"]]
    wants = {False: coverage_of(rows, tb["lens"], False), True: coverage_of(rows, tb["lens"], True)}
    assert len(wants[False]["runs"][0]) > 10000 and len(wants[True]["runs"][0]) > 1000

    def paths(tag):
        return [str(tmp_path / ("%s.%s" % (tag, ext))) for ext in ("out", "bedgraph", "cov.tsv")]
    plain = {}
    for key, args, stdin in (("bam", [in_bam], None), ("sort", [in_bam, "--sort"], None), ("sam", ["-"], sam_text)):
        o = paths("plain_" + key)[0]
        plain[key] = (o, _run(args + ["-G", gtf], o, stdin=stdin))
    q_tsv = str(tmp_path / "q.tsv")
    cases = (("both", "bam", [in_bam], [], False, None), ("primary", "bam", [in_bam], ["--coverage-primary"], True, None),
             ("sortquant", "sort", [in_bam, "--sort", "--quant", q_tsv], [], False, None), ("pipe", "sam", ["-"], [], False, sam_text))
    for tag, base, args, more, primary, stdin in cases:
        want = wants[primary]
        o1, bed, tsv = paths(tag)
        r1 = _run(args + ["-G", gtf, "--coverage", bed, "--coverage-summary", tsv] + more, o1, stdin=stdin)
        assert open(bed).read() == _bedgraph(want, names), tag
        _assert_summary(open(tsv).read(), want, names, tb["lens"], tag)
        # the projected output is the run's without the switches, and so is the report but for one line in front of it
        o0, r0 = plain[base]
        h0, s0 = _body(o0, False)
        h1, s1 = _body(o1, False)
        assert h0 == h1 and np.array_equal(s0, s1) and len(s0) > 100000, tag
        out0, out1 = r0.stdout.decode().split("\n"), r1.stdout.decode().split("\n")
        line = [l for l in out1 if l.startswith("[bramble] coverage: ")]
        assert len(line) == 1 and not any("coverage" in l for l in out0), tag
        assert line[0].startswith("[bramble] coverage: %d records, %d aligned bases on %d of %d bases in %d runs (add " % (
            want["rows_counted"], int(want["aligned_bases"].sum()), int(want["covered_bases"].sum()),
            int(sum(max(int(v), 0) for v in tb["lens"])), len(want["runs"][0]))), (tag, line)
        assert out1.index(line[0]) + 2 == out1.index("[bramble] final report:"), tag
        extra_lines = 1 + sum(1 for l in out1 if l.startswith("[bramble] quantified "))
        assert len(out1) == len(out0) + extra_lines and _report(r1) == _report(r0) and len(_report(r1)) == 5, tag
        for p in (o1, bed, tsv):
            assert os.path.exists(p) and not os.path.exists(p + ".tmp-bramble"), tag
    # either switch alone turns the feature on
    o, bed, tsv = paths("bed_only")
    _run([in_bam, "-G", gtf, "--coverage", bed], o)
    assert open(bed).read() == _bedgraph(wants[False], names) and not os.path.exists(tsv)
    o, bed, tsv = paths("tsv_only")
    _run([in_bam, "-G", gtf, "--coverage-summary", tsv, "-O", "sam"], o)
    _assert_summary(open(tsv).read(), wants[False], names, tb["lens"], "tsv_only")
    assert not os.path.exists(bed)
    # a --coverage path that cannot be written fails the run: no output, no temporary file
    o = str(tmp_path / "fail.out")
    r = _run([in_bam, "-G", gtf, "--coverage", str(tmp_path / "no_such_dir" / "c.bedgraph"), "--coverage-summary", str(tmp_path / "fail.tsv")], o, ok=False)
    assert r.returncode == 1 and b"c.bedgraph" in r.stderr
    assert not [p for p in os.listdir(str(tmp_path)) if p.startswith("fail")]
