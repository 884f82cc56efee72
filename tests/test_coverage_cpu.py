"""--coverage without a GPU: the tests' own restatement of the coverage definitions in bramble_amd.h (br_coverage: counted row, covered
bases, depth, per transcript, run), which the GPU tests compare the device against; that yardstick against cases worked out by hand;
what the synthetic inputs hold; the new ABI without a device; the command line's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_quant_fld_cpu import ROW_FIRST, ROW_MINUS, ROW_PAIRED, ROW_PRIMARY, rows_of, wide_rows

COVER_OPS = (0, 7, 8)   # M = X cover and advance
SKIP_OPS = (2, 3)       # D N advance


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def intervals_of(pos, words):
    """the covered intervals [s, e) of one row, unclamped, adjacent ones merged (Python integers: no width to overflow)"""
    p, out = int(pos), []
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op in COVER_OPS:
            if n:
                if out and out[-1][1] == p:
                    out[-1][1] = p + n
                else:
                    out.append([p, p + n])
            p += n
        elif op in SKIP_OPS:
            p += n
    return out


def coverage_of(rows, lens, primary_only=False):
    """rows: tid, pos, meta per row and the rewritten CIGARs as cigar_off / cigar (tests.test_quant_fld_cpu.rows_of); lens: one
    length per transcript.  -> dict: depth (a uint32 array per transcript), runs (tid, start, end, depth: uint32 arrays), records /
    aligned_bases / covered_bases (uint64) and max_depth (uint32) per transcript, rows_counted, rows_skipped, clipped_bases, bad_tid
    (a row named a transcript that does not exist: it is skipped), n_intervals (clamped, non-empty)"""
    n_tx = len(lens)
    own = [max(int(v), 0) for v in lens]
    diff = [np.zeros(n + 1, dtype=np.int64) for n in own]
    records = np.zeros(n_tx, dtype=np.uint64)
    counted = skipped = clipped = n_intervals = 0
    bad_tid = False
    off, cig = rows["cigar_off"], rows["cigar"]
    for r in range(len(rows["tid"])):
        t, meta = int(rows["tid"][r]), int(rows["meta"][r])
        if primary_only and not meta & ROW_PRIMARY:
            skipped += 1
            continue
        if t >= n_tx:
            skipped += 1
            bad_tid = True
            continue
        counted += 1
        records[t] += 1
        for s, e in intervals_of(rows["pos"][r], cig[int(off[r]):int(off[r + 1])]):
            cs, ce = min(s, own[t]), min(e, own[t])
            clipped += (e - s) - (ce - cs)
            if ce > cs:
                diff[t][cs] += 1
                diff[t][ce] -= 1
                n_intervals += 1
    depth = [np.cumsum(d[:-1]).astype(np.uint32) for d in diff]
    runs = [[], [], [], []]
    for t, d in enumerate(depth):
        if not len(d):
            continue
        edge = np.flatnonzero(np.diff(d.astype(np.int64))) + 1          # where the depth changes inside the transcript
        starts = np.concatenate([[0], edge])
        ends = np.concatenate([edge, [len(d)]])
        keep = d[starts] > 0
        for col, v in zip(runs, (np.full(int(keep.sum()), t), starts[keep], ends[keep], d[starts][keep])):
            col.append(np.asarray(v, dtype=np.uint32))
    runs = tuple(np.concatenate(c) if c else np.zeros(0, dtype=np.uint32) for c in runs)
    return {"depth": depth, "runs": runs, "records": records,
            "aligned_bases": np.asarray([int(d.sum(dtype=np.uint64)) for d in depth], dtype=np.uint64),
            "covered_bases": np.asarray([int(np.count_nonzero(d)) for d in depth], dtype=np.uint64),
            "max_depth": np.asarray([int(d.max()) if len(d) else 0 for d in depth], dtype=np.uint32),
            "rows_counted": counted, "rows_skipped": skipped, "clipped_bases": clipped, "bad_tid": bad_tid, "n_intervals": n_intervals}


def run_list(cov):
    return [tuple(int(v) for v in r) for r in zip(*cov["runs"])]


# ---- the yardstick against cases worked out by hand ------------------------------------------------------------------------------
def test_cigar_walk_by_hand():
    # 3S10M2D5M from 100: the clip does not move, [100, 110), the deletion leaves 110 and 111 open, [112, 117)
    cov = coverage_of(rows_of([(0, 100, 0, "3S10M2D5M")]), [1000])
    assert run_list(cov) == [(0, 100, 110, 1), (0, 112, 117, 1)]
    assert cov["depth"][0][99:118].tolist() == [0] + [1] * 10 + [0, 0] + [1] * 5 + [0]
    assert (int(cov["aligned_bases"][0]), int(cov["covered_bases"][0]), int(cov["max_depth"][0]), int(cov["records"][0])) == (15, 15, 1, 1)
    # 5M100N5M from 0: [0, 5) and [105, 110)
    assert run_list(coverage_of(rows_of([(0, 0, 0, "5M100N5M")]), [200])) == [(0, 0, 5, 1), (0, 105, 110, 1)]
    # 4=1X: = and X cover like M, and the two ops touch: one run of 5
    assert run_list(coverage_of(rows_of([(0, 7, 0, "4=1X")]), [50])) == [(0, 7, 12, 1)]
    # I, P and H do not move: 2H5M3I2P5M covers [20, 30) in one piece, with nothing lost
    cov = coverage_of(rows_of([(0, 20, 0, "2H5M3I2P5M4H")]), [50])
    assert run_list(cov) == [(0, 20, 30, 1)] and cov["n_intervals"] == 1 and cov["clipped_bases"] == 0
    # no ops at all, and ops that cover nothing: a counted row without a base
    cov = coverage_of(rows_of([(0, 5, 0, []), (0, 5, 0, "4S"), (0, 5, 0, "3D")]), [50])
    assert run_list(cov) == [] and cov["rows_counted"] == 3 and int(cov["records"][0]) == 3 and cov["clipped_bases"] == 0


def test_pairs_and_primaries_by_hand():
    # two mates, [10, 30) and [20, 40): the ten bases they share are counted twice
    pair = [(0, 10, ROW_PAIRED | ROW_FIRST | ROW_PRIMARY, "20M"), (0, 20, ROW_PAIRED | ROW_MINUS | ROW_PRIMARY, "20M")]
    cov = coverage_of(rows_of(pair), [100])
    assert run_list(cov) == [(0, 10, 20, 1), (0, 20, 30, 2), (0, 30, 40, 1)]
    assert (int(cov["aligned_bases"][0]), int(cov["covered_bases"][0]), int(cov["max_depth"][0])) == (40, 30, 2)
    # a secondary record counts by default and is skipped under primary_only
    rows = rows_of(pair + [(1, 0, ROW_FIRST, "10M")])
    cov = coverage_of(rows, [100, 100])
    assert cov["rows_counted"] == 3 and cov["rows_skipped"] == 0 and cov["records"].tolist() == [2, 1]
    cov = coverage_of(rows, [100, 100], primary_only=True)
    assert cov["rows_counted"] == 2 and cov["rows_skipped"] == 1 and cov["records"].tolist() == [2, 0]
    assert run_list(cov) == [(0, 10, 20, 1), (0, 20, 30, 2), (0, 30, 40, 1)]


def test_clamping_by_hand():
    # L = 25: [20, 30) keeps [20, 25) and loses 5; [30, 40) lies wholly past the end and loses 10, yet the row is a record;
    # [15, 25) ends exactly at L and [25, 26) starts there
    rows = rows_of([(0, 20, 0, "10M"), (0, 30, 0, "10M"), (0, 15, 0, "10M"), (0, 25, 0, "1M")])
    cov = coverage_of(rows, [25])
    assert run_list(cov) == [(0, 15, 20, 1), (0, 20, 25, 2)]
    assert cov["clipped_bases"] == 5 + 10 + 0 + 1 and cov["rows_counted"] == 4 and int(cov["records"][0]) == 4
    assert len(cov["depth"][0]) == 25
    # L = 0 and L = -1 own no base: everything on them is lost, the records count; the neighbours are untouched
    rows = rows_of([(0, 0, 0, "10M"), (1, 0, 0, "10M"), (2, 3, 0, "4M2D4M"), (3, 0, 0, "10M")])
    cov = coverage_of(rows, [10, 0, -1, 10])
    assert run_list(cov) == [(0, 0, 10, 1), (3, 0, 10, 1)]
    assert cov["clipped_bases"] == 10 + 8 and cov["records"].tolist() == [1, 1, 1, 1]
    assert [len(d) for d in cov["depth"]] == [10, 0, 0, 10]
    assert cov["covered_bases"].tolist() == [10, 0, 0, 10] and cov["max_depth"].tolist() == [1, 0, 0, 1]
    # the walk is not 32-bit: from 2^32 - 10 a 100M passes 2^32 and all of it is lost on a short transcript
    cov = coverage_of(rows_of([(0, 2 ** 32 - 10, 0, "100M")]), [1000])
    assert cov["clipped_bases"] == 100 and run_list(cov) == []


def test_runs_stop_at_transcript_boundaries():
    # two neighbours covered end to end at depth 1: two runs, not one of 20
    cov = coverage_of(rows_of([(0, 0, 0, "10M"), (1, 0, 0, "10M")]), [10, 10])
    assert run_list(cov) == [(0, 0, 10, 1), (1, 0, 10, 1)]
    # a transcript id past the table is skipped and flagged
    cov = coverage_of(rows_of([(0, 0, 0, "10M"), (2, 0, 0, "10M")]), [10, 10])
    assert cov["bad_tid"] and cov["rows_skipped"] == 1 and run_list(cov) == [(0, 0, 10, 1)]


# ---- what the synthetic inputs hold ------------------------------------------------------------------------------------------------
def _holds(mode):
    tb, rows = wide_rows(mode)
    cov = coverage_of(rows, tb["lens"])
    ops = sorted(set(int(w) & 15 for w in rows["cigar"]))
    changes = sum(int(np.count_nonzero(np.diff(d.astype(np.int64)))) for d in cov["depth"])
    return {"rows": len(rows["tid"]), "transcripts": int(tb["n_tx"]), "bases": int(sum(max(int(v), 0) for v in tb["lens"])),
            "intervals": cov["n_intervals"], "max_depth": int(cov["max_depth"].max()), "covered": int(cov["covered_bases"].sum()),
            "changes": changes, "primary": int(np.count_nonzero(rows["meta"] & ROW_PRIMARY)), "clipped": cov["clipped_bases"],
            "cover_ops": int(np.count_nonzero(np.isin(rows["cigar"] & 15, COVER_OPS) & (rows["cigar"] >> 4 > 0))),
            "ops": "".join("MIDNSHP=X"[o] for o in ops), "max_ops": int(np.diff(rows["cigar_off"].astype(np.int64)).max())}


def test_inputs_hold_what_the_feature_is_about():
    pe, ont = _holds("pe"), _holds("ont")
    print("pe: %s\nont: %s" % (pe, ont))
    for h in (pe, ont):   # the coarse versions of what was measured when the feature was built
        assert h["max_depth"] >= 8 and h["changes"] >= 10000 and 0 < h["primary"] < h["rows"] / 2
        assert h["clipped"] == 0 and h["ops"] == "MIDS" and h["intervals"] >= h["rows"]
    assert (pe["rows"], pe["transcripts"], pe["bases"]) == (27007, 2181, 3592347)
    assert (ont["rows"], ont["transcripts"], ont["bases"]) == (3559, 1310, 2188326)
    assert (pe["max_depth"], pe["covered"], pe["primary"]) == (32, 1384268, 4804) and (ont["max_depth"], ont["primary"]) == (12, 799)
    assert (pe["cover_ops"], ont["cover_ops"]) == (27316, 33024)   # (before touching ops are merged: "intervals" is after)
    assert ont["max_ops"] > 64   # pooled CIGARs long enough for the wave's walk


# ---- ABI and usage errors -------------------------------------------------------------------------------------------------------
SYMBOLS = ("br_coverage_new", "br_coverage_set_param", "br_coverage_add_rows", "br_coverage_add_last", "br_coverage_finish",
           "br_coverage_runs", "br_coverage_depth", "br_coverage_summary", "br_coverage_stats", "br_coverage_free")


def test_new_symbols_without_a_device():
    """BR_ERR_NO_DEVICE for a device that does not exist (every device, on a machine without one)."""
    from bramble_amd import lib
    L = lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    L.br_coverage_new.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]
    lens = np.asarray([100, 0, 2 ** 32 - 1], dtype=np.int64)
    h = C.c_void_p()
    assert L.br_coverage_new(4096, 3, lens.ctypes.data, C.byref(h)) == -2 and not h.value   # BR_ERR_NO_DEVICE
    lens[2] = 2 ** 32
    assert L.br_coverage_new(4096, 3, lens.ctypes.data, C.byref(h)) == -1 and not h.value   # a length above 2^32 - 1
    assert L.br_coverage_new(4096, -1, None, C.byref(h)) == -1 and L.br_coverage_new(4096, 3, lens.ctypes.data, None) == -1
    L.br_coverage_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.br_coverage_add_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    L.br_coverage_add_last.argtypes = [C.c_void_p, C.c_void_p]
    L.br_coverage_finish.argtypes = [C.c_void_p, C.c_void_p]
    L.br_coverage_runs.argtypes = [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4
    L.br_coverage_depth.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.br_coverage_summary.argtypes = [C.c_void_p] * 5
    L.br_coverage_stats.argtypes = [C.c_void_p] * 8
    L.br_coverage_free.argtypes = [C.c_void_p]
    rows = lib.BrDeviceRows()
    assert L.br_coverage_set_param(None, b"primary_only", 1) == -1                       # BR_ERR_INVALID_ARG without an object
    assert L.br_coverage_add_rows(None, C.byref(rows), 0, 0, 0, None) == -1 and L.br_coverage_add_last(None, None) == -1
    assert L.br_coverage_finish(None, None) == -1 and L.br_coverage_runs(None, 0, 0, None, None, None, None) == -1
    assert L.br_coverage_depth(None, 0, None) == -1 and L.br_coverage_summary(None, None, None, None, None) == -1
    assert L.br_coverage_stats(None, None, None, None, None, None, None, None) == -1
    L.br_coverage_free(None)
    for name in ("add_rows_host", "add_rows_device", "add_last", "finish", "runs", "depth", "summary", "stats", "close"):
        assert hasattr(lib.Coverage, name), name


@pytest.mark.parametrize("extra", [
    ["--coverage-primary"],
    ["--coverage-primary", "--quant", "q.tsv"],
    ["--coverage", "c.bedgraph", "--devices", "0,1"],
    ["--coverage-summary", "c.tsv", "--devices", "0,1"],
    ["--coverage"],
])
def test_cli_usage_errors(tmp_path, extra):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    extra = [str(tmp_path / e) if e.endswith((".tsv", ".bedgraph")) else e for e in extra]
    r = subprocess.run([os.path.join(root, "bramble_amd", "bin", "bramble"), str(tmp_path / "missing.bam"), "-G", str(gtf), "-o",
                        str(tmp_path / "o.bam")] + extra, capture_output=True, timeout=60)
    assert r.returncode == 2
    assert b"--coverage" in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]
