"""--coverage-weight without a GPU: the tests' own restatement of the weighted-coverage definitions in bramble_amd.h (br_coverage:
weighted depth, weight nh, weight em, per transcript, run; br_quant: posterior, name classes), which the GPU tests compare the
device against; that yardstick against cases worked out on paper; what the synthetic inputs hold; the new ABI without a device; the
command line's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_coverage_cpu import intervals_of
from tests.test_quant_cpu import classes_of
from tests.test_quant_fld_cpu import ROW_FIRST, ROW_PAIRED, ROW_PRIMARY, rows_of, wide_rows

ONE = 1 << 32            # one unit of depth
NO_CLASS = 0xffffffff    # name_cls of a name without rows
SMALL_OPS = 64           # COV_SMALL_OPS: a longer CIGAR is the wave's walk, which keeps every covering op as an entry of its own


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def weight_words_nh(nh):
    """q per row for weight nh: (2^32 + nh / 2) / nh in integers; None for nh == 0 (the row is skipped)"""
    return [((ONE + int(v) // 2) // int(v)) if int(v) >= 1 else None for v in nh]


def posteriors_of(cl, theta, w):
    """cl: tests.test_quant_cpu.classes_of.  -> float64 per label entry, class after class: x_t / d_c with x_t = theta_t * w_t and
    d_c the sum of x over the class's labels in ascending order, one after the other (np.float64 scalars: one rounding an
    operation); 0 where d_c == 0"""
    theta, w = np.asarray(theta, dtype=np.float64), np.asarray(w, dtype=np.float64)
    out = []
    for s in cl["labels"]:
        d = np.float64(0.0)
        for t in s:
            d = d + theta[t] * w[t]
        for t in s:
            out.append(np.float64(0.0) if d == 0.0 else (theta[t] * w[t]) / d)
    return np.asarray(out, dtype=np.float64)


def name_classes_of(tids, row_off, group_off):
    """-> uint32 per read name: the index of its class in classes_of's order, NO_CLASS for a name without rows"""
    cl = classes_of(tids, row_off, group_off)
    index = {s: c for c, s in enumerate(cl["labels"])}
    out = np.full(len(group_off) - 1, NO_CLASS, dtype=np.uint32)
    for g in range(len(group_off) - 1):
        r0, r1 = int(row_off[int(group_off[g])]), int(row_off[int(group_off[g + 1])])
        s = tuple(sorted(set(int(t) for t in tids[r0:r1])))
        if s:
            out[g] = index[s]
    return out


def row_names_of(n_rows, row_off, group_off):
    """-> the add-order read name of every row"""
    out = np.zeros(n_rows, dtype=np.int64)
    for g in range(len(group_off) - 1):
        out[int(row_off[int(group_off[g])]):int(row_off[int(group_off[g + 1])])] = g
    return out


def weight_words_em(cl, post, name_cls, row_name, tids):
    """q per row for weight em: rint(p * 2^32), ties to even, p the posterior of (the row's name, the row's transcript)"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in cl["labels"]])])
    out = []
    for r, t in enumerate(tids):
        c = int(name_cls[int(row_name[r])])
        e = int(off[c]) + cl["labels"][c].index(int(t))
        out.append(int(np.rint(np.float64(post[e]) * np.float64(4294967296.0))))
    return out


def weighted_coverage_of(rows, lens, q_per_row, primary_only=False):
    """coverage_of (tests.test_coverage_cpu) with a weight word per row (None: the row has no weight and is skipped).  -> dict: depth
    (uint64 per transcript, units of 2^-32), runs (tid, start, end uint32; depth uint64), records, weight_sum, aligned_hi,
    aligned_lo, covered_bases, max_depth (uint64 per transcript), rows_counted, rows_skipped, clipped_bases, no_weight, n_entries
    (what weight em keeps: the clamped non-empty intervals -- every covering op by itself above SMALL_OPS ops -- and one entry
    for a counted row without any)"""
    n_tx = len(lens)
    own = [max(int(v), 0) for v in lens]
    diff = [np.zeros(n + 1, dtype=np.int64) for n in own]
    records, weight_sum = [0] * n_tx, [0] * n_tx
    counted = skipped = clipped = n_entries = 0
    no_weight = False
    off, cig = rows["cigar_off"], rows["cigar"]
    assert len(rows["tid"]) < 1 << 30   # (so that no sum of weight words leaves an int64; the intervals themselves are Python integers)
    for r in range(len(rows["tid"])):
        t, meta = int(rows["tid"][r]), int(rows["meta"][r])
        if (primary_only and not meta & ROW_PRIMARY) or t >= n_tx:
            skipped += 1
            continue
        if q_per_row[r] is None:
            skipped += 1
            no_weight = True
            continue
        q = int(q_per_row[r])
        assert 0 <= q <= ONE
        counted += 1
        records[t] += 1
        weight_sum[t] += q
        words = cig[int(off[r]):int(off[r + 1])]
        kept = 0
        for s, e in intervals_of(rows["pos"][r], words):
            cs, ce = min(s, own[t]), min(e, own[t])
            clipped += (e - s) - (ce - cs)
            if ce > cs:
                diff[t][cs] += q
                diff[t][ce] -= q
                kept += 1
        if len(words) > SMALL_OPS:
            kept = sum(1 for s, e in sum((intervals_of(p, [w]) for p, w in _op_positions(rows["pos"][r], words)), []) if min(e, own[t]) > min(s, own[t]))
        n_entries += max(kept, 1)
    depth = []
    for d in diff:
        acc = np.cumsum(d[:-1])
        assert not len(acc) or acc.min() >= 0
        depth.append(acc.astype(np.uint64))
    runs = [[], [], [], []]
    for t, d in enumerate(depth):
        if not len(d):
            continue
        edge = np.flatnonzero(d[1:] != d[:-1]) + 1
        starts = np.concatenate([[0], edge]).astype(np.int64)
        ends = np.concatenate([edge, [len(d)]]).astype(np.int64)
        keep = d[starts] > 0
        for col, v, dt in zip(runs, (np.full(int(keep.sum()), t), starts[keep], ends[keep], d[starts][keep]), (np.uint32,) * 3 + (np.uint64,)):
            col.append(np.asarray(v, dtype=dt))
    runs = tuple(np.concatenate(c) if c else np.zeros(0, dtype=dt) for c, dt in zip(runs, (np.uint32,) * 3 + (np.uint64,)))
    u64 = lambda v: np.asarray(v, dtype=np.uint64)   # noqa: E731
    return {"depth": depth, "runs": runs, "records": u64(records), "weight_sum": u64(weight_sum),
            "aligned_hi": u64([sum(int(x) >> 32 for x in d) for d in depth]), "aligned_lo": u64([sum(int(x) & 0xffffffff for x in d) for d in depth]),
            "covered_bases": u64([int(np.count_nonzero(d)) for d in depth]), "max_depth": u64([int(d.max()) if len(d) else 0 for d in depth]),
            "rows_counted": counted, "rows_skipped": skipped, "clipped_bases": clipped, "no_weight": no_weight, "n_entries": n_entries}


def _op_positions(pos, words):
    """(position, op word) of every op of a CIGAR, as the walk meets them"""
    p, out = int(pos), []
    for w in words:
        out.append((p, int(w)))
        if int(w) & 15 in (0, 7, 8, 2, 3):
            p += int(w) >> 4
    return out


def run_list(cov):
    return [tuple(int(v) for v in r) for r in zip(*cov["runs"])]


def nh_of(n_rows, row_off, group_off):
    """NH of every row: the rows of its read name"""
    nh = np.zeros(n_rows, dtype=np.uint32)
    for g in range(len(group_off) - 1):
        r0, r1 = int(row_off[int(group_off[g])]), int(row_off[int(group_off[g + 1])])
        nh[r0:r1] = r1 - r0
    return nh


# ---- the yardstick against cases worked out on paper --------------------------------------------------------------------------
def test_nh_words_by_hand():
    assert weight_words_nh([1, 2, 3, 7, 0]) == [4294967296, 2147483648, 1431655765, 613566757, None]
    # NH 1, 2, 3 and 7 on one base; three rows of NH 3 give 3 * 1431655765 = 2^32 - 1, not 2^32
    rows = rows_of([(0, 5, 0, "1M")] * 3)
    cov = weighted_coverage_of(rows, [10], weight_words_nh([3, 3, 3]))
    assert run_list(cov) == [(0, 5, 6, 3 * 1431655765)] and 3 * 1431655765 == ONE - 1
    assert cov["weight_sum"].tolist() == [ONE - 1] and cov["records"].tolist() == [3]
    assert (cov["aligned_hi"].tolist(), cov["aligned_lo"].tolist(), cov["max_depth"].tolist()) == ([0], [ONE - 1], [ONE - 1])
    rows = rows_of([(0, 5, 0, "1M")] * 4)
    cov = weighted_coverage_of(rows, [10], weight_words_nh([1, 2, 3, 7]))
    assert run_list(cov) == [(0, 5, 6, 4294967296 + 2147483648 + 1431655765 + 613566757)]
    assert cov["aligned_hi"].tolist() == [1] and cov["aligned_lo"].tolist() == [4192706170] and cov["covered_bases"].tolist() == [1]
    # a row of NH 0 has no weight: skipped, and flagged
    cov = weighted_coverage_of(rows_of([(0, 5, 0, "1M")] * 2), [10], weight_words_nh([0, 1]))
    assert cov["no_weight"] and (cov["rows_counted"], cov["rows_skipped"]) == (1, 1) and run_list(cov) == [(0, 5, 6, ONE)]


def test_posteriors_by_hand():
    # a one-label class gives exactly 1.0, so q = 2^32: 33 bits
    cl = {"labels": [(4,)], "counts": [9]}
    post = posteriors_of(cl, [0, 0, 0, 0, 0.3], [1, 1, 1, 1, 0.001])
    assert post.tolist() == [1.0] and weight_words_em(cl, post, [0], [0], [4]) == [ONE] and ONE.bit_length() == 33
    # theta w = 1 and 3: 0.25 and 0.75
    cl = {"labels": [(0, 1)], "counts": [2]}
    post = posteriors_of(cl, [2.0, 12.0], [0.5, 0.25])
    assert post.tolist() == [0.25, 0.75]
    assert weight_words_em(cl, post, [0, 0], [0, 1], [0, 1]) == [0x40000000, 0xC0000000]
    # d_c == 0: all zero, and the rows are still records
    post = posteriors_of(cl, [0.0, 0.0], [0.5, 0.25])
    assert post.tolist() == [0.0, 0.0]
    cov = weighted_coverage_of(rows_of([(0, 0, 0, "5M"), (1, 0, 0, "5M")]), [10, 10], weight_words_em(cl, post, [0, 0], [0, 1], [0, 1]))
    assert run_list(cov) == [] and cov["records"].tolist() == [1, 1] and cov["weight_sum"].tolist() == [0, 0] and cov["rows_counted"] == 2
    # the sum is sequential: 1e16 + 1 + 1 loses both ones, 1 + 1 + 1e16 keeps them
    big = {"labels": [(0, 1, 2)], "counts": [1]}
    assert posteriors_of(big, [1e16, 1.0, 1.0], [1, 1, 1])[0] == 1.0
    assert posteriors_of(big, [1.0, 1.0, 1e16], [1, 1, 1])[2] == 1e16 / (1e16 + 2.0) < 1.0
    # ties to even: p = 2^-33 is half a unit -> 0; 3 * 2^-33 -> 2
    one = {"labels": [(0,)], "counts": [1]}
    assert weight_words_em(one, [2.0 ** -33], [0], [0], [0]) == [0] and weight_words_em(one, [3 * 2.0 ** -33], [0], [0], [0]) == [2]


def test_runs_by_hand():
    # two adjacent transcripts of equal depth stay two runs
    cov = weighted_coverage_of(rows_of([(0, 0, 0, "10M"), (1, 0, 0, "10M")]), [10, 10], [ONE // 2, ONE // 2])
    assert run_list(cov) == [(0, 0, 10, ONE // 2), (1, 0, 10, ONE // 2)]
    # depths one unit of 2^-32 apart stay two runs
    cov = weighted_coverage_of(rows_of([(0, 0, 0, "10M"), (0, 5, 0, "5M")]), [10], [1431655765, 1])
    assert run_list(cov) == [(0, 0, 5, 1431655765), (0, 5, 10, 1431655766)]
    # an interval clipped at a transcript's end: its - q lands on the next transcript's first base, beside another weight's + q
    cov = weighted_coverage_of(rows_of([(0, 5, 0, "10M"), (1, 0, 0, "3M")]), [10, 10], [ONE, 7])
    assert run_list(cov) == [(0, 5, 10, ONE), (1, 0, 3, 7)] and cov["clipped_bases"] == 5
    # a pair on two transcripts, both mates counted with their own weight; aligned_hi / aligned_lo split the fixed-point sum
    pair = [(0, 0, ROW_PAIRED | ROW_FIRST | ROW_PRIMARY, "4M"), (1, 2, ROW_PAIRED, "4M")]
    cov = weighted_coverage_of(rows_of(pair), [10, 10], [0xC0000000, 0x40000000])
    assert cov["aligned_hi"].tolist() == [0, 0] and cov["aligned_lo"].tolist() == [4 * 0xC0000000, 4 * 0x40000000]
    assert weighted_coverage_of(rows_of(pair), [10, 10], [ONE, ONE], primary_only=True)["records"].tolist() == [1, 0]
    # what weight em keeps: merged intervals, and one entry for a row without any
    cov = weighted_coverage_of(rows_of([(0, 0, 0, "5M2I5M3D4M"), (0, 0, 0, "4S"), (0, 50, 0, "5M")]), [20], [1, 1, 1])
    assert cov["n_entries"] == 2 + 1 + 1 and cov["records"].tolist() == [3] and cov["weight_sum"].tolist() == [3]


# ---- what the synthetic inputs hold -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_inputs_hold_what_the_feature_is_about(mode):
    tb, rows = wide_rows(mode)
    n_rows = len(rows["tid"])
    nh = nh_of(n_rows, tb["row_off"], tb["group_off"])
    cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    ncls = name_classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    names = row_names_of(n_rows, tb["row_off"], tb["group_off"])
    held = {"names_nh3": int(np.count_nonzero(np.bincount(names[nh >= 3]) > 0)), "classes_2plus": sum(1 for s in cl["labels"] if len(s) >= 2),
            "no_rows": int(np.count_nonzero(ncls == NO_CLASS))}
    # a pair on two transcripts: a read name whose paired rows lie on more than one transcript (the inputs emit no pair whose two
    # mates sit on different transcripts -- ROW_PAIRED without ROW_SAME_TX; the GPU tests' hand-built table holds that one)
    paired = rows["meta"] & ROW_PAIRED != 0
    pair_two = sum(1 for g in np.unique(names[paired]) if len(set(rows["tid"][paired & (names == g)].tolist())) >= 2)
    held["pair_on_two"] = pair_two
    print(mode, held)
    assert held["names_nh3"] >= 100 and held["classes_2plus"] >= 100 and held["no_rows"] >= 1
    if mode == "pe":
        assert held["pair_on_two"] >= 1
    # the weights differ: the unit track, the nh track and a posterior track are three different answers
    q_nh = weight_words_nh(nh)
    assert len(set(q_nh)) >= 4 and all(q is not None for q in q_nh)


# ---- ABI and usage errors -------------------------------------------------------------------------------------------------------
SYMBOLS = ("br_quant_name_classes", "br_quant_posteriors", "br_coverage_add_names", "br_coverage_finish_em", "br_coverage_runs64",
           "br_coverage_depth64", "br_coverage_summary64")


def test_new_symbols_without_a_device():
    from bramble_amd import lib
    L = lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    L.br_quant_name_classes.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    L.br_quant_posteriors.argtypes = [C.c_void_p, C.c_void_p]
    L.br_coverage_add_names.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.br_coverage_finish_em.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.br_coverage_runs64.argtypes = [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4
    L.br_coverage_depth64.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.br_coverage_summary64.argtypes = [C.c_void_p] * 7
    L.br_coverage_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.br_quant_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.br_coverage_new.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]
    rows = lib.BrDeviceRows()
    out = np.zeros(4, dtype=np.uint64)
    assert L.br_quant_name_classes(None, 0, 0, out.ctypes.data) == -1 and L.br_quant_posteriors(None, None) == -1   # BR_ERR_INVALID_ARG
    assert L.br_coverage_add_names(None, C.byref(rows), None, 0, 0, None) == -1 and L.br_coverage_finish_em(None, None, None) == -1
    assert L.br_coverage_runs64(None, 0, 0, None, None, None, None) == -1 and L.br_coverage_depth64(None, 0, None) == -1
    assert L.br_coverage_summary64(None, None, None, None, None, None, None) == -1
    assert L.br_coverage_set_param(None, b"weight", 1) == -1 and L.br_quant_set_param(None, b"keep_names", 1) == -1
    lens = np.asarray([100], dtype=np.int64)
    h = C.c_void_p()
    assert L.br_coverage_new(4096, 1, lens.ctypes.data, C.byref(h)) == -2 and not h.value   # BR_ERR_NO_DEVICE
    for name in ("add_names_host", "add_names_device", "finish_em", "runs64", "depth64", "summary64"):
        assert hasattr(lib.Coverage, name), name
    for name in ("name_classes", "posteriors"):
        assert hasattr(lib.Quant, name), name


@pytest.mark.parametrize("extra,word", [
    (["--coverage-weight", "nh"], b"--coverage-weight"),                                        # without --coverage / --coverage-summary
    (["--coverage", "c.bedgraph", "--coverage-weight", "em"], b"--quant"),                      # em without --quant
    (["--coverage", "c.bedgraph", "--coverage-weight", "half"], b"--coverage-weight"),          # an unknown word
])
def test_cli_usage_errors(tmp_path, extra, word):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    extra = [str(tmp_path / e) if e.endswith((".tsv", ".bedgraph")) else e for e in extra]
    r = subprocess.run([os.path.join(root, "bramble_amd", "bin", "bramble"), str(tmp_path / "missing.bam"), "-G", str(gtf), "-o",
                        str(tmp_path / "o.bam")] + extra, capture_output=True, timeout=60)
    assert r.returncode == 2
    assert word in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]
