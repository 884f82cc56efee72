"""--quant without a GPU: the tests' own restatement of the definitions in bramble_amd.h (br_quant) -- read names to transcript
sets to equivalence classes, unique / ambiguous counts, the EM with its stopping rule, the two output files -- which the GPU tests
compare the device against; checks of those yardsticks against cases worked out by hand; what the synthetic inputs hold; the ABI
without a device."""
import ctypes as C
import math

import numpy as np
import pytest

MIN_THETA = 1e-8      # a transcript below this does not take part in the relative change
CHECK_EVERY = 16      # the change is looked at after every iteration whose number is a multiple of this, and after the last


# ---- the yardsticks -----------------------------------------------------------------------------------------------------------
def classes_of(tids, row_off, group_off):
    """tids: transcript_id per row; read name g has the rows row_off[group_off[g]] .. row_off[group_off[g + 1]].
    -> dict: labels (a sorted tuple per class), counts, first (the name that opened the class), in the order of first;
    n_names, n_unassigned"""
    index, labels, counts, first, n_unassigned = {}, [], [], [], 0
    n_names = len(group_off) - 1
    for g in range(n_names):
        r0, r1 = int(row_off[int(group_off[g])]), int(row_off[int(group_off[g + 1])])
        s = tuple(sorted(set(int(t) for t in tids[r0:r1])))
        if not s:
            n_unassigned += 1
            continue
        if s not in index:
            index[s] = len(labels)
            labels.append(s)
            counts.append(0)
            first.append(g)
        counts[index[s]] += 1
    return {"labels": labels, "counts": counts, "first": first, "n_names": n_names, "n_unassigned": n_unassigned}


def unique_ambig(cl, n_tx):
    uniq, ambig = np.zeros(n_tx, dtype=np.uint64), np.zeros(n_tx, dtype=np.uint64)
    for s, n in zip(cl["labels"], cl["counts"]):
        for t in s:
            (uniq if len(s) == 1 else ambig)[t] += n
    return uniq, ambig


def weights(lens, n_tx, length_norm):
    if not length_norm:
        return np.ones(n_tx, dtype=np.float64)
    lens = np.asarray(lens, dtype=np.float64)
    return np.where(lens > 0, 1.0 / np.where(lens > 0, lens, 1.0), 0.0)


def class_order(n_cls, order):
    """the order in which a transcript's sum takes its classes: "forward", "reversed", or an integer seed for a shuffle"""
    if order == "forward":
        return np.arange(n_cls)
    if order == "reversed":
        return np.arange(n_cls)[::-1].copy()
    return np.random.RandomState(int(order)).permutation(n_cls)


def em_reference(cl, n_tx, lens=None, length_norm=True, max_iters=10000, tolerance=1e-2, order="forward", trace=None):
    """-> dict theta, tpm, n_iters, rel_change.  Every sum is a sequential float64 loop (np.bincount adds its weights one by one
    in input order): a class's over its labels ascending, a transcript's over its classes in `order`.  trace: a list that
    receives (sum of theta, log-likelihood) after every iteration."""
    w = weights(lens, n_tx, length_norm)
    n_cls = len(cl["labels"])
    cnt = np.asarray(cl["counts"], dtype=np.float64)
    e_cls = np.asarray([c for c, s in enumerate(cl["labels"]) for _ in s], dtype=np.int64)
    e_tid = np.asarray([t for s in cl["labels"] for t in s], dtype=np.int64)
    rank = np.empty(n_cls, dtype=np.int64)
    rank[class_order(n_cls, order)] = np.arange(n_cls)
    perm = np.argsort(rank[e_cls], kind="stable") if len(e_cls) else np.zeros(0, dtype=np.int64)
    t_cls, t_tid = e_cls[perm], e_tid[perm]
    theta = np.ones(n_tx, dtype=np.float64)
    it, rel = 0, 0.0
    while it < max_iters:
        it += 1
        x = theta * w
        d = np.bincount(e_cls, weights=x[e_tid], minlength=n_cls) if n_cls else np.zeros(0)
        q = np.where(d > 0, cnt / np.where(d > 0, d, 1.0), 0.0)
        s = np.bincount(t_tid, weights=q[t_cls], minlength=n_tx) if n_cls else np.zeros(n_tx)
        new = x * s
        if trace is not None:
            total = float(new.sum())
            dn = np.bincount(e_cls, weights=(new * w)[e_tid], minlength=n_cls)
            trace.append((total, float(sum(n * math.log(v / total) for n, v in zip(cl["counts"], dn) if v > 0))))
        look = it % CHECK_EVERY == 0 or it == max_iters
        if look:
            m = new > MIN_THETA
            rel = float(np.max(np.abs(new[m] - theta[m]) / new[m])) if m.any() else 0.0
        theta = new
        if look and rel < tolerance:
            break
    x = theta * w
    tot = 0.0
    for v in x:   # (transcript order, one by one)
        tot += float(v)
    tpm = 1e6 * x / tot if tot > 0 else np.zeros(n_tx)
    return {"theta": theta, "tpm": tpm, "n_iters": it, "rel_change": rel}


def format_quant_tsv(names, lens, theta, tpm, uniq, ambig):
    out = ["Name\tLength\tNumReads\tTPM\tUniqueReads\tAmbigReads"]
    for k, nm in enumerate(names):
        out.append("%s\t%d\t%.6f\t%.6f\t%d\t%d" % (nm, lens[k], theta[k], tpm[k], uniq[k], ambig[k]))
    return "\n".join(out) + "\n"


def parse_quant_tsv(text):
    lines = text.split("\n")
    assert lines[0] == "Name\tLength\tNumReads\tTPM\tUniqueReads\tAmbigReads" and lines[-1] == ""
    rows = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 6
        rows.append((f[0], int(f[1]), f[2], f[3], int(f[4]), int(f[5])))   # the floats stay text: they are compared as printed
    return rows


def format_eq_classes(names, labels, counts):
    """salmon's eq_classes.txt: the number of transcripts, the number of classes, the names, then k t1 .. tk count per class"""
    out = [str(len(names)), str(len(labels))] + list(names)
    for s, n in zip(labels, counts):
        out.append("\t".join([str(len(s))] + [str(t) for t in s] + [str(n)]))
    return "\n".join(out) + "\n"


def parse_eq_classes(text):
    lines = text.split("\n")
    assert lines[-1] == ""
    n_tx, n_cls = int(lines[0]), int(lines[1])
    names = lines[2:2 + n_tx]
    body = lines[2 + n_tx:-1]
    assert len(body) == n_cls
    labels, counts = [], []
    for l in body:
        f = [int(v) for v in l.split("\t")]
        assert len(f) == f[0] + 2
        labels.append(tuple(f[1:-1]))
        counts.append(f[-1])
    return names, labels, counts


# ---- the oracle's rows of the synthetic inputs, framed as the device tables are -------------------------------------------------
def oracle_tables(mode, recs=None, guide_order=False):
    """The oracle's projection of tests.test_gpu_collate._inputs(mode) -- or of `recs`, a collated list of that input's mapped
    records: tids per row, a row_off that gives every read name's rows to its first alignment (only row_off[group_off[g]] is
    ever read), group_off, the transcripts' lengths (guide_order: with the transcripts numbered as the command line's guide
    loader numbers them, bamio.guide_order); and the input itself (the record stream, its offsets, the oracle's reader-side
    tables)."""
    from oracle import oracle_binding as ob
    from bramble_amd import lib
    from tests.test_collate_cpu import read_name
    from tests.test_gpu_collate import _cat, _inputs
    annd, all_recs, _ = _inputs(mode)
    recs = all_recs if recs is None else recs
    if guide_order:
        from tests import bamio
        annd = dict(annd, transcripts=[annd["transcripts"][t] for t in bamio.guide_order(annd)])
    flags = {"lr": 1} if mode == "ont" else {}
    stream = _cat(recs)
    roff, rlen, _, _ = lib.bam_split(stream)
    oi = ob.OracleIndex(annd)
    rows, _, _, parsed = ob.run_bam(oi, ob.make_flags(**flags), stream, roff, rlen, np.arange(len(annd["refnames"]), dtype=np.int32))
    names = [read_name(r) for r in recs]
    starts = [0] + [i for i in range(1, len(names)) if names[i] != names[i - 1]] + [len(names)]
    group_off = np.asarray(starts, dtype=np.uint32)
    n_groups = len(starts) - 1
    aln_group = np.repeat(np.arange(n_groups), np.diff(starts))
    grp = np.asarray(rows["group"], dtype=np.int64)
    assert np.all(np.diff(grp) >= 0) and (len(grp) == 0 or grp[-1] < n_groups)
    assert np.array_equal(aln_group[np.asarray(rows["input_index"], dtype=np.int64)], grp)   # a row belongs to its alignment's read name
    per_group = np.bincount(grp, minlength=n_groups)
    row_off = np.zeros(len(names) + 1, dtype=np.uint64)
    per_aln = np.zeros(len(names), dtype=np.int64)
    per_aln[group_off[:-1]] = per_group
    row_off[1:] = np.cumsum(per_aln)
    n_tx = oi.num_transcripts()
    lens = np.asarray([oi.transcript_len(t) for t in range(n_tx)], dtype=np.int64)
    return {"tids": np.asarray(rows["tid"], dtype=np.uint32), "row_off": row_off, "group_off": group_off, "n_tx": n_tx, "lens": lens,
            "annd": annd, "flags": flags, "stream": stream, "roff": roff, "rlen": rlen, "parsed": {k: np.array(v) for k, v in parsed.items()}}


# ---- the yardsticks against cases worked out by hand ------------------------------------------------------------------------------
def test_classes_by_hand():
    #            name 0: a pair on transcripts 5 and 2 (a discordant pair: both count); name 1: no rows; name 2: {2, 5} again, from
    #            three rows; name 3: {7}; name 4: {5}
    tids = [5, 2, 2, 5, 5, 7, 5]
    row_off = [0, 2, 2, 2, 4, 5, 6, 7]          # alignments 0 .. 6; alignments 1 and 2 (name 1) emit nothing
    group_off = [0, 1, 3, 5, 6, 7]
    cl = classes_of(tids, row_off, group_off)
    assert cl["labels"] == [(2, 5), (7,), (5,)] and cl["counts"] == [2, 1, 1] and cl["first"] == [0, 3, 4]
    assert cl["n_names"] == 5 and cl["n_unassigned"] == 1
    uniq, ambig = unique_ambig(cl, 8)
    assert uniq.tolist() == [0, 0, 0, 0, 0, 1, 0, 1] and ambig.tolist() == [0, 0, 2, 0, 0, 2, 0, 0]


def test_em_two_transcripts_closed_form():
    # 30 names on {0}, 10 on {1}, 60 on {0, 1}, equal weights: at the fixed point theta0 = 30 + 60 theta0 / 100, so theta0 = 75
    cl = {"labels": [(0,), (1,), (0, 1)], "counts": [30, 10, 60]}
    r = em_reference(cl, 2, length_norm=False, max_iters=2000, tolerance=0)
    assert r["n_iters"] == 2000
    assert abs(r["theta"][0] - 75.0) < 1e-9 and abs(r["theta"][1] - 25.0) < 1e-9
    assert abs(r["tpm"][0] - 750000.0) < 1e-4
    # lengths 1000 and 2000: the fixed point of theta0 = 30 + 60 theta0 w0 / (theta0 w0 + theta1 w1) with theta1 = 100 - theta0
    r = em_reference(cl, 2, lens=[1000, 2000], max_iters=4000, tolerance=0)
    t0, t1 = r["theta"]
    assert abs(t0 - (30 + 60 * t0 / 1000 / (t0 / 1000 + t1 / 2000))) < 1e-9 and abs(t0 + t1 - 100) < 1e-9
    assert abs(r["tpm"].sum() - 1e6) < 1e-3


def test_em_keeps_the_names_and_never_loses_likelihood():
    rng = np.random.RandomState(5)
    labels = sorted(set(tuple(sorted(set(rng.randint(0, 40, size=rng.randint(1, 6)).tolist()))) for _ in range(120)))
    cl = {"labels": labels, "counts": rng.randint(1, 50, size=len(labels)).tolist()}
    trace = []
    em_reference(cl, 40, lens=rng.randint(300, 5000, size=40), max_iters=300, tolerance=0, trace=trace)
    n = sum(cl["counts"])
    assert all(abs(total - n) <= 1e-9 * n for total, _ in trace)
    assert all(b[1] >= a[1] - 1e-9 * abs(a[1]) for a, b in zip(trace, trace[1:]))
    assert trace[-1][1] > trace[0][1]


def test_em_stopping_rule():
    cl = {"labels": [(0,), (1,), (0, 1)], "counts": [30, 10, 60]}
    r = em_reference(cl, 2, length_norm=False)
    assert r["n_iters"] % CHECK_EVERY == 0 and r["rel_change"] < 1e-2 and r["n_iters"] < 10000
    r = em_reference(cl, 2, length_norm=False, max_iters=21, tolerance=1e-300)
    assert r["n_iters"] == 21   # the last iteration is looked at whatever its number
    # a class whose transcripts all have weight 0 contributes nothing
    r = em_reference({"labels": [(0,), (1,)], "counts": [5, 7]}, 2, lens=[100, 0], max_iters=3, tolerance=0)
    assert r["theta"].tolist() == [5.0, 0.0]


def test_files_round_trip():
    cl = {"labels": [(0, 2), (1,)], "counts": [3, 9]}
    text = format_eq_classes(["a", "b", "c"], cl["labels"], cl["counts"])
    assert text == "3\n2\na\nb\nc\n2\t0\t2\t3\n1\t1\t9\n"
    assert parse_eq_classes(text) == (["a", "b", "c"], cl["labels"], cl["counts"])
    tsv = format_quant_tsv(["a", "b"], [100, 2000], [1.5, 0.0], [1e6, 0.0], [1, 0], [2, 0])
    assert tsv == "Name\tLength\tNumReads\tTPM\tUniqueReads\tAmbigReads\na\t100\t1.500000\t1000000.000000\t1\t2\nb\t2000\t0.000000\t0.000000\t0\t0\n"
    assert parse_quant_tsv(tsv) == [("a", 100, "1.500000", "1000000.000000", 1, 2), ("b", 2000, "0.000000", "0.000000", 0, 0)]


@pytest.mark.parametrize("mode,floors", [("pe", (1100, 900, 450, 20)), ("ont", (480, 350, 140, 15))])
def test_inputs_hold_what_the_feature_is_about(mode, floors):
    tb = oracle_tables(mode)
    cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    n_cls = len(cl["labels"])
    multi = sum(1 for s in cl["labels"] if len(s) > 1)
    repeated = sum(1 for n in cl["counts"] if n > 1)
    largest = max(len(s) for s in cl["labels"])
    print("%s: %d read names, %d classes, %d multi-label, %d with count > 1, largest %d labels, %d unassigned"
          % (mode, cl["n_names"], n_cls, multi, repeated, largest, cl["n_unassigned"]))
    assert n_cls >= floors[0] and multi >= floors[1] and repeated >= floors[2] and largest >= floors[3]
    assert max(max(s) for s in cl["labels"]) < tb["n_tx"]


# ---- ABI and usage errors -------------------------------------------------------------------------------------------------------
def test_quant_new_without_a_device():
    """BR_ERR_NO_DEVICE for a device that does not exist (every device, on a machine without one)."""
    from bramble_amd import lib
    L = lib.lib()
    L.br_quant_new.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]
    L.br_quant_free.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert L.br_quant_new(4096, 10, None, C.byref(h)) == -2   # BR_ERR_NO_DEVICE
    assert not h.value
    assert L.br_quant_new(-1, 10, None, C.byref(h)) == -2
    L.br_quant_free(None)
    for name in ("br_quant_set_param", "br_quant_set_tolerance", "br_quant_add", "br_quant_add_last", "br_quant_finish", "br_quant_classes",
                 "br_quant_em", "br_quant_result", "br_quant_stats"):
        assert hasattr(L, name), name
    assert L.br_quant_finish(None, None, None) == -1 and L.br_quant_em(None, None, None) == -1


@pytest.mark.parametrize("extra,word", [
    (["--quant-classes", "c.txt"], b"--quant"),
    (["--quant", "q.tsv", "--devices", "0,0"], b"--quant"),
])
def test_cli_quant_usage_errors(tmp_path, extra, word):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    out = str(tmp_path / "o.bam")
    extra = [str(tmp_path / e) if e.endswith((".txt", ".tsv")) else e for e in extra]
    r = subprocess.run([os.path.join(root, "bramble_amd", "bin", "bramble"), str(tmp_path / "missing.bam"), "-G", str(gtf), "-o", out] + extra,
                       capture_output=True, timeout=60)
    assert r.returncode == 2
    assert word in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]
