"""--quant on the GPU: br_quant's classes, counts and EM against the tests' restatement of the definitions (test_quant_cpu.py) on the
oracle's rows of the synthetic inputs, fed from the host, from HBM and from a context's last projection call, with colliding hashes
on purpose; a hand-built input for the wave-sized paths; the errors; and the command line with --quant against the run without
it."""
import functools
import os
import subprocess

import numpy as np
import pytest

from bramble_amd import lib, synth
from tests import bamio
from tests.test_collate_cpu import collate_order, mapped_records
from tests.test_gpu_collate import BIN, _cat, _coordinate_stream, _files, _inputs, _report, _run, _strip
from tests.test_quant_cpu import (classes_of, em_reference, oracle_tables, parse_eq_classes, parse_quant_tsv, unique_ambig)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tables(mode):
    return oracle_tables(mode)


def _rows_a(tids):
    a = np.zeros((len(tids), 4), dtype=np.uint32)
    a[:, 0] = tids
    return a


def _batch_of(tb):
    """the oracle's reader-side tables of the records as a flat batch (what br_project_batch_device takes, uploaded)"""
    p, stream = tb["parsed"], bytes(tb["stream"])
    n = int(p["n_aln"])
    cig, names = [], []
    for o in tb["roff"]:
        o = int(o)
        l_name, n_cig = stream[o + 8], int.from_bytes(stream[o + 12:o + 14], "little")
        names.append(stream[o + 32:o + 32 + l_name - 1])
        cig.append(np.frombuffer(stream[o + 32 + l_name:o + 32 + l_name + 4 * n_cig], dtype="<u4"))
    b = {k: p[k] for k in ("ref_id", "ref_start", "flags", "xs", "ts", "mate_ref_id", "mate_start", "l_qseq")}
    b["n_aln"] = n
    b["cigar_off"] = np.concatenate([[0], np.cumsum([len(c) for c in cig])]).astype(np.uint64)
    b["cigar"] = np.concatenate(cig).astype(np.uint32)
    b["name_off"] = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint64)
    b["names"] = np.frombuffer(b"".join(names), dtype=np.uint8).copy()
    b["seq_off"] = b["seqs"] = None
    assert np.array_equal(b["cigar_off"], p["cigar_off"])
    return b


def _fill(q, tb, how):
    """the input's read names into `q`: from host memory, from HBM in 1 or 3 calls, or from a context's last projection call"""
    import torch
    if how == "host":
        q.add_host(_rows_a(tb["tids"]), tb["row_off"], tb["group_off"])
    elif how in ("dev1", "dev3"):
        a = torch.from_numpy(_rows_a(tb["tids"]).view(np.int32)).cuda()
        ro = torch.from_numpy(tb["row_off"].view(np.int64)).cuda()
        go = torch.from_numpy(tb["group_off"].view(np.int32)).cuda()
        n_groups = len(tb["group_off"]) - 1
        cuts = [0, n_groups] if how == "dev1" else [0, n_groups // 3, n_groups // 3 + 1, n_groups]   # (a call of one name among them)
        for g0, g1 in zip(cuts, cuts[1:]):
            q.add_device(a, ro, go, g0, g1)
    else:
        idx = lib.Index(tb["annd"], device=0)
        ctx = lib.Context(idx)
        cfg = lib.make_config(**tb["flags"])
        if how == "last_batch":
            from bramble_amd import device
            db = device.upload_batch(_batch_of(tb))   # (group_off is the caller's memory: it lives until the add)
            ctx.project_batch_device(cfg, db)
            q.add_last(ctx)
        else:   # the records through a collator's bundles (the input is collated: they come out as they went in), a call each
            c = lib.Collator(0)
            c.add_host(tb["stream"])
            c.finish()
            ref_map = np.arange(len(tb["annd"]["refnames"]), dtype=np.int32)
            n_bundles = 0
            while True:
                b = c.next_records(700)
                if b.n_aln == 0:
                    break
                ctx.project_bam_resident(cfg, b, ref_map)
                q.add_last(ctx)
                n_bundles += 1
            assert n_bundles > 1
            c.close()
        ctx.close()
        idx.close()


def _new(tb, length_norm=None, **params):
    q = lib.Quant(tb["n_tx"], tb["lens"])
    for k, v in params.items():
        q.set_param(k, v)
    if length_norm is not None:
        q.set_param("length_norm", length_norm)
    return q


def _assert_classes(q, cl, n_tx):
    n_names, n_classes = q.n_names, q.n_classes
    off, labels, counts, first = q.classes()
    got = [tuple(int(t) for t in labels[int(off[c]):int(off[c + 1])]) for c in range(n_classes)]
    assert n_names == cl["n_names"] and n_classes == len(cl["labels"])
    assert got == cl["labels"]
    assert counts.tolist() == cl["counts"] and first.tolist() == cl["first"]
    r = q.result(em=False)
    uniq, ambig = unique_ambig(cl, n_tx)
    assert np.array_equal(r["unique"], uniq) and np.array_equal(r["ambig"], ambig)
    st = q.stats()
    assert st["n_unassigned"] == cl["n_unassigned"] and st["n_labels"] == sum(len(s) for s in cl["labels"])
    assert st["peak_bytes"] >= st["held_bytes"] > 0
    return st


# ---- classes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("how", ["host", "dev1", "dev3", "last_batch", "last_resident"])
def test_classes_match_the_yardstick(mode, how):
    tb = _tables(mode)
    cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    q = _new(tb)
    _fill(q, tb, how)
    q.finish()
    st = _assert_classes(q, cl, tb["n_tx"])
    assert st["collisions"] == 0
    q.close()


@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("bits", [64, 8, 1])
def test_hash_collisions_change_nothing(mode, bits):
    tb = _tables(mode)
    cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    q = _new(tb, hash_bits=bits)
    _fill(q, tb, "dev3")
    q.finish()
    st = _assert_classes(q, cl, tb["n_tx"])
    assert (st["collisions"] > 0) == (bits != 64)
    q.close()


def _hand_built():
    """A class of 200 labels (from a name of 200 rows, and a second name with the same set), a name of 300 rows over 150
    transcripts, a transcript that sits in 5 000 classes, a name without rows, and small names around them."""
    rng = np.random.RandomState(3)
    n_tx = 6000
    names = []
    wide = rng.permutation(np.arange(100, 700))[:200]
    names.append(list(wide))
    names.append([7, 3])
    dup = rng.permutation(np.arange(800, 950))
    names.append(list(dup) + list(rng.permutation(dup)))            # 300 rows, every transcript twice
    names.append([])
    for j in range(5000):
        names.append([1000 + j, 0] if j % 2 else [0, 1000 + j])     # transcript 0 in 5 000 classes
    # some of those classes twice and some of their transcripts with a name of their own, so that the 5 000 terms transcript 0
    # sums differ and their order shows in the last bits (5 000 equal terms add up alike in any order)
    for j in range(0, 5000, 11):
        names.append([0, 1000 + j])
    for j in range(0, 5000, 7):
        names.append([1000 + j] * (1 + j % 3))
    names.append(list(rng.permutation(wide)))                       # the 200-label class once more
    names.append([3, 7, 7])
    names.append([0])
    tids = np.asarray([t for nm in names for t in nm], dtype=np.uint32)
    # every name is two alignments; the rows are split between them (the second may have none)
    row_off, group_off = [0], [0]
    for nm in names:
        h = len(nm) // 2
        row_off += [row_off[-1] + h, row_off[-1] + len(nm)]
        group_off.append(group_off[-1] + 2)
    return tids, np.asarray(row_off, dtype=np.uint64), np.asarray(group_off, dtype=np.uint32), n_tx


def test_hand_built_wide_inputs():
    tids, row_off, group_off, n_tx = _hand_built()
    cl = classes_of(tids, row_off, group_off)
    assert max(len(s) for s in cl["labels"]) == 200 and cl["counts"][0] == 2 and cl["n_unassigned"] == 1
    assert sum(1 for s in cl["labels"] if 0 in s) >= 5000
    for bits in (64, 4):
        q = lib.Quant(n_tx)
        q.set_param("hash_bits", bits)
        q.add_host(_rows_a(tids), row_off, group_off)
        q.finish()
        _assert_classes(q, cl, n_tx)
        q.close()
    # the EM over them: a class and a transcript that a wave sums, against the sequential restatement, under the rule of
    # test_em_values below
    q = lib.Quant(n_tx)
    q.set_param("max_iters", 100)
    q.set_param("tolerance", 0)
    q.add_host(_rows_a(tids), row_off, group_off)
    q.finish()
    assert q.em()[0] == 100
    _assert_em(q.result(), cl, n_tx, None, False, 100, "hand-built")
    q.close()


# ---- EM --------------------------------------------------------------------------------------------------------------------
def _spread(cl, n_tx, lens, length_norm, iters):
    """(the forward reference, s): s = the largest relative difference, over theta > 1e-6, between the restatement run in forward,
    reversed and a seeded-shuffle class order -- what the order of a sum alone does to the result"""
    runs = [em_reference(cl, n_tx, lens, length_norm, max_iters=iters, tolerance=0, order=o) for o in ("forward", "reversed", 12345)]
    s = 0.0
    for key in ("theta", "tpm"):
        ref = runs[0][key]
        m = ref > 1e-6
        for other in runs[1:]:
            s = max(s, float(np.max(np.abs(other[key][m] - ref[m]) / ref[m])))
    return runs[0], s


def _assert_em(got, cl, n_tx, lens, length_norm, iters, tag):
    ref, s = _spread(cl, n_tx, lens, length_norm, iters)
    _assert_em_to(got, ref, s, iters, tag)


def _assert_em_to(got, ref, s, iters, tag):
    """the rule itself, for callers that hold one _spread of an input to several device runs"""
    print("%s: spread s of the restatement over three class orders after %d iterations = %.3e" % (tag, iters, s))
    assert 0 < s < 1e-9
    for key in ("theta", "tpm"):
        r, g = ref[key], got[key]
        m = r > 1e-6
        rel = float(np.max(np.abs(g[m] - r[m]) / r[m]))
        ab = float(np.max(np.abs(g[~m] - r[~m]))) if (~m).any() else 0.0
        print("%s: %s device against the forward restatement: relative %.3e (bound %.3e), absolute below 1e-6 %.3e (bound %.3e)"
              % (tag, key, rel, 64 * s, ab, 64 * s * 1e-6))
        assert rel <= 64 * s and ab <= 64 * s * 1e-6


@pytest.mark.parametrize("mode,length_norm", [("pe", 1), ("ont", 0), ("pe", 0), ("ont", 1)])
def test_em_values(mode, length_norm):
    tb = _tables(mode)
    cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    results = []
    for how in ("dev1", "dev3", "dev1"):
        q = _new(tb, length_norm=length_norm, max_iters=200, tolerance=0)
        _fill(q, tb, how)
        q.finish()
        n_iters, _ = q.em()
        assert n_iters == 200
        results.append(q.result())
        q.close()
    for other in results[1:]:   # two runs, and 1-call against 3-call adds: the same bits
        for key in ("theta", "tpm"):
            assert np.array_equal(results[0][key].view(np.uint64), other[key].view(np.uint64)), key
    _assert_em(results[0], cl, tb["n_tx"], tb["lens"], bool(length_norm), 200, "%s length_norm=%d" % (mode, length_norm))
    if mode == "ont" and not length_norm:
        n = cl["n_names"] - cl["n_unassigned"]
        assert abs(float(results[0]["theta"].sum()) - n) <= 1e-9 * n


@pytest.mark.parametrize("mode,length_norm", [("pe", 1), ("ont", 0)])
def test_em_stops_where_the_restatement_stops(mode, length_norm):
    tb = _tables(mode)
    cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    ref = em_reference(cl, tb["n_tx"], tb["lens"], bool(length_norm))   # max_iters 10000, tolerance 1e-2
    print("%s: the restatement stops after %d iterations at a relative change of %.3e" % (mode, ref["n_iters"], ref["rel_change"]))
    assert ref["n_iters"] < 10000
    q = _new(tb, length_norm=length_norm)
    _fill(q, tb, "host")
    q.finish()
    n_iters, rel = q.em()
    assert n_iters == ref["n_iters"] and (n_iters % 16 == 0 or n_iters == 10000)
    assert rel < 1e-2 and abs(rel - ref["rel_change"]) <= 1e-6 * ref["rel_change"]
    q.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors():
    tb = _tables("ont")
    a, ro, go = _rows_a(tb["tids"]), tb["row_off"], tb["group_off"]
    q = _new(tb)
    assert lib.lib().br_quant_em(q.h, None, None) == -1          # em before finish
    q.add_host(a, ro, go)
    q.finish()
    assert q.add_raw(a.ctypes.data, ro.ctypes.data, go.ctypes.data, len(go) - 1, False) == -1   # add after finish
    assert lib.lib().br_quant_finish(q.h, None, None) == -1
    q.close()
    q = lib.Quant(int(tb["tids"].max()), tb["lens"][:int(tb["tids"].max())])   # one transcript short
    q.add_host(a, ro, go)
    assert lib.lib().br_quant_finish(q.h, None, None) == -1      # a tid >= n_transcripts
    assert lib.lib().br_quant_em(q.h, None, None) == -1
    q.close()
    lens = tb["lens"].copy()
    lens[int(tb["tids"][0])] = 0
    q = lib.Quant(tb["n_tx"], lens)
    q.add_host(a, ro, go)
    assert lib.lib().br_quant_finish(q.h, None, None) == -1      # lengths normalise and a transcript with reads has none
    q.close()
    q = lib.Quant(tb["n_tx"], lens)
    q.set_param("length_norm", 0)
    q.add_host(a, ro, go)
    q.finish()
    q.close()
    bad = ro.copy()
    bad[int(go[5])] = bad[-1] + 10                               # offsets that descend behind name 5
    q = _new(tb)
    assert q.add_raw(a.ctypes.data, bad.ctypes.data, go.ctypes.data, len(go) - 1, False) == -1
    q.close()
    q = _new(tb)                                                  # nothing added: no names, no classes, theta = 0
    assert q.finish() == (0, 0)
    assert q.em()[0] >= 1 and not q.result()["theta"].any()
    q.close()


# ---- command line ------------------------------------------------------------------------------------------------------------
def _api_result(tb, cl, length_norm):
    q = _new(tb, length_norm=length_norm)
    q.add_host(_rows_a(tb["tids"]), tb["row_off"], tb["group_off"])
    q.finish()
    n_iters, _ = q.em()
    r = q.result()
    q.close()
    return r, n_iters


def _body(path, sam):
    """the output without what names the command line: (header lines without bramble's @PG, the records)"""
    if sam:
        lines = open(path, "rb").read().decode().split("\n")
        return [l for l in lines if not l.startswith("@PG\tID:bramble")], None
    t, refs, s = bamio.read_bam(path)
    return (_strip(t), refs), s


@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_cli_quant(tmp_path, mode):
    annd, recs, stream = _inputs(mode)
    lr = ["--lr"] if mode == "ont" else []
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    extra = ["-G", gtf] + lr
    names = annd["refnames"]
    in_bam, hdr = _files(tmp_path, annd, stream, "in")
    in_sam = str(tmp_path / "in.sam")
    open(in_sam, "wb").write(hdr.encode() + synth.records_to_sam(stream, names))
    sorted_bam, _ = _files(tmp_path, annd, _coordinate_stream(stream), "sorted")
    permuted = mapped_records(_coordinate_stream(stream))
    tb_in = oracle_tables(mode, guide_order=True)   # (the command line numbers the transcripts in guide order)
    tb_col = oracle_tables(mode, [permuted[i] for i in collate_order(permuted)], guide_order=True)
    n_records = len(recs)
    runs = {
        "device": ([in_bam, "--device-reader"], tb_in),
        "host": ([in_bam, "--host-reader"], tb_in),
        "sam": ([in_sam], tb_in),
        "collate": ([sorted_bam, "--collate"], tb_col),
        "sort": ([in_bam, "--sort"], tb_in),
        "samout": ([in_bam, "-O", "sam"], tb_in),
        "one": ([in_bam, "--bundle-size", str(10 * n_records)], tb_in),
        "many": ([in_bam, "--bundle-size", str(n_records // 8)], tb_in),
    }
    tx_names = [t["id"] for t in tb_in["annd"]["transcripts"]]
    api = {}
    for tag, (args, tb) in runs.items():
        cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
        if id(tb) not in api:
            api[id(tb)] = _api_result(tb, cl, 0 if lr else 1)
        res, n_iters = api[id(tb)]
        sam = tag == "samout"
        o0, o1 = str(tmp_path / ("plain_%s.out" % tag)), str(tmp_path / ("quant_%s.out" % tag))
        tsv, eqc = str(tmp_path / ("%s.tsv" % tag)), str(tmp_path / ("%s.eq.txt" % tag))
        r0 = _run(args + extra, o0)
        r1 = _run(args + extra + ["--quant", tsv, "--quant-classes", eqc], o1)
        h0, s0 = _body(o0, sam)
        h1, s1 = _body(o1, sam)
        assert h0 == h1 and (sam or np.array_equal(s0, s1)), tag
        assert sam or len(s0) > 100000
        # the classes
        sq, labels, counts = parse_eq_classes(open(eqc).read())
        assert sq == tx_names, tag
        assert labels == cl["labels"] and counts == cl["counts"], tag
        # the table: integers exact, floats as the API's print
        rows = parse_quant_tsv(open(tsv).read())
        uniq, ambig = unique_ambig(cl, tb["n_tx"])
        assert [r[0] for r in rows] == tx_names and [r[1] for r in rows] == tb["lens"].tolist(), tag
        assert [r[4] for r in rows] == uniq.tolist() and [r[5] for r in rows] == ambig.tolist(), tag
        assert [r[2] for r in rows] == ["%.6f" % v for v in res["theta"]], tag
        assert [r[3] for r in rows] == ["%.6f" % v for v in res["tpm"]], tag
        # the report
        out1 = r1.stdout.decode().split("\n")
        line = "[bramble] quantified %d read names in %d classes (%d iterations, " % (cl["n_names"], len(cl["labels"]), n_iters)
        assert sum(1 for l in out1 if l.startswith(line)) == 1, (tag, [l for l in out1 if "quantified" in l])
        assert not any("quantified" in l for l in r0.stdout.decode().split("\n"))
        assert _report(r1) == _report(r0) and len(_report(r1)) == 5, tag
        assert out1.index(next(l for l in out1 if l.startswith(line))) < out1.index("[bramble] final report:"), tag
        for p in (tsv, eqc, o1):
            assert not os.path.exists(p + ".tmp-bramble")
    # the length normalisation follows the preset unless told otherwise
    tb, cl = tb_in, classes_of(tb_in["tids"], tb_in["row_off"], tb_in["group_off"])
    flip = "--quant-length-norm" if lr else "--quant-no-length-norm"
    tsv = str(tmp_path / "flip.tsv")
    _run([in_bam] + extra + ["--quant", tsv, flip], str(tmp_path / "flip.bam"))
    res, _ = _api_result(tb, cl, 1 if lr else 0)
    assert [r[2] for r in parse_quant_tsv(open(tsv).read())] == ["%.6f" % v for v in res["theta"]]


def test_cli_quant_errors(tmp_path):
    annd, _, stream = _inputs("ont")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, _ = _files(tmp_path, annd, stream, "in")
    out = str(tmp_path / "o.bam")
    r = _run([in_bam, "-G", gtf, "--quant", str(tmp_path / "q.tsv"), "--devices", "0,0"], out, ok=False)
    assert r.returncode == 2 and b"--quant" in r.stderr and b"usage:" in r.stderr
    r = _run([in_bam, "-G", gtf, "--quant-classes", str(tmp_path / "c.txt")], out, ok=False)
    assert r.returncode == 2 and b"--quant" in r.stderr and b"usage:" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp-bramble")
    # a --quant path that cannot be written fails the run: no output, no temporary file
    bad = str(tmp_path / "no_such_dir" / "q.tsv")
    r = subprocess.run([BIN, in_bam, "-G", gtf, "--lr", "-o", out, "--quant", bad], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"q.tsv" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["g.gtf", "in.bam"]
