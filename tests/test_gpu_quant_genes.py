"""--quant-genes on the GPU: br_quant_genes' gene classes, counts, per-gene sums and gene bootstrap against the tests' restatement
of the definitions (test_quant_genes_cpu.py), never against the device's own gene output: the integer tables exactly, the doubles
bit for bit.  The device's transcript-level theta / tpm / effective lengths / replicates are inputs to the yardstick (the other
quant tests hold them to their references).  On the oracle's rows of the synthetic inputs under three maps, on hand-built tables
for the wave-sized and the large paths, with colliding hashes on purpose, in every order of the calls; what is refused; and the
command line.  One test holds the two levels to each other: the gene classes against finish on rows relabelled by gene."""
import functools
import os
import re

import numpy as np
import pytest

from bramble_amd import lib
from tests import bamio
from tests.test_gpu_collate import _files, _inputs, _report, _run
from tests.test_gpu_quant import _body, _fill, _new, _rows_a, _tables
from tests.test_gpu_quant_boot import _quant_of, _same_bits, _simple
from tests.test_quant_cpu import classes_of, oracle_tables, parse_eq_classes, unique_ambig
from tests.test_quant_genes_cpu import gene_boot, gene_classes_of, gene_maps, gene_result

pytestmark = pytest.mark.gpu

EM = {"max_iters": 32, "tolerance": 0}   # (the EM is an input here: a short one)
NORM = {"pe": 1, "ont": 0}


@functools.lru_cache(maxsize=None)
def _classes(mode):
    tb = _tables(mode)
    return classes_of(tb["tids"], tb["row_off"], tb["group_off"])


@functools.lru_cache(maxsize=None)
def _maps(mode):
    return gene_maps(mode, _tables(mode)["n_tx"])


def _gene_cl(q):
    off, labels, counts, first = q.gene_classes()
    return {"labels": [tuple(int(t) for t in labels[int(off[c]):int(off[c + 1])]) for c in range(q.n_gene_classes)],
            "counts": counts.tolist(), "first": first.tolist()}


def _assert_gene_classes(q, cl, tx_gene, n_genes):
    """classes (labels, counts, first, order), unique / ambig / n_transcripts against the yardstick -> the yardstick's classes"""
    want = gene_classes_of(cl, tx_gene)
    got = _gene_cl(q)
    assert q.n_gene_classes == len(want["labels"])
    assert got["labels"] == want["labels"] and got["counts"] == want["counts"] and got["first"] == want["first"]
    r = q.gene_result(em=False)
    uniq, ambig = unique_ambig(want, n_genes)
    assert np.array_equal(r["unique"], uniq) and np.array_equal(r["ambig"], ambig)
    assert np.array_equal(r["n_transcripts"], np.bincount(np.asarray(tx_gene, dtype=np.int64), minlength=n_genes)[:n_genes])
    assert q.gene_stats()["n_gene_labels"] == sum(len(s) for s in want["labels"])
    return want


def _assert_gene_sums(q, tx_gene, n_genes, lens, eff=None):
    """num_reads / tpm / length (/ eff_length) bits from the device's own theta and tpm"""
    t = q.result()
    want = gene_result(tx_gene, n_genes, t["theta"], t["tpm"], lens, eff)
    got = q.gene_result()
    for key in ("num_reads", "tpm", "length") + (("eff_length",) if eff is not None else ()):
        assert _same_bits(got[key], want[key]), key
    assert ("eff_length" in got) == (eff is not None)
    return got


def _assert_gene_boot(q, tx_gene, n_genes):
    rows, mean, var = gene_boot(tx_gene, n_genes, q.boot_theta())
    got = q.gene_boot()
    assert got.shape == rows.shape and _same_bits(got, rows)
    if q.bootstraps > 1:
        assert _same_bits(q.gene_boot(1, q.bootstraps - 1), rows[1:])
    gm, gv = q.gene_boot_summary()
    assert _same_bits(gm, mean) and _same_bits(gv, var)
    return got, gm, gv


# ---- the synthetic inputs under the three maps --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("which", ["own", "thirds", "random"])
def test_gene_tables_match_the_yardstick(mode, which):
    tb, cl = _tables(mode), _classes(mode)
    tx_gene, n_genes = _maps(mode)[which]
    q = _new(tb, length_norm=NORM[mode], **EM)
    _fill(q, tb, "host")
    q.finish()
    q.em()
    assert q.genes(tx_gene, n_genes) == len(gene_classes_of(cl, tx_gene)["labels"])
    _assert_gene_classes(q, cl, tx_gene, n_genes)
    got = _assert_gene_sums(q, tx_gene, n_genes, tb["lens"])
    owns = got["n_transcripts"] > 0   # (the random map leaves some genes without transcripts: all their results are 0)
    assert np.all(got["length"][owns] > 0) and not got["length"][~owns].any() and not got["num_reads"][~owns].any()
    assert abs(float(got["tpm"].sum()) - 1e6) < 1e-3
    assert q.gene_stats()["collisions"] == 0 and q.gene_stats()["seconds"] > 0
    q.close()


def test_effective_lengths_per_gene():
    tb = _tables("pe")
    tx_gene, n_genes = _maps("pe")["own"]
    q = _new(tb, eff_len=1, **EM)
    _fill(q, tb, "last_batch")   # (the whole row table: the fragments are counted)
    q.finish()
    q.em()
    q.genes(tx_gene, n_genes)
    eff = q.eff_lengths()
    assert np.any(eff != tb["lens"])
    got = _assert_gene_sums(q, tx_gene, n_genes, tb["lens"], eff)
    assert np.all(got["eff_length"] <= got["length"]) and np.any(got["eff_length"] < got["length"])
    q.close()


def test_identity_and_constant_maps():
    tb, cl = _tables("ont"), _classes("ont")
    n_tx = tb["n_tx"]
    q = _new(tb, length_norm=0, **EM)
    _fill(q, tb, "host")
    q.finish()
    q.em()
    q.genes(np.arange(n_tx, dtype=np.uint32), n_tx)
    off, labels, counts, first = q.classes()
    goff, glabels, gcounts, gfirst = q.gene_classes()
    assert np.array_equal(off, goff) and np.array_equal(labels, glabels) and np.array_equal(counts, gcounts) and np.array_equal(first, gfirst)
    t, g = q.result(), q.gene_result()
    assert np.array_equal(t["unique"], g["unique"]) and np.array_equal(t["ambig"], g["ambig"]) and np.all(g["n_transcripts"] == 1)
    assert _same_bits(t["theta"], g["num_reads"]) and _same_bits(t["tpm"], g["tpm"])
    m = t["tpm"] > 0
    assert np.array_equal(g["length"][~m], tb["lens"][~m].astype(np.float64))
    assert _same_bits(g["length"][m], t["tpm"][m] * tb["lens"][m].astype(np.float64) / t["tpm"][m])
    q.close()
    q = _new(tb, length_norm=0)
    _fill(q, tb, "host")
    q.finish()
    assert q.genes(np.zeros(n_tx, dtype=np.uint32), 1) == 1
    g = _gene_cl(q)
    n_labelled = cl["n_names"] - cl["n_unassigned"]
    assert g["labels"] == [(0,)] and g["counts"] == [n_labelled] and g["first"] == [cl["first"][0]]
    r = q.gene_result(em=False)
    assert r["unique"].tolist() == [n_labelled] and r["ambig"].tolist() == [0] and r["n_transcripts"].tolist() == [n_tx]
    q.close()


# ---- hand-built tables --------------------------------------------------------------------------------------------------------------
def _wide():
    """A class of 65 labels onto 65 genes (twice, through other transcripts: the two merge under lists a wave hashes), one of 130
    labels onto 2 genes, one of 64 onto 64, small names around them"""
    n_tx, n_genes = 700, 200
    tx_gene = np.full(n_tx, 199, dtype=np.uint32)
    tx_gene[0:65] = np.arange(65)
    tx_gene[400:465] = np.arange(65)[::-1]            # the same 65 genes, descending in t
    tx_gene[100:230] = 70 + (np.arange(130) % 2)
    tx_gene[300:364] = 100 + np.arange(64)
    tx_gene[600:610] = 70
    names = [[7], list(range(65)), [601, 100], list(range(100, 230)), list(range(300, 364)), [3, 5], list(range(400, 465)), [600, 101, 602],
             list(range(300, 364)), [405, 403], [650], [601]]
    return names, n_tx, tx_gene, n_genes


@pytest.mark.parametrize("bits", [64, 3, 1])
def test_wide_classes(bits):
    names, n_tx, tx_gene, n_genes = _wide()
    cl = classes_of(*_simple(names))
    q = _quant_of(names, n_tx, hash_bits=bits)
    q.genes(tx_gene, n_genes)
    want = _assert_gene_classes(q, cl, tx_gene, n_genes)
    assert sorted(len(s) for s in want["labels"])[-3:] == [2, 64, 65] and want["counts"][want["labels"].index(tuple(range(65)))] == 2
    assert (q.gene_stats()["collisions"] > 0) == (bits != 64)
    q.close()


@pytest.mark.parametrize("bits", [64, 1])
def test_gene_classes_are_finish_on_relabelled_rows(bits):
    """The defining property, device against device: the gene classes are what finish makes of the same names when every row's
    transcript id is its gene before the adds (the add drops the repeats inside a name).  Some names come twice or more, so
    the transcript classes that merge do not all count 1.  At hash_bits 1 both levels go through the collision repair."""
    names, n_tx, tx_gene, n_genes = _wide()
    names = names + [names[1], names[6], names[3], names[0], names[0], names[9]]
    a = _quant_of(names, n_tx, hash_bits=bits)
    assert max(a.classes()[2].tolist()) > 1
    a.genes(tx_gene, n_genes)
    b = _quant_of([[int(tx_gene[t]) for t in nm] for nm in names], n_genes, hash_bits=bits)
    assert a.n_gene_classes == b.n_classes
    for got, want in zip(a.gene_classes(), b.classes()):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    ga, tb = a.gene_result(em=False), b.result(em=False)
    assert np.array_equal(ga["unique"], tb["unique"]) and np.array_equal(ga["ambig"], tb["ambig"])
    assert a.gene_stats()["n_gene_labels"] == b.stats()["n_labels"]
    assert (a.gene_stats()["collisions"] > 0) == (b.stats()["collisions"] > 0) == (bits != 64)
    a.close()
    b.close()


def test_a_gene_of_200_transcripts():
    rng = np.random.RandomState(6)
    n_tx = 260
    tx_gene = np.concatenate([np.zeros(200, dtype=np.uint32), 1 + np.arange(60, dtype=np.uint32)])
    perm = rng.permutation(n_tx)
    tx_gene = tx_gene[perm]                         # the large gene's transcripts lie anywhere
    names = [sorted(set(rng.randint(0, n_tx, size=rng.randint(1, 5)).tolist())) for _ in range(3000)]
    lens = rng.randint(200, 5000, size=n_tx)
    tids, row_off, group_off = _simple(names)
    q = lib.Quant(n_tx, lens)
    for k, v in dict(EM, bootstraps=3, boot_seed=9).items():
        q.set_param(k, v)
    q.add_host(_rows_a(tids), row_off, group_off)
    q.finish()
    q.em()
    q.bootstrap()
    q.genes(tx_gene, 61)
    _assert_gene_classes(q, classes_of(tids, row_off, group_off), tx_gene, 61)
    got = _assert_gene_sums(q, tx_gene, 61, lens)
    assert got["num_reads"][0] > 1000   # 200 terms of different sizes: their order shows in the last bits
    _assert_gene_boot(q, tx_gene, 61)
    q.close()


def test_many_classes_into_few():
    n_tx = 70000
    t = np.arange(n_tx)
    tx_gene = np.where(t < 66000, 0, 1 + t % 6).astype(np.uint32)
    rng = np.random.RandomState(2)
    names = [[int(v)] for v in rng.permutation(n_tx)] + [[int(v)] for v in rng.randint(0, n_tx, size=500)]
    cl = classes_of(*_simple(names))
    assert len(cl["labels"]) == n_tx
    q = _quant_of(names, n_tx)
    assert q.genes(tx_gene, 7) == 7
    want = _assert_gene_classes(q, cl, tx_gene, 7)
    assert max(want["counts"]) > (1 << 16) and sum(want["counts"]) == len(names)
    q.close()


@pytest.mark.parametrize("names", [[], [[], [], []]], ids=["no names", "all unassigned"])
def test_no_named_reads(names):
    q = _quant_of(names, 6, bootstraps=2, **EM)
    tx_gene = np.asarray([2, 0, 0, 3, 2, 2], dtype=np.uint32)
    assert q.genes(tx_gene, 5) == 0
    off, labels, counts, first = q.gene_classes()
    assert off.tolist() == [0] and len(labels) == len(counts) == len(first) == 0
    q.em()
    q.bootstrap()
    r = q.gene_result()
    assert r["n_transcripts"].tolist() == [2, 0, 3, 1, 0]
    assert not r["unique"].any() and not r["ambig"].any() and not r["num_reads"].any() and not r["tpm"].any()
    assert not q.gene_boot().any() and not q.gene_boot_summary()[0].any() and not q.gene_boot_summary()[1].any()
    q.close()


# ---- colliding hashes change nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 3])
def test_hash_collisions_change_nothing(bits):
    tb, cl = _tables("pe"), _classes("pe")
    tx_gene, n_genes = _maps("pe")["own"]
    q = _new(tb, hash_bits=bits)
    _fill(q, tb, "host")
    q.finish()
    q.genes(tx_gene, n_genes)
    _assert_gene_classes(q, cl, tx_gene, n_genes)
    assert q.gene_stats()["collisions"] > 0
    q.close()


# ---- the order of the calls ---------------------------------------------------------------------------------------------------------
def _everything(q):
    off, labels, counts, first = q.gene_classes()
    r = q.gene_result()
    m, v = q.gene_boot_summary()
    t = q.result()
    return ([off, labels, counts, first, r["unique"], r["ambig"], r["n_transcripts"]],
            [r["num_reads"], r["tpm"], r["length"], q.gene_boot(), m, v, t["theta"], t["tpm"], q.boot_theta()])


@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_order_of_the_calls(mode):
    tb = _tables(mode)
    tx_gene, n_genes = _maps(mode)["thirds"]
    runs = []
    for how, order in (("dev1", "geb"), ("dev3", "egb"), ("host", "ebg"), ("dev1", "bge"), ("dev1", "geb")):
        q = _new(tb, length_norm=NORM[mode], bootstraps=3, boot_seed=5, **EM)
        _fill(q, tb, how)
        q.finish()
        point = None
        for step in order:
            if step == "g":
                before = (q.classes(), q.result(em=False))
                q.genes(tx_gene, n_genes)
                after = (q.classes(), q.result(em=False))   # the transcript tables are untouched
                assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
                assert all(np.array_equal(before[1][k], after[1][k]) for k in before[1])
                if point is not None:
                    assert _same_bits(q.result()["theta"], point)
            elif step == "e":
                q.em()
                point = q.result()["theta"]
            else:
                q.bootstrap()
        runs.append(_everything(q))
        q.close()
    for ints, floats in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0][0], ints))
        assert all(_same_bits(a, b) for a, b in zip(runs[0][1], floats))


# ---- the gene bootstrap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_boot,chunk", [(5, 2), (1, 0)])
def test_gene_bootstrap(n_boot, chunk):
    tb = _tables("pe")
    tx_gene, n_genes = _maps("pe")["own"]
    q = _new(tb, bootstraps=n_boot, boot_seed=3, boot_chunk=chunk, **EM)
    _fill(q, tb, "host")
    q.finish()
    q.genes(tx_gene, n_genes)
    q.bootstrap()
    rows, mean, var = _assert_gene_boot(q, tx_gene, n_genes)
    assert rows.shape == (n_boot, n_genes)
    if n_boot == 1:
        assert not var.any() and _same_bits(mean, rows[0])
    else:   # isoforms inside a gene move against each other: the gene's variance is not the sum of theirs
        tv = np.bincount(tx_gene.astype(np.int64), weights=q.boot_summary()[1], minlength=n_genes)
        assert np.any(var < 0.9 * tv) and var.any()
    q.close()


# ---- what is refused ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = lib.lib()
    tb = _tables("ont")
    n_tx = tb["n_tx"]
    tx_gene, n_genes = _maps("ont")["own"]
    buf = np.zeros(max(n_tx, n_genes) * 8, dtype=np.float64)
    q = _new(tb, length_norm=0, bootstraps=2, **EM)
    _fill(q, tb, "host")
    assert q.genes_raw(tx_gene.ctypes.data, n_genes) == -1                       # before finish
    q.finish()
    for f in (lambda: L.br_quant_gene_classes(q.h, None, None, None, None), lambda: L.br_quant_gene_result(q.h, None, None, None, None, None, None, None),
              lambda: L.br_quant_gene_boot(q.h, 0, 0, None), lambda: L.br_quant_gene_boot_summary(q.h, None, None)):
        assert f() == -1                                                         # before br_quant_genes
    before = (q.classes(), q.result(em=False))
    bad = tx_gene.copy()
    bad[n_tx // 2] = n_genes                                                     # an entry equal to n_genes
    assert q.genes_raw(bad.ctypes.data, n_genes) == -1
    bad[n_tx // 2] = 0xffffffff
    assert q.genes_raw(bad.ctypes.data, n_genes) == -1
    assert q.genes_raw(None, n_genes) == -1                                      # a NULL map with transcripts
    assert q.genes_raw(tx_gene.ctypes.data, -1) == -1 and q.genes_raw(tx_gene.ctypes.data, 1 << 32) == -1
    assert q.genes_raw(tx_gene.ctypes.data, int(tx_gene.max())) == -1            # n_genes one short
    after = (q.classes(), q.result(em=False))
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and all(np.array_equal(before[1][k], after[1][k]) for k in before[1])
    q.genes(tx_gene, n_genes)                                                    # (the refusals left it ready for the call)
    want = _assert_gene_classes(q, _classes("ont"), tx_gene, n_genes)
    assert q.genes_raw(tx_gene.ctypes.data, n_genes) == -1                       # a second call
    assert _gene_cl(q)["labels"] == want["labels"]
    for k in (1, 2, 3):                                                          # num_reads / tpm / length before the EM
        args = [None] * 7
        args[k - 1] = buf.ctypes.data
        assert L.br_quant_gene_result(q.h, *args) == -1
    assert L.br_quant_gene_result(q.h, None, None, None, None, buf.ctypes.data, None, None) == 0
    assert L.br_quant_gene_boot(q.h, 0, 1, buf.ctypes.data) == -1 and L.br_quant_gene_boot_summary(q.h, buf.ctypes.data, None) == -1   # before the bootstrap
    q.em()
    assert L.br_quant_gene_result(q.h, None, None, None, buf.ctypes.data, None, None, None) == -1   # eff_length without "eff_len"
    _assert_gene_sums(q, tx_gene, n_genes, tb["lens"])
    q.bootstrap()
    assert L.br_quant_gene_boot(q.h, 1, 2, buf.ctypes.data) == -1 and L.br_quant_gene_boot(q.h, -1, 1, buf.ctypes.data) == -1
    assert L.br_quant_gene_boot(q.h, 0, 2, None) == 0 and L.br_quant_gene_boot_summary(q.h, None, None) == 0   # every out-pointer may be NULL
    _assert_gene_boot(q, tx_gene, n_genes)
    _assert_gene_classes(q, _classes("ont"), tx_gene, n_genes)
    q.close()


# ---- command line -------------------------------------------------------------------------------------------------------------------
def _parse_genes_tsv(text, eff, boot):
    head = ["Name", "Length"] + (["EffectiveLength"] if eff else []) + ["NumReads", "TPM", "UniqueReads", "AmbigReads", "NumTranscripts"] + (["BootMean", "BootSD"] if boot else [])
    lines = text.split("\n")
    assert lines[0] == "\t".join(head) and lines[-1] == ""
    rows = [dict(zip(head, l.split("\t"))) for l in lines[1:-1]]
    assert all(len(l.split("\t")) == len(head) for l in lines[1:-1])
    return rows


def _gene_numbers(names):
    """genes numbered in order of first appearance"""
    number = {}
    for g in names:
        number.setdefault(g, len(number))
    return np.asarray([number[g] for g in names], dtype=np.uint32), list(number)


@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_cli_quant_genes(tmp_path, mode):
    annd, recs, stream = _inputs(mode)
    lr = ["--lr"] if mode == "ont" else []
    own = _maps(mode)["own"][0]
    gene_of_id = {t["id"]: "gene%d" % own[k] for k, t in enumerate(annd["transcripts"])}
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    text = re.sub(r'gene_id "g_(tx\d+)"', lambda m: 'gene_id "%s"' % gene_of_id[m.group(1)], open(gtf).read())
    open(gtf, "w").write(text)
    in_bam, _ = _files(tmp_path, annd, stream, "in")
    tb = oracle_tables(mode, guide_order=True)   # (the command line numbers the transcripts in guide order)
    tx_names = [t["id"] for t in tb["annd"]["transcripts"]]
    tx_gene, gene_names = _gene_numbers([gene_of_id[n] for n in tx_names])
    n_genes = len(gene_names)
    base = [in_bam, "-G", gtf] + lr

    def api(eff, n_boot):
        q = _new(tb, length_norm=NORM[mode], **(dict(eff_len=1) if eff else {}), **(dict(bootstraps=n_boot) if n_boot else {}))
        _fill(q, tb, "last_batch" if eff else "host")
        q.finish()
        n_iters = q.em()[0]
        if n_boot:
            q.bootstrap()
        q.genes(tx_gene, n_genes)
        out = (q.gene_result(), _gene_cl(q), q.gene_boot_summary() if n_boot else None, n_iters)
        q.close()
        return out

    def check(rows, res, summary, eff):
        assert [r["Name"] for r in rows] == gene_names
        assert [r["Length"] for r in rows] == ["%.3f" % v for v in res["length"]]
        assert [r["NumReads"] for r in rows] == ["%.6f" % v for v in res["num_reads"]] and [r["TPM"] for r in rows] == ["%.6f" % v for v in res["tpm"]]
        assert [int(r["UniqueReads"]) for r in rows] == res["unique"].tolist() and [int(r["AmbigReads"]) for r in rows] == res["ambig"].tolist()
        assert [int(r["NumTranscripts"]) for r in rows] == res["n_transcripts"].tolist()
        if eff:
            assert [r["EffectiveLength"] for r in rows] == ["%.3f" % v for v in res["eff_length"]]
        if summary:
            assert [r["BootMean"] for r in rows] == ["%.6f" % v for v in summary[0]] and [r["BootSD"] for r in rows] == ["%.6f" % v for v in np.sqrt(summary[1])]

    res, gcl, _, n_iters = api(False, 0)
    assert gcl == {k: gene_classes_of(classes_of(tb["tids"], tb["row_off"], tb["group_off"]), tx_gene)[k] for k in ("labels", "counts", "first")}
    f = {k: str(tmp_path / k) for k in ("q0.tsv", "c0.txt", "o0.bam", "q1.tsv", "c1.txt", "o1.bam", "g1.tsv", "gc1.txt", "q2.tsv", "c2.txt", "o2.bam", "g2.tsv",
                                       "gc2.txt", "map.tsv", "q3.tsv", "o3.bam", "g3.tsv")}
    r0 = _run(base + ["--quant", f["q0.tsv"], "--quant-classes", f["c0.txt"]], f["o0.bam"])
    r1 = _run(base + ["--quant", f["q1.tsv"], "--quant-classes", f["c1.txt"], "--quant-genes", f["g1.tsv"], "--quant-gene-classes", f["gc1.txt"]], f["o1.bam"])
    # everything there was is byte-identical (the BAM but for the @PG line that holds the command line)
    assert open(f["q0.tsv"], "rb").read() == open(f["q1.tsv"], "rb").read() and open(f["c0.txt"], "rb").read() == open(f["c1.txt"], "rb").read()
    h0, s0 = _body(f["o0.bam"], False)
    h1, s1 = _body(f["o1.bam"], False)
    assert h0 == h1 and np.array_equal(s0, s1)
    # the report differs by exactly the one new line, in front of the quantified line
    drop = re.compile(r"\d+\.\d+s")   # (the seconds)
    out0 = [drop.sub("", l) for l in r0.stdout.decode().split("\n")]
    out1 = [drop.sub("", l) for l in r1.stdout.decode().split("\n")]
    new = [l for l in out1 if l.startswith("[bramble] gene level: ")]
    assert new == ["[bramble] gene level: %d genes, %d classes ()" % (n_genes, len(gcl["labels"]))]
    k = out1.index(new[0])
    assert out1[:k] + out1[k + 1:] == out0 and out1[k + 1].startswith("[bramble] quantified %d read names" % tb_names(tb))
    assert _report(r1) == _report(r0)
    # the two new files parse back to the API's values
    check(_parse_genes_tsv(open(f["g1.tsv"]).read(), False, False), res, None, False)
    names, labels, counts = parse_eq_classes(open(f["gc1.txt"]).read())
    assert names == gene_names and labels == gcl["labels"] and counts == gcl["counts"]
    # a map that restates the GTF's genes (with a comment, an empty line, a further column and a transcript the run does not know)
    open(f["map.tsv"], "w").write("# tx2gene\n\n" + "".join("%s\t%s\tx\n" % (n, gene_of_id[n]) for n in reversed(tx_names)) + "unknown_tx\tgeneX\n")
    _run(base + ["--quant", f["q2.tsv"], "--quant-classes", f["c2.txt"], "--quant-genes", f["g2.tsv"], "--quant-gene-classes", f["gc2.txt"], "--quant-gene-map", f["map.tsv"]],
         f["o2.bam"])
    for a, b in (("g1.tsv", "g2.tsv"), ("gc1.txt", "gc2.txt"), ("q1.tsv", "q2.tsv"), ("c1.txt", "c2.txt")):
        assert open(f[a], "rb").read() == open(f[b], "rb").read(), a
    if mode == "pe":   # the optional columns
        res, _, summary, _ = api(True, 4)
        _run(base + ["--quant", f["q3.tsv"], "--quant-genes", f["g3.tsv"], "--quant-eff-length", "--quant-bootstraps", "4"], f["o3.bam"])
        check(_parse_genes_tsv(open(f["g3.tsv"]).read(), True, True), res, summary, True)
    assert not any(n.endswith(".tmp-bramble") for n in os.listdir(str(tmp_path)))


def tb_names(tb):
    return len(tb["group_off"]) - 1
