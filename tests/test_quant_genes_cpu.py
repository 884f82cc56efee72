"""--quant-genes without a GPU: the tests' own restatement of the gene-level definitions in bramble_amd.h (br_quant) -- the gene
classes of transcript classes, unique / ambiguous names per gene, the gene abundances and lengths, the gene bootstrap -- which the
GPU tests compare the device against; the defining property on the oracle's rows (relabelling the classes by gene is relabelling
the rows before the adds); cases worked out by hand; the guide loader's gene ids; the ABI without a device and the usage errors."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests.test_quant_boot_cpu import boot_summary
from tests.test_quant_cpu import classes_of, oracle_tables, unique_ambig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bramble_amd", "bin", "bramble")
SYNTH = {"pe": (500, 3), "ont": (300, 2)}   # (genes, references) of tests.test_gpu_collate._inputs


# ---- the yardsticks -----------------------------------------------------------------------------------------------------------
def gene_classes_of(cl, tx_gene):
    """cl: classes_of's dict -> the same dict of the gene classes: every class's labels mapped, the sorted set, classes of equal
    sets merged (counts summed, the smallest first), in the order of first"""
    index, labels, counts, first = {}, [], [], []
    for s, n, f in zip(cl["labels"], cl["counts"], cl["first"]):
        gs = tuple(sorted(set(int(tx_gene[t]) for t in s)))
        if gs not in index:
            index[gs] = len(labels)
            labels.append(gs)
            counts.append(0)
            first.append(f)
        k = index[gs]
        counts[k] += n
        first[k] = min(first[k], f)
    order = sorted(range(len(labels)), key=lambda k: first[k])
    return {"labels": [labels[k] for k in order], "counts": [counts[k] for k in order], "first": [first[k] for k in order],
            "n_names": cl.get("n_names"), "n_unassigned": cl.get("n_unassigned")}


def gene_sums(tx_gene, n_genes, v):
    """per gene the sum of v over its transcripts, one after the other in ascending transcript order (np.bincount adds its weights
    one by one in input order)"""
    return np.bincount(np.asarray(tx_gene, dtype=np.int64), weights=np.asarray(v, dtype=np.float64), minlength=n_genes)[:n_genes] if n_genes else np.zeros(0)


def gene_result(tx_gene, n_genes, theta, tpm, lens=None, eff=None):
    """-> dict num_reads, tpm, length, eff_length (None without eff), n_transcripts"""
    tx_gene = np.asarray(tx_gene, dtype=np.int64)
    n_tx = np.bincount(tx_gene, minlength=n_genes)[:n_genes].astype(np.uint32) if n_genes else np.zeros(0, dtype=np.uint32)
    g_tpm = gene_sums(tx_gene, n_genes, tpm)

    def mean_len(l):
        if l is None:
            return np.zeros(n_genes)
        l = np.asarray(l).astype(np.float64)
        weighted = gene_sums(tx_gene, n_genes, np.asarray(tpm, dtype=np.float64) * l)   # each product rounded, then added
        plain = gene_sums(tx_gene, n_genes, l)
        out = np.zeros(n_genes)
        for g in range(n_genes):
            if n_tx[g]:
                out[g] = weighted[g] / g_tpm[g] if g_tpm[g] > 0 else plain[g] / np.float64(n_tx[g])
        return out
    return {"num_reads": gene_sums(tx_gene, n_genes, theta), "tpm": g_tpm, "length": mean_len(lens),
            "eff_length": None if eff is None else mean_len(eff), "n_transcripts": n_tx}


def gene_boot(tx_gene, n_genes, boot_theta):
    """boot_theta [B, T] -> ([B, G], mean, var)"""
    rows = np.asarray([gene_sums(tx_gene, n_genes, r) for r in boot_theta]).reshape(len(boot_theta), n_genes)
    return (rows,) + boot_summary(rows)


def gene_maps(mode, n_tx):
    """the three maps of the tests: the synthetic annotation's own genes, t // 3, a seeded random map onto T // 4 genes"""
    from bramble_amd import synth
    own = synth.Annotation("G", n_genes=SYNTH[mode][0], n_refs=SYNTH[mode][1]).flat["tx_gene"].astype(np.uint32)
    assert len(own) == n_tx
    rnd = np.random.RandomState(17).randint(0, n_tx // 4, size=n_tx).astype(np.uint32)
    assert np.any(np.diff(rnd.astype(np.int64)) < 0)   # not monotone in t
    return {"own": (own, int(own.max()) + 1), "thirds": ((np.arange(n_tx) // 3).astype(np.uint32), (n_tx + 2) // 3), "random": (rnd, n_tx // 4)}


# ---- the defining property ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_gene_classes_are_the_classes_of_relabelled_rows(mode):
    tb = oracle_tables(mode)
    cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    for name, (tx_gene, n_genes) in gene_maps(mode, tb["n_tx"]).items():
        got = gene_classes_of(cl, tx_gene)
        want = classes_of(tx_gene[tb["tids"]], tb["row_off"], tb["group_off"])
        assert got == want
        assert max(max(s) for s in got["labels"]) < n_genes
        collapse = sum(1 for s in cl["labels"] if len(s) > 1 and len(set(int(tx_gene[t]) for t in s)) == 1)
        merged = len(cl["labels"]) - len(got["labels"])
        print("%s, %s map: %d classes -> %d gene classes, %d multi-label classes collapse to one gene" % (mode, name, len(cl["labels"]), len(got["labels"]), collapse))
        if name == "own":   # what the feature is about is in the input
            assert collapse >= 1 and merged >= 2
        uniq, ambig = unique_ambig(got, n_genes)
        assert int(uniq.sum()) == sum(n for s, n in zip(got["labels"], got["counts"]) if len(s) == 1)
        assert sum(got["counts"]) == sum(cl["counts"])


# ---- cases worked out by hand ---------------------------------------------------------------------------------------------------
def test_ambiguous_among_isoforms_is_unique_at_the_gene():
    cl = {"labels": [(0, 1), (2,)], "counts": [5, 1], "first": [0, 3]}
    g = gene_classes_of(cl, [0, 0, 1])
    assert g["labels"] == [(0,), (1,)] and g["counts"] == [5, 1] and g["first"] == [0, 3]
    uniq, ambig = unique_ambig(g, 2)
    assert uniq.tolist() == [5, 1] and ambig.tolist() == [0, 0]
    tu, ta = unique_ambig(cl, 3)
    assert tu.tolist() == [0, 0, 1] and ta.tolist() == [5, 5, 0]


def test_two_classes_merge_and_first_is_the_smaller():
    cl = {"labels": [(3,), (0, 1), (0, 2), (1, 2)], "counts": [2, 4, 8, 16], "first": [0, 1, 5, 9]}
    g = gene_classes_of(cl, [0, 1, 1, 2])   # {0,1} -> {0,1}; {0,2} -> {0,1}; {1,2} -> {1}
    assert g["labels"] == [(2,), (0, 1), (1,)] and g["counts"] == [2, 12, 16] and g["first"] == [0, 1, 9]
    # a later class with the smaller first name cannot occur in finish's order, but the definition says min: it holds then too
    g = gene_classes_of({"labels": [(0,), (1,)], "counts": [1, 1], "first": [7, 2]}, [0, 0])
    assert g["first"] == [2] and g["counts"] == [2]


def test_a_descending_map():
    cl = {"labels": [(0, 1, 2), (2,)], "counts": [3, 1], "first": [0, 1]}
    g = gene_classes_of(cl, [2, 1, 0])
    assert g["labels"] == [(0, 1, 2), (0,)]   # labels ascend inside a class whatever the map does
    r = gene_result([2, 1, 0], 3, [1.0, 2.0, 4.0], [10.0, 20.0, 40.0], [100, 200, 300])
    assert r["num_reads"].tolist() == [4.0, 2.0, 1.0] and r["length"].tolist() == [300.0, 200.0, 100.0]


def test_an_unused_gene_and_the_length_fallback():
    #                gene 0: transcripts 0 and 2, tpm 0: the plain mean; gene 1: nobody; gene 2: transcripts 1 and 3
    r = gene_result([0, 2, 0, 2], 3, [0.0, 1.0, 0.0, 3.0], [0.0, 250000.0, 0.0, 750000.0], [100, 1000, 301, 2000], eff=[50.0, 900.0, 250.0, 1900.0])
    assert r["n_transcripts"].tolist() == [2, 0, 2]
    assert r["num_reads"].tolist() == [0.0, 0.0, 4.0] and r["tpm"].tolist() == [0.0, 0.0, 1e6]
    assert r["length"].tolist() == [200.5, 0.0, (250000.0 * 1000 + 750000.0 * 2000) / 1e6]
    assert r["eff_length"].tolist() == [150.0, 0.0, (250000.0 * 900 + 750000.0 * 1900) / 1e6]
    assert not gene_result([0, 2, 0, 2], 3, [1.0] * 4, [1.0] * 4)["length"].any()   # a quantifier without lengths
    g = gene_classes_of({"labels": [(1,), (0, 3)], "counts": [1, 2], "first": [0, 1]}, [0, 2, 0, 2])
    uniq, ambig = unique_ambig(g, 3)
    assert uniq.tolist() == [0, 0, 1] and ambig.tolist() == [2, 0, 2]


def test_sums_run_in_ascending_transcript_order():
    v = [1e16, 1.0, -1e16, 1.0]
    assert gene_sums([0, 0, 0, 0], 1, v).tolist() == [((1e16 + 1.0) - 1e16) + 1.0] == [1.0]
    assert gene_sums([0, 1, 0, 1], 2, v).tolist() == [0.0, 2.0]


def test_gene_bootstrap_by_hand():
    theta = np.asarray([[1.0, 2.0, 4.0], [3.0, 2.0, 0.0], [2.0, 2.0, 2.0]])
    rows, mean, var = gene_boot([1, 0, 1], 2, theta)
    assert rows.tolist() == [[2.0, 5.0], [2.0, 3.0], [2.0, 4.0]]
    assert mean.tolist() == [2.0, 4.0] and var.tolist() == [0.0, 1.0]   # the isoforms vary, the gene's sum does not
    rows, mean, var = gene_boot([1, 0, 1], 2, theta[:1])
    assert mean.tolist() == [2.0, 5.0] and var.tolist() == [0.0, 0.0]   # B = 1


# ---- the guide loader's gene ids ------------------------------------------------------------------------------------------------
def _genes(path, threads=None):
    from bramble_amd import lib
    a = lib.load_annotation(str(path), threads)
    return {t["id"]: g for t, g in zip(a["transcripts"], a["gene_ids"])}, [t["id"] for t in a["transcripts"]]


def _gtf(ref, feature, s, e, attrs):
    return "\t".join([ref, "x", feature, str(s), str(e), ".", "+", ".", attrs]) + "\n"


def test_loader_gtf_gene_ids(tmp_path):
    p = tmp_path / "a.gtf"
    p.write_text(
        _gtf("chr1", "gene", 10, 900, 'gene_id "gA";')
        + _gtf("chr1", "transcript", 10, 500, 'gene_id "gA"; transcript_id "t1";')           # from the transcript line
        + _gtf("chr1", "exon", 10, 500, 'gene_id "other"; transcript_id "t1";')              # (a later line does not change it)
        + _gtf("chr1", "exon", 2000, 2100, 'transcript_id "t2"; gene_id "gB";')              # from exon lines only
        + _gtf("chr1", "exon", 2200, 2300, 'transcript_id "t2"; gene_id "gB";')
        + _gtf("chr1", "exon", 5000, 5100, 'transcript_id "t4";')                            # no gene_id on the first line
        + _gtf("chr1", "exon", 5200, 5300, 'gene_id "gD"; transcript_id "t4";')              # the first line that has one
        + _gtf("chr2", "exon", 10, 50, 'transcript_id "t5"; gene_id "";')                    # nothing non-empty: its own id
        + _gtf("chr1", "exon", 600, 900, 'gene_id "gA"; transcript_id "t3";'))               # gA again, far apart in the file
    genes, order = _genes(p)
    assert genes == {"t1": "gA", "t2": "gB", "t3": "gA", "t4": "gD", "t5": "t5"}
    assert order == ["t1", "t3", "t2", "t4", "t5"]   # the order is the loader's, whatever the genes are


def test_loader_gff3_gene_ids(tmp_path):
    def line(feature, s, e, attrs):
        return "\t".join(["chr1", "x", feature, str(s), str(e), ".", "+", ".", attrs]) + "\n"
    p = tmp_path / "a.gff3"
    p.write_text(
        "##gff-version 3\n"
        + line("gene", 10, 900, "ID=gene1")
        + line("mRNA", 10, 500, "ID=r1;Parent=gene1;gene_id=G1")          # gene_id= wins over Parent=
        + line("exon", 10, 500, "Parent=r1")
        + line("mRNA", 600, 900, "ID=r2;Parent=gene1,gene9")              # Parent= only: its first entry
        + line("exon", 600, 900, "Parent=r2")
        + line("mRNA", 2000, 2500, "ID=r3")                               # neither: its own id
        + line("exon", 2000, 2500, "Parent=r3")
        + line("exon", 3000, 3100, "Parent=r4")                           # exon lines only: its own id
        + line("exon", 4000, 4100, "Parent=r5;gene_id=G5")                # ... unless they carry a gene_id
        + line("mRNA", 5000, 5100, "ID=r6;Parent=gene1")
        + line("exon", 5000, 5100, "Parent=r6;gene_id=G6"))               # an exon line's gene_id beats the transcript line's parent
    genes, _ = _genes(p)
    assert genes == {"r1": "G1", "r2": "gene1", "r3": "r3", "r4": "r4", "r5": "G5", "r6": "G6"}


def test_loader_gzip_and_thread_count(tmp_path):
    rng = np.random.RandomState(4)
    lines, want = [], {}
    for k in range(3000):
        tid, gid = "t%d" % k, "g%d" % rng.randint(0, 700)
        want[tid] = gid
        s = 100 + 50 * k
        with_gene_on_first = k % 3 != 0
        lines.append(_gtf("chr%d" % (k % 4), "exon", s, s + 20, 'transcript_id "%s";%s' % (tid, ' gene_id "%s";' % gid if with_gene_on_first else "")))
        lines.append(_gtf("chr%d" % (k % 4), "exon", s + 30, s + 40, 'gene_id "%s"; transcript_id "%s";' % (gid, tid)))
    plain, packed = tmp_path / "a.gtf", tmp_path / "a.gtf.gz"
    plain.write_text("".join(lines))
    with gzip.open(str(packed), "wb") as f:
        f.write("".join(lines).encode())
    one, order1 = _genes(plain, 1)
    assert one == want
    for path, threads in ((plain, 8), (packed, 1), (packed, 8), (plain, None)):
        got, order = _genes(path, threads)
        assert got == want and order == order1


# ---- ABI and usage errors -------------------------------------------------------------------------------------------------------
def test_gene_abi_without_a_device():
    from bramble_amd import lib
    L = lib.lib()
    names = ("br_quant_genes", "br_quant_gene_classes", "br_quant_gene_result", "br_quant_gene_boot", "br_quant_gene_boot_summary",
             "br_quant_gene_stats", "br_annotation_gene_ids")
    for name in names:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    P = C.c_void_p
    L.br_quant_genes.argtypes = [P, P, C.c_int64, P]
    L.br_quant_gene_classes.argtypes = [P] * 5
    L.br_quant_gene_result.argtypes = [P] * 8
    L.br_quant_gene_boot.argtypes = [P, C.c_int32, C.c_int32, P]
    L.br_quant_gene_boot_summary.argtypes = [P] * 3
    L.br_quant_gene_stats.argtypes = [P] * 4
    L.br_annotation_gene_ids.restype, L.br_annotation_gene_ids.argtypes = P, [P]
    assert L.br_quant_genes(None, None, 0, None) == -1 and L.br_quant_gene_classes(None, None, None, None, None) == -1
    assert L.br_quant_gene_result(None, None, None, None, None, None, None, None) == -1
    assert L.br_quant_gene_boot(None, 0, 0, None) == -1 and L.br_quant_gene_boot_summary(None, None, None) == -1
    assert L.br_quant_gene_stats(None, None, None, None) == -1
    assert L.br_annotation_gene_ids(None) is None


def _cli(tmp_path, extra):
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\nchr1\tx\texon\t10\t700\t.\t+\t.\tgene_id "g"; transcript_id "t2";\n')
    extra = [str(tmp_path / e) if e.endswith((".txt", ".tsv")) else e for e in extra]
    return subprocess.run([BIN, str(tmp_path / "missing.bam"), "-G", str(gtf), "-o", str(tmp_path / "o.bam")] + extra, capture_output=True, timeout=60)


@pytest.mark.parametrize("extra,word", [
    (["--quant-genes", "g.tsv"], b"--quant"),
    (["--quant", "q.tsv", "--quant-gene-classes", "c.txt"], b"--quant-genes"),
    (["--quant", "q.tsv", "--quant-gene-map", "m.tsv"], b"--quant-genes"),
    (["--quant-genes", "g.tsv", "--quant-gene-classes", "c.txt", "--quant-gene-map", "m.tsv"], b"--quant"),
    (["--quant", "q.tsv", "--quant-genes"], b"--quant-genes"),
])
def test_cli_gene_usage_errors(tmp_path, extra, word):
    r = _cli(tmp_path, extra)
    assert r.returncode == 2
    assert word in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]


def test_cli_gene_map_that_lacks_a_transcript(tmp_path):
    (tmp_path / "m.tsv").write_text("# tx2gene\n\nt1\tgeneA\tmore\nt9\tgeneZ\n")
    r = _cli(tmp_path, ["--quant", "q.tsv", "--quant-genes", "g.tsv", "--quant-gene-map", "m.tsv"])
    assert r.returncode == 2
    assert b"t2" in r.stderr and b"--quant-gene-map" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["g.gtf", "m.tsv"]   # raised before any output is written
    r = _cli(tmp_path, ["--quant", "q.tsv", "--quant-genes", "g.tsv", "--quant-gene-map", "none.tsv"])
    assert r.returncode == 2 and b"none.tsv" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["g.gtf", "m.tsv"]


def test_usage_names_the_switches():
    r = subprocess.run([BIN, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0
    for w in (b"--quant-genes", b"--quant-gene-classes", b"--quant-gene-map", b"gene level:"):
        assert w in r.stdout
