"""The fixed-seed full-alphabet batches (tests/adversarial.py) that tests/test_gpu_cigar_alphabet.py compares with the
oracle, kept apart from that file so that tests/test_cigar_alphabet_cpu.py can check on the CPU, with the oracle alone,
that they are worth running: enough reads with rows, enough paired rows, every CIGAR op in the output, and every
merge_ops cell a large sweep of the generator reaches."""
import functools

import numpy as np

from tests import adversarial as adv

PRESETS = {"default": {}, "strict": {"strict": 1}, "fr": {"fr": 1}, "rf": {"rf": 1}, "lr": {"lr": 1}, "lr_hq": {"lr_hq": 1},
           "override": {"max_clip": 2, "max_junc_ins": 3, "max_junc_gap": 3}}
SHORT = ("default", "strict", "fr", "rf", "override")
LONG = ("lr", "lr_hq")
# the read mix of the -S batches: most reads clipped, the clips long enough to be rescued (5 bases and more), and a padded,
# busy tail in most reads -- the merge cells (real M D P = X, override op) are reached by nothing else
RESCUE_MIX = {"p_clip": 0.8, "p_tail_pad": 0.6, "p_long_clip": 0.9}


def family(flags):
    """route family of a parametrisation: the -S rescue, the similarity-filter presets (match table), the rest"""
    if flags.get("use_fasta"):
        return "rescue"
    return "long" if flags.get("lr") or flags.get("lr_hq") else "short"


def dense_annotation():
    """the dense locus of tests/test_gpu_pairing_dense.py: 150 isoforms on each strand share two exons, so a read there
    has more than 64 candidate rows (k_big)"""
    from tests.test_gpu_pairing_dense import annotation
    return annotation()


@functools.lru_cache(maxsize=None)
def _annotation(kind, genome):
    if kind == "dense":
        ann = dense_annotation()
        if genome:
            rng = np.random.RandomState(17)
            size = max(e[1] for t in ann["transcripts"] for e in t["exons"]) + 200
            ann["ref_seqs"] = {0: "".join("ACGT"[int(x)] for x in rng.randint(0, 4, size=size))}
        return ann
    return adv.annotation(11, n_genes=40, with_genome=genome)


@functools.lru_cache(maxsize=None)
def _records(kind, mode, n, seed, orient, genome, alphabet):
    ann = _annotation(kind, genome)
    if mode == "near":      # the light-class near misses with ordinary pairs of the same generator behind them
        return adv.near_misses(ann, seed, alphabet=alphabet, orient=orient) + \
            adv.reads(ann, n, "pe", seed + 1, alphabet=alphabet, orient=orient, prefix="z")
    return adv.reads(ann, n, mode, seed, alphabet=alphabet, orient=orient, with_seq=genome, **(RESCUE_MIX if genome else {}))


class Case:
    """One batch and one parametrisation.  kind: 'adv' (tests/adversarial.py's annotation) or 'dense'."""

    def __init__(self, kind, mode, n, seed, preset, use_fasta=False):
        self.kind, self.mode, self.n, self.seed, self.preset, self.genome = kind, mode, n, seed, preset, use_fasta
        self.flags = dict(PRESETS[preset])
        if use_fasta:
            self.flags["use_fasta"] = 1
        self.orient = preset if preset in ("fr", "rf") else None
        self.id = "%s-%s-%s%s-%d" % (kind, mode, preset, "-S" if use_fasta else "", seed)
        self.family = family(self.flags)

    def annotation(self):
        return _annotation(self.kind, self.genome)

    def records(self, alphabet="full"):
        return _records(self.kind, self.mode, self.n, self.seed, self.orient, self.genome, alphabet)

    def batch(self, alphabet="full"):
        return adv.batch(self.records(alphabet))


def _cases():
    out = []
    for p in SHORT:
        out += [Case("adv", "se", 2500, 21, p), Case("adv", "pe", 2000, 22, p), Case("adv", "mm", 1200, 23, p),
                Case("adv", "near", 600, 24, p)]
    for p in ("default", "strict", "fr"):
        out.append(Case("dense", "pe", 700, 25, p))
    # the dense locus under the similarity-filter presets and -S: the match table's pass over the alignments with more than
    # 64 candidate rows (k_project's emit form, k_project_fa)
    out += [Case("dense", "long", 500, 31, "lr"), Case("dense", "pe", 700, 25, "lr_hq"),
            Case("dense", "long", 800, 32, "lr", use_fasta=True)]
    for p in LONG:
        out += [Case("adv", "long", 2500, 26, p), Case("adv", "pe", 1500, 27, p), Case("adv", "near", 400, 28, p)]
        out.append(Case("adv", "long", 6000, 29, p, use_fasta=True))
    # (a second draw: the rarest override cells, real = or X under an ideal insertion, turn up a few times in 10 000 reads)
    out.append(Case("adv", "long", 6000, 30, "lr", use_fasta=True))
    return out


CASES = _cases()
# records in / records out: one batch of every kind
_BAM = ("adv-pe-default-22", "adv-se-strict-21", "adv-mm-fr-23", "adv-near-default-24", "adv-near-rf-24", "dense-pe-default-25",
        "adv-long-lr-26", "adv-long-lr_hq-26", "adv-pe-override-22", "adv-long-lr-S-29", "dense-long-lr-S-32")
BAM_CASES = [c for c in CASES if c.id in _BAM]
assert len(BAM_CASES) == len(_BAM) and len({c.id for c in CASES}) == len(CASES)


def conditions(case, orc, batch):
    """What keeps a comparison from passing emptily (checked on the CPU and again where the GPU test runs): the share of
    reads with rows, the share of paired rows, and every CIGAR op in the rewritten CIGARs."""
    n = batch["n_aln"]
    with_rows = len(np.unique(orc["input_index"]))
    if case.mode in ("pe", "near"):
        assert 3 * with_rows >= n, (case.id, with_rows, n)
        assert 2 * int(orc["is_paired"].sum()) >= orc["n_rows"], (case.id, int(orc["is_paired"].sum()), orc["n_rows"])
    else:
        assert 2 * with_rows >= n, (case.id, with_rows, n)
    ops = set((orc["cigar"] & 0xF).tolist())
    assert ops >= set(range(9)), (case.id, "".join(adv.OPS[o] for o in sorted(ops)))
    if case.family == "rescue":
        assert int((orc["clip_score"] != 0).sum()) > 100, (case.id, "rescued rows", int((orc["clip_score"] != 0).sum()))
    nops = np.diff(batch["cigar_off"].astype(np.int64))
    assert 5 * int((nops > 8).sum()) >= n or case.mode == "near", (case.id, "CIGARs of more than 8 ops", int((nops > 8).sum()), n)
    # (the dense locus has three-exon transcripts: no read over it gets to 64 ops)
    assert int((nops > 64).sum()) > 0 or case.mode != "long" or case.kind == "dense", (case.id, "no CIGAR of more than 64 ops")
