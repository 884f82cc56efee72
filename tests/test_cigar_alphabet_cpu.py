"""The full CIGAR alphabet on the CPU side: the oracle's merge_ops against the reference's rule order cell by cell
(tests/golden/merge_ops_table.json, transcribed by hand), and what the fixed batches of tests/test_gpu_cigar_alphabet.py
are worth -- counted with the oracle's merge-cell counter (ob.merge_hits): they reach every (real op, ideal op) cell a
large sweep of tests/adversarial.py reaches, per route family, and that set is a strict superset of what the same
generator reaches when it spells its reads with M I D N S alone."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import oracle_binding as ob
from tests import adversarial as adv
from tests import alphabet_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = ob.CIGAR_ALPHABET + "?~"       # column 15 ('~'): the front-clip phase with the ideal CIGAR exhausted


def test_merge_ops_table_cell_by_cell():
    with open(os.path.join(ROOT, "tests", "golden", "merge_ops_table.json")) as f:
        fx = json.load(f)
    seen = set()
    for c in fx["cells"]:
        assert ob.merge_ops(c["real"], c["ideal"]) == c["out"], c
        seen.add((c["real"], c["ideal"]))
    assert seen == {(r, i) for r in fx["real_ops"] for i in fx["ideal_ops"]} and len(fx["cells"]) == 90


def test_merge_hits_counts_one_known_merge():
    """By hand: 2S8M over the ideal 8M -> the front-clip phase evaluates (S, M) once (the ideal op is not an override: it
    stays), the main loop (M, M) once; nothing is counted outside the block."""
    with ob.merge_hits() as h:
        out = ob.merge_cigar(ob.parse_cigar("2S8M"), ob.parse_cigar("8M"))
    c = h.cells()
    assert ob.format_cigar(out) == "2S8M"
    assert c[4, 0] == 1 and c[0, 0] == 1 and c.sum() == 2
    ob.merge_cigar(ob.parse_cigar("2S8M"), ob.parse_cigar("8M"))
    assert h.cells().sum() == 2


def _names(cells):
    return sorted("%s%s" % (LETTERS[r], LETTERS[i]) for r, i in zip(*np.nonzero(cells)))


def _run_counted(ann, batch, flags):
    with ob.merge_hits() as h:
        orc, _, _ = ob.run(ob.OracleIndex(ann), ob.make_flags(**flags), batch, want_matches=False)
    return orc, h.cells() > 0


# the sweep: per family the read modes and the presets of the GPU tests, 4000 read names per mode and seed (plus the near
# misses) on an annotation of its own per seed.  Sized by doubling: short and long reach their 15 cells with one seed and
# no more with two or four; the rescue reaches 27 cells with two seeds, 28 with four and no more with eight.
SWEEP = {"short": (("se", "pe", "mm", "long"), ac.SHORT), "long": (("se", "pe", "mm", "long"), ac.LONG),
         "rescue": (("long",), ac.LONG)}
SWEEP_SEEDS = {"short": (1, 2), "long": (1, 2), "rescue": (1, 2, 3, 4)}


@functools.lru_cache(maxsize=None)
def _sweep_batches(seed, n, alphabet, genome, modes):
    """(annotation, batches) of one sweep seed: the short and the long family project the same reads"""
    ann = adv.annotation(100 + seed, n_genes=40, with_genome=genome)
    batches = [adv.batch(adv.reads(ann, n, m, seed, alphabet=alphabet, with_seq=genome, **(ac.RESCUE_MIX if genome else {})))
               for m in modes]
    batches.append(adv.batch(adv.near_misses(ann, seed, alphabet=alphabet)))
    return ann, batches


def sweep(fam, alphabet, n, seeds):
    modes, presets = SWEEP[fam]
    genome = fam == "rescue"
    reached = np.zeros((16, 16), dtype=bool)
    for seed in seeds:
        ann, batches = _sweep_batches(seed, n, alphabet, genome, modes)
        for p in presets:
            flags = dict(ac.PRESETS[p], **({"use_fasta": 1} if genome else {}))
            for b in batches:
                reached |= _run_counted(ann, b, flags)[1]
    return reached


@pytest.fixture(scope="module")
def fixed():
    """every fixed batch through the oracle: conditions checked, cells per family"""
    cells = {}
    for case in ac.CASES:
        b = case.batch()
        orc, hit = _run_counted(case.annotation(), b, case.flags)
        ac.conditions(case, orc, b)
        cells[case.family] = cells.get(case.family, np.zeros((16, 16), dtype=bool)) | hit
    return cells


@pytest.mark.parametrize("fam", ["short", "long", "rescue"])
def test_fixed_batches_reach_every_cell_of_the_sweep(fixed, fam):
    full = sweep(fam, "full", 4000, SWEEP_SEEDS[fam])
    basic = sweep(fam, "basic", 4000, SWEEP_SEEDS[fam])
    print("\n%s: sweep reaches %d merge cells with the full alphabet: %s" % (fam, int(full.sum()), " ".join(_names(full))))
    print("%s: %d with M I D N S alone: %s" % (fam, int(basic.sum()), " ".join(_names(basic))))
    print("%s: the fixed batches reach %d: %s" % (fam, int(fixed[fam].sum()), " ".join(_names(fixed[fam]))))
    assert not (basic & ~full).any() and int(full.sum()) > int(basic.sum())
    missing = full & ~fixed[fam]
    assert not missing.any(), "cells the fixed batches miss: %s" % " ".join(_names(missing))


def test_generator_draws_what_it_promises():
    ann = adv.annotation(3, n_genes=40)
    lens = {e[1] - e[0] for t in ann["transcripts"] for e in t["exons"]}
    introns = {b[0] - a[1] for t in ann["transcripts"] for a, b in zip(t["exons"][:-1], t["exons"][1:])}
    assert lens >= set(adv.EXON_LENS) and introns >= set(adv.INTRON_LENS)
    assert {t["strand"] for t in ann["transcripts"]} == {"+", "-"} and any(len(t["exons"]) == 1 for t in ann["transcripts"])
    assert min(e[0] for t in ann["transcripts"] for e in t["exons"]) == 1
    for mode in adv.MODES:
        recs = adv.reads(ann, 3000, mode, seed=4)
        again = adv.reads(ann, 3000, mode, seed=4)
        assert len(recs) == len(again) and all(a["ref_start"] == b["ref_start"] and np.array_equal(a["cigar"], b["cigar"])
                                               for a, b in zip(recs, again))
        nops = np.array([len(r["cigar"]) for r in recs])
        assert 5 * int((nops > 8).sum()) >= len(recs), mode
        if mode == "long":
            assert int((nops > 64).sum()) > 0
        text = [ob.format_cigar(r["cigar"]) for r in recs]
        ops = set("".join(text)) - set("0123456789")
        assert ops == set("MIDNSHP=X"), (mode, ops)
        assert any(r["ref_start"] == 1 for r in recs), mode
        # an I next to an N on either side, two N in a row, a leading I behind the clips, H + S at the front
        import re
        for pat in (r"\dI\d+N", r"N\d+I", r"N\d+N", r"^(\d+H)?(\d+S)?\d+I", r"^\d+H\d+S", r"\d+S\d+H$"):
            assert any(re.search(pat, t) for t in text), (mode, pat)
    pe = adv.reads(ann, 2000, "pe", seed=5)
    assert all((r["flags"] & 0x1) and (r["flags"] & 0xC0) in (0x40, 0x80) for r in pe)
    assert any(r["flags"] & 0x8 for r in pe) and any(r["flags"] & 0x100 for r in pe)
    basic = adv.reads(ann, 2000, "se", seed=5, alphabet="basic")
    assert set("".join(ob.format_cigar(r["cigar"]) for r in basic)) - set("0123456789") == set("MIDNS")


def test_fuzz_seeds_include_adversarial_rounds():
    """tests/test_gpu_fuzz.py runs 25 rounds per seed: the seed added for the adversarial rounds has some (the round draw
    replayed; the stream that decides it is separate from the one that draws the rounds' parameters)."""
    from tests import fuzz_gpu
    assert fuzz_gpu.adversarial_rounds(25, 303) == [0, 5, 6, 8, 12, 20]
    assert all(len(fuzz_gpu.adversarial_rounds(25, s)) >= 1 for s in (101, 202))
    n = len(fuzz_gpu.adversarial_rounds(4000, 9))
    assert 900 < n < 1100       # a quarter of the rounds
