"""The split count pass (k_project<G, false, false, 1 / 2> over CountArgs) against the CPU oracle, preset by preset: the
short-read instantiation (its preset flags compiled in, also under --strict, fr and rf) and the generic one
(--max-error-exon with and without looser tolerances, --lr without the similarity filter), on both row paths, on a dense
locus whose alignments reach walk_list and big_list, and on GENCODE-shaped reads.  With the looser tolerances the dense
locus's > 64-candidate alignments also outgrow the direct-rows path's first side arena, so that path's grow-and-repeat
round runs too."""
import numpy as np
import pytest

from bramble_amd import lib, synth
from bramble_amd.batch import make_batch
from oracle import oracle_binding as ob
from tests.parity import assert_rows_equal

pytestmark = pytest.mark.gpu

# (flags, what the count pass runs): the first four take the short-read instantiation, the others the generic one
PRESETS = [
    ({}, "short"),
    ({"strict": 1}, "short"),
    ({"fr": 1}, "short"),
    ({"rf": 1}, "short"),
    ({"max_error_exon": 30}, "generic"),
    ({"max_error_exon": 30, "max_clip": 40, "max_junc_ins": 10, "max_junc_gap": 10}, "generic"),
    ({"lr": 1, "sim_thr": 1.0}, "generic"),
]


def dense_locus(n_iso=150, seed=7):
    """One gene of n_iso isoforms on each strand: a shared first exon end, a short shared middle exon and staggered outer
    edges, so that a read inside the first exon has more than 64 candidate rows (big_list) and a read across all three
    exons needs the exon walk (walk_list)."""
    rng = np.random.RandomState(seed)
    txs = []
    for k in range(n_iso):
        for strand in "+-":
            a = 1000 + int(rng.randint(0, 60))
            c = 2300 + int(rng.randint(0, 60))
            exons = [[a, 1300], [1500, 1540], [2000, c]]
            if k % 7 == 3:
                exons.insert(2, [1700, 1720])   # an extra small exon: the walk skips or misses it
            txs.append({"id": "t%d%s" % (k, strand), "ref_id": 0, "strand": strand, "exons": exons})
    ann = {"refnames": ["chrD"], "transcripts": txs}
    recs = []
    cigars = [(1100, "100M"), (1150, "100M"), (1240, "60M200N40M"), (1270, "30M200N40M460N30M"),
              (1270, "30M200N40M160N20M280N10M"), (1200, "100M200N40M"), (1290, "10M200N40M460N50M"),
              (1280, "20M200N40M2I458N38M"), (1520, "20M460N80M"), (1005, "95M5S")]
    for i in range(4000):
        start, cg = cigars[i % len(cigars)]
        start += int(rng.randint(-3, 4))
        recs.append({"name": "r%d" % i, "ref_id": 0, "ref_start": start, "cigar": cg, "read_len": 100})
    return ann, make_batch(recs)


def project(ann_dict, batch, flags, direct_rows):
    idx = lib.Index(ann_dict, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("group_lanes", 8)
    ctx.set_param("small_batch", 0)       # the ordinary pipeline: the count pass split in two kernels
    ctx.set_param("direct_rows", direct_rows)
    rows = ctx.project_batch(lib.make_config(**flags), batch)
    ctx.close()
    idx.close()
    return rows


def oracle(ann_dict, batch, flags):
    orc, _, _ = ob.run(ob.OracleIndex(ann_dict), ob.make_flags(**flags), batch, want_matches=False)
    return orc


@pytest.fixture(scope="module")
def dense():
    return dense_locus()


@pytest.fixture(scope="module")
def gencode_like():
    ann = synth.Annotation("G", n_genes=4000, n_refs=3)
    return ann.as_dict(), ann.reads(60000, "pe", p_multimap=0.2)


@pytest.mark.parametrize("flags,kind", PRESETS)
@pytest.mark.parametrize("direct_rows", [1, 0])
def test_dense_locus(dense, flags, kind, direct_rows):
    ann, batch = dense
    orc = oracle(ann, batch, flags)
    assert orc["n_rows"] > 0
    assert_rows_equal(project(ann, batch, flags, direct_rows), orc)


@pytest.mark.parametrize("flags,kind", PRESETS)
def test_gencode_like(gencode_like, flags, kind):
    ann, batch = gencode_like
    orc = oracle(ann, batch, flags)
    assert orc["n_rows"] > 0
    assert_rows_equal(project(ann, batch, flags, 1), orc)
