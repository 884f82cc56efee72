"""The main count kernel (k_project<G, false, false, 1> over CountArgs) at the edges of its grid-stride loop and of its
rounds of G candidate rows, against the CPU oracle, exactly.  Written for the variants of that kernel that keep the loads
of the next alignments and of the next round of rows in flight (measured, not kept), and kept for
whatever restructures the loop next: an alignment that a group meets one or two strides on is what such a variant reads
early, so the shapes put every kind of neighbour there.

  - batches that end at, just before and just after a whole number of strides (no alignment a stride on, one a stride on
    but none two strides on, ...), with alignments at those positions that have no read exons (head = {0, 0, 0, 0}),
    that lie on a reference without rows on one strand, or beyond their reference's last bin;
  - a dense locus whose alignments take every branch (0, 1..G, G+1..2G, 17..64 and more than 64 candidate rows, walk_list),
    shuffled, so that every transition between rounds and branches happens inside one group's sequence;
  - the same batch under three launch shapes (blocks_per_cu 1, the default, 64);
  - both row paths and the short, strict and one generic preset (the generic instantiation of the kernel).  The
    grid-stride cases run the match-table path (direct_rows = 0) for the first rotation of the special kinds only: the
    main count kernel is the same on both paths, and the neighbour cases run both paths on every preset.
"""
import numpy as np
import pytest

from bramble_amd import lib, synth
from bramble_amd.batch import make_batch
from oracle import oracle_binding as ob
from tests.parity import assert_rows_equal
from tests.test_gpu_count_preset import dense_locus

pytestmark = pytest.mark.gpu

# batch sizes in alignments, as functions of the group width G and of groups_total = n_cu * 256 / G (blocks_per_cu = 1)
SIZES = [
    ("1", lambda g, gt: 1),
    ("G-1", lambda g, gt: g - 1),
    ("33", lambda g, gt: 33),
    ("gt-1", lambda g, gt: gt - 1),
    ("gt", lambda g, gt: gt),
    ("gt+1", lambda g, gt: gt + 1),
    ("2gt+5", lambda g, gt: 2 * gt + 5),
]


def edge_annotation():
    """chrA: three isoforms on each strand; chrP: the same gene on '+' only (its '-' slab is empty)."""
    txs = []
    for k in range(3):
        exons = [[1000 + 10 * k, 1300], [1500, 1540], [2000, 2300 + 10 * k]]
        for strand in "+-":
            txs.append({"id": "a%d%s" % (k, strand), "ref_id": 0, "strand": strand, "exons": exons})
        txs.append({"id": "p%d" % k, "ref_id": 1, "strand": "+", "exons": exons})
    return {"refnames": ["chrA", "chrP"], "transcripts": txs}


def edge_batch(n, gt, rot):
    """n alignments: real matches, with the three special kinds (in turn, starting at `rot`) at every other position and
    at the first positions one and two strides on (gt.., 2 gt..); the last three alignments are real matches."""
    special = set(range(1, n, 2)) | set(range(gt, gt + 8)) | set(range(2 * gt, 2 * gt + 8))
    special -= set(range(max(0, n - 3), n))
    real = [(1100, "100M"), (1240, "60M200N40M"), (1150, "100M")]
    recs = []
    for i in range(n):
        r = {"name": "e%d" % i, "ref_id": 0, "read_len": 100}
        if i in special:
            kind = (i + rot) % 3
            if kind == 0:      # no read exons: the segmenter leaves head = {0, 0, 0, 0}
                r.update(ref_id=-1, ref_start=1100, cigar="100M")
            elif kind == 1:    # a reference with no rows on '-'
                r.update(ref_id=1, ref_start=1100 + i % 5, cigar="100M")
            else:              # beyond the last bin of chrA
                r.update(ref_start=900000 + 517 * (i % 7), cigar="100M")
        else:
            start, cg = real[i % len(real)]
            r.update(ref_start=start + i % 4, cigar=cg)
        recs.append(r)
    return make_batch(recs)


def neighbour_case(n):
    """The dense locus of test_gpu_count_preset (more than 64 candidate rows: the exact-range branch and big_list; three
    and more read exons: walk_list) plus '+' loci of k isoforms each, far apart, whose stranded reads have about k
    candidate rows; n alignments of all kinds, shuffled."""
    ann, _ = dense_locus()
    ks = [1, 2, 5, 8, 9, 12, 16, 17, 24, 40, 64]
    for j, k in enumerate(ks):
        base = 100000 + 20000 * j
        for i in range(k):
            ann["transcripts"].append({"id": "k%d_%d" % (k, i), "ref_id": 0, "strand": "+",
                                       "exons": [[base + i, base + 300], [base + 5000, base + 5200 + i]]})
    kinds = [(1100, "100M", 0), (1150, "100M", 0), (1240, "60M200N40M", 0), (1270, "30M200N40M460N30M", 0),
             (1270, "30M200N40M160N20M280N10M", 0), (1200, "100M200N40M", 0), (1290, "10M200N40M460N50M", 0),
             (1520, "20M460N80M", 0), (1005, "95M5S", 0), (1100, "100M", "+"), (1240, "60M200N40M", "-"),
             (50000, "100M", 0), (60000, "50M300N50M", 0)]    # the last two: no candidate row
    for j, k in enumerate(ks):
        base = 100000 + 20000 * j
        kinds += [(base + 100, "100M", "+"), (base + 240, "60M4700N40M", "+"), (base + 120, "100M", 0)]
    rng = np.random.RandomState(11)
    pick = rng.randint(0, len(kinds), size=n)
    jit = rng.randint(-2, 3, size=n)
    recs = []
    for i in range(n):
        start, cg, xs = kinds[i - n] if n - i <= len(kinds) else kinds[pick[i]]   # every kind at least once, at the end
        recs.append({"name": "n%d" % i, "ref_id": 0, "ref_start": start + int(jit[i]), "cigar": cg, "read_len": 100, "xs": xs})
    return ann, make_batch(recs)


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def project(ann_dict, batch, flags, direct_rows=1, group_lanes=8, blocks_per_cu=None, diag=False):
    idx = lib.Index(ann_dict, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("group_lanes", group_lanes)
    ctx.set_param("small_batch", 0)       # the ordinary pipeline: the count pass split in two kernels
    ctx.set_param("direct_rows", direct_rows)
    if blocks_per_cu is not None:
        ctx.set_param("blocks_per_cu", blocks_per_cu)
    rows = ctx.project_batch(lib.make_config(**flags), batch)
    d = ctx.direct_diag() if diag else None
    ctx.close()
    idx.close()
    return (rows, d) if diag else rows


def oracle(ann_dict, batch, flags):
    orc, _, _ = ob.run(ob.OracleIndex(ann_dict), ob.make_flags(**flags), batch, want_matches=False)
    return orc


@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("group_lanes", [8, 16])
def test_grid_stride_edges(group_lanes, size, rot):
    gt = n_cu() * 256 // group_lanes
    ann = edge_annotation()
    batch = edge_batch(size[1](group_lanes, gt), gt, rot)
    orc = oracle(ann, batch, {})
    assert orc["n_rows"] > 0
    for direct_rows in ((1, 0) if rot == 0 else (1,)):
        assert_rows_equal(project(ann, batch, {}, direct_rows, group_lanes, blocks_per_cu=1), orc)


@pytest.fixture(scope="module")
def neighbours():
    # five strides and a little (G = 8, blocks_per_cu = 1): every group meets five alignments, of kinds drawn at random
    return neighbour_case(5 * (n_cu() * 256 // 8) + 77)


@pytest.mark.parametrize("flags", [{}, {"strict": 1}, {"max_error_exon": 30}], ids=["short", "strict", "generic"])
@pytest.mark.parametrize("direct_rows", [1, 0])
def test_neighbours_of_different_kinds(neighbours, flags, direct_rows):
    ann, batch = neighbours
    orc = oracle(ann, batch, flags)
    assert orc["n_rows"] > 0
    assert_rows_equal(project(ann, batch, flags, direct_rows, 8, blocks_per_cu=1), orc)


def test_neighbours_sixteen_lanes(neighbours):
    ann, batch = neighbours
    orc = oracle(ann, batch, {})
    assert orc["n_rows"] > 0
    assert_rows_equal(project(ann, batch, {}, 1, 16, blocks_per_cu=1), orc)


def test_launch_shape_independence():
    a = synth.Annotation("G", n_genes=4000, n_refs=3)
    ann, batch = a.as_dict(), a.reads(30000, "pe", p_multimap=0.2)
    orc = oracle(ann, batch, {})
    assert orc["n_rows"] > 0
    diags = []
    for bpc in (1, None, 64):
        rows, d = project(ann, batch, {}, 1, 8, blocks_per_cu=bpc, diag=True)
        assert_rows_equal(rows, orc)
        diags.append((d["n_big"], d["light"]))
    assert diags[0] == diags[1] == diags[2], diags
