"""Inputs and the CPU restatement for k_pair_mask's two ways of intersecting two mates' survivor sets (64-bit tid masks where
the two lists span at most 64 tids and the partner lies in the wave's window; tid lists otherwise): shared by
tests/test_pair_bitmask_cpu.py and tests/test_gpu_pair_bitmask.py.

The annotation is hand-made so that a read's survivors are known by construction.  A locus is a run of transcripts with
consecutive tids; every transcript has a short first exon of its own, staggered so that location order is tid order, and one
exon in each SLOT it belongs to.  A slot is 200 bases that nothing else overlaps, so a read placed in a slot survives on
exactly the slot's members:

  E  70 transcripts: pairs of two-survivor lists that span exactly 63 (A x B) and exactly 64 (A x C), the smallest tid on either
     side (A x G, G x A), one survivor each without a common transcript (P1 x P2), 1 + 2 and 2 + 2 without one (P1 x Q, Q x R);
  L  70 transcripts: lists of 1, 8, 9, 16, 17 and 64 survivors (slots L1 .. L64) and two slots that overlap them in part (M17,
     M9), so that the common transcripts are a strict subset of both lists;
  D  70 transcripts: a slot of all 70 (more than 64 candidate rows: k_pair_big's) beside small ones.

The batch is a few hundred alignments: pairs of every kind in turn (mates are neighbours), one read name of four records
whose mates are two apart, placed across a window edge, and one read name of 66 pairs whose mates are 66 apart (always outside
the window).  batch(1) is the same with one single-end read in front: every pair sits at an odd offset then.

Nothing here is derived from a device run: survivors come from the oracle's match lists, and the path a pair takes is predicted
from them by the span rule (max tid - min tid over both lists <= 63) and the window rule (an owner at index i, in the window
w = i // 62, has its partner inside iff 62 w - 1 <= m <= 62 w + 62)."""
import functools

import numpy as np

WINDOW = 62
SLOT_LEN, SLOT_STEP, SLOT0 = 200, 2000, 4000
LOCUS_STEP = 100000
EMPTY = 900000   # no transcript here


def _r(a, b):
    return list(range(a, b))


LOCI = {
    "E": (70, {"A": [0, 1], "B": [0, 63], "C": [0, 64], "G": [1, 63], "P1": [2], "P2": [3], "Q": [4, 5], "R": [6, 7],
               "F": _r(8, 63) + _r(65, 70)}),
    "L": (70, {"L1": [0], "L8": _r(0, 8), "L9": _r(0, 9), "L16": _r(0, 16), "L17": _r(0, 17), "L64": _r(0, 64),
               "M17": _r(8, 25), "M9": _r(56, 65), "Fz": _r(65, 70)}),
    "D": (70, {"BIG": _r(0, 70), "S": [0, 1], "S2": [2]}),
}
LIST_LENGTHS = (1, 8, 9, 16, 17, 64)


def _locus_base(name):
    return 10000 + LOCUS_STEP * list(LOCI).index(name)


def _slot_start(locus, slot):
    return _locus_base(locus) + SLOT0 + SLOT_STEP * list(LOCI[locus][1]).index(slot)


@functools.lru_cache(maxsize=None)
def annotation():
    txs = []
    for name, (n, slots) in LOCI.items():
        base = _locus_base(name)
        for i in range(n):
            exons = [[base + 20 * i, base + 20 * i + 10]]
            exons += [[_slot_start(name, s), _slot_start(name, s) + SLOT_LEN] for s, members in slots.items() if i in members]
            assert len(exons) >= 2, (name, i)
            txs.append({"id": "%s%d" % (name, i), "ref_id": 0, "strand": "+", "exons": exons})
    return {"refnames": ["chrM1"], "transcripts": txs}


def tid_of(locus, i):
    return sum(LOCI[k][0] for k in list(LOCI)[:list(LOCI).index(locus)]) + i


def members(where):
    """the tids a read at `where` = (locus, slot) survives on, by construction (None: a read beside every transcript)"""
    if where is None:
        return []
    return [tid_of(where[0], i) for i in LOCI[where[0]][1][where[1]]]


# (read 1, read 2) of a pair
E = lambda s: ("E", s)
L = lambda s: ("L", s)
D = lambda s: ("D", s)
KINDS = [
    (E("A"), E("B")),        # span 63: masks; one common transcript of two and two
    (E("A"), E("C")),        # span 64: lists
    (E("A"), E("G")),        # the smallest tid in read 1's list
    (E("G"), E("A")),        # ... in read 2's
    (E("B"), E("G")),
    (E("P1"), E("P2")),      # 1 + 1, nothing common: both kept, not PF_SAME
    (E("P1"), E("Q")),       # 1 + 2, nothing common: nothing kept
    (E("Q"), E("R")),        # 2 + 2
    (E("A"), E("A")),        # everything common
    (E("C"), E("G")),        # span 64 and nothing common
    (E("P1"), E("C")),       # 1 + 2 on the list path
    (E("P1"), E("P1")),      # 1 + 1, the same transcript
    (L("L1"), L("L64")), (L("L8"), L("L64")), (L("L9"), L("L64")), (L("L16"), L("L64")), (L("L17"), L("L64")),
    (L("L64"), L("L64")),
    (L("L17"), L("M17")),    # 17 + 17, nine common: the second round of eight on both sides
    (L("L64"), L("M17")),
    (L("L9"), L("L17")),
    (L("L64"), L("M9")),     # 64 + 9 that span 65: long lists on the list path
    (L("L8"), L("M17")),     # 8 + 17, nothing common
    (L("L1"), L("M17")),
    (D("S"), D("BIG")),      # a mate with more than 64 candidate rows: k_pair_big's
    (D("BIG"), D("S")),
    (D("S2"), D("BIG")),
    (D("S"), D("S2")),       # ... next to ordinary pairs of the same locus
    (E("A"), None),          # a mate without survivors
    (None, L("L9")),
    (E("B"), E("C")),        # span 64 with a common transcript
]
# the kinds of the far-apart read name: both paths, 1 + 1, long lists, a deferred pair (two different slots each: the starts
# of one read name must be distinct)
FAR_KINDS = [KINDS[i] for i in (0, 1, 2, 5, 6, 18, 20, 21, 24)]
N_FRONT, N_FAR, N_BACK = 61, 66, 59


def _read(where, o):
    """(start, cigar) of an 80-base read at offset o (< 100) inside the slot"""
    if where is None:
        return (EMPTY + 300 * o, "80M")
    return (_slot_start(*where) + 5 + o, "80M")


def _pair(name, kind, o, swap):
    from tests.test_gpu_pairing_dense import _pair as pair_records
    a, b = kind
    return pair_records(name, _read(a, o), _read(b, (o + 13) % 100), swap)


def records(shift=0):
    recs = []
    if shift:
        recs.append({"name": "single", "ref_id": 0, "ref_start": _read(E("A"), 3)[0], "cigar": "80M", "read_len": 80})
    p = 0
    for _ in range(N_FRONT):           # alignments 0 .. 121 (+ shift)
        recs += _pair("p%d" % p, KINDS[p % len(KINDS)], (7 * p) % 87, (p // len(KINDS)) % 2 == 1)
        p += 1
    # a read name of four records, read 1s first: mates two apart, across the edge between windows 1 and 2
    q = [_pair("quad", KINDS[0], 10, False), _pair("quad", KINDS[1], 40, False)]
    recs += [q[0][0], q[1][0], q[0][1], q[1][1]]
    for _ in range(N_BACK):
        recs += _pair("p%d" % p, KINDS[p % len(KINDS)], (7 * p) % 87, (p // len(KINDS)) % 2 == 1)
        p += 1
    far = [_pair("far", FAR_KINDS[k % len(FAR_KINDS)], k, False) for k in range(N_FAR)]
    recs += [f[0] for f in far] + [f[1] for f in far]
    for _ in range(8):
        recs += _pair("p%d" % p, KINDS[p % len(KINDS)], (7 * p) % 87, True)
        p += 1
    return recs


@functools.lru_cache(maxsize=None)
def batch(shift=0):
    from bramble_amd.batch import make_batch
    return make_batch(records(shift))


@functools.lru_cache(maxsize=None)
def oracle(shift=0):
    """(the oracle's rows, its match lists) of batch(shift), default preset"""
    from oracle import oracle_binding as ob
    orc, matches, _ = ob.run(ob.OracleIndex(annotation()), ob.make_flags(), batch(shift), want_matches=True)
    return orc, matches


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def survivor_lists(matches):
    off = np.asarray(matches["aln_off"], dtype=np.int64)
    tid = np.asarray(matches["tid"], dtype=np.int64)
    return [tid[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def in_window(i, m):
    w = i // WINDOW
    return WINDOW * w - 1 <= m <= WINDOW * w + WINDOW


def span_of(x, y):
    return int(max(x.max(), y.max()) - min(x.min(), y.min()))


def kept_by_mask(x, y):
    """Steps 2-4 of the mask path for a lane whose list is x and whose partner's is y (span <= 63): (kept tids of x, same)"""
    base = int(min(x.min(), y.min()))
    assert int(max(x.max(), y.max())) - base <= 63
    tm = functools.reduce(lambda a, t: a | (1 << (int(t) - base)), x, 0)
    tm_p = functools.reduce(lambda a, t: a | (1 << (int(t) - base)), y, 0)
    assert tm < (1 << 64) and tm_p < (1 << 64)
    common = tm & tm_p
    if common:
        return [int(t) for t in x if (common >> (int(t) - base)) & 1], True
    if len(x) == 1 and len(y) == 1:
        return [int(t) for t in x], False
    return [], False


def kept_by_sets(x, y):
    """process_mate_pair's rule on the two sets of transcript ids"""
    c = set(int(t) for t in x) & set(int(t) for t in y)
    if c:
        return [int(t) for t in x if int(t) in c], True
    if len(x) == 1 and len(y) == 1:
        return [int(t) for t in x], False
    return [], False


def pairs_of(matches):
    """[(i, m)], i < m: the PAIRs -- mutual mates that both have survivors"""
    mate = np.asarray(matches["mate_idx"], dtype=np.int64)
    lists = survivor_lists(matches)
    out = []
    for i in range(len(mate)):
        m = int(mate[i])
        if m > i and int(mate[m]) == i and len(lists[i]) and len(lists[m]):
            out.append((i, m))
    return out


def predict(matches):
    """-> {"list_path": the owners the list path resolves (br_ctx_direct_diag out[6]), "path": {alignment: "mask" | "list" |
    "big"} for both alignments of every PAIR, "n_big": alignments with more than 64 survivors}.  An alignment with more than 64
    survivors has more than 64 candidate rows; by construction no other alignment of these inputs has (the GPU test checks the
    count against the device's big list)."""
    lists = survivor_lists(matches)
    path = {}
    for i, m in pairs_of(matches):
        big = len(lists[i]) > 64 or len(lists[m]) > 64
        fits = not big and span_of(lists[i], lists[m]) <= 63
        for a, b in ((i, m), (m, i)):
            path[a] = "big" if big else "mask" if fits and in_window(a, b) else "list"
    return {"list_path": sum(1 for v in path.values() if v == "list"), "path": path,
            "n_big": sum(1 for x in lists if len(x) > 64)}
