"""Inputs and the CPU restatement for the emit kernels' two ways of ranking a kept survivor among its alignment's (by counting
the bits of the tid word k_pair_mask leaves -- DirectArgs::kt, br_ctx_direct_tidwords -- or by the loop over the kept
survivors' tids): shared by tests/test_rank_tid_cases_cpu.py and tests/test_gpu_emit_rank.py.

The annotation is hand-made like that of tests/pair_bitmask_cases.py: a locus is a run of transcripts with consecutive tids,
every transcript has a short first exon of its own, staggered so that location order is tid order, and three exons E1, E2, E3 in
each SLOT it belongs to.  Here E1 STARTS IN THE OPPOSITE ORDER: transcript i's E1 begins N - 1 - i bases behind the slot's
start, so the slab rows of a slot (ordered by exon start) run from the largest tid to the smallest, and the rank of a survivor
among the kept tids is never its place in candidate order.  E1 ends, E2 and E3 are the same for all members, so a read may be

  M  one M op inside E1                        (simple class,              k_emit_rows<1>)
  L  "x M 200 N 50 M" from E1 into E2, exact   (light two-exon class,      k_emit_rows<1>)
  3  three read exons E1, E2, E3               (general class,             k_emit_rows<2>)
  I  one read exon with an insertion inside E1 (general class,             k_emit_rows<2>)

and survives on exactly the slot's members.  Locus R is all '+'; in locus S even transcripts are '+' and odd ones '-', so an
unstranded read there has survivors on both strands (candidate items from n0 on).

Nothing here is derived from a device run: survivors are the oracle's match lists, the path of a pair is pair_bitmask_cases'
prediction (span rule, window rule), and the word of an alignment follows from the two lists."""
import functools

import numpy as np

from tests import pair_bitmask_cases as pc

KT_NONE = 0xffffffff
SLOT_STEP, SLOT0, LOCUS_STEP = 2000, 4000, 100000
E1_END, E2, E3 = 300, (500, 600), (800, 900)   # relative to the slot's start
EMPTY = 900000


def _r(a, b):
    return list(range(a, b))


LOCI = {
    "R": (70, "+", {"R2": [10, 11], "R9": _r(20, 29), "R17": _r(20, 37), "R64": _r(0, 64), "P": [0, 63],
                    "X": [2, 3, 6, 7, 10, 11, 20], "Y": [0, 3, 5, 7, 11, 30], "A": [0, 1], "C": [1, 64], "Fz": _r(65, 70)}),
    "S": (20, "+-", {"S6": _r(0, 6), "S12": _r(0, 12), "T": [1, 2, 3, 8], "Sz": _r(12, 20)}),
}


def _locus_base(name):
    return 10000 + LOCUS_STEP * list(LOCI).index(name)


def _slot_start(locus, slot):
    return _locus_base(locus) + SLOT0 + SLOT_STEP * list(LOCI[locus][2]).index(slot)


@functools.lru_cache(maxsize=None)
def annotation():
    txs = []
    for name, (n, strands, slots) in LOCI.items():
        base = _locus_base(name)
        for i in range(n):
            exons = [[base + 20 * i, base + 20 * i + 10]]
            for s, members in slots.items():
                if i in members:
                    s0 = _slot_start(name, s)
                    exons += [[s0 + (n - 1 - i), s0 + E1_END], [s0 + E2[0], s0 + E2[1]], [s0 + E3[0], s0 + E3[1]]]
            assert len(exons) >= 4, (name, i)
            txs.append({"id": "%s%d" % (name, i), "ref_id": 0, "strand": strands[i % len(strands)], "exons": exons})
    return {"refnames": ["chrK1"], "transcripts": txs}


def tid_of(locus, i):
    return sum(LOCI[k][0] for k in list(LOCI)[:list(LOCI).index(locus)]) + i


def members(where):
    if where is None:
        return []
    return [tid_of(where[0], i) for i in LOCI[where[0]][2][where[1]]]


def _read(where, shape, o):
    """(start, cigar) of a read of `shape` at offset o (< 100) in the slot"""
    if where is None:
        return (EMPTY + 300 * o, "80M")
    s0 = _slot_start(*where)
    x = 20 + o % 60
    if shape == "M":
        return (s0 + 100 + o, "80M")
    if shape == "I":
        return (s0 + 100 + o, "40M2I38M")
    if shape == "L":
        return (s0 + E1_END - x, "%dM%dN50M" % (x, E2[0] - E1_END))
    assert shape == "3"
    return (s0 + E1_END - x, "%dM%dN%dM%dN30M" % (x, E2[0] - E1_END, E2[1] - E2[0], E3[0] - E2[1]))


R = lambda s: ("R", s)
S = lambda s: ("S", s)
# (read 1's slot, its shape, read 2's slot, its shape)
KINDS = [
    (R("R2"), "M", R("R2"), "M"),       # two survivors, both common: round one
    (R("R9"), "M", R("R17"), "M"),      # nine kept of nine and of seventeen: round two
    (R("R17"), "M", R("R17"), "L"),     # seventeen: the loop's second step; simple + light
    (R("R17"), "M", R("R17"), "3"),     # simple + general
    (R("R17"), "I", R("R64"), "M"),     # general + simple; 17 kept of 64
    (R("R64"), "M", R("R64"), "3"),     # every bit of the word
    (R("P"), "M", R("R64"), "L"),       # the bit edges: kept tids at base and at base + 63
    (R("P"), "3", R("P"), "M"),
    (R("X"), "M", R("Y"), "M"),         # kept {3, 7, 11}: dropped below, between and above on both sides; base 0 is not kept
    (R("X"), "L", R("Y"), "3"),
    (R("Y"), "I", R("X"), "M"),
    (R("A"), "M", R("C"), "M"),         # span 64: the list path, one common transcript
    (R("A"), "L", R("C"), "3"),
    (S("S6"), "M", S("S12"), "M"),      # both strands
    (S("S12"), "L", S("S6"), "3"),
    (S("T"), "M", S("S12"), "I"),
    (S("T"), "M", S("S6"), "M"),        # kept {1, 2, 3}: dropped on either side, both strands
    (R("R9"), "M", None, "M"),          # a mate without survivors: a SOLO alignment with nine survivors in reversed order
    (None, "M", R("R17"), "3"),
    (R("R2"), "L", R("R2"), "L"),
]
SINGLES = [(R("R17"), "M"), (R("R9"), "3"), (S("S12"), "L"), (R("X"), "I"), (S("T"), "M")]
N_FRONT, N_BACK = 61, 130


def _qlen(cigar):
    from bramble_amd.batch import parse_cigar
    return int(sum(int(w) >> 4 for w in parse_cigar(cigar) if (int(w) & 0xF) in (0, 1, 4, 7, 8)))


def _rec(name, read, flags=0, mate=None):
    r = {"name": name, "ref_id": 0, "ref_start": read[0], "cigar": read[1], "flags": flags, "read_len": _qlen(read[1])}
    if mate is not None:
        r["mate_ref_id"], r["mate_start"] = 0, mate[0]
    return r


def _pair(name, kind, o, swap):
    w1, s1, w2, s2 = kind
    r1, r2 = _read(w1, s1, o), _read(w2, s2, (o + 13) % 100)
    a, b = _rec(name, r1, 0x1 | 0x40 | 0x20, r2), _rec(name, r2, 0x1 | 0x80 | 0x10, r1)
    return [b, a] if swap else [a, b]


def records(shift=0):
    recs = []
    if shift:   # every pair sits at an odd offset then: (61, 62) straddles the edge between windows 0 and 1
        recs.append(_rec("single", _read(R("R9"), "M", 3)))
    p = 0
    for _ in range(N_FRONT):
        recs += _pair("p%d" % p, KINDS[p % len(KINDS)], (7 * p) % 87, (p // len(KINDS)) % 2 == 1)
        p += 1
    # a read name of four records, read 1s first: mates two apart, across the edge between windows 1 and 2 (partners outside)
    q = [_pair("quad", KINDS[2], 10, False), _pair("quad", KINDS[8], 40, False)]
    recs += [q[0][0], q[1][0], q[0][1], q[1][1]]
    for _ in range(N_BACK):
        recs += _pair("p%d" % p, KINDS[p % len(KINDS)], (7 * p) % 87, (p // len(KINDS)) % 2 == 1)
        p += 1
    for k in range(3 * len(SINGLES)):   # SOLO alignments of every shape
        recs.append(_rec("s%d" % k, _read(*SINGLES[k % len(SINGLES)], (11 * k) % 90), 0x10 if k % 2 else 0))
    return recs


@functools.lru_cache(maxsize=None)
def batch(shift=0):
    from bramble_amd.batch import make_batch
    return make_batch(records(shift))


def run_oracle(b):
    """(the oracle's rows, its match lists) of a batch over this annotation, default preset"""
    from oracle import oracle_binding as ob
    orc, matches, _ = ob.run(ob.OracleIndex(annotation()), ob.make_flags(), b, want_matches=True)
    return orc, matches


@functools.lru_cache(maxsize=None)
def oracle(shift=0):
    return run_oracle(batch(shift))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def kept_counts(orc, n_aln):
    return np.bincount(np.asarray(orc["input_index"], dtype=np.int64), minlength=n_aln)


def expected_words(orc, matches):
    """{alignment: (base, [kept tid - base, ...]) | None} for every alignment that keeps a survivor and has at most 64 of them
    (one with more has more than 64 candidate rows: its ranks are in the side arena, its word means nothing).  A word: both
    mates of a PAIR that pair_bitmask_cases.predict puts on the mask path and that have a transcript in common -- base is the
    smallest tid of the two lists, the bits are the common tids.  None (the marker): everything else."""
    lists = pc.survivor_lists(matches)
    nk = kept_counts(orc, len(lists))
    path = pc.predict(matches)["path"]
    want = {a: None for a in range(len(lists)) if nk[a] and len(lists[a]) <= 64}
    for i, m in pc.pairs_of(matches):
        common = sorted(set(int(t) for t in lists[i]) & set(int(t) for t in lists[m]))
        base = int(min(lists[i].min(), lists[m].min()))
        for a in (i, m):
            if path[a] == "mask" and common:
                assert nk[a] == len(common), (a, nk[a], common)   # (the oracle keeps exactly the common ones)
                want[a] = (base, [t - base for t in common])
    return want


def check_words(want, common, base, n_aln):
    """the downloaded words against expected_words; -> (words, markers) checked"""
    n_word = n_none = 0
    for a, w in want.items():
        if w is None:
            assert int(base[a]) == KT_NONE, (a, int(base[a]), hex(int(common[a])))
            n_none += 1
        else:
            bits = functools.reduce(lambda x, b: x | (1 << b), w[1], 0)
            assert int(base[a]) == w[0] and int(common[a]) == bits, (a, int(base[a]), hex(int(common[a])), w)
            n_word += 1
    return n_word, n_none
