"""The definitions of br_whitelist (include/bramble_amd.h) restated in plain Python, and the inputs of their tests.

The restatement finds the candidates of an observed barcode by brute-force Hamming distance over the whole whitelist; it knows
nothing of variants, hashes or tables.  The whitelists that exercise correction are over ACGT, where this search and the kernel's
(one byte replaced by one of A C G T) agree.  The input builders reuse tests/dedup_cases.py and tests/cells_cases.py."""
import functools
from collections import Counter

import numpy as np

from tests import cells_cases as cc
from tests import dedup_cases as dc

CORRECT = {"exact": 0, "1mm": 1, "1mm-multi": 2}
NONE = 0xffffffff
NO_BARCODE, EXACT, CORRECTED, NO_MATCH, AMBIGUOUS = range(5)
WORD_EDGES = (0, 7, 8, 15, 16, 23, 24, 31)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def entries_of(whitelist):
    """the distinct barcodes in ascending (length, bytes) order: entry w is entries[w]"""
    return sorted({bytes(b) for b in whitelist}, key=lambda b: (len(b), b))


def distance(a, b):
    return None if len(a) != len(b) else sum(x != y for x, y in zip(a, b))


def resolve(whitelist, observed, correct):
    """observed: per name its barcode (bytes) or None -> (entry uint32 per name, NONE for none; status uint8 per name; the resolved
    barcode per name, or None)"""
    entries = entries_of(whitelist)
    at = {b: w for w, b in enumerate(entries)}
    count = Counter(at[b] for b in observed if b is not None and b in at)
    verdict = {}
    for b in {b for b in observed if b is not None}:
        if b in at:
            verdict[b] = (at[b], EXACT)
            continue
        cands = [w for w, e in enumerate(entries) if distance(e, b) == 1] if correct else []
        if correct == 2:
            cands = [w for w in cands if count[w] > 0]
            top = max([count[w] for w in cands] + [0])
            cands = [w for w in cands if count[w] == top]
        verdict[b] = (cands[0], CORRECTED) if len(cands) == 1 else (NONE, AMBIGUOUS if cands else NO_MATCH)
    entry = np.asarray([NONE if b is None else verdict[b][0] for b in observed] + [0], np.uint32)[:-1]
    status = np.asarray([NO_BARCODE if b is None else verdict[b][1] for b in observed] + [0], np.uint8)[:-1]
    resolved = [None if e == NONE else entries[e] for e in entry]
    return entry, status, resolved


def reaches_every_branch(whitelist, observed):
    """the condition on a GPU test's input: each of the statuses 1, 2, 3, 4 occurs under "correct" 1 and under 2, and the two
    disagree on a name"""
    s1, s2 = resolve(whitelist, observed, 1)[1], resolve(whitelist, observed, 2)[1]
    return all(k in s1 and k in s2 for k in (EXACT, CORRECTED, NO_MATCH, AMBIGUOUS)) and bool((s1 != s2).any())


# ---- barcodes ----------------------------------------------------------------------------------------------------------------------
def random_barcodes(rng, n, length):
    return [bytes(rng.choice(cc.ACGT, size=length).tolist()) for _ in range(n)]


def put(b, at, byte):
    out = bytearray(b)
    out[at] = byte
    return bytes(out)


def every_error(b):
    """every barcode one base from b"""
    return [put(b, p, x) for p in range(len(b)) for x in b"ACGT" if x != b[p]]


def far_whitelist(rng, n, length):
    """n barcodes of one length, every two of them at least three bytes apart: a single error has exactly one candidate"""
    out = []
    while len(out) < n:
        b = random_barcodes(rng, 1, length)[0]
        if all(distance(b, o) >= 3 for o in out):
            out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def branch_case(seed=0, n_random=60, length=12):
    """(whitelist, observed) that reaches every branch: a random far whitelist with exact hits, single errors, double errors and an N;
    beside it X, Y, Z two bytes from each other around M (one byte from each): M is ambiguous under "correct" 1 and goes to the most
    abundant under 2; T1, T2 around their middle with equal counts: a tie; Q with a single error whom nobody carries exactly: corrected
    under 1, no match under 2; names without a barcode"""
    rng = np.random.default_rng(seed)
    far = far_whitelist(rng, n_random, length)
    m = b"AACCGGTTAACC"[:length]
    x, y, z = put(m, 3, ord("A")), put(m, 3, ord("G")), put(m, 3, ord("T"))   # m[3] is C
    tm = b"GGTTAACCGGTT"[:length]
    t1, t2 = put(tm, 0, ord("A")), put(tm, 0, ord("C"))
    q = b"TTTTGGGGCCCC"[:length]
    whitelist = far + [x, y, z, t1, t2, q, far[0], far[1]]   # (two duplicates)
    observed = []
    for k, b in enumerate(far[:40]):
        observed += [b] * (1 + k % 3)
        if k % 4 == 0:
            observed.append(put(b, k % length, b"ACGT"[(b"ACGT".index(b[k % length]) + 1 + k % 3) % 4]))   # one error
        if k % 5 == 0:
            observed.append(put(put(b, 0, ord("N")), 1, ord("N")))                                          # two: no match
    observed += [put(far[3], 5, ord("N")), put(far[4], 0, ord("N"))]                                         # an N: corrected
    observed += [x] * 3 + [y] * 2 + [m, m]               # z has no name: X wins under 2
    observed += [t1, t2, tm]                              # a tie under 2, ambiguous under 1
    observed += [put(q, 11 % length, ord("A"))]           # q itself is never seen
    observed += [None, None, far[5][:length - 1], far[5] + b"A"]   # no barcode; the same prefix at another length: no match
    order = rng.permutation(len(observed))
    return tuple(whitelist), tuple(observed[i] for i in order)


# ---- runs for br_cells and br_dedup ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run_case(seed=1):
    """(run, whitelist): branch_case's barcodes as read names READ_CB_UMI over a small pool of transcript sets and UMIs, so that cells
    share signatures and UMIs; in front of them a molecule whose second copy carries a barcode error, and a name corrected under
    "correct" 2 by names that come at the run's very end; a name without rows"""
    rng = np.random.default_rng(seed)
    whitelist, observed = branch_case(seed)
    far = whitelist[:60]
    pool = [[3], [4, 5], [10], [3, 12], [20, 21, 22]]
    umis = [b"ACGTAC", b"ACGTAA", b"TTGACC"]
    a, base = far[50], far[52]           # (no name of branch_case carries them)
    run = [cc._name(0, a, [3], umi=b"GGGGGG", pos=700), cc._name(1, dc.mutate(a, 4), [3], umi=b"GGGGGG", pos=700)]
    # `late` is one byte from base, c1 and c2: three candidates; c1 has one name, c2 three, and they arrive last
    c1, c2, late = (put(base, 0, x) for x in b"ACGT" if x != base[0])
    whitelist = whitelist + (c1, c2)
    run.append(cc._name(2, late, [10], umi=b"CCCCCC", pos=300))
    run.append(cc._name(3, c1, [10], umi=b"CCCCCC", pos=300))
    k = 4
    for bc in observed:
        tids = pool[int(rng.integers(len(pool)))]
        run.append(cc._name(k, bc, tids, umi=umis[int(rng.integers(len(umis)))]))
        k += 1
    run.insert(9, dc.name_row(b"norows_" + a + b"_ACGTAC", []))
    run += [cc._name(k + j, c2, [10], umi=b"CCCCC" + b"ACGT"[j:j + 1], pos=300) for j in range(3)]
    return tuple(run), whitelist


@functools.lru_cache(maxsize=None)
def values_case(seed=0):
    """(run, whitelist) for the float modes: cells_cases.standard_run, whose cells are large enough for the order of a sum to show, with
    an error in the barcode of every ninth name; the whitelist is the run's own barcodes"""
    base = cc.standard_run(seed)
    whitelist, run = set(), []
    for i, nm in enumerate(base):
        parts = nm["name"].split(b"_")
        if len(parts) >= 3 and 1 <= len(parts[-2]) <= cc.BC_MAX:
            whitelist.add(parts[-2])
            if i % 9 == 0:
                parts[-2] = dc.mutate(parts[-2], i % len(parts[-2]))
        run.append(dc.name_row(b"_".join(parts), nm["rows"], nm["aux"]))
    return tuple(run), tuple(sorted(whitelist))


def observed_of(groups):
    return cc.barcodes_of(groups)[0]


# ---- record streams in: the command line's input -----------------------------------------------------------------------------------
def cli_whitelist(n_cells=12, seed=0):
    """the cells of cells_cases.with_cells_records(seed), for cell 0 a partner two bytes away, the pair TIE two bytes apart, a barcode
    nobody carries and a duplicate"""
    rng = np.random.default_rng(seed)
    cells = [cc._bc(rng, 8 + k % 3) for k in range(n_cells)]
    partner = dc.mutate(dc.mutate(cells[0], 1), 2)
    return cells, cells + [partner, TIE[0], TIE[1], b"TTTTTTTT", cells[3]]


TIE = (b"ACGTACGTAA", b"ACGTACGTCC", b"ACGTACGTAC")   # two entries one name each carries, and the barcode between them


def with_barcode_errors(recs, n_cells=12, seed=0):
    """cells_cases.with_cells_records' framed records with barcode errors put in, name by name: every fifth name with a barcode gets
    one error (at a position that moves), every thirteenth two errors, and of cell 0's names every third the barcode between the cell
    and its partner; the second, fourth and sixth name carry TIE's barcodes"""
    cells, _ = cli_whitelist(n_cells, seed)
    out, last, new, i = [], None, None, 0
    for r in cc.with_cells_records(recs, n_cells, seed):
        nm = bytes(r[36:36 + r[12] - 1])
        if nm != last:
            last, new = nm, nm
            parts = nm.split(b"_")
            if len(parts) >= 3:
                i += 1
                bc = parts[-2]
                if i in (2, 4, 6):
                    bc = TIE[i // 2 - 1]
                elif bc == cells[0] and i % 3 == 0:
                    bc = dc.mutate(bc, 1)
                elif i % 13 == 0:
                    bc = dc.mutate(dc.mutate(bc, 0), len(bc) - 1)
                elif i % 5 == 0:
                    bc = dc.mutate(bc, i % len(bc))
                parts[-2] = bc
                new = b"_".join(parts)
        out.append(dc.renamed(bytes(r), new) if new != nm else r)
    return out
