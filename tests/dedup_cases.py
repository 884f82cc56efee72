"""The definitions of br_dedup (include/bramble_amd.h) restated in plain Python, and the inputs of its tests.

The restatement works from an uncompressed output record stream cut into read names -- `groups`: per name the list of its records
(bytes from refID on, without block_size) -- and reads ONLY the records: refID, pos, flag, name, aux and the CIGAR (the CG:B,I spill
form included).  The directional method is written as umi_tools writes it (adjacency list, breadth-first search from the nodes in
count order, first claim wins); labels_by_propagation is the other formulation, the one the device uses, and the CPU test holds the
two against each other.

The inputs are built from a description (`run`: per name its name bytes, aux bytes and rows (tid, pos, CIGAR words, flag)) into both
things the device takes: the records (tests/bamio.bam_record) and the row tables."""
import struct
from collections import Counter, deque

import numpy as np

from tests import bamio

METHODS = {"unique": 0, "directional": 1}
SOURCES = {"name": 0, "tag": 1}
UMI_MAX = 32
NONE = 0xffffffff
ROW_MINUS, ROW_FIRST, ROW_PRIMARY = 1 << 24, 1 << 27, 1 << 28
OPS = "MIDNSHP=X"
AUX_SIZES = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}


def cig(text):
    """'5S20M3H' -> BAM-packed words"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append(int(num) << 4 | OPS.index(ch))
            num = ""
    return out


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def aux_walk(aux):
    """-> ([(tag bytes, type, value bytes)], clean): the fields up to the first that has a type outside AcCsSiIfZHB or runs past the end"""
    out, p, n = [], 0, len(aux)
    while p < n:
        if p + 3 > n:
            return out, False
        tag, typ = aux[p:p + 2], aux[p + 2]
        p += 3
        if typ in AUX_SIZES:
            size = AUX_SIZES[typ]
        elif typ in (ord("Z"), ord("H")):
            e = aux.find(b"\0", p)
            if e < 0:
                return out, False
            size = e - p + 1
        elif typ == ord("B"):
            if p + 5 > n or aux[p] not in AUX_SIZES or aux[p] == ord("A"):
                return out, False
            size = 5 + AUX_SIZES[aux[p]] * struct.unpack_from("<I", aux, p + 1)[0]
        else:
            return out, False
        if p + size > n:
            return out, False
        out.append((tag, typ, aux[p:p + size]))
        p += size
    return out, True


def umi_of_record(rec, source="name", sep=b"_", tag=b"RX"):
    """-> (umi bytes or None, why): why in ("", "none", "too_long", "bad_aux")"""
    f = bamio.record_fields(rec)
    umi = None
    if source == "name":
        at = f["name"].rfind(sep)
        if at >= 0:
            umi = f["name"][at + 1:]
    else:
        fields, clean = aux_walk(f["aux"])
        for t, typ, val in fields:
            if t == tag and typ == ord("Z"):
                umi = val[:-1]
                break
        if umi is None and not clean:
            return None, "bad_aux"
    if umi is None or len(umi) == 0:
        return None, "none"
    if len(umi) > UMI_MAX:
        return None, "too_long"
    return bytes(umi), ""


def umis_of(groups, source="name", sep=b"_", tag=b"RX"):
    """-> (per name its UMI or None, {"no_umi", "too_long", "bad_aux"}); a name without records has none and is counted nowhere"""
    out, cnt = [], {"no_umi": 0, "too_long": 0, "bad_aux": 0}
    for g in groups:
        if not g:
            out.append(None)
            continue
        u, why = umi_of_record(g[0], source, sep, tag)
        out.append(u)
        cnt["no_umi"] += u is None
        cnt["too_long"] += why == "too_long"
        cnt["bad_aux"] += why == "bad_aux"
    return out, cnt


def real_cigar(f):
    """the record's CIGAR words: the CG:B,I entry's when the field holds the <l_seq>S<reflen>N spill form"""
    c = [int(w) for w in f["cigar"]]
    if len(c) == 2 and c[0] == (f["l_seq"] << 4 | 4) and (c[1] & 15) == 3:
        for t, typ, val in aux_walk(f["aux"])[0]:
            if t == b"CG" and typ == ord("B") and val[0] == ord("I"):
                return [int(w) for w in np.frombuffer(val[5:], dtype="<u4")]
    return c


def entry_of(rec):
    f = bamio.record_fields(rec)
    c = real_cigar(f)
    flag = f["flag"] & 0xD1
    reflen = sum(w >> 4 for w in c if (w & 15) in (0, 2, 3, 7, 8))

    def clip(ops):
        for w in ops:
            if (w & 15) == 5:
                continue
            return w >> 4 if (w & 15) == 4 else 0
        return 0
    lead, trail = clip(c), clip(c[::-1])
    five = f["pos"] - lead if not (flag & 0x10) else f["pos"] + reflen + trail
    return (f["ref_id"] & 0xffffffff, five, flag)


def signatures_of(groups):
    """per name the sorted tuple of its entries; None for a name without records"""
    return [tuple(sorted(entry_of(r) for r in g)) if g else None for g in groups]


def groups_of(sigs):
    """-> group_first per name (NONE for a name without records)"""
    first, out = {}, []
    for i, s in enumerate(sigs):
        if s is None:
            out.append(NONE)
        else:
            out.append(first.setdefault(s, i))
    return np.asarray(out, dtype=np.uint32)


def node_order(counts):
    return sorted(counts, key=lambda u: (-counts[u], len(u), u))


def hamming1(a, b):
    return len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1


def adjacency(counts):
    nodes = list(counts)
    return {u: [v for v in nodes if v != u and hamming1(u, v) and counts[u] >= 2 * counts[v] - 1] for u in nodes}


def roots_by_bfs(counts):
    """umi_tools' directional clusters: from the nodes in count order, everything a node reaches that nobody claimed is its own"""
    adj, root = adjacency(counts), {}
    for r in node_order(counts):
        if r in root:
            continue
        seen, todo = {r}, deque([r])
        while todo:
            u = todo.popleft()
            for v in adj[u]:
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
        for v in seen:
            root.setdefault(v, r)
    return root


def labels_by_propagation(counts):
    """-> (root per node, the sweeps until nothing changed, that last one included): every sweep reads the labels of the one before"""
    order = node_order(counts)
    place = {u: p for p, u in enumerate(order)}
    adj = adjacency(counts)
    into = {v: [] for v in order}
    for u in order:
        for v in adj[u]:
            into[v].append(u)
    label, sweeps = dict(place), 0
    while True:
        sweeps += 1
        new = {v: min([label[v]] + [label[u] for u in into[v]]) for v in order}
        if new == label:
            break
        label = new
    return {v: order[label[v]] for v in order}, sweeps


def molecules_of(method, sigs, umis):
    """-> rep per name (NONE for a name without records)"""
    rep = np.full(len(sigs), NONE, dtype=np.uint32)
    members = {}
    for i, s in enumerate(sigs):
        if s is not None:
            members.setdefault(s, []).append(i)
    for names in members.values():
        carrying = {}
        for i in names:
            if umis[i] is None:
                rep[i] = i   # its own molecule
            else:
                carrying.setdefault(umis[i], []).append(i)
        counts = {u: len(v) for u, v in carrying.items()}
        root = {u: u for u in counts} if method == "unique" else roots_by_bfs(counts)
        for u, mine in carrying.items():
            for i in mine:
                rep[i] = carrying[root[u]][0]
    return rep


rep_of = molecules_of


def dup_of(rep):
    return ((rep != NONE) & (rep != np.arange(len(rep), dtype=np.uint32))).astype(np.uint8)


def hist_of(rep, hist_max=1000):
    h = np.zeros(hist_max + 1, dtype=np.uint64)
    for size in Counter(int(r) for r in rep if r != NONE).values():
        h[min(size, hist_max)] += 1
    return h


def counts_of(rep):
    """-> (names, molecules, duplicates)"""
    with_rows = int(np.count_nonzero(rep != NONE))
    mols = len(set(int(r) for r in rep if r != NONE))
    return len(rep), mols, with_rows - mols


def expected_stream(groups, dup, mark):
    out = []
    for g, d in zip(groups, dup):
        for r in g:
            if mark and d:
                b = bytearray(r)
                b[14:16] = struct.pack("<H", struct.unpack_from("<H", r, 14)[0] | 0x400)
                r = bytes(b)
            if mark or not d:
                out.append(r)
    return bamio.frame(out) if out else np.zeros(0, np.uint8)


def umi_matrix(umis):
    m, ln = np.zeros((len(umis), UMI_MAX), np.uint8), np.zeros(len(umis), np.uint8)
    for i, u in enumerate(umis):
        if u is not None:
            m[i, :len(u)] = np.frombuffer(u, np.uint8)
            ln[i] = len(u)
    return m, ln


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
def name_row(name, rows, aux=b""):
    return {"name": name, "aux": aux, "rows": list(rows)}


def records_of(run, spill_every=0):
    """per name the list of its records; spill_every: every that-many-th record of more than two ops takes the CG:B,I form"""
    out, k = [], 0
    for nm in run:
        mine = []
        for tid, pos, ops, flag in nm["rows"]:
            k += 1
            l_seq = sum(w >> 4 for w in ops if (w & 15) in (0, 1, 4, 7, 8))
            spill = bool(spill_every) and len(ops) > 2 and k % spill_every == 0
            mine.append(bamio.bam_record(nm["name"], tid, pos, ops, l_seq, flag=flag, aux=nm["aux"], spill=spill))
        out.append(mine)
    return out


def stream_of(groups):
    recs = [r for g in groups for r in g]
    return bamio.frame(recs) if recs else np.zeros(0, np.uint8)


def minus_row(tid, pos):
    """whether the tables give this placement BR_ROW_MINUS (a property of the placement, so that copies agree)"""
    return (tid + pos) % 3 == 0


def tables_of(run):
    """-> dict a [n, 4] uint32, cigar uint64, pool uint32, row_off uint64, group_off uint32: the rows of `run` as the projection leaves
    them.  Names alternate between one alignment a row and one alignment for all rows; a name without rows alternates between no
    alignment and one that emitted nothing.  A third of the rows lie on a '-' transcript (minus_row): their ops are stored reversed"""
    a, cigar, pool, row_off, group_off = [], [], [0xdead], [0], [0]
    for g, nm in enumerate(run):
        rows = nm["rows"]
        for j, (tid, pos, ops, flag) in enumerate(rows):
            minus = minus_row(tid, pos)
            if minus:   # the row holds the ops in transcript order, the record (records_of) in the reverse
                ops = ops[::-1]
            a.append((tid, pos, len(ops) | ROW_FIRST | (ROW_PRIMARY if j == 0 else 0) | (ROW_MINUS if minus else 0), len(rows)))
            if len(ops) <= 2:
                cigar.append((ops[0] if ops else 0) | (ops[1] if len(ops) > 1 else 0) << 32)
            else:
                cigar.append(len(pool))
                pool += ops
                pool.append(0xbeef)   # (the arena is sparse on the device as well)
            if g % 2 == 0:
                row_off.append(len(a))
        if g % 2 == 1 and (rows or g % 4 == 1):
            row_off.append(len(a))
        group_off.append(len(row_off) - 1)
    return {"a": np.asarray(a, dtype=np.uint32).reshape(-1, 4), "cigar": np.asarray(cigar, dtype=np.uint64), "pool": np.asarray(pool, dtype=np.uint32),
            "row_off": np.asarray(row_off, dtype=np.uint64), "group_off": np.asarray(group_off, dtype=np.uint32)}


def random_umi(rng, n=8):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).tolist())


def mutate(umi, at, rng=None):
    b = bytearray(umi)
    b[at] = b"ACGT"[(b"ACGT".index(b[at]) + 1) % 4]
    return bytes(b)


PLAN = ("exact3", "join", "nojoin", "single", "none", "exact2", "tag_only", "long")


def with_umis(base, seed=0, tag=False):
    """every name of `base` re-emitted under <orig>.<j>_<UMI> (tag: with RX:Z as well) by a plan that cycles over the names:
    exact copies (exact3, exact2), a one-mismatch copy at counts 3 : 2 (join: directional one molecule, unique two) and 2 : 2 (nojoin),
    a single read, a name without separator (none), one whose UMI is in the tag only and one whose suffix is 33 bytes.  The copies
    of a name list its rows in rotated orders: the signature does not care"""
    rng = np.random.default_rng(seed)
    out = []
    for i, nm in enumerate(base):
        kind = PLAN[i % len(PLAN)]
        u = random_umi(rng)
        v = mutate(u, int(rng.integers(len(u))))
        umis = {"exact3": [u] * 3, "exact2": [u] * 2, "join": [u, v, u, v, u], "nojoin": [u, v, v, u], "single": [u], "none": [None, None],
                "tag_only": [None, None], "long": [u * 4 + b"A"] * 2}[kind]
        for j, x in enumerate(umis):
            name = nm["name"] + b".%d" % j + (b"_" + x if x is not None else b"")
            aux = nm["aux"]
            if tag or kind == "tag_only":
                aux = b"NHC\x01" + b"RXZ" + (u if x is None else x[:UMI_MAX]) + b"\0" + aux
            rows = nm["rows"][j % max(len(nm["rows"]), 1):] + nm["rows"][:j % max(len(nm["rows"]), 1)]
            out.append(name_row(name, rows, aux))
    return out


def base_names(seed=1, n=40):
    """read names as a projection leaves them: one to many rows on several transcripts, forward and reverse, paired flags, clips in S and
    H, inline and pooled CIGARs; names of 64, 65 and 200 rows among them, and names without rows"""
    rng = np.random.default_rng(seed)
    shapes = ["30M", "5S25M", "25M5S", "3H4S20M", "20M4S3H", "10M100N10M5S", "2H28M", "4S10M2D10M1I5M3S", "30=", "12M3X15M", "5H25M", "6S24M"]
    out = []
    for i in range(n):
        k = {7: 64, 13: 65, 21: 200, 5: 0, 18: 0, 29: 17, 31: 16}.get(i, int(rng.integers(1, 5)))
        rows = []
        for j in range(k):
            flag = int(rng.choice([0, 16, 0x41 | 0x20, 0x81 | 0x10, 0x100, 0x110]))
            rows.append((int(rng.integers(0, 50)) if k < 60 else j, int(rng.integers(40, 2000)), cig(shapes[int(rng.integers(len(shapes)))]), flag))
        out.append(name_row(b"read%03d" % i, rows))
    return out


def nodes_group(m, tid, pos, seed, prefix):
    """a position group of exactly m distinct UMIs (8 bytes over ACGT, random: some lie one mismatch apart) with counts 1 .. 3"""
    rng = np.random.default_rng(seed)
    umis = set()
    while len(umis) < m:
        u = random_umi(rng)
        umis.add(u)
        if len(umis) < m and rng.integers(3) == 0:
            umis.add(mutate(u, int(rng.integers(8))))
    out = []
    for k, u in enumerate(sorted(umis)):
        for j in range(int(rng.integers(1, 4))):
            out.append(name_row(prefix + b"%d.%d_" % (k, j) + u, [(tid, pos, cig("30M"), 0)]))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def chain(n, tid=60, pos=500, prefix=b"chain"):
    """a position group whose n UMIs (32 bytes over ACGT) form a path of one-byte steps with all counts 1: step k raises byte k mod 32,
    so the UMIs ascend along the path, the first is the root of all, and its label needs n - 1 sweeps to reach the last"""
    assert 1 <= n <= 3 * UMI_MAX + 1
    u, out = bytearray(b"A" * UMI_MAX), []
    for k in range(n):
        out.append(name_row(prefix + b"%d_" % k + bytes(u), [(tid, pos, cig("30M"), 16)]))
        if k < 3 * UMI_MAX:   # (byte k mod 32: two steps apart differ in two bytes, so only neighbours are joined)
            u[k % UMI_MAX] = b"ACGT"[b"ACGT".index(u[k % UMI_MAX]) + 1]
    return out[::-1]   # (the far end first: nothing depends on the order of the names)


def paper_network():
    """the six UMIs of the UMI-tools paper's figure at one position"""
    counts = [(b"ACGT", 456), (b"AAAT", 90), (b"ACAT", 72), (b"TCGT", 2), (b"CCGT", 2), (b"ACAG", 1)]
    out = []
    for u, c in counts[::-1]:
        for j in range(c):
            out.append(name_row(b"p%s.%d_" % (u, j) + u, [(3, 100, cig("30M"), 0)]))
    return out


def standard_run(tag=False, seed=0):
    """the input of the GPU tests: base_names through with_umis, the groups around the tiles and the chain"""
    run = with_umis(base_names(), seed=seed, tag=tag)
    for m, t in ((1, 70), (2, 71), (63, 72), (64, 73), (65, 74), (257, 75)):
        run += nodes_group(m, t, 300 + m, seed=m, prefix=b"n%d." % m)
    run += chain(96)
    if tag:   # every name that carries its UMI in the name carries it in RX:Z as well
        for nm in run:
            at = nm["name"].rfind(b"_")
            if at >= 0 and b"RXZ" not in nm["aux"]:
                nm["aux"] = b"RXZ" + nm["name"][at + 1:][:UMI_MAX] + b"\0" + nm["aux"]
    return run


# ---- record streams in: the command line's inputs ------------------------------------------------------------------------------------
def renamed(rec, name):
    """a framed record ([block_size][record]) under another read name"""
    body = rec[4:]
    l_old = body[8]
    new = body[:8] + bytes([len(name) + 1]) + body[9:32] + name + b"\0" + body[32 + l_old:]
    return struct.pack("<I", len(new)) + new


def with_umis_records(recs, seed=0):
    """with_umis for an input file: every read-name group of `recs` (framed records, collated) re-emitted under <orig>.<j>_<UMI> by
    the same plan -> the framed records"""
    rng = np.random.default_rng(seed)
    groups = []
    for r in recs:
        nm = bytes(r[36:36 + r[12] - 1])
        if groups and groups[-1][0] == nm:
            groups[-1][1].append(r)
        else:
            groups.append((nm, [r]))
    out = []
    for i, (nm, mine) in enumerate(groups):
        kind = PLAN[i % len(PLAN)]
        u = random_umi(rng)
        v = mutate(u, int(rng.integers(len(u))))
        umis = {"exact3": [u] * 3, "exact2": [u] * 2, "join": [u, v, u, v, u], "nojoin": [u, v, v, u], "single": [u], "none": [None, None],
                "tag_only": [None], "long": [u * 4 + b"A"] * 2}[kind]
        for j, x in enumerate(umis):
            name = nm.replace(b"_", b"-") + b".%d" % j + (b"_" + x if x is not None else b"")
            out += [renamed(bytes(r), name) for r in mine]
    return out


def name_groups(stream):
    """the records of an output stream (without block_size) cut where the read name changes -> [(name, [records])]"""
    out = []
    for r in bamio.split_stream(stream):
        nm = bytes(r[32:32 + r[8] - 1])
        if out and out[-1][0] == nm:
            out[-1][1].append(r)
        else:
            out.append((nm, [r]))
    return out
