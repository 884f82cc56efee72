"""Test infrastructure: an adversarial read generator in plain numpy (seeded, no GPU, nothing compiled).

The synthetic generator of the product (bramble_amd/csrc/synth.cpp) writes the CIGAR ops M I D N S, one indel per short
read and clips of at most 5 bases.  This one writes what real aligners write besides: = and X runs (minimap2 --eqx),
hard clips (supplementary records), pads, several indels per exon, an I next to an N, two N in a row, a leading I,
reads whose start and junctions sit on an exon edge and 1-2 bases off it, reads that end inside, at and past the last
exon, CIGARs of more than 8 and of more than 64 ops.  The annotation has genes on both strands, overlapping isoforms
(a dropped middle exon, a shifted last exon end), exons of 1, 2, 5, 20, 35, 36, 120 and 400 bases, introns of 1, 2, 20,
70 and 500 bases, single-exon transcripts, and a gene that starts at reference position 1.

    ann = annotation(seed, n_genes=40, with_genome=False)       the dict lib.Index / ob.OracleIndex take
    recs = reads(ann, n, mode, seed, ...)                       the record dicts bramble_amd.batch.make_batch takes
    recs = near_misses(ann, seed)                               light-class spellings next to their general twins
    b = batch(recs)                                             make_batch(recs)
    stream = bam_stream(recs)                                   the same records as an uncompressed BAM alignment section

alphabet="basic" spells the same reads (same draws, same geometry) with M I D N S alone: = and X become M, H and P go.
"""
import numpy as np

from bramble_amd.batch import make_batch

OPS = "MIDNSHP=X"
M, I, D, N, S, H, P, EQ, X = range(9)
EXON_LENS = (1, 2, 5, 20, 35, 36, 120, 400)
EXON_W = (0.03, 0.03, 0.05, 0.10, 0.10, 0.10, 0.37, 0.22)
INTRON_LENS = (1, 2, 20, 70, 500)
INTRON_W = (0.06, 0.06, 0.28, 0.30, 0.30)
MODES = ("se", "pe", "mm", "long")


def annotation(seed=1, n_genes=40, n_refs=2, with_genome=False):
    """Genes laid side by side on n_refs references; the first gene of reference 0 starts at position 1.  Each gene has
    a base isoform and, where it has the exons for it, one without a middle exon and one with another last exon end.
    Exons are [start, end) 1-based."""
    rng = np.random.RandomState(seed)
    txs = []
    ref_len = [0] * n_refs
    for g in range(n_genes):
        ref = g % n_refs
        strand = "+-"[int(rng.randint(0, 2))]
        n_ex = 1 if rng.rand() < 0.15 else int(rng.randint(2, 13))
        pos = 1 if ref_len[ref] == 0 else ref_len[ref] + int(rng.randint(150, 1200))
        exons = []
        for k in range(n_ex):
            ln = int(rng.choice(EXON_LENS, p=EXON_W))
            exons.append([pos, pos + ln])
            pos += ln + int(rng.choice(INTRON_LENS, p=INTRON_W))
        ref_len[ref] = exons[-1][1] + 40
        txs.append({"id": "g%d.a" % g, "ref_id": ref, "strand": strand, "exons": [list(e) for e in exons]})
        if n_ex >= 3 and rng.rand() < 0.7:
            drop = int(rng.randint(1, n_ex - 1))
            txs.append({"id": "g%d.b" % g, "ref_id": ref, "strand": strand,
                        "exons": [list(e) for k, e in enumerate(exons) if k != drop]})
        if n_ex >= 2 and rng.rand() < 0.7:
            ex = [list(e) for e in exons]
            ex[-1][1] += int(rng.choice([1, 2, 7, 30]))
            ref_len[ref] = max(ref_len[ref], ex[-1][1] + 40)
            txs.append({"id": "g%d.c" % g, "ref_id": ref, "strand": strand, "exons": ex})
    ann = {"refnames": ["adv%d" % r for r in range(n_refs)], "transcripts": txs}
    if with_genome:
        ann["ref_seqs"] = {r: "".join("ACGT"[int(x)] for x in rng.randint(0, 4, size=ref_len[r] + 200))
                           for r in range(n_refs)}
    return ann


def _push(cg, op, ln):
    if ln <= 0:
        return
    if cg and cg[-1][0] == op:
        cg[-1][1] += ln
    else:
        cg.append([op, ln])


def _block(rng, cg, length, dense):
    """One match block of `length` reference bases: runs of M = X, with I / P (no reference bases) and D (reference
    bases, counted in `length`) between the runs.  dense: up to a dozen runs, else a few."""
    if length <= 0:
        return
    u = rng.rand()
    if length == 1 or u < 0.35:
        k = 1
    elif dense:
        k = int(rng.randint(2, 14))
    else:
        k = int(rng.randint(2, 5))
    k = min(k, length)
    cuts = sorted(set(rng.randint(1, length, size=k - 1).tolist())) if k > 1 else []
    edges = [0] + cuts + [length]
    parts = [b - a for a, b in zip(edges[:-1], edges[1:])]
    style = rng.rand()        # one third of the blocks are pure M, the rest mix the three match ops
    for j, ln in enumerate(parts):
        if j:
            v = rng.rand()
            if v < 0.35:
                cg.append([I, int(rng.randint(1, 4))])
            elif v < 0.50:
                cg.append([P, int(rng.randint(1, 4))])
            elif v < 0.56:
                cg.append([I, int(rng.randint(1, 3))])
                cg.append([P, 1])
        if 0 < j < len(parts) - 1 and ln <= 6 and rng.rand() < 0.5:
            cg.append([D, ln])
            continue
        if style < 0.34:
            op = M
        else:
            op = (M, EQ, EQ, X)[int(rng.randint(0, 4))]
            if op == X and ln > 3:
                op = EQ
        _push(cg, op, ln)           # (two runs of one op with nothing between them are one op)


def _edge(rng, p_off):
    """offset of a read edge from the exon edge: 0 (exactly on it) or -2..+2"""
    if rng.rand() >= p_off:
        return 0
    return (-2, -1, 1, 2)[int(rng.randint(0, 4))]


def _one_read(rng, tx, long_read, p_off, p_clip, p_tail_pad, p_long_clip=None, first=None, span=None):
    """-> (ref_start, [[op, len]...], (first exon, last exon)) for one read drawn from transcript tx."""
    ex = tx["exons"]
    n_ex = len(ex)
    i0 = int(rng.randint(0, n_ex)) if first is None else first
    if span is None:
        if long_read:
            span = n_ex - i0 if rng.rand() < 0.5 else int(rng.randint(1, n_ex - i0 + 1))
        else:
            span = min(n_ex - i0, (1, 1, 2, 2, 3, 4)[int(rng.randint(0, 6))])
    i1 = i0 + span - 1
    dense = rng.rand() < (0.45 if long_read else 0.2)
    cg = []
    # where the read starts in its first exon and ends in its last
    s0, e0 = ex[i0]
    u = rng.rand()
    if u < 0.30 or (span > 1 and e0 - s0 <= 2):
        start = s0 + _edge(rng, p_off)
    else:
        start = int(rng.randint(s0, e0))
    start = max(start, 1)
    if span == 1 and start >= e0:
        start = s0
    s1, e1 = ex[i1]
    u = rng.rand()
    if u < 0.25:
        end = e1                                # ends exactly at the exon end
    elif u < 0.33:
        end = e1 + int(rng.randint(1, 4))       # past it
    else:
        lo = max(s1, start) + 1
        end = int(rng.randint(lo, e1 + 1)) if lo <= e1 else e1
    if not long_read and span == 1 and end - start > 150:
        end = start + int(rng.randint(30, 151))
    if end <= start:
        end = start + 1
    pos = start
    for k in range(i0, i1 + 1):
        b_end = end if k == i1 else ex[k][1] + _edge(rng, p_off)
        if b_end <= pos:
            b_end = pos + 1
        _block(rng, cg, b_end - pos, dense)
        if k == i1:
            break
        nxt = ex[k + 1][0] + _edge(rng, p_off)
        if nxt <= b_end:
            nxt = b_end + 1
        gap = nxt - b_end
        u = rng.rand()
        if u < 0.06:
            cg.append([I, int(rng.randint(1, 4))])          # an I directly before the N
        if gap >= 2 and rng.rand() < 0.04:
            a = int(rng.randint(1, gap))
            cg.append([N, a])
            cg.append([N, gap - a])                         # two N in a row
        else:
            cg.append([N, gap])
        if 0.06 <= u < 0.12:
            cg.append([I, int(rng.randint(1, 4))])          # an I directly after the N
        pos = nxt
    if rng.rand() < p_tail_pad:
        # a pad inside the last run of the read: P takes ideal bases without taking reference bases, so what follows lags
        # behind the ideal CIGAR and the read's last ops meet the ideal ops of the end (a rescued clip's override ops)
        for w in range(len(cg) - 1, -1, -1):
            if cg[w][0] in (M, EQ, X) and cg[w][1] >= 2:
                a = int(rng.randint(max(1, cg[w][1] - 8), cg[w][1]))
                tail, left = [], cg[w][1] - a
                while left > 0:             # and a busy tail behind it: runs of 1-2 bases of every reference-taking op
                    ln = min(left, int(rng.randint(1, 3)))
                    op = (M, EQ, X, D, EQ, M)[int(rng.randint(0, 6))]
                    if op == D and ln == left:
                        op = M
                    _push(tail, op, ln)
                    left -= ln
                    if left and rng.rand() < 0.25:
                        tail.append([P, 1])
                cg[w:w + 1] = [[cg[w][0], a], [P, int(rng.randint(2, 9))]] + tail
                break
    front, back = [], []
    p_big = (0.5 if long_read else 0.15) if p_long_clip is None else p_long_clip
    u = rng.rand()
    if u < p_clip:
        kind = int(rng.randint(0, 3))           # H, S, H+S
        big = rng.rand() < p_big
        ln = lambda: int(rng.randint(1, 31)) if big else int(rng.randint(1, 6))
        if kind in (0, 2):
            front.append([H, ln()])
        if kind in (1, 2):
            front.append([S, ln()])
    if rng.rand() < 0.04:
        front.append([I, int(rng.randint(1, 4))])           # a leading I (behind the clips)
    u = rng.rand()
    if u < p_clip:
        kind = int(rng.randint(0, 3))
        big = rng.rand() < p_big
        ln = lambda: int(rng.randint(1, 31)) if big else int(rng.randint(1, 6))
        if kind in (1, 2):
            back.append([S, ln()])
        if kind in (0, 2):
            back.append([H, ln()])
    return start, front + cg + back, (i0, i1)


def _basic(cg):
    """the same read with M I D N S alone"""
    out = []
    for op, ln in cg:
        if op in (H, P):
            continue
        _push(out, M if op in (EQ, X) else op, ln)
    return out


def _words(cg):
    return np.array([(ln << 4) | op for op, ln in cg], dtype=np.uint32)


def _comp(c):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}.get(c, "A")


def _indel(rng, tb, front):
    """half of the rescuable clips of 8 bases and more differ from the transcript by one base lost or gained in the
    middle (the rescue's alignment then holds a gap); the length stays"""
    if len(tb) < 8 or rng.rand() >= 0.5:
        return tb
    # (behind the read the gap sits in the clip's first bases, where a read that lags behind its ideal CIGAR meets it)
    m = int(rng.randint(3, len(tb) - 3)) if front else int(rng.randint(1, 4))
    if rng.rand() < 0.5:
        return tb[:m] + tb[m + 1:]
    t = tb[:m] + _comp(tb[m]) + tb[m:]
    return t[1:] if front else t[:-1]


def _sequence(rng, ann, tx, start, cg, rescuable):
    """SEQ of the read, reference-forward as BAM stores it: genome bases under M / =, another base under X, random
    inserted bases, and for the soft clips either the transcript's neighbouring bases (the clip rescue finds them; see
    _indel) or random ones."""
    g = ann["ref_seqs"][tx["ref_id"]]
    tseq_pos = []     # genomic position of every transcript base
    for s, e in tx["exons"]:
        tseq_pos.extend(range(s, e))
    index = {p: k for k, p in enumerate(tseq_pos)}
    rnd = lambda n: "".join("ACGT"[int(x)] for x in rng.randint(0, 4, size=n))
    pos = start
    out = []
    first_ref, last_ref = None, None
    for op, ln in cg:
        if op in (M, EQ, X):
            if first_ref is None:
                first_ref = pos
            seg = g[pos - 1:pos - 1 + ln]
            seg = seg + "A" * (ln - len(seg))
            out.append((op, "".join(_comp(c) for c in seg) if op == X else seg))
            pos += ln
            last_ref = pos - 1
        elif op in (D, N):
            pos += ln
        elif op == I:
            out.append((op, rnd(ln)))
        elif op == S:
            out.append((op, None, ln))
    res = []
    seen_match = False
    for item in out:
        if item[0] != S:
            seen_match = True
            res.append(item[1])
            continue
        ln = item[2]
        if not rescuable or first_ref is None:
            res.append(rnd(ln))
        elif not seen_match:    # front clip: the transcript bases before the first aligned base
            k = index.get(first_ref)
            tb = "" if k is None else "".join(g[p - 1] for p in tseq_pos[max(0, k - ln):k])
            tb = _indel(rng, tb, True)
            res.append(rnd(ln - len(tb)) + tb)
        else:
            k = index.get(last_ref)
            tb = "" if k is None else "".join(g[p - 1] for p in tseq_pos[k + 1:k + 1 + ln])
            tb = _indel(rng, tb, False)
            res.append(tb + rnd(ln - len(tb)))
    return "".join(res)


def _qlen(cg):
    return int(sum(ln for op, ln in cg if op in (M, I, S, EQ, X)))


def _r1_forward(rng, tx, orient, p=0.9):
    """Orientation of a single-end read or of read 1 of a pair (its mate faces the other way).  Under --fr a forward
    read 1 (or single-end read) takes the '-' strand, under --rf the '+' strand (read_strand in the oracle,
    src/bramble.cpp:213-244): with orient set, nine reads in ten are turned so that the rule gives their transcript's
    strand; the rest, and every read without orient, are turned at random."""
    if orient in ("fr", "rf") and rng.rand() < p:
        return (tx["strand"] == "-") == (orient == "fr")
    return rng.rand() < 0.5


def reads(ann, n, mode="se", seed=1, alphabet="full", with_seq=False, orient=None, p_off=0.12, p_clip=0.3,
          p_tail_pad=0.15, p_long_clip=None, p_same_tx=0.85, prefix="r"):
    """n read names -> record dicts in name-collated order.

    mode   "se" single-end short reads; "pe" two records per name (0x1|0x40, 0x1|0x80, mate fields set; a share of the
           mates lies on another transcript, a few are unmapped, a few names carry two pairs); "mm" multi-mappers (1-4
           records per name, all but the first secondary); "long" reads that span up to every exon of their transcript.
    orient "fr" / "rf": reads are turned so that the --fr / --rf rule gives the strand of their transcript (_r1_forward).
    p_off  share of read edges and junctions that sit 1-2 bases off the exon edge; p_clip share of read ends that carry
           H, S or both; p_tail_pad share of reads with a pad and a busy tail before their end (see _one_read); p_long_clip
           share of the clips that are 1-30 bases long and not 1-5 (default: half for long reads, 0.15 otherwise).
    with_seq needs annotation(with_genome=True): records carry SEQ (clipped bases rescuable or random, half each)."""
    assert mode in MODES and alphabet in ("full", "basic")
    rng = np.random.RandomState(seed)
    txs = ann["transcripts"]
    long_read = mode == "long"
    out = []

    def rec(name, tx, flags, mate=None, **kw):
        start, cg, _ = _one_read(rng, tx, long_read, p_off, p_clip, p_tail_pad, p_long_clip, **kw)
        rescuable = rng.rand() < 0.5
        if alphabet == "basic":
            cg = _basic(cg)
        r = {"name": name, "ref_id": tx["ref_id"], "ref_start": start, "cigar": _words(cg), "flags": flags,
             "read_len": _qlen(cg)}
        if with_seq:
            r["seq"] = _sequence(rng, ann, tx, start, cg, rescuable)
        return r

    for k in range(n):
        name = "%s%d" % (prefix, k)
        t = int(rng.randint(0, len(txs)))
        tx = txs[t]
        rev = 0 if _r1_forward(rng, tx, orient) else 0x10
        if mode in ("se", "long"):
            out.append(rec(name, tx, rev))
            if long_read and rng.rand() < 0.05:       # a supplementary-style second record of the same name
                out.append(rec(name, txs[int(rng.randint(0, len(txs)))], 0x100 | rev))
        elif mode == "mm":
            m = (1, 2, 2, 3, 4)[int(rng.randint(0, 5))]
            for j in range(m):
                txj = tx if j == 0 or rng.rand() < 0.4 else txs[int(rng.randint(0, len(txs)))]
                if j:
                    rev = 0 if _r1_forward(rng, txj, orient) else 0x10
                out.append(rec(name, txj, rev | (0x100 if j else 0)))
        else:
            for j in range(2 if rng.rand() < 0.1 else 1):      # a few names carry two pairs
                sec = 0x100 if j else 0
                if j:
                    tx = txs[int(rng.randint(0, len(txs)))]
                u = rng.rand()
                r1_fwd = _r1_forward(rng, tx, orient)
                f1 = 0x1 | 0x40 | sec | (0 if r1_fwd else 0x10) | (0x20 if r1_fwd else 0)
                f2 = 0x1 | 0x80 | sec | (0x10 if r1_fwd else 0) | (0 if r1_fwd else 0x20)
                a = rec(name, tx, f1)
                if u < 0.05:                                   # the mate is unmapped: its record is absent
                    a["flags"] |= 0x8
                    out.append(a)
                    continue
                tx2 = tx if u < 0.05 + p_same_tx else txs[int(rng.randint(0, len(txs)))]
                b = rec(name, tx2, f2)
                a["mate_ref_id"], a["mate_start"] = b["ref_id"], b["ref_start"]
                b["mate_ref_id"], b["mate_start"] = a["ref_id"], a["ref_start"]
                out.extend([a, b])
    return out


def near_misses(ann, seed=1, alphabet="full", per_site=1, orient=None):
    """Reads that match one exon, or two exons through the annotated junction, exactly in coordinates -- spelled once
    as M / M N M (the two light emit classes) and once each with =, X, M/= mixes and with H, S, P added: single-end
    records of every spelling, then pairs whose two mates are different spellings (a light one beside a general one),
    then a multi-mapper name holding every spelling of one site."""
    rng = np.random.RandomState(seed)
    out = []
    serial = [0]

    def spell_one(ln):
        a = max(1, ln // 3)
        sp = [[[M, ln]], [[EQ, ln]], [[X, ln]]]
        if ln >= 2:
            sp += [[[M, a], [EQ, ln - a]], [[EQ, a], [M, ln - a]], [[M, ln - 1], [X, 1]], [[M, a], [P, 2], [M, ln - a]],
                   [[EQ, a], [P, 1], [X, ln - a]]]
        sp += [[[H, 3], [M, ln]], [[M, ln], [H, 30]], [[H, 2], [M, ln], [H, 2]], [[S, 3], [M, ln]], [[M, ln], [S, 2]],
               [[H, 4], [S, 1], [M, ln], [S, 5], [H, 1]], [[S, 2], [EQ, ln]], [[H, 1], [EQ, ln]]]
        return sp

    def spell_two(x, gap, y):
        sp = [[[M, x], [N, gap], [M, y]], [[EQ, x], [N, gap], [EQ, y]], [[M, x], [N, gap], [EQ, y]],
              [[EQ, x], [N, gap], [M, y]], [[M, x], [N, gap], [X, y]], [[X, x], [N, gap], [M, y]],
              [[H, 3], [M, x], [N, gap], [M, y]], [[M, x], [N, gap], [M, y], [H, 7]],
              [[S, 2], [M, x], [N, gap], [M, y]], [[M, x], [N, gap], [M, y], [S, 4]],
              [[H, 2], [S, 3], [M, x], [N, gap], [M, y], [S, 1], [H, 9]]]
        if y >= 2:
            sp += [[[M, x], [N, gap], [M, 1], [P, 2], [M, y - 1]], [[M, x], [N, gap], [M, 1], [EQ, y - 1]]]
        if x >= 2:
            sp += [[[M, x - 1], [P, 1], [M, 1], [N, gap], [M, y]], [[EQ, x - 1], [M, 1], [N, gap], [M, y]]]
        if gap >= 2:
            sp += [[[M, x], [N, 1], [N, gap - 1], [M, y]]]
        return sp

    def add(name, tx, start, cg, flags=0, **mate):
        if alphabet == "basic":
            cg = _basic(cg)
        r = {"name": name, "ref_id": tx["ref_id"], "ref_start": start, "cigar": _words(cg), "flags": flags,
             "read_len": _qlen(cg)}
        r.update(mate)
        out.append(r)
        return r

    sites = []      # (tx, start, spellings)
    for tx in ann["transcripts"]:
        ex = tx["exons"]
        for _ in range(per_site):
            k = int(rng.randint(0, len(ex)))
            s, e = ex[k]
            a = int(rng.randint(s, e))
            b = int(rng.randint(a + 1, e + 1))
            if rng.rand() < 0.3:
                a, b = s, e                       # the whole exon, edge to edge
            sites.append((tx, a, spell_one(b - a)))
            if len(ex) >= 2:
                k = int(rng.randint(0, len(ex) - 1))
                (s0, e0), (s1, e1) = ex[k], ex[k + 1]
                x = int(rng.randint(1, min(e0 - s0, 90) + 1))
                y = int(rng.randint(1, min(e1 - s1, 90) + 1))
                sites.append((tx, e0 - x, spell_two(x, s1 - e0, y)))
    for tx, start, sps in sites:                  # single-end, every spelling
        for cg in sps:
            serial[0] += 1
            add("nm%d" % serial[0], tx, start, cg, 0 if _r1_forward(rng, tx, orient) else 0x10)
    by_tx = {}
    for tx, start, sps in sites:
        by_tx.setdefault(tx["id"], []).append((tx, start, sps))
    for lst in by_tx.values():                    # pairs within one transcript: spelling j beside spelling j + 1 (0 = light)
        for q in range(len(lst)):
            (tx, sa, spa), (_, sb, spb) = lst[q], lst[(q + 1) % len(lst)]
            for j in range(max(len(spa), len(spb))):
                ca, cb = spa[j % len(spa)], spb[(j + 1) % len(spb)]
                serial[0] += 1
                name = "np%d" % serial[0]
                fwd = _r1_forward(rng, tx, orient)
                add(name, tx, sa, ca, 0x1 | 0x40 | (0 if fwd else 0x10), mate_ref_id=tx["ref_id"], mate_start=sb)
                add(name, tx, sb, cb, 0x1 | 0x80 | (0x10 if fwd else 0), mate_ref_id=tx["ref_id"], mate_start=sa)
    for tx, start, sps in sites[:: max(1, len(sites) // 12)]:     # every spelling of one site under one name
        serial[0] += 1
        for j, cg in enumerate(sps):
            add("nq%d" % serial[0], tx, start, cg, (0x100 if j else 0) | (0 if _r1_forward(rng, tx, orient, 1.0) else 0x10))
    return out


def batch(records):
    return make_batch(records)


def bam_stream(records):
    """The records as an uncompressed BAM alignment section ([block_size][record]...), through tests/bamio.py."""
    from tests import bamio
    code = {c: k for k, c in enumerate("=ACMGRSVTWYHKDBN")}
    recs = []
    for r in records:
        cg = r["cigar"]
        lq = r["read_len"]
        seq = None
        if r.get("seq"):
            s = r["seq"]
            nib = [code[c] for c in s] + [0]
            seq = bytes((nib[2 * k] << 4) | nib[2 * k + 1] for k in range((len(s) + 1) // 2))
        mate = (r.get("mate_ref_id", -1), r.get("mate_start", 0) - 1, 0)
        recs.append(bamio.bam_record(r["name"].encode(), r["ref_id"], r["ref_start"] - 1, cg, lq, flag=r.get("flags", 0),
                                     aux=b"NMC\x00", mate=mate, seq=seq))
    return bamio.frame(recs)
