"""Hand-built reads for the -S soft-clip rescue's front end (test infrastructure: no GPU, no test functions), one decision
of k_project_fa / k_fa_fill / clip_segment / apply_clips per case.  tests/test_rescue_cases_cpu.py checks on the CPU that
every case sits on the edge it names (its predicate, asked of tests/rescue_ref.py's answer, never of a kernel) and that
the restatement and the oracle agree; tests/test_gpu_rescue_cases.py runs the cases through every route.

The annotation: one reference of about 16 kb, generated from SEED, every locus once per strand:

  three   100 / 100 / 100           the workhorse: anchor in the middle, a neighbour longer than qlen + 40 on either side
  low     100 / 100 / 100           the outer exons (and the introns next to them) lower-case in the reference sequence
  nn      100 / 100 / 100           an N in either outer exon, 3 bases from the junction
  runs    90 7 1 6 / 80 / 6 1 7 90  short exons on either side of the anchor, a long one behind them
  edge    3 1 6 / 80 / 6 1 3        short exons up to the transcript's edge: 10 bases on either side
  long    500 / 100 / 500           room for a clip of 400 bases: a target beyond the register-array shapes of k_ksw_dp
  longn   500 / 100 / 500           the same with an N in either outer exon
  dozen   100 / 100 / 100, 12 x     more candidate rows than FA_GROUP_LANES
  crowd   100 / 100 / 100, 70 x     more than 64 candidate rows: k_project_fa<3>'s own emit
  end     100 / 81 or 66            the last exon runs 20 (25) bases past the end of the reference sequence

A read is one block on the anchor exon (or two blocks, `span`), its clip written from the junction outwards: J[0] is the
base next to the anchor.  `nb` takes such bases from the spliced neighbour exons, `comp` makes them foreign (A<->C, G<->T:
a mismatch at every base, nothing left to chance).  Every read here is a plain read in tests/rescue_ref.py's sense, so
every case has final rows."""
import functools

import numpy as np

from tests import rescue_ref as rr

SEED = 8128
INTRON = 60
SPECS = (("three", (100, 100, 100), 1), ("low", (100, 100, 100), 1), ("nn", (100, 100, 100), 1),
         ("runs", (90, 7, 1, 6, 80, 6, 1, 7, 90), 1), ("edge", (3, 1, 6, 80, 6, 1, 3), 1), ("long", (500, 100, 500), 1),
         ("longn", (500, 100, 500), 1), ("dozen", (100, 100, 100), 12), ("crowd", (100, 100, 100), 70))
ANCHOR = {"three": 1, "low": 1, "nn": 1, "runs": 4, "edge": 3, "long": 1, "longn": 1, "dozen": 1, "crowd": 1, "end": 0}
N_OFF = {"nn": 3, "longn": 100}     # distance of the planted N from the junction


@functools.lru_cache(maxsize=None)
def annotation():
    """-> the annotation dict lib.Index / ob.OracleIndex take: refnames, transcripts, ref_seqs"""
    rng = np.random.RandomState(SEED)
    txs, loci, p = [], {}, 201
    for strand in "+-":
        for name, lens, copies in SPECS:
            exons = []
            for n in lens:
                exons.append([p, p + n])
                p += n + INTRON
            p += 140
            loci[name + strand] = exons
            for c in range(copies):
                txs.append({"id": name + strand + (".%d" % c if copies > 1 else ""), "ref_id": 0, "strand": strand, "exons": exons})
    size = p + 400
    loci["end+"] = [[size - 300, size - 200], [size - 60, size + 21]]
    loci["end-"] = [[size - 190, size - 100], [size - 40, size + 26]]
    for strand in "+-":
        txs.append({"id": "end" + strand, "ref_id": 0, "strand": strand, "exons": loci["end" + strand]})
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, size)].copy()      # g[k] is 1-based position k + 1
    for strand in "+-":
        for name, off in N_OFF.items():
            ex = loci[name + strand]
            a = ANCHOR[name]
            g[ex[a - 1][1] - 1 - off - 1] = ord("N")      # left neighbour: `off` bases between the N and the exon's end
            g[ex[a + 1][0] + off - 1] = ord("N")
        ex = loci["low" + strand]
        for s, e in (ex[0], ex[2]):
            g[s - 1 - 10:e - 1 + 10] |= 0x20
    genome = g.tobytes().decode()
    assert genome[loci["low+"][0][0] - 1:loci["low+"][0][1] - 1].islower() and len(genome) == size
    return {"refnames": ["chr1"], "transcripts": txs, "ref_seqs": {0: genome}}


def tx_of(name):
    return next(t for t in annotation()["transcripts"] if t["id"] in (name, name + ".0"))


def genome():
    return annotation()["ref_seqs"][0]


def comp(s):
    return s.translate(str.maketrans("ACGTN", "CATGA"))


def nb(tx, anchor, side, n, skip=0, keep_n=False):
    """n bases of the spliced neighbour exons, from the junction outwards, leaving out the `skip` nearest; an N of the
    reference is written as A unless keep_n (the read then disagrees with the N, as any base does)"""
    seqs = [rr.exon_sequence(genome(), s, e) for s, e in tx["exons"]]
    j = "".join(seqs[:anchor])[::-1] if side == "left" else "".join(seqs[anchor + 1:])
    out = j[skip:skip + n]
    assert len(out) == n
    return out if keep_n else out.replace("N", "A")


def record(name, tx, first, last, left="", right="", lover="", rover="", loff=0, roff=0, seq=True):
    """One alignment: blocks on exons first..last of tx; left / right: the clips and lover / rover the bases the first /
    last block hangs over its exon, all written from the junction outwards; loff / roff: bases the block begins / ends
    inside its exon.  seq: True = the read's own sequence, a string = that one, None = the record carries none."""
    g, ex = genome(), tx["exons"]
    words, body = [], ""
    for i in range(first, last + 1):
        s, e = ex[i]
        s += loff if i == first else 0
        e -= roff if i == last else 0
        n = e - s + (len(lover) if i == first else 0) + (len(rover) if i == last else 0)
        words.append("%dM" % n)
        if i < last:
            words.append("%dN" % (ex[i + 1][0] - e))
        body += g[s - 1:e - 1].upper()
    start = ex[first][0] + loff - len(lover)
    text = ("%dS" % len(left) if left else "") + "".join(words) + ("%dS" % len(right) if right else "")
    own = left[::-1] + lover[::-1] + body + rover + right
    rec = {"name": name, "ref_id": 0, "ref_start": start, "cigar": text, "read_len": len(own)}
    rec["seq"] = own if seq is True else (seq or "")
    return rec


class Case:
    """id; about: the decision; records; pred: what must hold of rescue_ref's answers A (per record a list of (transcript
    index, answers) for the transcripts the read lies on) for the case to be on its edge"""

    def __init__(self, cid, about, records, pred):
        self.id, self.about, self.records, self.pred = cid, about, records, pred

    @functools.lru_cache(maxsize=None)
    def answers(self):
        return answers_of(self.records)


def answers_of(records, preset="lr"):
    """rescue_ref's answers for a name-collated list of records: per record [(transcript index, answers)]"""
    from bramble_amd.batch import parse_cigar
    ann = annotation()
    out, k = [], 0
    while k < len(records):
        j = k
        while j < len(records) and records[j]["name"] == records[k]["name"]:
            j += 1
        seq = rr.shared_sequence([r.get("seq") or "" for r in records[k:j]])
        for r in records[k:j]:
            real = parse_cigar(r["cigar"])
            per = []
            for t, tx in enumerate(ann["transcripts"]):
                a = rr.answers(tx, ann["ref_seqs"][0], r["ref_start"], real, seq, preset)
                if a is not None:
                    per.append((t, a))
            out.append(per)
        k = j
    return out


def expected(records, preset="lr"):
    """-> (rows sorted [[record, transcript id, pos, strand, cigar, clip_score]], problems, rescued) by rescue_ref"""
    from bramble_amd.batch import parse_cigar
    ann = annotation()
    rows, problems, rescued = [], 0, 0
    for k, per in enumerate(answers_of(records, preset)):
        for t, a in per:
            problems += a["left"]["exists"] + a["right"]["exists"]
            rescued += a["left"]["accepted"] + a["right"]["accepted"]
            tx = ann["transcripts"][t]
            row = rr.plain_row(tx, records[k]["ref_start"], parse_cigar(records[k]["cigar"]), a, preset)
            if row is not None:
                rows.append([k, tx["id"], row["pos"], row["strand"], row["cigar"], row["clip_score"]])
    return sorted(rows), int(problems), int(rescued)


def _one(A):
    assert len(A) == 1 and len(A[0]) == 1, [len(x) for x in A]
    return A[0][0][1]


def _has(ops, n, op):
    return (n, op) in [tuple(o) for o in ops]


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(cid, about, records, pred):
        out.append(Case(cid, about, records if isinstance(records, list) else [records], pred))

    for strand in "+-":
        T = {name: tx_of(name + strand) for name, _, _ in SPECS}
        T["end"] = tx_of("end" + strand)
        for side in ("left", "right"):
            tag = "%s%s" % (strand, side[0].upper())
            near, far = (-1, 0) if side == "left" else (0, -1)      # the override op nearest to / farthest from the anchor

            def one(name, txn, clip, anchor=None, **kw):
                tx = T[txn]
                a = ANCHOR[txn] if anchor is None else anchor
                kw.update({"left": clip} if side == "left" else {"right": clip})
                return record("%s.%s" % (name, tag), tx, a, a, **kw)

            def J(txn, n, skip=0, anchor=None, **kw):
                return nb(T[txn], ANCHOR[txn] if anchor is None else anchor, side, n, skip, **kw)

            S = lambda A, side=side: _one(A)[side]      # noqa: E731  the side the case is about

            add("clip4." + tag, "fewer than 5 clipped bases: no problem", one("clip4", "three", J("three", 4)),
                lambda A, S=S: not S(A)["exists"] and S(A)["why"] == "clip shorter than 5")
            add("clip5." + tag, "5 clipped bases make a problem; it scores 5 and is rejected", one("clip5", "three", J("three", 5)),
                lambda A, S=S: S(A)["exists"] and S(A)["max"] == 5 and not S(A)["accepted"])
            add("score9." + tag, "best score 9: rejected", one("score9", "three", J("three", 9)),
                lambda A, S=S: S(A)["exists"] and S(A)["max"] == 9 and not S(A)["accepted"])
            add("score10." + tag, "best score 10: accepted", one("score10", "three", J("three", 10)),
                lambda A, S=S: S(A)["max"] == 10 and S(A)["accepted"] and S(A)["refc"] == 10)
            add("tN10." + tag, "an N in the target lowers an accepted score to exactly 10", one("tN10", "nn", J("nn", 12)),
                lambda A, S=S: S(A)["t_has_n"] and not S(A)["q_has_n"] and S(A)["max"] == 10 and S(A)["accepted"] and len(S(A)["query"]) == 12)
            add("tN9." + tag, "an N in the target lowers an accepted score to 9", one("tN9", "nn", J("nn", 11)),
                lambda A, S=S: S(A)["t_has_n"] and S(A)["max"] == 9 and not S(A)["accepted"] and len(S(A)["query"]) == 11)
            qn = J("three", 14)
            add("qN." + tag, "an N in the query", one("qN", "three", qn[:5] + "N" + qn[6:]),
                lambda A, S=S: S(A)["q_has_n"] and not S(A)["t_has_n"] and S(A)["max"] == 12 and S(A)["accepted"])
            add("iupac." + tag, "IUPAC codes other than N in the query count as N", one("iupac", "three", qn[:4] + "R" + qn[5:9] + "y" + qn[10:]),
                lambda A, S=S: S(A)["q_has_n"] and "N" not in S(A)["query"].upper() and S(A)["max"] == 10 and S(A)["accepted"])
            add("lower." + tag, "a lower-case target is upper-cased", one("lower", "low", J("low", 12)),
                lambda A, S=S: S(A)["target"].isupper() and S(A)["max"] == 12 and S(A)["accepted"])
            add("edge_exon." + tag, "anchor on the transcript's first / last exon: no neighbour, no problem",
                one("edge_exon", "three", comp(J("three", 12)), anchor=0 if side == "left" else 2),
                lambda A, S=S: not S(A)["exists"] and S(A)["why"] == "no neighbour exon")
            add("second." + tag, "anchor on the second / second-to-last exon: one neighbour", one("second", "three", J("three", 20)),
                lambda A, S=S: S(A)["exists"] and S(A)["n_exons"] == 1 and S(A)["accepted"] and S(A)["max"] == 20)
            add("gap." + tag, "the block begins / ends 3 bases inside its exon: the gap suppresses the rescue",
                one("gap", "three", J("three", 12), **({"loff": 3} if side == "left" else {"roff": 3})),
                lambda A, S=S: not S(A)["exists"] and S(A)["why"] == "gap")
            add("overhang." + tag, "the block hangs 3 bases over its exon: they join the query and the rescue clears them",
                one("overhang", "three", J("three", 12, skip=3), **({"lover": J("three", 3)} if side == "left" else {"rover": J("three", 3)})),
                lambda A, S=S: S(A)["overhang"] == 3 and len(S(A)["query"]) == 15 and S(A)["max"] == 15 and S(A)["accepted"])
            add("overhang_kept." + tag, "an overhang whose rescue is rejected stays a clip",
                one("overhang_kept", "three", comp(J("three", 12, skip=3)), **({"lover": comp(J("three", 3))} if side == "left" else {"rover": comp(J("three", 3))})),
                lambda A, S=S: S(A)["overhang"] == 3 and len(S(A)["query"]) == 15 and S(A)["exists"] and not S(A)["accepted"])
            add("one_long." + tag, "one neighbour exon longer than qlen + 40: trimmed", one("one_long", "three", J("three", 12)),
                lambda A, S=S: S(A)["n_exons"] == 1 and S(A)["trimmed"] and len(S(A)["target"]) == 52 and S(A)["accepted"])
            add("to_edge." + tag, "short exons up to the transcript's edge, together shorter than the query",
                one("to_edge", "edge", J("edge", 10) + comp(J("three", 5))),
                lambda A, S=S: S(A)["n_exons"] == 3 and S(A)["collected"] == 10 < len(S(A)["query"]) and not S(A)["trimmed"] and S(A)["max"] == 10 and S(A)["accepted"])
            add("three_short." + tag, "a target of three exons of 6 + 1 + 7 bases", one("three_short", "runs", J("runs", 12)),
                lambda A, S=S: S(A)["n_exons"] == 3 and S(A)["collected"] == 14 and not S(A)["trimmed"] and S(A)["max"] == 12 and S(A)["accepted"])
            add("trim_inside." + tag, "several short exons and a long one: trimmed inside the last one collected", one("trim_inside", "runs", J("runs", 20)),
                lambda A, S=S: S(A)["n_exons"] == 4 and S(A)["collected"] == 104 and S(A)["trimmed"] and len(S(A)["target"]) == 60 and S(A)["max"] == 20)
            add("foreign." + tag, "a foreign stretch outside a matching one: the remainder stays S", one("foreign", "three", J("three", 12) + comp(J("three", 3, skip=12))),
                lambda A, S=S, far=far: S(A)["max"] == 12 and S(A)["accepted"] and tuple(S(A)["ops"][far]) == (3, rr.CLIP_OVR))
            add("del2." + tag, "a 2-base deletion directly at the anchor", one("del2", "three", J("three", 30, skip=2)),
                lambda A, S=S, near=near: S(A)["accepted"] and tuple(S(A)["ops"][near]) == (2, rr.DEL_OVR) and S(A)["refc"] == 32)
            add("ins2." + tag, "a 2-base insertion directly at the anchor", one("ins2", "three", comp(J("three", 2)) + J("three", 30)),
                lambda A, S=S, near=near: S(A)["accepted"] and tuple(S(A)["ops"][near]) == (2, rr.INS_OVR) and S(A)["refc"] == 30)
            add("midgap." + tag, "a gap in the middle of the clip", one("midgap", "three", J("three", 15) + J("three", 15, skip=17)),
                lambda A, S=S: S(A)["accepted"] and len(S(A)["ops"]) == 3 and tuple(S(A)["ops"][1]) == (2, rr.DEL_OVR) and S(A)["refc"] == 32)
            add("long." + tag, "a clip of 400 bases: a target beyond the register-array shapes", one("long", "long", J("long", 400)),
                lambda A, S=S: len(S(A)["target"]) == 440 and not S(A)["t_has_n"] and S(A)["max"] == 400 and S(A)["accepted"])
            add("longN." + tag, "the same with an N in the target", one("longN", "longn", J("longn", 400)),
                lambda A, S=S: len(S(A)["target"]) == 440 and S(A)["t_has_n"] and S(A)["max"] == 398 and S(A)["accepted"])
            add("crowd." + tag, "more than 64 candidate rows, the clip rescued on each", one("crowd", "crowd", J("crowd", 16)),
                lambda A, side=side: len(A[0]) == 70 and all(a[side]["accepted"] and a[side]["max"] == 16 for _, a in A[0]))
            # two blocks: the far end of the chain decides pos on '-'
            tx = T["three"]
            if side == "left":
                span = record("span." + tag, tx, 1, 2, left=nb(tx, 1, "left", 18))
            else:
                span = record("span." + tag, tx, 0, 1, right=nb(tx, 1, "right", 18))
            add("span." + tag, "a read of two blocks, the clip beyond its outer junction", span,
                lambda A, S=S: S(A)["accepted"] and S(A)["max"] == 18 and _one(A)["place"]["last"] - _one(A)["place"]["first"] == 1)
            # the read-name group's shared sequence
            good = one("group", "three", J("three", 12))
            bad = one("group", "three", comp(J("three", 12)))
            add("group." + tag, "the first record has no sequence, the second one, the third another: all use the second's",
                [dict(good, seq=""), good, bad],
                lambda A, side=side: len(A) == 3 and all(len(p) == 1 and p[0][1][side]["accepted"] and p[0][1][side]["max"] == 12 for p in A))
            short = nb(tx, 1, side, 20)
            short = short[::-1] if side == "left" else short
            holder = dict(record("cap." + tag, tx, 1, 1, loff=30, roff=50), seq=short)
            assert holder["cigar"] == "20M" and len(short) == 20
            sec = dict(one("cap", "three", J("three", 30)), seq="")
            add("cap." + tag, "a secondary record's clip of 30 bases against a shared sequence of 20: the query is capped", [holder, sec],
                lambda A, side=side: A[1][0][1][side]["capped"] and len(A[1][0][1][side]["query"]) == 20 and A[1][0][1][side]["max"] == 20
                and A[1][0][1][side]["accepted"] and not A[0][0][1][side]["exists"])
            add("noseq." + tag, "a group without any sequence: no problem",
                [dict(one("noseq", "three", J("three", 12)), seq=""), record("noseq_other." + tag, tx, 1, 1)],
                lambda A, side=side: not A[0][0][1][side]["exists"] and A[0][0][1][side]["why"] == "no sequence")
        # right side only: the reference sequence has one end that an exon can run past
        tag = strand + "R"
        tx = T["end"]
        n_fill = tx["exons"][1][1] - 1 - len(genome())             # positions of the last exon beyond the sequence
        n_real = tx["exons"][1][1] - tx["exons"][1][0] - n_fill
        add("past_end." + tag, "a target that reaches past the end of the reference sequence: N-filled",
            record("past_end." + tag, tx, 0, 0, right=nb(tx, 0, "right", n_real) + "ACGTACGTAC"),
            lambda A, n_fill=n_fill, n_real=n_real: n_fill >= 20 and _one(A)["right"]["target"].endswith("N" * n_fill)
            and not _one(A)["right"]["target"].endswith("N" * (n_fill + 1)) and _one(A)["right"]["t_has_n"]
            and _one(A)["right"]["max"] == n_real and _one(A)["right"]["accepted"])
        # both ends
        tx = T["three"]
        L, R = nb(tx, 1, "left", 14), nb(tx, 1, "right", 14)
        add("both." + strand, "both ends clipped, both rescued", record("both." + strand, tx, 1, 1, left=L, right=R),
            lambda A: _one(A)["left"]["accepted"] and _one(A)["right"]["accepted"])
        add("both_left." + strand, "both ends clipped, the left one rescued", record("both_left." + strand, tx, 1, 1, left=L, right=comp(R)),
            lambda A: _one(A)["left"]["accepted"] and _one(A)["right"]["exists"] and not _one(A)["right"]["accepted"])
        add("both_right." + strand, "both ends clipped, the right one rescued", record("both_right." + strand, tx, 1, 1, left=comp(L), right=R),
            lambda A: _one(A)["right"]["accepted"] and _one(A)["left"]["exists"] and not _one(A)["left"]["accepted"])
        add("both_none." + strand, "both ends clipped, neither rescued", record("both_none." + strand, tx, 1, 1, left=comp(L), right=comp(R)),
            lambda A: _one(A)["left"]["exists"] and _one(A)["right"]["exists"] and not _one(A)["left"]["accepted"] and not _one(A)["right"]["accepted"])
        tx = T["dozen"]
        add("dozen." + strand, "12 identical transcripts, both ends clipped: 24 problems of one alignment",
            record("dozen." + strand, tx, 1, 1, left=nb(tx, 1, "left", 13), right=nb(tx, 1, "right", 17)),
            lambda A: len(A[0]) == 12 and sum(a["left"]["exists"] + a["right"]["exists"] for _, a in A[0]) == 24
            and all(a["left"]["max"] == 13 and a["right"]["max"] == 17 for _, a in A[0]))
    assert len({c.id for c in out}) == len(out)
    return out


def fillers():
    """alignments that want no rescue: unclipped, clipped by fewer than 5 bases, or off every transcript"""
    out = []
    for k, (name, first, last) in enumerate((("three+", 0, 2), ("runs-", 0, 8), ("edge+", 3, 3), ("dozen-", 0, 1), ("long+", 1, 2),
                                             ("low-", 1, 1), ("nn+", 0, 0), ("end+", 0, 0), ("crowd+", 2, 2), ("longn-", 0, 1))):
        tx = tx_of(name)
        out.append(record("fill%d" % k, tx, first, last, left="ACG" if k % 3 == 0 else "", loff=k % 2 * 4, roff=k % 4))
    out.append({"name": "nowhere", "ref_id": 0, "ref_start": 60, "cigar": "9S80M", "read_len": 89, "seq": "ACGTTGCAG" + genome()[59:139].upper()})
    return out


def groups_of(records):
    out = []
    for r in records:
        if out and out[-1][0]["name"] == r["name"]:
            out[-1].append(r)
        else:
            out.append([r])
    return out


@functools.lru_cache(maxsize=None)
def mixed(reverse=False):
    """every case's records in one name-collated list with the fillers between them; reverse: the groups in reversed order"""
    fill = fillers()
    groups, k = [], 0
    for i, c in enumerate(cases()):
        groups += groups_of(c.records)
        if i % 9 == 4:
            groups.append([dict(fill[k % len(fill)], name="fill%d.%d" % (k % len(fill), k))])
            k += 1
    if reverse:
        groups = groups[::-1]
    return [r for g in groups for r in g]


@functools.lru_cache(maxsize=None)
def crowded(n=16):
    """n reads on the 70-transcript locus, both ends clipped by their neighbours' bases: 140 problems each, with mixed() more
    than the 2048 problems the streamed DP wants before it cuts a call into pieces"""
    tx = tx_of("crowd+")
    return mixed() + [record("crowded%d" % k, tx, 1, 1, left=nb(tx, 1, "left", 20 + 2 * k), right=nb(tx, 1, "right", 51 - 2 * k)) for k in range(n)]


def batch_of(records):
    """the flat batch of a record list; it always carries a sequence table (a -S call is refused without one)"""
    from bramble_amd.batch import make_batch
    b = make_batch(records)
    if b["seq_off"] is None:
        b["seq_off"] = np.zeros(len(records) + 1, dtype=np.uint64)
        b["seqs"] = np.zeros(0, dtype=np.uint8)
    return b
