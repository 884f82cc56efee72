"""An independent statement of the -S soft-clip rescue's front end (test infrastructure: no GPU, no test functions), written
from the reference's source alone -- src/evaluate.cpp:319-656, src/g2t.cpp:50-55,103-257, src/core.cpp:353-378 and, for the
final row of a plain read, src/evaluate.cpp:658-786,824-886 and src/bam.cpp:22-315.  Nothing here comes from oracle/ or
from the kernels; the DP is tests/ksw2_check.gotoh (the full-matrix checker, independent of both).

What it answers, for a read that lies on consecutive exons of one transcript and for each side (left / right):

  * is there a rescue problem at all (>= 5 clipped bases, no gap at that end, a neighbour exon, a non-empty query);
  * the query (first / last clip + overhang bases of the read-name group's shared sequence, capped at its length) and the
    target (neighbour exons collected until they cover the query, trimmed to qlen + 40), and whether either holds an N;
  * acceptance (max >= 10, the walk not z-dropped), max, refc and the override ops of the clip segment.

For a "plain" read -- real CIGAR [S] M (N M)* [S], every junction of the read on a junction of the transcript -- it also
gives the final row: transcript, pos, strand, output CIGAR, clip_score.

Coordinates are the reference's: exons 1-based half-open [start, end) in genomic order, ref_start the 1-based SAM POS."""
import numpy as np

from tests import ksw2_check

OP_M, OP_I, OP_D, OP_N, OP_S = 0, 1, 2, 3, 4
MATCH_OVR, DEL_OVR, INS_OVR, CLIP_OVR = 10, 11, 12, 13       # include/evaluate.h: BAM_C*_OVERRIDE
MIN_CLIP = 5          # src/evaluate.cpp:946-963: a clip of fewer bases is not tried
MIN_MAX = 10          # :484, :643
WINDOW = 40           # :374, :630
LETTERS = "MIDNSHP=XB,./;"

# src/evaluate.cpp:1182-1201 (the long-read presets; the threshold is a float widened to double)
PRESETS = {"lr": {"max_clip": 40, "max_junc_ins": 40, "max_junc_gap": 40, "threshold": float(np.float32(0.60))},
           "lr_hq": {"max_clip": 5, "max_junc_ins": 10, "max_junc_gap": 10, "threshold": float(np.float32(0.90))}}


def fmt(ops):
    return "".join("%d%s" % (n, LETTERS[op]) for n, op in ops)


def add_op(ops, n, op):
    """Cigar::add_operation (include/evaluate.h:21-128): equal neighbours coalesce"""
    if ops and ops[-1][1] == op:
        ops[-1] = (ops[-1][0] + n, op)
    else:
        ops.append((n, op))


# ---- sequences ---------------------------------------------------------------------------------------------------------
def exon_sequence(ref_seq, start, end):
    """src/g2t.cpp:50-55: the exon's bases [start, end) (1-based) of the reference sequence, upper-cased; positions beyond
    the end of the sequence read as N"""
    return "".join(ref_seq[p - 1].upper() if 1 <= p <= len(ref_seq) else "N" for p in range(start, end))


def shared_sequence(seqs):
    """src/core.cpp:353-378: the records of one read name share the sequence of the first record that carries one"""
    for s in seqs:
        if s:
            return s
    return ""


def dp_letters(s):
    """src/evaluate.cpp:296-305: A C G T in either case code 0..3, every other letter the N code"""
    return "".join(c if c in "ACGT" else "N" for c in s.upper())


def rescue_query(seq, side, clip, overhang):
    """get_left_rescue_query / get_right_rescue_query (src/evaluate.cpp:319-330, 500-511)"""
    total = min(clip + overhang, len(seq))
    return seq[:total] if side == "left" else seq[len(seq) - total:]


def collect_target(exon_seqs, anchor, side, qlen):
    """collect_left_exons / collect_right_exons (src/evaluate.cpp:333-365, 513-546): exon_seqs in genomic order, anchor the
    index of the read's first (left) / last (right) exon.  Neighbours are taken -- leftwards or rightwards on the genome,
    whatever the strand: has_prev / has_next swap with it (:343, :524) -- while the query is longer than what has been
    collected.  -> (sequence, exons taken) or None when there is no neighbour (or nothing to cover)."""
    got, k, step = "", anchor, (-1 if side == "left" else 1)
    n = 0
    while qlen > len(got):
        k += step
        if k < 0 or k >= len(exon_seqs):
            break
        got = exon_seqs[k] + got if side == "left" else got + exon_seqs[k]
        n += 1
    return (got, n) if n else None


def trim_target(gseq, side, qlen):
    """align_reversed :374-375 keeps the last qlen + 40 bases, right_clip_rescue :630 the first"""
    return gseq[max(0, len(gseq) - (qlen + WINDOW)):] if side == "left" else gseq[:qlen + WINDOW]


# ---- the clip segment ----------------------------------------------------------------------------------------------------
def clip_segment(side, cigar, qlen):
    """build_left_clip_segment / build_right_clip_segment (src/evaluate.cpp:397-448, 548-598) on the DP's CIGAR (forward
    order, BAM-packed M / I / D words; for the left side the CIGAR of the reversed strings).  -> (refc, ops): the
    reference bases consumed and the override ops in the read's orientation."""
    words = [(int(w) >> 4, int(w) & 15) for w in cigar]
    consumed_q = sum(n for n, op in words if op in (OP_M, OP_I))
    refc = sum(n for n, op in words if op in (OP_M, OP_D))
    rest = qlen - consumed_q
    ops = []

    def emit(n, op, outermost):
        if outermost and op == OP_D:
            return                                   # :440, :586: a deletion at the far end is dropped
        if outermost and op == OP_I:
            add_op(ops, n, CLIP_OVR)                 # :441, :587: an insertion there is a clip
        else:
            add_op(ops, n, {OP_M: MATCH_OVR, OP_I: INS_OVR, OP_D: DEL_OVR}[op])

    last = len(words) - 1
    if side == "left":
        if rest > 0:
            add_op(ops, rest, CLIP_OVR)              # :431-432
        for k in range(last, -1, -1):                # :435: the reversed strings' CIGAR, walked backwards
            emit(words[k][0], words[k][1], k == last)
    else:
        for k in range(last + 1):
            emit(words[k][0], words[k][1], k == last)
        if rest > 0:
            add_op(ops, rest, CLIP_OVR)              # :594-595
    return refc, ops


def align_side(side, query, target):
    """align / align_reversed with the acceptance rule: -> dict(max, score, accepted, cigar, refc, ops)"""
    q, t = dp_letters(query), dp_letters(target)
    if side == "left":
        q, t = q[::-1], t[::-1]                      # :377-380
    g = ksw2_check.gotoh(t, q)
    out = {"max": g["max"], "score": g["score"], "cigar": g["cigar"], "refc": 0, "ops": [],
           "accepted": g["max"] >= MIN_MAX and g["score"] != ksw2_check.NEG_INF}
    if out["accepted"]:
        out["refc"], out["ops"] = clip_segment(side, g["cigar"], len(q))
    return out


# ---- a read on a transcript ------------------------------------------------------------------------------------------------
def read_ends(real):
    """get_clips (src/evaluate.cpp:69-109) for a CIGAR without hard clips, and the read's blocks: -> (left clip, right clip,
    [aligned lengths of the blocks], [skips between them])"""
    ops = [(int(w) >> 4, int(w) & 15) for w in real]
    lc = ops[0][0] if ops[0][1] == OP_S else 0
    rc = ops[-1][0] if len(ops) > 1 and ops[-1][1] == OP_S else 0
    blocks, skips = [0], []
    for n, op in ops:
        if op == OP_N:
            skips.append(n)
            blocks.append(0)
        elif op == OP_M:
            blocks[-1] += n
        else:
            assert op == OP_S, "rescue_ref.read_ends: a plain read has S, M and N only"
    return lc, rc, blocks, skips


def place(tx, ref_start, real, preset):
    """The read's blocks against the transcript's exons, as findOverlapping (src/g2t.cpp:103-257) sees its first and last
    block: -> None when the read is not a plain read on this transcript, else dict(first, last: exon indices, left_gap,
    left_ins, right_gap, right_ins, blocks [(qstart, qend)]).  Inner junctions must be the transcript's own."""
    cfg = PRESETS[preset]
    lc, rc, lens, skips = read_ends(real)
    blocks, p = [], ref_start
    for k, n in enumerate(lens):
        blocks.append((p, p + n))
        p += n + (skips[k] if k < len(skips) else 0)
    exons = tx["exons"]
    first = next((i for i, (s, e) in enumerate(exons) if s < blocks[0][1] and blocks[0][0] < e), None)
    if first is None or first + len(blocks) > len(exons):
        return None
    last = first + len(blocks) - 1
    for k, (qs, qe) in enumerate(blocks):
        s, e = exons[first + k]
        if (k > 0 and qs != s) or (k < len(blocks) - 1 and qe != e) or not (s < qe and qs < e):
            return None
    (qs, _), (s, _) = blocks[0], exons[first]
    (_, qe), (_, e) = blocks[-1], exons[last]
    left_gap, left_ins = max(qs - s, 0), max(s - qs, 0)
    right_gap, right_ins = max(e - qe, 0), max(qe - e, 0)
    # the overhang of a first / only block is held to max_clip (:171, :218), that of a last / only block to max_clip on
    # '+' (:182) and to max_junc_ins on '-' (:204: `status == FIRST_EXON || MIDDLE_EXON` is always true)
    if left_ins > cfg["max_clip"]:
        return None
    if right_ins > (cfg["max_clip"] if tx["strand"] == "+" else cfg["max_junc_ins"]):
        return None
    # a block that overlaps a second exon of the transcript is no plain read
    for i, (s2, e2) in enumerate(exons):
        if (i < first or i > last) and any(s2 < b[1] and b[0] < e2 for b in blocks):
            return None
    return {"first": first, "last": last, "left_gap": left_gap, "left_ins": left_ins, "right_gap": right_gap,
            "right_ins": right_ins, "blocks": blocks}


def side_answer(tx, ref_seq, pl, side, clip, seq):
    """left_clip_rescue / right_clip_rescue (src/evaluate.cpp:451-498, 600-656) up to the clip segment.  -> dict: exists,
    and when it does query, target, q_has_n, t_has_n, n_exons (collected), collected (bases before the trim), trimmed, max,
    score, accepted, refc, ops; `why` names the rule that kept a problem from existing."""
    gap, ins = (pl["left_gap"], pl["left_ins"]) if side == "left" else (pl["right_gap"], pl["right_ins"])
    none = {"exists": False, "accepted": False, "max": 0, "refc": 0, "ops": []}
    if clip < MIN_CLIP:
        return dict(none, why="clip shorter than 5")                   # :946-963
    if gap > 0:
        return dict(none, why="gap")                                   # :459, :608
    query = rescue_query(seq, side, clip, ins)
    exon_seqs = [exon_sequence(ref_seq, s, e) for s, e in tx["exons"]]
    got = collect_target(exon_seqs, pl["first"] if side == "left" else pl["last"], side, len(query))
    if got is None:
        return dict(none, why="no sequence" if not query else "no neighbour exon")
    target = trim_target(got[0], side, len(query))
    out = {"exists": True, "why": "", "query": query, "target": target, "n_exons": got[1], "collected": len(got[0]),
           "trimmed": len(target) < len(got[0]), "q_has_n": "N" in dp_letters(query), "t_has_n": "N" in dp_letters(target),
           "capped": clip + ins > len(seq), "overhang": ins}
    out.update(align_side(side, query, target))
    return out


def answers(tx, ref_seq, ref_start, real, seq, preset="lr"):
    """-> None (not a plain read on this transcript) or dict(place, left, right)"""
    pl = place(tx, ref_start, real, preset)
    if pl is None:
        return None
    lc, rc, _, _ = read_ends(real)
    return {"place": pl, "left": side_answer(tx, ref_seq, pl, "left", lc, seq),
            "right": side_answer(tx, ref_seq, pl, "right", rc, seq)}


# ---- the final row of a plain read -----------------------------------------------------------------------------------------
def pos_starts(tx):
    """src/bramble.cpp:161-175: the spliced offset of every exon (genomic order) in transcript order"""
    lens = [e - s for s, e in tx["exons"]]
    order = range(len(lens)) if tx["strand"] == "+" else range(len(lens) - 1, -1, -1)
    out, acc = [0] * len(lens), 0
    for i in order:
        out[i] = acc
        acc += lens[i]
    return out


def merge_plain(real, ideal, front_clip):
    """merge_cigars (src/bam.cpp:113-315) for a real CIGAR of S / M / N and an ideal CIGAR of S / M / override ops.
    :159-219 the real front clip first: against an override op both advance (a deletion override consumes no read base),
    against anything else the clip stays and the ideal CIGAR waits; :222-290 then base by base, a skip of the real CIGAR
    dropped (:244), a deletion of the ideal one written whole (:268), the rest by merge_ops (:22-111): an override op gives
    its plain op, an ideal S wins over a real M, a real S over an ideal M; :292-300 an insertion between two clips is a
    clip."""
    plain = {MATCH_OVR: OP_M, DEL_OVR: OP_D, INS_OVR: OP_I, CLIP_OVR: OP_S}
    real = [[n, op] for n, op in real if op != OP_N]
    ideal = [[n, op] for n, op in ideal]
    out = []
    ri = ii = 0
    left = front_clip
    while left > 0 and ri < len(real):
        if ii < len(ideal) and ideal[ii][1] in plain:
            if ideal[ii][1] == DEL_OVR:
                add_op(out, ideal[ii][0], OP_D)
                ii += 1
                continue
            n = min(left, real[ri][0], ideal[ii][0])
            add_op(out, n, plain[ideal[ii][1]])
            ideal[ii][0] -= n
            ii += ideal[ii][0] == 0
        else:
            n = min(left, real[ri][0])
            add_op(out, n, OP_S)
        left -= n
        real[ri][0] -= n
        ri += real[ri][0] == 0
    while ri < len(real) or ii < len(ideal):
        if ri >= len(real):
            add_op(out, ideal[ii][0], ideal[ii][1])      # :223-229: what is left of the ideal CIGAR, as it is
            ii += 1
        elif ii >= len(ideal):
            add_op(out, real[ri][0], real[ri][1])
            ri += 1
        elif ideal[ii][1] == DEL_OVR:
            add_op(out, ideal[ii][0], OP_D)
            ii += 1
        else:
            n = min(real[ri][0], ideal[ii][0])
            r_op, i_op = real[ri][1], ideal[ii][1]
            add_op(out, n, plain[i_op] if i_op in plain else OP_S if OP_S in (r_op, i_op) else OP_M)
            real[ri][0] -= n
            ideal[ii][0] -= n
            ri += real[ri][0] == 0
            ii += ideal[ii][0] == 0
    for k in range(1, len(out) - 1):
        if out[k][1] == OP_I and out[k - 1][1] == OP_S and out[k + 1][1] == OP_S:
            out[k] = (out[k][0], OP_S)
    done = []
    for n, op in out:
        add_op(done, n, op)
    return done


def plain_row(tx, ref_start, real, ans, preset="lr"):
    """The row evaluate_exon_chains (src/evaluate.cpp:888-1134) and write_to_bam leave for a plain read whose per-side
    answers are `ans`: dict(pos, strand, cigar, clip_score, ideal), or None when the similarity filter (:843-886) drops it."""
    pl, L, R = ans["place"], ans["left"], ans["right"]
    ps = pos_starts(tx)
    exons = tx["exons"]
    # an accepted rescue clears the overhang of its end (:489-490, :648)
    left_ins = 0 if L["accepted"] else pl["left_ins"]
    right_ins = 0 if R["accepted"] else pl["right_ins"]
    matched = sum(min(qe, exons[pl["first"] + k][1]) - max(qs, exons[pl["first"] + k][0]) for k, (qs, qe) in enumerate(pl["blocks"]))
    ideal = [tuple(o) for o in L["ops"]]
    if left_ins:
        add_op(ideal, left_ins, OP_S)            # :699-706 (first / only exon, no left clip segment)
    add_op(ideal, matched, OP_M)                 # :740-747; exact junctions add nothing between the exons
    if right_ins:
        add_op(ideal, right_ins, OP_S)           # :752-759
    for n, op in R["ops"]:
        add_op(ideal, n, op)                     # build_cigar_clip :824-841
    # filter_by_similarity: matched bases over matched bases + unrescued overhangs
    total = matched + left_ins + right_ins
    if not matched / total > PRESETS[preset]["threshold"]:
        return None
    if tx["strand"] == "+":
        # create_match :658-673 takes the first segment with a guide exon: the left clip segment's dummy exon
        # (pos_start - ref_consumed, :427), else the first exon's pos (g2t.cpp:159,165)
        pos = ps[pl["first"]] - L["refc"] if L["accepted"] else ps[pl["first"]] + pl["left_gap"]
    else:
        # rcpos follows the last segment with a guide exon (:1058-1063): the right clip segment's dummy exon (:578), else
        # the last exon's pos (g2t.cpp:194,201)
        pos = ps[pl["last"]] - R["refc"] if R["accepted"] else ps[pl["last"]] + pl["right_gap"]
    lc, _, _, _ = read_ends(real)
    merged = merge_plain([(int(w) >> 4, int(w) & 15) for w in real], ideal, lc)
    return {"pos": pos, "strand": tx["strand"], "cigar": fmt(merged), "clip_score": L["max"] * L["accepted"] + R["max"] * R["accepted"],
            "ideal": fmt(ideal)}


def query_length(ops_text):
    """read bases a CIGAR text consumes (M I S = X)"""
    n, num = 0, ""
    for ch in ops_text:
        if ch.isdigit():
            num += ch
        else:
            n += int(num) if ch in "MIS=X" else 0
            num = ""
    return n
