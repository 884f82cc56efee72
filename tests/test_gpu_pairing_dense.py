"""Mate pairing of alignments with more than 64 candidate rows (big_list: k_big<0> + k_pair_big on the direct-rows path)
against the oracle's process_mate_pair, on one hand-made annotation:

  * 150 isoforms on each strand share a first exon and a middle exon: a read there has more than 64 candidate rows;
  * each isoform's last exon lies in one of 8 loci, 3 kb apart and far from the dense exons: a read there has fewer than
    64 candidate rows and a survivor mask;
  * six isoforms have a first exon end of their own and a last exon of their own (a spliced read through that first exon
    end, inside the dense bins, or a read inside that last exon has exactly one survivor), and each locus has a
    single-exon transcript that no other read reaches.

Paired records cover every role of the pairing: big x big, big leader with a masked mate and the reverse, one survivor
on each side without a common transcript (one or both sides big), no common transcript with more than one survivor on
a side (both dropped), a mate without survivors (the leader emits alone; a leader without survivors drops both),
multi-mapper read names of 32 and of 140 records whose mates lie far apart, and runs of masked pairs whose survivor
lists overflow k_pair_mask's staging area (k_pair_mask_wide).  Rows are compared column by column on the three routes
(direct rows, the match table, the small-batch path), the direct-rows call's pairing flags prove that every role was
reached, and the side arena's grow-and-repeat round is checked under a small first capacity and at a size that needs
several times the default one."""
import numpy as np
import pytest

from bramble_amd import lib
from bramble_amd.batch import make_batch, parse_cigar
from oracle import oracle_binding as ob
from tests.parity import assert_rows_equal
from tests.test_gpu_bam_bundle import _record, assert_streams_equal

pytestmark = pytest.mark.gpu

N_ISO = 150
N_LOCI = 8
N_UNIQ = 6
FIRST_END, MID = 1300, (1500, 1540)


def _locus(L):
    return 6000 + 3000 * L


def _uniq_end(j):
    return 1150 + 20 * j


def annotation(seed=5):
    rng = np.random.RandomState(seed)
    txs = []
    for k in range(N_ISO):
        L = k % N_LOCI
        for strand in "+-":
            a = 1000 + int(rng.randint(0, 60))
            d = int(rng.randint(0, 60))
            txs.append({"id": "t%d%s" % (k, strand), "ref_id": 0, "strand": strand,
                        "exons": [[a, FIRST_END], list(MID), [_locus(L) + d, _locus(L) + 500]]})
    for j in range(N_UNIQ):   # a first exon end and a last exon of their own
        txs.append({"id": "u%d" % j, "ref_id": 0, "strand": "+",
                    "exons": [[1000, _uniq_end(j)], list(MID), [_locus(j) + 600, _locus(j) + 700]]})
    for L in range(N_LOCI):   # single-exon transcripts nothing else overlaps
        txs.append({"id": "x%d" % L, "ref_id": 0, "strand": "+", "exons": [[_locus(L) + 1200, _locus(L) + 1300]]})
    return {"refnames": ["chrP"], "transcripts": txs}


# read kinds: (start, cigar)
def DA(s):      # inside the shared first exon: > 64 candidate rows, every isoform survives
    return (1061 + s % 100, "100M")


def DB(x):      # first exon -> middle exon: > 64 candidate rows, every isoform survives
    x = 30 + x % 31
    return (FIRST_END - x, "%dM%dN40M" % (x, MID[0] - FIRST_END))


def DU(j):      # through the first exon end of u<j>: > 64 candidate rows, one survivor
    e = _uniq_end(j % N_UNIQ)
    return (e - 30, "30M%dN40M" % (MID[0] - e))


def LA(L, s):   # inside the last exons of locus L: a mask, ~38 survivors
    return (_locus(L % N_LOCI) + 60 + s % 300, "100M")


def LU(j, s=0):  # inside the last exon of u<j>: a mask, one survivor
    return (_locus(j % N_UNIQ) + 605 + s % 15, "80M")


def LX(L, s=0):  # inside x<L>: a mask, one survivor, shared with nothing
    return (_locus(L % N_LOCI) + 1205 + s % 15, "80M")


def Z(s):       # no transcript: no survivors
    return (40000 + s, "100M")


def _qlen(cigar):
    return int(sum(int(w) >> 4 for w in parse_cigar(cigar) if (int(w) & 0xF) in (0, 1, 4, 7, 8)))


def _pair(name, r1, r2, swap):
    """read1 / read2 records of one pair (FR orientation); swap lists read2 first (it becomes the leader)."""
    (s1, c1), (s2, c2) = r1, r2
    a = {"name": name, "ref_id": 0, "ref_start": s1, "cigar": c1, "flags": 0x1 | 0x40 | 0x20, "mate_ref_id": 0,
         "mate_start": s2, "read_len": _qlen(c1)}
    b = {"name": name, "ref_id": 0, "ref_start": s2, "cigar": c2, "flags": 0x1 | 0x80 | 0x10, "mate_ref_id": 0,
         "mate_start": s1, "read_len": _qlen(c2)}
    return [b, a] if swap else [a, b]


def _kinds(rng):
    """one pair of every role (read1, read2), positions drawn from rng"""
    s = lambda: int(rng.randint(0, 1000))
    j, k = int(rng.randint(0, N_UNIQ)), int(rng.randint(0, N_UNIQ))
    k = k if k != j else (j + 1) % N_UNIQ
    L = int(rng.randint(0, N_LOCI))
    return [
        (DA(s()), DB(s())),          # big x big, common transcripts
        (DA(s()), DA(s() + 1)),      # big x big
        (DA(s()), LA(L, s())),       # big x masked, common transcripts
        (LA(L, s()), DB(s())),       # masked x big
        (DU(j), LU(k, s())),         # one each, no common transcript: big x masked
        (DU(j), DU(k)),              # one each, both big
        (DU(j), LX(L, s())),         # one each, big x masked
        (DU(j), LU(j, s())),         # one survivor each, the same transcript
        (DA(s()), LX(L, s())),       # no common transcript, 300 survivors on one side: both dropped
        (DU(j), LA(L, s())),         # no common transcript, one vs many: both dropped
        (DA(s()), Z(s())),           # a mate without survivors
        (LA(L, s()), Z(s())),
        (LA(L, s()), LA(L, s() + 7)),  # masked x masked
    ]


def _group(name, n_pairs, rng):
    """one read name of n_pairs multi-mapping pairs of mixed roles, every read1 listed first: mates n_pairs records
    apart.  All starts of the name are distinct (the mate key is the start): a draw that repeats one is skipped."""
    r1s, r2s, used = [], [], set()
    while len(r1s) < n_pairs:
        ks = _kinds(rng)
        a, b = ks[int(rng.randint(0, len(ks)))]
        if a[0] in used or b[0] in used or a[0] == b[0]:
            continue
        used.update((a[0], b[0]))
        ra, rb = _pair(name, a, b, False)
        r1s.append(ra)
        r2s.append(rb)
    return r1s + r2s


def paired_dense_records(seed=3):
    rng = np.random.RandomState(seed)
    recs = []
    n = 0
    # every role, in both listing orders, a few times
    for rep in range(6):
        for q, (a, b) in enumerate(_kinds(rng)):
            recs += _pair("p%d" % n, a, b, (rep + q) % 2 == 1)
            n += 1
    # a few unpaired big reads (SOLO)
    for i in range(4):
        st, cg = DA(int(rng.randint(0, 100)))
        recs.append({"name": "u%d" % i, "ref_id": 0, "ref_start": st, "cigar": cg, "read_len": 100})
    # multi-mapper read names whose mates lie far apart: 16 and 12 pairs (the open list of <= 32 records), 70 pairs (the map)
    for name, n_pairs in (("mm_small", 16), ("mm_small2", 12), ("mm_big", 70)):
        recs += _group(name, n_pairs, rng)
    # a run of masked pairs with ~38 survivors on each side: the windows' lists outgrow k_pair_mask's staging area
    for i in range(160):
        L = int(rng.randint(0, N_LOCI))
        recs += _pair("w%d" % i, LA(L, int(rng.randint(0, 300))), LA(L, int(rng.randint(0, 300))), i % 3 == 0)
    # more of the roles, after the run
    for rep in range(4):
        for q, (a, b) in enumerate(_kinds(rng)):
            recs += _pair("q%d_%d" % (rep, q), a, b, (rep * 5 + q) % 3 == 0)
    return recs


@pytest.fixture(scope="module")
def dense_pairs():
    ann = annotation()
    recs = paired_dense_records()
    return ann, recs, make_batch(recs)


PRESETS = [{}, {"strict": 1}, {"fr": 1}]
_ORC = {}


def _oracle(ann, batch, flags):
    key = (id(batch), tuple(sorted(flags.items())))
    if key not in _ORC:
        _ORC[key] = ob.run(ob.OracleIndex(ann), ob.make_flags(**flags), batch, want_matches=True)[:2]
    return _ORC[key]


# (route, context parameters)
ROUTES = [("direct", {"small_batch": 0}), ("match_table", {"small_batch": 0, "direct_rows": 0}), ("small", {})]


@pytest.mark.parametrize("flags", PRESETS, ids=["default", "strict", "fr"])
@pytest.mark.parametrize("lanes", [8, 64])
@pytest.mark.parametrize("route,params", ROUTES, ids=[r[0] for r in ROUTES])
def test_paired_dense_rows_equal_oracle(dense_pairs, flags, lanes, route, params):
    ann, _, batch = dense_pairs
    orc, _ = _oracle(ann, batch, flags)
    assert orc["n_rows"] > 10000
    idx = lib.Index(ann, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("group_lanes", lanes)
    for k, v in params.items():
        ctx.set_param(k, v)
    for _ in range(2):
        assert_rows_equal(ctx.project_batch(lib.make_config(**flags), batch), orc)
    ctx.close()
    idx.close()


def reach(batch, matches, pflags):
    """How often each pairing role occurred in a direct-rows call: its pairing flags (PF_*) with the oracle's survivors
    (a read with more than 64 survivors has more than 64 candidate rows)."""
    n = batch["n_aln"]
    nsurv = np.diff(matches["aln_off"].astype(np.int64))
    mate = matches["mate_idx"]
    group = np.cumsum(np.r_[0, [batch["names"][int(batch["name_off"][i]):int(batch["name_off"][i + 1])].tobytes() !=
                                batch["names"][int(batch["name_off"][i - 1]):int(batch["name_off"][i])].tobytes()
                                for i in range(1, n)]])
    gsize = np.bincount(group)[group]
    big = (pflags & lib.PF_BIG) != 0
    paired = (pflags & lib.PF_PAIRED) != 0
    same = (pflags & lib.PF_SAME) != 0
    c = dict.fromkeys(["big_big", "big_leader_masked_mate", "masked_leader_big_mate", "big_is_mate", "one_each_big",
                       "one_each_both_big", "big_dropped", "big_solo_mate_empty", "empty_leader_big_mate",
                       "far_big_small_group", "far_big_large_group"], 0)
    for i in range(n):
        m = int(mate[i])
        if m < 0 or m < i:
            continue   # each pair once, from its leader i < m
        if big[i] and big[m] and paired[i] and paired[m]:
            c["big_big"] += 1
        if big[i] and not big[m] and paired[i] and paired[m]:
            c["big_leader_masked_mate"] += 1
        if not big[i] and big[m] and paired[i] and paired[m]:
            c["masked_leader_big_mate"] += 1
        if big[m] and paired[m] and (pflags[m] & lib.PF_MATE):
            c["big_is_mate"] += 1
        if (big[i] or big[m]) and paired[i] and not same[i] and nsurv[i] == 1 and nsurv[m] == 1:
            c["one_each_big"] += 1
            c["one_each_both_big"] += int(big[i] and big[m])
        if (big[i] or big[m]) and nsurv[i] and nsurv[m] and not paired[i] and not paired[m]:
            c["big_dropped"] += 1
        if big[i] and nsurv[i] and nsurv[m] == 0 and not paired[i]:
            c["big_solo_mate_empty"] += 1
        if nsurv[i] == 0 and nsurv[m] > 64:
            c["empty_leader_big_mate"] += 1
        if (big[i] or big[m]) and paired[i]:
            if gsize[i] > 32 and m - i > 62:
                c["far_big_large_group"] += 1   # (the mate index of the >32-record name from the map)
            elif 4 < gsize[i] <= 32 and m - i >= 8:
                c["far_big_small_group"] += 1   # (from the open list)
    return c


def test_paired_dense_reaches_every_pairing_role(dense_pairs):
    """The direct-rows call must reach every role of k_pair_big (and k_pair_mask_wide): a roster that stops reaching
    one fails here, not silently."""
    ann, _, batch = dense_pairs
    orc, matches = _oracle(ann, batch, {})
    idx = lib.Index(ann, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("small_batch", 0)
    rows = ctx.project_batch(lib.make_config(), batch)
    d = ctx.direct_diag(batch["n_aln"])
    assert_rows_equal(rows, orc)
    c = reach(batch, matches, d["pflags"])
    print("reach:", c, "n_big", d["n_big"], "pm_n", d["pm_n"], "side", d["side_used"], "/", d["side_cap"])
    for k, v in c.items():
        assert v >= 3, (k, c)
    assert d["n_big"] >= 100 and d["pm_n"] > 0 and d["side_attempts"] == 1
    # an alignment that leads nothing and drops nothing emits exactly its kept matches: every big alignment of the oracle's
    # rows is flagged, and no alignment the oracle drops has its paired flag
    out_idx = np.unique(orc["input_index"])
    emitted = np.zeros(batch["n_aln"], dtype=bool)
    emitted[out_idx] = True
    nsurv = np.diff(matches["aln_off"].astype(np.int64))
    assert ((d["pflags"] & lib.PF_BIG) != 0)[emitted & (nsurv > 64)].all()
    assert not ((d["pflags"] & lib.PF_PAIRED) != 0)[~emitted].any()
    # the diagnostic describes direct-rows calls only
    ctx.set_param("direct_rows", 0)
    ctx.project_batch(lib.make_config(), batch)
    with pytest.raises(lib.BrambleError):
        ctx.direct_diag()
    ctx.close()
    idx.close()


def test_side_arena_grows_once_under_a_small_first_capacity(dense_pairs):
    """side_cap (test hook): a first arena of 4096 entries is far too small; the call repeats once with the arena grown to
    the exact total its big alignments asked for, and the next call on the same context fits at once."""
    ann, _, batch = dense_pairs
    orc, _ = _oracle(ann, batch, {})
    idx = lib.Index(ann, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("small_batch", 0)
    ctx.set_param("side_cap", 4096)
    assert_rows_equal(ctx.project_batch(lib.make_config(), batch), orc)
    d = ctx.direct_diag()
    assert d["side_attempts"] == 2, d
    assert d["side_used"] > 4 * 4096 and d["side_used"] <= d["side_cap"], d
    assert_rows_equal(ctx.project_batch(lib.make_config(), batch), orc)
    d2 = ctx.direct_diag()
    assert d2["side_attempts"] == 1 and d2["side_used"] == d["side_used"] and d2["side_cap"] == d["side_cap"], (d, d2)
    with pytest.raises(lib.BrambleError):
        ctx.set_param("side_cap", 63)
    ctx.close()
    idx.close()


def many_big_records(n_pairs=16000, seed=9):
    """n_pairs big alignments of ~300 survivors (464 arena entries each) whose mates share no transcript with them (both
    dropped: the oracle stays quick), and a few hundred pairs that emit."""
    rng = np.random.RandomState(seed)
    recs = []
    for i in range(n_pairs):
        recs += _pair("d%d" % i, DA(int(rng.randint(0, 100))), LX(int(rng.randint(0, N_LOCI)), int(rng.randint(0, 15))), i % 2 == 1)
    for i in range(300):
        a, b = _kinds(rng)[i % 13]
        recs += _pair("e%d" % i, a, b, i % 2 == 0)
    return recs


def test_side_arena_overflow_several_times_the_first_arena():
    """A fresh context, no hook: the big alignments need several times the first arena (max(n / 4, 2^20) entries).  The
    call succeeds on its second attempt and equals the oracle (before the overflow kept counting every entry's need, the
    arena grew to 1.25x a partial sum per attempt and the call gave up with BR_ERR_CAPACITY after four)."""
    ann = annotation()
    batch = make_batch(many_big_records())
    orc, _, _ = ob.run(ob.OracleIndex(ann), ob.make_flags(), batch, want_matches=False)
    idx = lib.Index(ann, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("small_batch", 0)
    rows = ctx.project_batch(lib.make_config(), batch)
    d = ctx.direct_diag()
    print("arena:", d)
    assert_rows_equal(rows, orc)
    first = max(batch["n_aln"] // 4, 1 << 20)
    assert d["side_attempts"] == 2 and d["side_used"] >= 4 * first and d["side_used"] <= d["side_cap"], (d, first)
    ctx.close()
    idx.close()


def _bam_stream(recs):
    out = bytearray()
    for r in recs:
        paired = r.get("flags", 0) & 0x1
        out += _record(r["name"], r["ref_id"], r["ref_start"] - 1, r.get("flags", 0), r["cigar"], 0 if paired else -1,
                       r["mate_start"] - 1 if paired else -1, r["read_len"])
    return np.frombuffer(bytes(out), dtype=np.uint8)


@pytest.mark.parametrize("flags", PRESETS, ids=["default", "strict", "fr"])
@pytest.mark.parametrize("small_batch", [1, 0])
def test_paired_dense_bam_records_equal_oracle(dense_pairs, flags, small_batch):
    """Records in, records out: mate fields, flags and TLEN follow the pairing flags."""
    ann, recs, _ = dense_pairs
    stream = _bam_stream(recs)
    roff, rlen, _, used = lib.bam_split(stream)
    assert used == stream.size and len(roff) == len(recs)
    ref_map = np.zeros(1, dtype=np.int32)
    idx = lib.Index(ann, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("small_batch", small_batch)
    got, counters = ctx.project_bam_bundle(lib.make_config(**flags), stream, roff, rlen, ref_map)
    ctx.close()
    idx.close()
    orc, _, _, _ = ob.run_bam(ob.OracleIndex(ann), ob.make_flags(**flags), stream, roff, rlen, ref_map)
    assert orc["n_rows"] > 10000 and counters["n_rows"] == orc["n_rows"]
    for k in ("total_complete", "total_unique", "dropped_reads", "total_processed"):
        assert counters[k] == orc[k], k
    assert_streams_equal(got, orc["bam_stream"])
