"""The general emit class of direct rows with "emit_general_preset" 1 (k_emit_rows<2, 1>: the short-read preset as constants,
the ideal and the rewritten CIGAR staged in the lane's LDS slot through typed pointers) and 0 (k_emit_rows<2, 0>, the kernel of
every other preset): rows with the detail column, and BAM records, against the oracle on a hand-made annotation.  Both
settings must equal the oracle, and therefore each other.  Nothing is left out of a comparison.

The fit rule under test (bramble_amd/csrc/project_kernels.hip, next to LDS_SLOT = 25):
    ideal CIGAR in LDS      iff  4 * n_seg + 2 <= 25                (read exons n_seg <= 5; 6 and 7 take the generic code)
    rewritten CIGAR in LDS  iff  n_real + 2 * n_ideal <= 25         (n_real: words of the alignment's CIGAR, n_ideal: ops of
                                                                     the ideal one)
The reads are built from that rule.  A read that lies inside its exons and meets every junction exactly has the ideal CIGAR
"xM" (n_ideal 1); each outer overhang of 1-5 bases adds an S (n_ideal 2, 3); n_real is set freely by spelling an M run as
alternating = / X pieces, by I and D inside an exon, and by S / H clips.  So the output limit is met exactly (25) and missed by
one word on either side (24, 26) with n_ideal 1, 2 and 3, on reads of one to five exons.

Shapes: read-exon counts 1..7 on both strands; rewritten CIGARs of 1, 2 (inline), 3 (the first arena copy) and 5 and more
ops; alignment CIGARs of 4, 5, 6 and more words (past the four that RealCig holds in registers); an I between clips (the
fix-up and re-coalescing tail of the merge); reads whose ideal or real side runs out first; fitting and non-fitting lanes
interleaved in one wave; general-class work lists of 63, 64, 65, 255, 256 and 257 entries; pairs with one mate per class,
multi-mapper names and an alignment with more than 64 candidate rows beside them; the presets --fr, --rf, looser tolerances,
and --max-error-exon and long reads without the filter, which keep the old kernel whatever the switch says."""
import numpy as np
import pytest

from bramble_amd import lib
from bramble_amd.batch import make_batch, parse_cigar
from oracle import oracle_binding as ob
from tests.parity import assert_rows_equal
from tests.test_gpu_bam_bundle import _record, assert_streams_equal

pytestmark = pytest.mark.gpu

LDS_SLOT = 25
ELEN, PERIOD, NEX = 60, 200, 9


def _exons(start, n=NEX):
    return [[start + PERIOD * k, start + PERIOD * k + ELEN] for k in range(n)]


P9, M9, U3 = _exons(1000), _exons(5000), _exons(20000, 3)
DENSE0, N_DENSE = 9000, 70


def annotation():
    txs = [{"id": "p9", "ref_id": 0, "strand": "+", "exons": P9},
           {"id": "p5", "ref_id": 0, "strand": "+", "exons": P9[:5]},      # several survivors over the first exons
           {"id": "p3", "ref_id": 0, "strand": "+", "exons": P9[1:4]},
           {"id": "m9", "ref_id": 0, "strand": "-", "exons": M9},
           {"id": "m4", "ref_id": 0, "strand": "-", "exons": M9[2:6]},
           {"id": "u3", "ref_id": 0, "strand": "+", "exons": U3}]          # one transcript alone: one record per read
    for k in range(N_DENSE):                                               # more than 64 candidate rows for one read exon
        txs.append({"id": "d%02d" % k, "ref_id": 0, "strand": "+",
                    "exons": [[DENSE0, DENSE0 + 100], [DENSE0 + 300, DENSE0 + 400 + k]]})
    return {"refnames": ["chrE"], "transcripts": [dict(t, exons=[list(e) for e in t["exons"]]) for t in txs]}


def _words(cigar):
    return len(parse_cigar(cigar))


def _qlen(cigar):
    return int(sum(int(w) >> 4 for w in parse_cigar(cigar) if (int(w) & 0xF) in (0, 1, 4, 7, 8)))


def _run(length, pieces=1, indel=None):
    """one exon's stretch of `length` reference bases: M, or `pieces` alternating = / X runs, or with an I / D inside"""
    if indel == "I":
        a = length // 2
        return "%dM2I%dM" % (a, length - a)
    if indel == "D":
        a = length // 2
        return "%dM1D%dM" % (a, length - a - 1)
    if pieces <= 1:
        return "%dM" % length
    assert length >= pieces
    out, left = [], length
    for p in range(pieces):
        n = 1 if p < pieces - 1 else left
        out.append("%d%s" % (n, "=X"[p % 2]))
        left -= n
    return "".join(out)


def chain(ex, i, n, x=20, y=20, lo=0, ro=0, pieces=None, indel=None, pre="", suf=""):
    """(start, cigar) of a read over exons ex[i .. i + n - 1]: the last x bases of the first (its whole length plus an overhang
    of lo when lo > 0), the inner ones whole, the first y bases of the last (whole plus ro).  pieces / indel: {read exon: ...}
    for _run.  pre / suf: clips around it."""
    pieces, indel = pieces or {}, indel or {}
    lens = []
    for k in range(n):
        e = ex[i + k]
        full = e[1] - e[0]
        if n == 1:
            ln = (full + lo + ro) if (lo or ro) else x
        elif k == 0:
            ln = full + lo if lo else x
        elif k == n - 1:
            ln = full + ro if ro else y
        else:
            ln = full
        lens.append(ln)
    if n == 1:
        start = ex[i][0] - lo if (lo or ro) else ex[i][0] + 10
    else:
        start = ex[i][1] - lens[0]
    parts = []
    for k in range(n):
        parts.append(_run(lens[k], pieces.get(k, 1), indel.get(k)))
        if k < n - 1:
            parts.append("%dN" % (ex[i + k + 1][0] - ex[i + k][1]))
    return (start, pre + "".join(parts) + suf)


def _pad_to(ex, i, n, n_real, **kw):
    """a chain whose CIGAR has exactly n_real words: exon 0's run is spelled in as many = / X pieces as that takes"""
    kw.setdefault("x", 40)
    base = _words(chain(ex, i, n, **kw)[1])
    assert n_real >= base
    k = chain(ex, i, n, pieces={0: 1 + n_real - base}, **kw)
    assert _words(k[1]) == n_real, (k, n_real)
    return k


def read_kinds():
    out = []
    for ex in (P9, M9):
        for n in range(1, 8):                                        # read exons 1..7 (5 | 6: either side of the ideal's limit)
            for i in (0, 1, 2):
                if i + n > NEX:
                    continue
                out.append(chain(ex, i, n))                          # inside: rewritten CIGAR "xM" (one op, inline)
                out.append(chain(ex, i, n, lo=3))                    # "3S xM": two ops, inline
                out.append(chain(ex, i, n, lo=2, ro=4))              # "2S xM 4S": three ops, the first arena copy
            out.append(chain(ex, 0, n, pre="3S"))                    # the alignment's own clips
            out.append(chain(ex, 1, n, suf="4S"))                    # (the ideal side runs out first)
            out.append(chain(ex, 1, n, pre="2H3S", suf="1S2H"))      # five and more ops
            out.append(chain(ex, 0, n, indel={0: "I"}))
            out.append(chain(ex, 0, n, indel={n - 1: "D"}))
            out.append(chain(ex, 1, n, indel={0: "D", n - 1: "I"}, pre="2S", lo=0))
            out.append(chain(ex, 0, n, pieces={0: 2}))               # n_real + 1, + 2, + 3: past RealCig's four registers
            out.append(chain(ex, 0, n, pieces={0: 3}))
            out.append(chain(ex, 0, n, pieces={n - 1: 4}))
        # the output limit n_real + 2 * n_ideal = 24 | 25 | 26 with n_ideal 1, 2 and 3, on one to five read exons
        for n in (1, 2, 3, 4, 5):
            for lim in (LDS_SLOT - 1, LDS_SLOT, LDS_SLOT + 1):
                out.append(_pad_to(ex, 1, n, lim - 2))                       # n_ideal 1
                out.append(_pad_to(ex, 1, n, lim - 4, lo=2))                 # n_ideal 2
                out.append(_pad_to(ex, 1, n, lim - 6, lo=1, ro=5))           # n_ideal 3
        # an I between clips: the overhang's S covers the bases around the alignment's I (fix-up, then re-coalescing)
        e = ex[2]
        out.append((e[0] - 5, "3M2I%dM" % (2 + 30)))
        out.append((e[0] - 5, "2H3M2I%dM" % (2 + 30)))
        out.append((e[0] - 4, "2S1M1I%dM%dN20M" % (3 + ELEN, PERIOD - ELEN)))
        out.append((e[1] - 30, "%dM2I3M" % (30 + 2)))                # ... on the right (the real side runs out last)
        out.append((e[1] - 30, "%dM1I1M2S" % (30 + 4)))
    # junctions off by 1-3 bases: survive under the looser tolerances only (D / I ops in the ideal CIGAR)
    for ex in (P9, M9):
        for n in (2, 3, 5, 6):
            for d in (-3, -1, 2):
                s, c = chain(ex, 1, n)
                w = c.split("N", 1)
                gap = int(w[0].rsplit("M", 1)[1])
                out.append((s, "%dM%dN%s" % (20 + d, gap - d, w[1])))    # the first read exon ends d bases off its exon's end
    out.append((U3[0][0] + 5, "30M"))                                 # the simple class beside them
    out.append((P9[0][0] + 10, "40M"))
    out.append((DENSE0 + 10, "60M"))                                  # more than 64 candidate rows: k_big
    out.append((DENSE0 + 50, "50M200N40M"))
    out.append((DENSE0 + 50, "2S10=1X39M200N40M3S"))
    return out


def _rec(name, k, flags, mate=None):
    s, c = k
    r = {"name": name, "ref_id": 0, "ref_start": s, "cigar": c, "flags": flags, "read_len": _qlen(c)}
    if mate is not None:
        r["mate_ref_id"], r["mate_start"] = 0, mate[0]
    return r


def records(seed=5):
    rng = np.random.RandomState(seed)
    kinds = read_kinds()
    recs, n = [], 0
    for rep in range(2):
        order = list(range(len(kinds))) if rep == 0 else list(rng.permutation(len(kinds)))   # fitting and non-fitting lanes, both orders
        for i in order:
            recs.append(_rec("s%d" % n, kinds[i], 0x10 if rep == 1 else 0))
            n += 1
    for i in range(len(kinds)):                                       # pairs of every two kinds: one mate per class among them
        a, b = kinds[i], kinds[(i * 11 + 5) % len(kinds)]
        if a[0] == b[0]:
            continue
        ra, rb = _rec("p%d" % n, a, 0x1 | 0x40 | 0x20, b), _rec("p%d" % n, b, 0x1 | 0x80 | 0x10, a)
        recs += [rb, ra] if i % 2 else [ra, rb]
        n += 1
    for g in range(5):                                                # multi-mapper read names
        used, r1, r2 = set(), [], []
        while len(r1) < 3 + g:
            a, b = kinds[int(rng.randint(len(kinds)))], kinds[int(rng.randint(len(kinds)))]
            if a[0] in used or b[0] in used or a[0] == b[0]:
                continue
            used.update((a[0], b[0]))
            r1.append(_rec("m%d" % g, a, 0x1 | 0x40 | 0x20, b))
            r2.append(_rec("m%d" % g, b, 0x1 | 0x80 | 0x10, a))
        recs += r1 + r2
    return recs


PRESETS = [{}, {"fr": 1}, {"rf": 1}, {"max_junc_gap": 12, "max_junc_ins": 12, "max_clip": 12},
           {"max_error_exon": 8}, {"lr": 1, "sim_thr": 1.0}]
PRESET_IDS = ["default", "fr", "rf", "loose", "max_error_exon", "long_reads_no_filter"]
SWITCH = [1, 0]


@pytest.fixture(scope="module")
def hand():
    ann = annotation()
    recs = records()
    return ann, recs, make_batch(recs), {}


def _oracle(hand, flags):
    ann, _, batch, memo = hand
    key = tuple(sorted(flags.items()))
    if key not in memo:
        memo[key] = ob.run(ob.OracleIndex(ann), ob.make_flags(**flags), batch, want_matches=False)[0]
    return memo[key]


def _direct_ctx(ann, preset, lanes=8):
    idx = lib.Index(ann, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("small_batch", 0)
    ctx.set_param("direct_rows", 1)
    ctx.set_param("group_lanes", lanes)
    ctx.set_param("emit_general_preset", preset)
    return idx, ctx


def test_shapes_are_the_ones_described(hand):
    """the generator holds what the docstring promises (no device work beyond the fixture): counted on the oracle's rows"""
    ann, recs, batch, _ = hand
    orc = _oracle(hand, {})
    n_out = np.diff(orc["cigar_off"].astype(np.int64))
    for k in (1, 2, 3):
        assert int((n_out == k).sum()) > 20, k
    assert int((n_out >= 5).sum()) > 20
    nseg = np.array([r["cigar"].count("N") + 1 for r in recs])
    nreal = np.array([_words(r["cigar"]) for r in recs])
    src = np.asarray(orc["input_index"])
    for k in range(1, 8):                                              # every read-exon count projects, on both strands
        for flag in (0, 0x10):
            sel = [i for i in set(src.tolist()) if nseg[i] == k and (recs[i]["flags"] & 0x1) == 0 and (recs[i]["flags"] & 0x10) == flag]
            assert len(sel) > 5, (k, flag)
    for w in (4, 5, 6, LDS_SLOT - 7, LDS_SLOT - 3, LDS_SLOT - 1):     # n_real at and around what the limits need
        assert int((nreal[src] == w).sum()) > 0, w
    # the output limit: projected reads with n_real + 2 * n_ideal = 24, 25, 26 for n_ideal = 1 (rewritten CIGAR without S)
    for lim in (LDS_SLOT - 1, LDS_SLOT, LDS_SLOT + 1):
        assert int(((nreal[src] == lim - 2) & (nseg[src] <= 5)).sum()) > 0, lim


@pytest.mark.parametrize("preset", SWITCH)
@pytest.mark.parametrize("flags", PRESETS, ids=PRESET_IDS)
def test_rows_equal_oracle(hand, flags, preset):
    ann, _, batch, _ = hand
    orc = _oracle(hand, flags)
    assert orc["n_rows"] > 300
    for lanes in (8, 64):
        idx, ctx = _direct_ctx(ann, preset, lanes)
        cfg = lib.make_config(**flags)
        for _ in range(2):
            assert_rows_equal(ctx.project_batch(cfg, batch), orc)
        d = ctx.direct_diag()
        assert d["n_big"] > 0, d
        ctx.close()
        idx.close()


@pytest.mark.parametrize("preset", SWITCH)
@pytest.mark.parametrize("n_general", [63, 64, 65, 255, 256, 257])
def test_work_list_edges(n_general, preset):
    """a general class of exactly n_general entries (three-exon reads of the lone transcript, one record each) behind a
    simple prefix: the last block's tail, and the LDS slot of the block's last thread"""
    ann = annotation()
    recs = [_rec("e%d" % i, (U3[0][0] + 5 + i % 7, "30M"), 0) for i in range(5)]
    kinds = [chain(U3, 0, 3, x=10 + i % 40, y=10 + (i * 3) % 40, pieces={1: 1 + i % 6}) for i in range(n_general - 2)]
    kinds += [chain(U3, 0, 3, lo=2, ro=3), _pad_to(U3, 0, 3, LDS_SLOT - 1)]   # the last two lanes: an arena copy, a lane that does not fit
    recs += [_rec("g%d" % i, k, 0) for i, k in enumerate(kinds)]
    batch = make_batch(recs)
    orc, _, _ = ob.run(ob.OracleIndex(ann), ob.make_flags(), batch, want_matches=False)
    assert orc["n_rows"] == 5 + n_general
    idx, ctx = _direct_ctx(ann, preset)
    assert_rows_equal(ctx.project_batch(lib.make_config(), batch), orc)
    ctx.close()
    idx.close()


def _bam_stream(recs):
    out = bytearray()
    for r in recs:
        paired = r.get("flags", 0) & 0x1
        out += _record(r["name"], r["ref_id"], r["ref_start"] - 1, r.get("flags", 0), r["cigar"], 0 if paired else -1,
                       r["mate_start"] - 1 if paired else -1, r["read_len"])
    return np.frombuffer(bytes(out), dtype=np.uint8)


@pytest.mark.parametrize("preset", SWITCH)
@pytest.mark.parametrize("flags", PRESETS[:2], ids=PRESET_IDS[:2])
def test_bam_records_equal_oracle(hand, flags, preset):
    """records in, records out: the encoder reads the detail column that the emit kernels write again on demand (the second
    launch site of the general class)"""
    ann, recs, _, memo = hand
    stream = _bam_stream(recs)
    roff, rlen, _, used = lib.bam_split(stream)
    assert used == stream.size and len(roff) == len(recs)
    ref_map = np.zeros(1, dtype=np.int32)
    key = ("bam",) + tuple(sorted(flags.items()))
    if key not in memo:
        memo[key] = ob.run_bam(ob.OracleIndex(ann), ob.make_flags(**flags), stream, roff, rlen, ref_map)[0]
    orc = memo[key]
    idx, ctx = _direct_ctx(ann, preset)
    got, counters = ctx.project_bam_bundle(lib.make_config(**flags), stream, roff, rlen, ref_map)
    ctx.close()
    idx.close()
    assert counters["n_rows"] == orc["n_rows"] > 300
    assert_streams_equal(got, orc["bam_stream"])
