"""--quant-eff-length without a GPU: the tests' own restatement of the fragment-length definitions in bramble_amd.h (br_quant:
fragment, observation, effective length), which the GPU tests compare the device against; checks of those yardsticks against cases
worked out by hand; what the synthetic inputs hold; the new ABI without a device; the command line's usage errors."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

ROW_MINUS, ROW_PAIRED, ROW_SAME_TX, ROW_FIRST, ROW_PRIMARY = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28
LEAD = ROW_PAIRED | ROW_SAME_TX | ROW_FIRST
REF_OPS = (0, 2, 3, 7, 8)        # M D N = X consume the reference
OPS = "MIDNSHP=X"


# ---- the yardsticks -----------------------------------------------------------------------------------------------------------
def reflen(words):
    return sum(int(w) >> 4 for w in words if (int(w) & 15) in REF_OPS)


def fragment_at(rows, r, r1):
    """row r leads a fragment inside a name whose rows end at r1"""
    tid, meta = rows["tid"], rows["meta"]
    if (int(meta[r]) & LEAD) != LEAD or r + 1 >= r1:
        return False
    m = int(meta[r + 1])
    return bool(m & ROW_PAIRED) and not (m & ROW_FIRST) and int(tid[r + 1]) == int(tid[r])


def fragment_length(rows, r):
    off, cig, pos = rows["cigar_off"], rows["cigar"], rows["pos"]
    ends = [int(pos[k]) + reflen(cig[int(off[k]):int(off[k + 1])]) for k in (r, r + 1)]
    return max(ends) - min(int(pos[r]), int(pos[r + 1]))


def fragments_of(rows, row_off, group_off, fld_max):
    """rows: tid, pos, meta per row and the rewritten CIGARs as cigar_off / cigar; read name g has the rows
    row_off[group_off[g]] .. row_off[group_off[g + 1]].  -> dict hist (uint64 [fld_max + 1]), n_obs, n_no_fragment, n_out_of_range"""
    hist = np.zeros(fld_max + 1, dtype=np.uint64)
    n_no_fragment = n_out_of_range = 0
    for g in range(len(group_off) - 1):
        r0, r1 = int(row_off[int(group_off[g])]), int(row_off[int(group_off[g + 1])])
        if len(set(int(t) for t in rows["tid"][r0:r1])) != 1:
            continue
        lead = next((r for r in range(r0, r1) if fragment_at(rows, r, r1)), None)
        if lead is None:
            n_no_fragment += 1
            continue
        f = fragment_length(rows, lead)
        if f == 0 or f > fld_max:
            n_out_of_range += 1
        else:
            hist[f] += 1
    return {"hist": hist, "n_obs": int(hist.sum()), "n_no_fragment": n_no_fragment, "n_out_of_range": n_out_of_range}


def prefix_at(hist, length, fld_max):
    x = min(int(length), fld_max)
    return sum(int(hist[f]) for f in range(x + 1)), sum(f * int(hist[f]) for f in range(x + 1))


def eff_lengths(hist, lens, fld_max):
    """-> float64 per transcript: (L + 1) C(x) - S(x) over C(x) at x = min(L, fld_max), L where C(x) is 0, 0 for L <= 0; the two
    integers are exact, each becomes a double (round to nearest even) and the division rounds once"""
    c_at = np.cumsum([int(v) for v in hist], dtype=object)
    s_at = np.cumsum([f * int(v) for f, v in enumerate(hist)], dtype=object)
    out = np.zeros(len(lens), dtype=np.float64)
    for t, length in enumerate(int(v) for v in lens):
        if length <= 0:
            continue
        x = min(length, fld_max)
        c, s = int(c_at[x]), int(s_at[x])
        out[t] = float(length) if c == 0 else float((length + 1) * c - s) / float(c)
    return out


# ---- rows in the yardstick's form and in the device's --------------------------------------------------------------------------------
def rows_of(items):
    """items: (tid, pos, meta bits, CIGAR text or a list of op words) per row -> the yardstick's rows; NCIGAR goes into meta"""
    words = [[(int(n) << 4) | OPS.index(o) for n, o in _split(c)] if isinstance(c, str) else [int(w) for w in c] for _, _, _, c in items]
    return {"tid": np.asarray([i[0] for i in items], dtype=np.uint32), "pos": np.asarray([i[1] for i in items], dtype=np.uint32),
            "meta": np.asarray([i[2] | len(w) for i, w in zip(items, words)], dtype=np.uint32),
            "cigar_off": np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.uint64),
            "cigar": np.asarray([x for w in words for x in w], dtype=np.uint32)}


def _split(text):
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((num, ch))
            num = ""
    return out


def packed_of(rows, gap=3):
    """the yardstick's rows as br_device_rows holds them: a uint32 [n, 4] (nh = 1), cigar uint64 [n] -- the ops themselves up to two
    (op 0 in the low word), else the offset of the ops in pool -- and a pool with `gap` unused words in front of every CIGAR (the
    device's arena is sparse as well)"""
    n = len(rows["tid"])
    a = np.zeros((n, 4), dtype=np.uint32)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = rows["tid"], rows["pos"], rows["meta"], 1
    ref = np.zeros(n, dtype=np.uint64)
    pool = []
    for r in range(n):
        w = [int(x) for x in rows["cigar"][int(rows["cigar_off"][r]):int(rows["cigar_off"][r + 1])]]
        assert len(w) == int(rows["meta"][r]) & 0xffffff
        if len(w) <= 2:
            ref[r] = (w[0] if w else 0) | ((w[1] if len(w) == 2 else 0) << 32)
        else:
            pool += [0xfffffff0] * gap   # (an M of 2^28 - 1 bases: a reader that strays into the gap shows)
            ref[r] = len(pool)
            pool += w
    return a, ref, np.asarray(pool, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def wide_rows(mode, guide_order=False, collated=False):
    """(tests.test_quant_cpu.oracle_tables of the input -- collated: of its coordinate-sorted, re-collated records --, the oracle's
    rows of it in the yardstick's form)"""
    from oracle import oracle_binding as ob
    from tests.test_quant_cpu import oracle_tables
    recs = None
    if collated:
        from tests.test_collate_cpu import collate_order, mapped_records
        from tests.test_gpu_collate import _coordinate_stream, _inputs
        permuted = mapped_records(_coordinate_stream(_inputs(mode)[2]))
        recs = [permuted[i] for i in collate_order(permuted)]
    tb = oracle_tables(mode, recs, guide_order=guide_order)
    wide, _, _, _ = ob.run_bam(ob.OracleIndex(tb["annd"]), ob.make_flags(**tb["flags"]), tb["stream"], tb["roff"], tb["rlen"],
                               np.arange(len(tb["annd"]["refnames"]), dtype=np.int32))
    from tests.route_cases import yardstick_rows
    rows, row_off, group_off = yardstick_rows(wide, tb["group_off"])
    assert np.array_equal(rows["tid"], tb["tids"]) and np.array_equal(row_off, tb["row_off"]) and np.array_equal(group_off, tb["group_off"])
    return tb, rows


# ---- the yardsticks against cases worked out by hand ------------------------------------------------------------------------------
def _one_name(items, fld_max=1000):
    rows = rows_of(items)
    return fragments_of(rows, [0, len(items)], [0, 1], fld_max)


def _only(fr):
    assert fr["n_obs"] == 1 and fr["n_no_fragment"] == 0 and fr["n_out_of_range"] == 0
    return int(np.flatnonzero(fr["hist"])[0])


def test_fragment_length_by_hand():
    lead, mate = LEAD, ROW_PAIRED | ROW_SAME_TX
    # the leader upstream, downstream, and one mate inside the other: 100 .. 300 each time
    assert _only(_one_name([(4, 100, lead, "50M"), (4, 250, mate | ROW_MINUS, "50M")])) == 200
    assert _only(_one_name([(4, 250, lead | ROW_MINUS, "50M"), (4, 100, mate, "50M")])) == 200
    assert _only(_one_name([(4, 100, lead, "200M"), (4, 150, mate, "50M")])) == 200
    assert _only(_one_name([(4, 150, lead, "50M"), (4, 100, mate, "200M")])) == 200
    # D and N count, I S H P do not: 10 + 4 + 20 + 6 = 40 from position 7; = and X count: 7 + 8 from 30 -> the mate ends at 45
    assert reflen(rows_of([(0, 0, 0, "5S10M3I4D20N6M2P5H")])["cigar"]) == 40
    assert _only(_one_name([(4, 7, lead, "5S10M3I4D20N6M2P5H"), (4, 30, mate, "7=8X9S")])) == 40
    assert _only(_one_name([(4, 7, lead, "5H10M"), (4, 30, mate, "2S7=3I8X1P")])) == 38
    # the first fragment counts, not a later one; rows in front of it that are no leaders are passed over
    fr = _one_name([(4, 0, ROW_FIRST, "30M"), (4, 10, lead, "30M"), (4, 100, mate, "30M"), (4, 10, lead, "30M"), (4, 500, mate, "30M")])
    assert _only(fr) == 120


def test_what_is_no_fragment_by_hand():
    lead, mate = LEAD, ROW_PAIRED | ROW_SAME_TX
    none = {"n_obs": 0, "n_no_fragment": 1, "n_out_of_range": 0}

    def counts(fr):
        return {k: fr[k] for k in none}
    assert counts(_one_name([(4, 100, ROW_FIRST, "50M")])) == none                                   # unpaired
    assert counts(_one_name([(4, 100, lead, "50M")])) == none                                        # the leader is the last row
    assert counts(_one_name([(4, 100, lead, "50M"), (4, 200, ROW_SAME_TX, "50M")])) == none          # the neighbour is not paired
    assert counts(_one_name([(4, 100, lead, "50M"), (4, 200, lead, "50M")])) == none                 # the neighbour leads itself
    assert counts(_one_name([(4, 100, lead & ~ROW_SAME_TX, "50M"), (4, 200, mate, "50M")])) == none  # SAME_TX is missing
    # a second label: the name is not unique and counts nowhere, with a fragment or without
    nowhere = {"n_obs": 0, "n_no_fragment": 0, "n_out_of_range": 0}
    assert counts(_one_name([(4, 100, lead, "50M"), (5, 200, mate, "50M")])) == nowhere
    assert counts(_one_name([(4, 100, lead, "50M"), (4, 200, mate, "50M"), (9, 0, ROW_FIRST, "50M")])) == nowhere
    assert counts(_one_name([])) == nowhere
    # a name's last row never pairs with the next name's first: two names, the second starts with what would be a mate
    rows = rows_of([(4, 100, lead, "50M"), (4, 200, mate, "50M"), (4, 300, lead, "50M")])
    fr = fragments_of(rows, [0, 1, 3], [0, 1, 2], 1000)
    assert counts(fr) == {"n_obs": 0, "n_no_fragment": 2, "n_out_of_range": 0}
    # lengths 0, fld_max and fld_max + 1
    out = {"n_obs": 0, "n_no_fragment": 0, "n_out_of_range": 1}
    assert counts(_one_name([(4, 100, lead, []), (4, 100, mate, "5S")])) == out
    assert counts(_one_name([(4, 0, lead, "38M"), (4, 10, mate, "5M")], fld_max=37)) == out
    assert _only(_one_name([(4, 0, lead, "37M"), (4, 10, mate, "5M")], fld_max=37)) == 37


def test_packed_rows_round_trip():
    rows = rows_of([(1, 5, LEAD, "3M"), (1, 9, ROW_PAIRED, "3M2I"), (2, 0, 0, "1S2M3D4M"), (2, 0, 0, []), (2, 1, ROW_MINUS, "9=1X2M")])
    a, ref, pool = packed_of(rows)
    assert a[:, 2].tolist() == [LEAD | 1, ROW_PAIRED | 2, 4, 0, ROW_MINUS | 3]
    assert ref.tolist() == [3 << 4, (3 << 4) | (((2 << 4) | 1) << 32), 3, 0, 10]
    assert pool[3:7].tolist() == [(1 << 4) | 4, 2 << 4, (3 << 4) | 2, 4 << 4] and len(pool) == 13


def test_effective_length_by_hand():
    hist = np.zeros(1001, dtype=np.uint64)
    hist[200], hist[300] = 2, 2
    # below the shortest observation: the length itself; at it: 200 - 200 + 1; between: 250 - 200 + 1; from 300 on the mean is 250
    lens = [150, 199, 200, 250, 299, 300, 1000, 5000, 0, -3]
    eff = eff_lengths(hist, lens, 1000)
    assert eff.tolist() == [150.0, 199.0, 1.0, 51.0, 100.0, 51.0, 751.0, 4751.0, 0.0, 0.0]
    assert prefix_at(hist, 250, 1000) == (2, 400) and prefix_at(hist, 5000, 1000) == (4, 1000)
    # no observation at all: every length is its own effective length
    assert eff_lengths(np.zeros(38, dtype=np.uint64), [1, 37, 38, 4000], 37).tolist() == [1.0, 37.0, 38.0, 4000.0]
    # a division that does not come out even is rounded once: (11 * 3 - 25) / 3
    h = np.zeros(38, dtype=np.uint64)
    h[7], h[9] = 1, 2
    assert eff_lengths(h, [10], 37)[0] == 8.0 / 3.0
    # eff >= 1 wherever the length is positive, and never above the length
    rng = np.random.RandomState(11)
    h = rng.randint(0, 5, size=301).astype(np.uint64)
    h[0] = 0
    lens = np.arange(1, 700)
    eff = eff_lengths(h, lens, 300)
    assert np.all(eff >= 1.0) and np.all(eff <= lens)


# ---- what the synthetic inputs hold ------------------------------------------------------------------------------------------------
def test_inputs_hold_what_the_feature_is_about():
    tb, rows = wide_rows("pe")
    fr = fragments_of(rows, tb["row_off"], tb["group_off"], 1000)
    n_unique = fr["n_obs"] + fr["n_no_fragment"] + fr["n_out_of_range"]
    seen = np.flatnonzero(fr["hist"])
    c_at = np.asarray([prefix_at(fr["hist"], length, 1000)[0] for length in tb["lens"]])
    fallback, partial = int(np.sum(c_at == 0)), int(np.sum((c_at > 0) & (c_at < fr["n_obs"])))
    print("pe: %d observations from %d unique names, %d distinct lengths from %d to %d, %d transcripts on the fallback, %d with "
          "0 < C(x) < n_obs" % (fr["n_obs"], n_unique, len(seen), seen[0], seen[-1], fallback, partial))
    assert fr["n_obs"] >= 300 and len(seen) >= 100 and fallback >= 100 and partial >= 150
    assert fr["n_out_of_range"] == 0
    tb, rows = wide_rows("ont")
    fr = fragments_of(rows, tb["row_off"], tb["group_off"], 1000)
    assert fr["n_obs"] == 0 and fr["n_out_of_range"] == 0 and fr["n_no_fragment"] > 100 and not fr["hist"].any()
    assert eff_lengths(fr["hist"], tb["lens"], 1000).tolist() == [float(v) if v > 0 else 0.0 for v in tb["lens"]]


# ---- ABI and usage errors -------------------------------------------------------------------------------------------------------
def test_new_symbols_without_a_device():
    from bramble_amd import lib
    L = lib.lib()
    for name in ("br_quant_add_rows", "br_quant_fld", "br_quant_eff_lengths"):
        assert hasattr(L, name), name
    L.br_quant_add_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.br_quant_fld.argtypes = [C.c_void_p] * 5
    L.br_quant_eff_lengths.argtypes = [C.c_void_p, C.c_void_p]
    rows = lib.BrDeviceRows()
    assert L.br_quant_add_rows(None, C.byref(rows), None, 0, 0, None) == -1   # BR_ERR_INVALID_ARG
    assert L.br_quant_fld(None, None, None, None, None) == -1
    eff = (C.c_double * 4)()
    assert L.br_quant_eff_lengths(None, eff) == -1
    for name in ("add_rows_host", "add_rows_device", "fld", "eff_lengths"):
        assert hasattr(lib.Quant, name), name


@pytest.mark.parametrize("extra", [
    ["--quant-eff-length"],
    ["--quant-fld", "f.tsv"],
    ["--quant-eff-length", "--quant-fld", "f.tsv"],
    ["--quant", "q.tsv", "--quant-fld", "f.tsv"],
    ["--quant", "q.tsv", "--quant-eff-length", "--quant-no-length-norm"],
    ["--quant", "q.tsv", "--quant-eff-length", "--lr"],
    ["--quant", "q.tsv", "--quant-eff-length", "--quant-fld", "f.tsv", "--lr-hq"],
])
def test_cli_usage_errors(tmp_path, extra):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    extra = [str(tmp_path / e) if e.endswith(".tsv") else e for e in extra]
    r = subprocess.run([os.path.join(root, "bramble_amd", "bin", "bramble"), str(tmp_path / "missing.bam"), "-G", str(gtf), "-o",
                        str(tmp_path / "o.bam")] + extra, capture_output=True, timeout=60)
    assert r.returncode == 2
    assert b"--quant" in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]
