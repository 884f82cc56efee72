"""--quant-bam without a GPU: the yardstick (tests/quant_bam_cases.py) against cases worked out by hand, a statistical check of the
yardstick's draw, what the inputs of the GPU tests hold, the new ABI without a device and the command line's usage errors."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bamio
from tests import quant_bam_cases as qb
from tests.test_coverage_weight_cpu import name_classes_of, posteriors_of, row_names_of
from tests.test_quant_boot_cpu import philox4x32_10
from tests.test_quant_cpu import classes_of
from tests.test_quant_fld_cpu import ROW_FIRST, ROW_PAIRED, ROW_SAME_TX, wide_rows

F = ROW_FIRST
LEAD, MATE = ROW_FIRST | ROW_PAIRED, ROW_PAIRED


_table = qb.table_of


def _weigh(names, theta, w_tx=None):
    tids, meta, row_off, group_off = _table(names)
    cl = classes_of(tids, row_off, group_off)
    theta = np.asarray(theta, dtype=np.float64)
    post = posteriors_of(cl, theta, np.ones(len(theta)) if w_tx is None else w_tx)
    pl = qb.placements_of(meta, row_off, group_off)
    w, m = qb.weights_of(post, cl, name_classes_of(tids, row_off, group_off), row_names_of(len(tids), row_off, group_off), tids, pl)
    return w, m, pl


# ---- by hand ---------------------------------------------------------------------------------------------------------------------
def test_one_placement_has_weight_one():
    w, m, pl = _weigh([[(3, F)]], [0, 0, 0, 0.7])
    assert w.tolist() == [1.0] and m.tolist() == [1] and pl[1] == [[0]]
    assert qb.zw_of(w).view(np.uint32).tolist() == [0x3f800000]
    assert qb.picks_of(w, pl, 0).tolist() == [0] and qb.kept_of(w, pl, "sample", 5).tolist() == [1]


def test_a_pair_on_two_transcripts_is_one_placement():
    # theta 1 and 3 on the transcripts 0 and 1: the posteriors are 0.25 and 0.75, and the pair's w is their sum, leader first
    w, m, pl = _weigh([[(0, LEAD), (1, MATE)]], [1.0, 3.0])
    assert pl[0].tolist() == [0, 0] and pl[1] == [[0]] and m.tolist() == [1, 1]
    assert w.tolist() == [1.0, 1.0]
    # beside a second placement on transcript 1 alone: p = (0.25, 0.75), m = (1, 2, 2): w = 0.25 + 0.375 and 0.375
    w, m, pl = _weigh([[(0, LEAD), (1, MATE), (1, F)]], [1.0, 3.0])
    assert m.tolist() == [1, 2, 2] and w.tolist() == [0.625, 0.625, 0.375] and pl[1] == [[0, 2]]


def test_two_placements_on_one_transcript_halve_the_posterior():
    w, m, pl = _weigh([[(0, F), (0, F), (1, F)]], [1.0, 1.0])
    assert m.tolist() == [2, 2, 1] and w.tolist() == [0.25, 0.25, 0.5]
    assert float(np.sum(w)) == 1.0


def test_a_class_without_mass_weighs_nothing_and_picks_placement_0():
    w, m, pl = _weigh([[(0, F), (1, F)]], [0.0, 0.0])
    assert w.tolist() == [0.0, 0.0]
    for seed in range(4):
        assert qb.picks_of(w, pl, seed).tolist() == [0]
    assert qb.kept_of(w, pl, "sample", 0).tolist() == [1, 0]


def test_a_target_on_a_boundary_picks_the_next_placement():
    # W = 1, U = 0.25: target == cum_0 exactly, and cum_0 > target is false
    assert qb.pick_of([0.25, 0.75], 0.25) == 1
    assert qb.pick_of([0.25, 0.75], np.nextafter(0.25, 0)) == 0
    assert qb.pick_of([0.25, 0.0, 0.75], 0.25) == 2      # a placement of weight 0 is never the first above the target
    assert qb.pick_of([0.5, 0.5], 0.0) == 0


def test_the_fallback_when_rounding_leaves_the_last_sum_at_the_target():
    # target > the last cum cannot be reached with U < 1 and the same order of summation, so the fallback is shown through a U of
    # 1.0, which the generator never gives: the last placement of positive weight, not the last one
    assert qb.pick_of([0.1, 0.2, 0.0], 1.0) == 1
    assert qb.pick_of([0.0, 0.0], 1.0) == 0
    ws = [0.1] * 10
    assert qb.pick_of(ws, 1.0 - 2.0 ** -53) == 9


def test_the_counter_differs_from_the_bootstraps():
    names = np.arange(64, dtype=np.uint64)
    z, one = np.zeros(64, np.uint64), np.ones(64, np.uint64)
    boot = philox4x32_10((names, z, z, z), (7, 0))       # draw i of replicate 0
    mine = philox4x32_10((names, z, z, one), (7, 0))
    assert not np.any((boot[0] == mine[0]) & (boot[1] == mine[1]))
    U = qb.uniform_of(names, 7)
    assert np.array_equal(U, ((mine[0] | (mine[1] << np.uint64(32))) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)
    assert U.min() >= 0.0 and U.max() < 1.0 and len(set(U.tolist())) == 64
    assert not np.array_equal(U, qb.uniform_of(names, 8))


def test_placements_that_are_none():
    for names in ([[(0, MATE)]],                           # a mate without a leader
                  [[(0, LEAD)]],                           # a leader without a mate
                  [[(0, LEAD)], [(0, MATE)]],              # the mate lies in the next name
                  [[(0, 0)]],                              # neither FIRST nor PAIRED
                  [[(0, LEAD), (0, F)]],                   # the next record is no mate
                  [[(0, LEAD), (0, MATE), (0, MATE)]]):    # a second mate
        tids, meta, row_off, group_off = _table(names)
        with pytest.raises(ValueError):
            qb.placements_of(meta, row_off, group_off)


def _record(name, aux, cigar=None, l_seq=20, flag=0x100 | 0x1, spill=None):
    body = bamio.bam_record(name, 2, 100, cigar or [(l_seq << 4) | 0], l_seq, flag=flag, aux=aux, mapq=1, spill=spill)
    return struct.pack("<I", len(body)) + body


def _tags(nh, hi, as_=None):
    out = b"NHi" + struct.pack("<i", nh)
    if as_ is not None:
        out += b"ASi" + struct.pack("<i", as_)
    return out + b"HIi" + struct.pack("<i", hi)


def test_rewrite_by_hand():
    front = b"NMC\x01" + b"MDZ20\0" + b"XBBs" + struct.pack("<Ihh", 2, -1, 5)
    one = _record(b"q1", front + _tags(8, 3))
    got = bytes(qb.rewrite([one], np.asarray([0.5], np.float32), [1], "tag"))
    assert got == struct.pack("<I", len(one) - 4 + 7) + one[4:] + b"ZWf" + struct.pack("<f", 0.5)
    got = bytes(qb.rewrite([one], np.asarray([0.5], np.float32), [1], "sample"))
    want = bytearray(struct.pack("<I", len(one) - 4 + 7) + one[4:] + b"ZWf" + struct.pack("<f", 0.5))
    want[4 + 9] = 255
    want[4 + 14:4 + 16] = struct.pack("<H", 0x1)
    at = len(one) - 14
    want[at + 3:at + 7] = struct.pack("<i", 1)
    want[at + 10:at + 14] = struct.pack("<i", 1)
    assert got == bytes(want)
    # long reads: AS:i between the two, MAPQ 3; a spilled CIGAR: the entries are in front of the CG tag, the ZW entry behind it
    lr = _record(b"q2", front + _tags(4, 2, as_=77), cigar=[(10 << 4) | 0, (5 << 4) | 2, (10 << 4) | 0], spill=True)
    got = bytes(qb.rewrite([one, lr], np.asarray([0.5, 0.25], np.float32), [0, 1], "sample", long_reads=True))
    f = bamio.record_fields(got[4:])
    tags = {e[1]: (e[0], e[2]) for e in qb.aux_entries(f["aux"])}
    assert list(tags) == [b"NM", b"MD", b"XB", b"NH", b"AS", b"HI", b"CG", b"ZW"]
    val = lambda t: struct.unpack_from("<i", f["aux"], tags[t][0] + 3)[0]   # noqa: E731
    assert (val(b"NH"), val(b"AS"), val(b"HI")) == (1, 77, 1) and f["mapq"] == 3 and f["flag"] == 0x1
    assert struct.unpack_from("<f", f["aux"], tags[b"ZW"][0] + 3)[0] == 0.25 and len(got) == len(lr) + 7
    assert qb.rewrite([one, lr], np.zeros(2, np.float32), [0, 0], "sample").size == 0


# ---- the draw is what it says --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2026])
def test_the_draw_follows_the_weights(seed):
    n = 4096
    names = [[(0, F), (1, F)] for _ in range(n)]
    w, _, pl = _weigh(names, [1.0, 3.0])
    assert set(w[0::2].tolist()) == {0.25} and set(w[1::2].tolist()) == {0.75}
    picks = qb.picks_of(w, pl, seed)
    share = float(np.count_nonzero(picks == 0)) / n
    sd = (0.25 * 0.75 / n) ** 0.5
    print(seed, share, sd)
    assert abs(share - 0.25) <= 4 * sd
    kept = qb.kept_of(w, pl, "sample", seed)
    assert int(kept.sum()) == n and np.array_equal(kept[0::2], (picks == 0).astype(np.uint8))


# ---- what the GPU tests' inputs hold -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_inputs_hold_what_the_feature_is_about(mode):
    """the hand-built table of tests/test_gpu_quant_bam.py supplies what a generated table lacks: the pair with SAME_TX clear
    (both modes: the inputs emit no pair whose mates sit on different transcripts) and, for ont, every pair"""
    tb, rows = wide_rows(mode)
    tids, meta = rows["tid"], rows["meta"]
    pl = qb.placements_of(meta, tb["row_off"], tb["group_off"])
    cl = classes_of(tids, tb["row_off"], tb["group_off"])
    theta = np.ones(tb["n_tx"])
    post = posteriors_of(cl, theta, np.ones(tb["n_tx"]))
    names = row_names_of(len(tids), tb["row_off"], tb["group_off"])
    w, m = qb.weights_of(post, cl, name_classes_of(tids, tb["row_off"], tb["group_off"]), names, tids, pl)
    picks = qb.picks_of(w, pl, 1)
    held = {"names_2_placements": sum(1 for mine in pl[1] if len(mine) >= 2), "m_2plus": int(np.count_nonzero(m >= 2)),
            "pick_not_0": int(np.count_nonzero(picks > 0)), "no_rows": int(np.count_nonzero(picks < 0)),
            "pairs": int(np.count_nonzero(meta & ROW_PAIRED)) // 2,
            "pairs_on_two": int(np.count_nonzero((meta & ROW_PAIRED != 0) & (meta & ROW_FIRST != 0) & (meta & ROW_SAME_TX == 0)))}
    print(mode, held)
    assert held["names_2_placements"] >= 100 and held["pick_not_0"] >= 50 and held["no_rows"] >= 1
    if mode == "pe":
        assert held["pairs"] >= 100
    sums = np.zeros(len(pl[1]))
    np.add.at(sums, names[pl[0] == np.arange(len(tids))], w[pl[0] == np.arange(len(tids))])
    has = np.asarray([len(mine) > 0 for mine in pl[1]])
    assert np.allclose(sums[has], 1.0, rtol=0, atol=1e-12)   # a name's placements share its posteriors
    hn, _ = qb.hand_built()
    htids, hmeta, hro, hgo = _table(hn)
    hpl = qb.placements_of(hmeta, hro, hgo)
    sizes = [len(nm) for nm in hn]
    assert int(np.count_nonzero((hmeta & ROW_PAIRED != 0) & (hmeta & ROW_FIRST != 0) & (hmeta & ROW_SAME_TX == 0))) >= 3
    assert sizes[3] == 1 and sizes[10] == 0 and sizes[9] > 0 and sizes[11] > 0
    assert len(hpl[1][5]) == 130 and len({t for t, _ in hn[5]}) == 70 and sizes[7] == 65 and len({t for t, _ in hn[7]}) == 1
    k = len(hn) // 3
    assert all(sizes[i] >= 2 for i in (0, k - 1, k, k + 1, len(hn) - 1))
    hcl = classes_of(htids, hro, hgo)
    hw, hm = qb.weights_of(posteriors_of(hcl, np.ones(qb.HAND_N_TX), np.ones(qb.HAND_N_TX)), hcl, name_classes_of(htids, hro, hgo),
                           row_names_of(len(htids), hro, hgo), htids, hpl)
    assert int(hm.max()) == 65 and held["m_2plus"] + int(np.count_nonzero(hm >= 2)) >= 100
    assert int(np.count_nonzero(qb.picks_of(hw, hpl, 1) > 0)) >= 5


# ---- ABI and usage errors ------------------------------------------------------------------------------------------------------
SYMBOLS = ("br_assign_new", "br_assign_set_param", "br_assign_add", "br_assign_add_last", "br_assign_finish", "br_assign_values", "br_assign_next",
           "br_assign_stats", "br_assign_free")


def test_new_symbols_without_a_device():
    from bramble_amd import lib
    L = lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    L.br_assign_new.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.br_assign_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.br_assign_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.br_assign_add_last.argtypes = [C.c_void_p, C.c_void_p]
    L.br_assign_finish.argtypes = [C.c_void_p] * 4
    L.br_assign_values.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.br_assign_next.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.br_assign_stats.argtypes = [C.c_void_p] * 7
    L.br_assign_free.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert L.br_assign_new(4096, C.byref(h)) == -2 and not h.value   # BR_ERR_NO_DEVICE
    assert L.br_assign_new(0, None) == -1
    rows, piece = lib.BrDeviceRows(), lib.BrDeviceBam()
    assert L.br_assign_values(None, 0, 0, None, None, None) == -1 and L.br_assign_next(None, 1, C.byref(piece)) == -1   # BR_ERR_INVALID_ARG
    assert L.br_assign_set_param(None, b"mode", 1) == -1 and L.br_assign_add(None, None, C.byref(rows), None, 0, 0, None) == -1
    assert L.br_assign_add_last(None, None) == -1 and L.br_assign_finish(None, None, None, None) == -1
    assert L.br_assign_stats(None, None, None, None, None, None, None) == -1
    L.br_assign_free(None)
    for name in ("set_param", "add_host", "add_device", "add_last", "finish", "values", "next_records", "stats"):
        assert hasattr(lib.Assign, name), name


@pytest.mark.parametrize("extra,word", [
    (["--quant-bam", "p.bam"], b"--quant-bam needs --quant"),
    (["--quant", "q.tsv", "--quant-bam-mode", "sample"], b"--quant-bam-mode needs --quant-bam"),
    (["--quant", "q.tsv", "--quant-bam", "p.bam", "--quant-bam-mode", "best"], b"unknown mode best"),
    (["--quant", "q.tsv", "--quant-bam", "p.bam", "--devices", "0,1"], b"one device"),
])
def test_cli_usage_errors(tmp_path, extra, word):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    extra = [str(tmp_path / e) if e.endswith((".tsv", ".bam")) else e for e in extra]
    r = subprocess.run([os.path.join(root, "bramble_amd", "bin", "bramble"), str(tmp_path / "missing.bam"), "-G", str(gtf), "-o",
                        str(tmp_path / "o.bam")] + extra, capture_output=True, timeout=60)
    assert r.returncode == 2
    assert word in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]
