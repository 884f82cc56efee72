"""The shared scan unit and the wave and block primitives (scan_kernels.hip, wave_inl.h, launch_scan3), each called directly
through libbramble_selftest.so and compared exactly with the references of tests/scan_ref.py, at the sizes, values and
alignments at which each path can go wrong.  test_scan_ref_cpu.py shows that these inputs fail wrong kernels.

Every output, scratch and total sits between guard words (tests/scan_probe.py); the scratch is exactly what scan_kernels.h
promises to stay within, prefilled with a nonzero pattern, and must be untouched by a one-launch scan."""
import functools

import numpy as np
import pytest

from tests import scan_ref as R
from tests.scan_probe import OUT_FILL, WAVE_OPS, WAVE_TYPES, Buf, call, check_scratch, lib, scratch_for, tiles_for

pytestmark = pytest.mark.gpu

SRC_FILL = 0x5a5a5a5a5a5a5a5a   # around the inputs: an item read past n would show in the sums
LARGE = tuple(n for n in R.SCAN_SIZES if n >= R.ROUND_ITEMS)


@functools.lru_cache(maxsize=2)
def _u32_sets(n):
    return R.scan_inputs_u32(n)


@functools.lru_cache(maxsize=8)
def _scan_ref(kind, n, name, bits):
    v = (_u32_sets(n) if kind == "u32" else R.scan_inputs_u64(n))[name]
    return R.excl_scan(v, bits)


def test_the_scratch_contract_is_the_headers():
    assert [tiles_for(n) for n in (0, 1, 2048, 2049, 8192, 8193)] == [0, 1, 1, 2, 4, 5] and lib().brst_scan_small_tiles() == 4
    assert R.TILE == 2048 and R.ONE_LAUNCH == 4 * 2048


# ---------------------------------------------------------------------------------------------------------------------
# launch_scan
# ---------------------------------------------------------------------------------------------------------------------

def scan_from_u32(v, out64, src_off=0, out_off=0, with_total=True, stream=None):
    n = v.size
    what = "launch_scan u32 -> u%d, n = %d, offsets %d / %d" % (64 if out64 else 32, n, src_off, out_off)
    src = Buf(np.uint32, n, src_off, fill=SRC_FILL, values=v)
    out = Buf(np.uint64 if out64 else np.uint32, n + 1, out_off)
    tmp, tot = scratch_for(n), Buf(np.uint64, 1)
    call(lib().brst_scan_u32, stream, src.ptr, n, tmp.ptr, out.ptr, int(out64), tot.ptr if with_total else None)
    got = out.read(what + ": out")
    check_scratch(tmp, n, what)
    src.assert_untouched(what + ": src")
    return got, int(tot.read(what + ": total")[0])


def scan_in_place(v, off=0):
    n = v.size
    what = "launch_scan u64 in place, n = %d, offset %d" % (n, off)
    a = Buf(np.uint64, n + 1, off, values=np.append(v, np.uint64(OUT_FILL)))
    tmp = scratch_for(n)
    call(lib().brst_scan_u64_inplace, None, a.ptr, n, tmp.ptr)
    got = a.read(what + ": a")
    check_scratch(tmp, n, what)
    return got


@pytest.mark.parametrize("out64", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("n", R.SCAN_SIZES)
def test_launch_scan_from_u32(n, out64):
    """every input set at every size: n > 4 194 304 runs the second round of k_scan_top (one full round, one tile into the
    second, a ragged second round); random u32 make the u32 output wrap and the total pass 2^32"""
    bits = 64 if out64 else 32
    for name, v in _u32_sets(n).items():
        want, total = _scan_ref("u32", n, name, bits)
        got, got_total = scan_from_u32(v, out64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s, n = %d: out[%d] = %d, not %d (%d wrong)" % (name, n, bad[0], got[bad[0]], want[bad[0]], bad.size)
        assert got.dtype == want.dtype and got_total == total, (name, got_total, total)
    if n > R.TILE:
        assert _scan_ref("u32", n, "random", bits)[1] >= 1 << 32


@pytest.mark.parametrize("n", R.SCAN_SIZES)
def test_launch_scan_in_place(n):
    for name, v in R.scan_inputs_u64(n).items():
        want, _ = _scan_ref("u64", n, name, 64)
        got = scan_in_place(v)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s, n = %d: a[%d] = %d, not %d (%d wrong)" % (name, n, bad[0], got[bad[0]], want[bad[0]], bad.size)


def test_launch_scan_without_a_total_and_on_a_stream_of_its_own():
    import torch
    n = 70001
    v = _u32_sets(n)["random"]
    want, total = _scan_ref("u32", n, "random", 64)
    got, untouched = scan_from_u32(v, True, with_total=False)
    assert np.array_equal(got, want) and untouched == OUT_FILL
    side = torch.cuda.Stream()
    got, got_total = scan_from_u32(v, True, stream=side.cuda_stream)
    assert np.array_equal(got, want) and got_total == total


@pytest.mark.parametrize("n", R.ALIGN_SIZES)
def test_launch_scan_at_every_alignment(n):
    """source and output each 0 ... 3 items behind a 16-byte boundary, independently (0 and 1 for u64): load8 and store8
    choose the vector or the item-by-item path each for itself"""
    v = _u32_sets(n)["random"]
    for out64, out_offs in ((False, range(4)), (True, range(2))):
        want, total = _scan_ref("u32", n, "random", 64 if out64 else 32)
        for src_off in range(4):
            for out_off in out_offs:
                got, got_total = scan_from_u32(v, out64, src_off, out_off)
                assert np.array_equal(got, want) and got_total == total, (n, out64, src_off, out_off)
    v64 = R.scan_inputs_u64(n)["random"]
    for off in range(2):
        assert np.array_equal(scan_in_place(v64, off), _scan_ref("u64", n, "random", 64)[0]), (n, off)


@pytest.mark.parametrize("n", LARGE)
def test_launch_scan_unaligned_through_two_rounds(n):
    v = _u32_sets(n)["random"]
    for out64, combos in ((False, ((1, 0), (0, 3))), (True, ((3, 0), (0, 1)))):
        want, total = _scan_ref("u32", n, "random", 64 if out64 else 32)
        for src_off, out_off in combos:
            got, got_total = scan_from_u32(v, out64, src_off, out_off)
            assert np.array_equal(got, want) and got_total == total, (n, out64, src_off, out_off)
    assert np.array_equal(scan_in_place(R.scan_inputs_u64(n)["random"], 1), _scan_ref("u64", n, "random", 64)[0])


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
@pytest.mark.parametrize("n", R.COPY8_SIZES)
def test_load8_and_store8_at_every_alignment(n, dtype):
    """load8 and store8 themselves, source and destination each at every offset: items at or past n read as 0 and are not
    written -- the destination has n items and a guard behind them that holds something else than a stored item would (the
    scans cannot show this: what they would store at out[n] is the total that belongs there)"""
    offs = range(4) if dtype == np.uint32 else range(2)
    v = (R.scan_inputs_u32(n) if dtype == np.uint32 else R.scan_inputs_u64(n))["random"]
    want, want_sums = R.copy8_ref(v)
    for src_off in offs:
        for dst_off in offs:
            what = "load8 / store8 <%s>, n = %d, offsets %d / %d" % (np.dtype(dtype), n, src_off, dst_off)
            src, dst = Buf(dtype, n, src_off, SRC_FILL, v), Buf(dtype, n, dst_off)
            sums = Buf(np.uint64, want_sums.size)
            call(lib().brst_copy8, None, WAVE_TYPES[np.dtype(dtype)], src.ptr, n, dst.ptr, sums.ptr)
            assert np.array_equal(dst.read(what + ": dst"), want), what
            assert np.array_equal(sums.read(what + ": sums"), want_sums), what + ": an item at or past n was not read as 0"


# ---------------------------------------------------------------------------------------------------------------------
# scan_top_rounds<C, ITEMS>
# ---------------------------------------------------------------------------------------------------------------------

TOP_CASES = [(c, items, n) for c, items, sizes in ((1, 8, R.TOP8_SIZES), (3, 8, R.TOP8_SIZES), (1, 32, R.TOP32_SIZES)) for n in sizes]


@pytest.mark.parametrize("with_total", [True, False], ids=["total", "no total"])
@pytest.mark.parametrize("channels,items,n_tiles", TOP_CASES)
def test_scan_top_rounds(channels, items, n_tiles, with_total):
    """one block over tile sums up to 2^40: more than 256 * ITEMS sums take a second round with a 64-bit carry"""
    t = R.top_inputs(n_tiles, channels)
    want, want_tot = R.top_rounds_ref(t, channels)
    what = "scan_top_rounds<%d, %d>, %d tiles" % (channels, items, n_tiles)
    sums, tot = Buf(np.uint64, t.size, values=t), Buf(np.uint64, channels)
    call(lib().brst_top_rounds, None, channels, items, sums.ptr, n_tiles, tot.ptr if with_total else None)
    got = sums.read(what)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: sum %d = %d, not %d (%d wrong)" % (what, bad[0], got[bad[0]], want[bad[0]], bad.size)
    if with_total:
        assert np.array_equal(tot.read(what + ": totals"), want_tot)
    else:
        tot.assert_untouched(what + ": totals not asked for")


# ---------------------------------------------------------------------------------------------------------------------
# launch_scan3
# ---------------------------------------------------------------------------------------------------------------------

def scan3(n, args, offs=(0, 0, 0, 0, 0, 0, 0)):
    nm, cf, co, ic = args
    what = "launch_scan3, n = %d, %s -S capacities, offsets %s" % (n, "with" if ic is not None else "without", offs)
    d_nm, d_cf = Buf(np.uint32, n, offs[0], SRC_FILL, nm), Buf(np.uint32, n, offs[1], SRC_FILL, cf)
    d_co = Buf(np.uint32, n + 1, offs[2], SRC_FILL, co) if ic is not None else None
    d_ic = Buf(np.uint32, n, offs[3], SRC_FILL, ic) if ic is not None else None
    mo, cb, fp = Buf(np.uint32, n + 1, offs[4]), Buf(np.uint64, n + 1, offs[5]), Buf(np.uint32, n + 1, offs[6])
    tmp, tot = scratch_for(n, 3), Buf(np.uint64, 3)
    call(lib().brst_scan3, None, n, d_nm.ptr, d_co.ptr if d_co else None, d_ic.ptr if d_ic else None, d_cf.ptr, tmp.ptr,
         mo.ptr, cb.ptr, fp.ptr, tot.ptr)
    got = (mo.read(what + ": match_off"), cb.read(what + ": cig_base"), fp.read(what + ": fast_pre"), tot.read(what + ": totals"))
    check_scratch(tmp, n, what)
    for b in (d_nm, d_cf, d_co, d_ic):
        if b:
            b.assert_untouched(what + ": inputs")
    return got


@pytest.mark.parametrize("with_caps", [False, True], ids=["class word", "-S capacities"])
@pytest.mark.parametrize("n", R.SCAN3_SIZES)
def test_launch_scan3(n, with_caps):
    """the three-value scan without the work list: n = 4 194 305 is the only way into the second round of k_scan3_top; the two
    32-bit outputs are the low words of the exact sums, cig_base and the totals are 64-bit"""
    for name, args in R.scan3_input_sets(n, with_caps).items():
        want = R.scan3_ref(*args)
        for offs in ((0, 0, 0, 0, 0, 0, 0), (1, 0, 3, 2, 2, 1, 0), (0, 3, 0, 1, 0, 0, 1)):
            got = scan3(n, args, offs)
            for out, g, w in zip(("match_off", "cig_base", "fast_pre", "totals"), got, want):
                bad = np.flatnonzero(g != w)
                assert g.dtype == w.dtype and bad.size == 0, "n = %d, %s, offsets %s: %s[%d] = %d, not %d (%d wrong)" % (
                    n, name, offs, out, bad[0], g[bad[0]], w[bad[0]], bad.size)
    if n > R.ROUND_ITEMS:
        assert all(int(t) >= 1 << 32 for t in want[3])


# ---------------------------------------------------------------------------------------------------------------------
# the wave primitives, block_excl_scan_256, block_bits
# ---------------------------------------------------------------------------------------------------------------------

def wave(op, v, w):
    src, out = Buf(v.dtype, v.size, fill=SRC_FILL, values=v), Buf(v.dtype, v.size)
    call(lib().brst_wave, None, WAVE_OPS[op], WAVE_TYPES[v.dtype], w, src.ptr, out.ptr, v.size // 256)
    return out.read("wave_%s<%s, %d>" % (op, v.dtype, w))


@pytest.mark.parametrize("w", R.WIDTHS)
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
@pytest.mark.parametrize("op", list(WAVE_OPS))
def test_wave_primitive(op, dtype, w):
    """4 blocks of 256: every group position in every wave of a block; every lane of a group holds the reduction, wave_scan the
    inclusive prefix of its group"""
    for name, v in R.wave_inputs(dtype, w).items():
        want = R.group_scan(v, w) if op == "scan" else R.group_reduce(op, v, w)
        got = wave(op, v, w)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "wave_%s<%s, %d>, %s: lane %d holds %#x, not %#x (%d wrong)" % (
            op, np.dtype(dtype), w, name, bad[0], got[bad[0]], want[bad[0]], bad.size)


@pytest.mark.parametrize("w", R.WIDTHS)
def test_wave_sum_of_doubles_keeps_its_order(w):
    """bit for bit the butterfly d = w / 2 ... 1 (the EM of the quantification is compared bit by bit)"""
    v = R.wave_doubles(w)
    got, want = wave("sum", v, w), R.butterfly_sum(v, w)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, "wave_sum<double, %d>: lane %d holds %r, not %r (%d wrong)" % (w, bad[0], got[bad[0]], want[bad[0]], bad.size)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
def test_block_excl_scan_256_three_times_through_one_sh(dtype):
    """three different inputs one after the other through the same sh[4], as k_scan3_* does: sh is free again when it returns"""
    planes = [R.wave_inputs(dtype, 64)["random"], R.wave_inputs(dtype, 32)["one cleared"], R.wave_inputs(dtype, 16)["random"]]
    assert not np.array_equal(planes[0], planes[2])
    v = np.concatenate(planes)
    src, out, tot = Buf(v.dtype, v.size, fill=SRC_FILL, values=v), Buf(v.dtype, v.size), Buf(v.dtype, v.size)
    call(lib().brst_block_scan, None, WAVE_TYPES[v.dtype], src.ptr, out.ptr, tot.ptr, planes[0].size // 256)
    got, got_tot = out.read("exclusive sums"), tot.read("totals")
    for j, p in enumerate(planes):
        want, want_tot = R.block_scan_ref(p)
        assert np.array_equal(got[j * p.size:(j + 1) * p.size], want), "scan %d of 3" % (j + 1)
        assert np.array_equal(got_tot[j * p.size:(j + 1) * p.size], want_tot), "totals of scan %d of 3" % (j + 1)


def test_block_bits_over_several_blocks_twice():
    """per-block OR / AND, with the only set (cleared) bit in thread 0, 63, 64 or 255 of a block; two launches back to back"""
    o, a = R.block_bits_inputs()
    want = R.block_bits_ref(o, a)
    d_o, d_a = Buf(np.uint64, o.size, fill=SRC_FILL, values=o), Buf(np.uint64, a.size, fill=SRC_FILL, values=a)
    out, out2 = Buf(np.uint64, want.size), Buf(np.uint64, want.size)
    call(lib().brst_block_bits, None, d_o.ptr, d_a.ptr, out.ptr, out2.ptr, o.size // 256)
    for k, b in enumerate((out, out2)):
        got = b.read("block_bits, launch %d" % (k + 1))
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "launch %d, block %d: %s = %#x, not %#x" % (k + 1, bad[0] // 2, "AND" if bad[0] & 1 else "OR", got[bad[0]], want[bad[0]])
