"""The references and inputs of test_gpu_scan_unit.py can tell right from wrong: the references agree with naive loops, every
input set separates every wrong scan (tests/scan_ref.py) from the reference, and the doubles give other bits in any other
order of summation.  No GPU."""
import numpy as np
import pytest

from tests import scan_ref as R
from tests.scan_probe import OUT_FILL

BOUNDS = {"a tile boundary": R.TILE, "the one-launch cut": R.ONE_LAUNCH, "a round boundary": R.ROUND_ITEMS}


def _bits(a):
    return np.asarray(a).view(np.uint64) if np.asarray(a).dtype == np.float64 else np.asarray(a)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and int(a[1]) == int(b[1])


# ---------------------------------------------------------------------------------------------------------------------
# the references against naive loops
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [0, 1, 2, 9, 300])
def test_exclusive_scan_is_the_naive_loop(n, bits):
    v = R.scan_inputs_u64(n)["random"] * np.uint64(1 << 23)   # below 2^63: the sums pass 2^64 within a few items
    want, acc = [], 0
    for x in v.tolist():
        want.append(acc % (1 << bits))
        acc += x
    want.append(acc % (1 << bits))
    out, total = R.excl_scan_exact(v, bits)
    assert out.dtype == (np.uint32 if bits == 32 else np.uint64) and out.tolist() == want and total == acc
    assert R.sums_mod64(v).tolist() == [w for w in R.excl_scan_exact(v, 64)[0].tolist()]
    if n:
        assert total >= 1 << 64 or n < 9


@pytest.mark.parametrize("make", [R.scan_inputs_u32, R.scan_inputs_u64])
def test_wrapping_sums_are_the_exact_ones(make):
    v = make(R.EXACT_UP_TO + 12345)["random"]
    for bits in (32, 64):
        a, b = R.excl_scan_exact(v, bits), R.excl_scan_wrapping(v, bits)
        assert a[0].dtype == b[0].dtype and _same(a, b)
    assert R.excl_scan(v, 64)[1] == int(v.astype(object).sum()) and R.excl_scan(v[:100], 64)[1] == int(v[:100].astype(object).sum())


@pytest.mark.parametrize("with_caps", [False, True])
def test_three_value_scan_is_the_naive_loop(with_caps):
    nm, cf, co, ic = R.scan3_inputs(700, with_caps)
    assert 0.3 < np.mean(nm == 0) < 0.7 and nm.max() > 4000 and 0.8 < np.mean(cf >> 31) < 0.95 and (cf & 0x7fffffff).max() > 0x7f000000
    acc, rows = [0, 0, 0], []
    for i in range(700):
        rows.append(list(acc))
        if nm[i]:
            cap = (int(co[i + 1]) - int(co[i]) + 2 * int(ic[i])) % (1 << 32) if with_caps else int(cf[i]) & 0x7fffffff
            acc[0] += int(nm[i]); acc[1] += int(nm[i]) * cap; acc[2] += int(nm[i]) if int(cf[i]) >> 31 else 0
    rows.append(list(acc))
    mo, cb, fp, tot = R.scan3_ref(nm, cf, co, ic)
    assert (mo.dtype, cb.dtype, fp.dtype) == (np.uint32, np.uint64, np.uint32)
    assert mo.tolist() == [r[0] % (1 << 32) for r in rows] and cb.tolist() == [r[1] for r in rows] and fp.tolist() == [r[2] % (1 << 32) for r in rows]
    assert tot.tolist() == acc


def test_copy_probe_reference_is_the_naive_loop():
    for n in R.COPY8_SIZES:
        v = R.scan_inputs_u32(n)["random"]
        out, sums = R.copy8_ref(v)
        assert out.dtype == v.dtype and out.tolist() == [x ^ 0xffffffff for x in v.tolist()]
        assert sums.tolist() == [sum(v[t:t + 8].tolist()) for t in range(0, max((n + 2047) // 2048, 1) * 2048, 8)]


def test_tile_sum_scan_is_the_naive_loop():
    t = R.top_inputs(37, 3)
    out, tot = R.top_rounds_ref(t, 3)
    for c in range(3):
        acc = 0
        for k in range(37):
            assert int(out[c * 37 + k]) == acc
            acc += int(t[c * 37 + k])
        assert int(tot[c]) == acc and acc > 1 << 32


@pytest.mark.parametrize("w", R.WIDTHS)
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_group_operations_are_the_naive_loops(dtype, w):
    mask = (1 << (np.dtype(dtype).itemsize * 8)) - 1
    for name, v in R.wave_inputs(dtype, w).items():
        got = {op: R.group_reduce(op, v, w) for op in ("sum", "max", "min", "or", "and")}
        scan = R.group_scan(v, w)
        assert scan.dtype == v.dtype and all(g.dtype == v.dtype for g in got.values())
        for g0 in range(0, v.size, w):
            lanes = [int(x) for x in v[g0:g0 + w]]
            acc, o, a = 0, 0, mask
            for k, x in enumerate(lanes):
                acc = (acc + x) & mask; o |= x; a &= x
                assert int(scan[g0 + k]) == acc, name
            want = {"sum": acc, "max": max(lanes), "min": min(lanes), "or": o, "and": a}
            for op, g in got.items():
                assert g[g0:g0 + w].tolist() == [want[op]] * w, (name, op)


def test_block_references_are_the_naive_loops():
    v = R.wave_inputs(np.uint64, 64)["random"]
    ex, tot = R.block_scan_ref(v)
    o, a = R.block_bits_inputs()
    bits = R.block_bits_ref(o, a)
    for b in range(v.size // 256):
        acc = 0
        for k in range(256):
            assert int(ex[b * 256 + k]) == acc
            acc = (acc + int(v[b * 256 + k])) & 0xffffffffffffffff
        assert tot[b * 256:(b + 1) * 256].tolist() == [acc] * 256
    for b in range(o.size // 256):
        oo, aa = 0, 0xffffffffffffffff
        for k in range(256):
            oo |= int(o[b * 256 + k]); aa &= int(a[b * 256 + k])
        assert (int(bits[2 * b]), int(bits[2 * b + 1])) == (oo, aa)
        assert 0 < oo < 0xffffffffffffffff and 0 < aa < 0xffffffffffffffff      # neither trivial
    for j in range(4):   # the position-revealing blocks: one set bit, one cleared bit
        assert bin(int(bits[2 * (4 + j)])).count("1") == 1 and bin(int(bits[2 * (4 + j) + 1])).count("1") == 63


# ---------------------------------------------------------------------------------------------------------------------
# the inputs fail wrong kernels
# ---------------------------------------------------------------------------------------------------------------------

def _assert_separated(values, bits, ref, bounds, step, what, with_total=True):
    wrong = R.scan_variants(values, bits, bounds, step, OUT_FILL)
    for name, w in wrong.items():
        differs = not np.array_equal(w[0], ref[0]) or (with_total and int(w[1]) != int(ref[1]))
        assert differs, "%s: a scan with %s gives the reference's result" % (what, name)
    return set(wrong)


@pytest.mark.parametrize("n", R.SCAN_SIZES)
def test_scan_inputs_fail_wrong_scans(n):
    """The input sets of one size separate the variants between them, not each on its own.  "random" alone separates every one
    that the size allows.  "ones" separates all but the 32-bit carry, which no input with a total below 2^32 can show.  A
    "single@k" set separates the inclusive scan, the missing out[n] and a carry dropped at any boundary above k; a carry
    dropped at or below k moves nothing, since every sum up to there is zero.  What these sets add is the place: out[i] == i,
    or the step from 0 to 1 behind k, names the misplaced item."""
    u32, u64 = R.scan_inputs_u32(n), R.scan_inputs_u64(n)
    names = set(u32)
    assert {"random", "ones"} <= names and (n == 0 or "single@%d" % (n - 1) in names)
    assert all(("single@%d" % b in names) == (b < n) for b in R.BOUNDARIES)
    for bits in (32, 64):      # u32 -> u32 with its 64-bit total, u32 -> u64
        met = _assert_separated(u32["random"], bits, R.excl_scan(u32["random"], bits), BOUNDS, R.TILE, "u32 -> u%d, n = %d" % (bits, n))
        assert ("32-bit carry" in met) == (n > R.TILE) and ("inclusive" in met) == (n > 0)
        assert all(("carry dropped at " + k in met) == (n > at) for k, at in BOUNDS.items())
    # in place: no total apart from a[n]
    for name, v in u64.items():
        step = R.TILE if name == "random" else n + 1
        met = _assert_separated(v, 64, R.excl_scan(v, 64), BOUNDS, step, "u64 in place, %s, n = %d" % (name, n), with_total=False)
        assert all(("carry dropped at " + k in met) == (n > at) for k, at in BOUNDS.items())
    # the position-revealing inputs (no 32-bit carry: step = n + 1 leaves that variant out)
    for name, v in u32.items():
        if name == "random":
            continue
        ref = R.excl_scan(v, 32)
        at_k = int(name.split("@")[1]) if "@" in name else -1
        above = {k: at for k, at in BOUNDS.items() if at > at_k}
        met = _assert_separated(v, 32, ref, above, n + 1, "u32 -> u32, %s, n = %d" % (name, n))
        assert "32-bit carry" not in met and ("inclusive" in met) == (n > 0) and "out[n] missing" in met
        assert all(("carry dropped at " + k in met) == (n > at) for k, at in above.items())
        assert np.array_equal(ref[0], np.arange(n + 1, dtype=np.uint32)) if name == "ones" else ref[1] == 1


@pytest.mark.parametrize("channels,items,sizes", [(1, 8, R.TOP8_SIZES), (3, 8, R.TOP8_SIZES), (1, 32, R.TOP32_SIZES)])
def test_tile_sum_inputs_fail_wrong_scans(channels, items, sizes):
    per_round = 256 * items
    assert any(s > per_round for s in sizes) and per_round in sizes and per_round + 1 in sizes
    for n_tiles in sizes:
        t = R.top_inputs(n_tiles, channels)
        assert t.max() > 1 << 32 or n_tiles == 1
        out, tot = R.top_rounds_ref(t, channels)
        for c in range(channels):
            ref = (np.append(out[c * n_tiles:(c + 1) * n_tiles], tot[c]), int(tot[c]))
            met = _assert_separated(t[c * n_tiles:(c + 1) * n_tiles], 64, ref, {"a round boundary": per_round}, per_round,
                                    "<%d, %d>, %d tiles, array %d" % (channels, items, n_tiles, c), with_total=False)
            assert ("carry dropped at a round boundary" in met) == ("32-bit carry" in met) == (n_tiles > per_round)
        if channels == 3:
            arrays = out.reshape(3, -1)
            for perm in ([2, 1, 0], [1, 0, 2], [0, 2, 1]):
                assert (n_tiles == 1 or not np.array_equal(arrays[perm], arrays)) and not np.array_equal(tot[perm], tot)


@pytest.mark.parametrize("with_caps", [False, True])
@pytest.mark.parametrize("n", R.SCAN3_SIZES)
def test_three_value_inputs_fail_wrong_scans(n, with_caps):
    """every set at every size, n = 1 included: no channel is all zeros.  From n = 2 on one set separates every variant.  At
    n = 1 there are two (scan3_input_sets says why): each separates all but one, and the two exceptions are checked to be
    the ones that a single alignment forces, and to be separated by the other set."""
    sets = R.scan3_input_sets(n, with_caps)
    assert set(sets) == ({"simple", "general"} if n == 1 else {"random"})
    not_separated = {}
    for name, args in sets.items():
        ref = R.scan3_ref(*args)
        vals = R.scan3_values(*args)
        missed = not_separated.setdefault(name, set())
        for c, bits in enumerate((32, 64, 32)):
            # (a 32-bit carry shows in a 32-bit output's 64-bit total only, once that passes 2^32)
            step = R.TILE if bits == 64 or int(ref[3][c]) >= 1 << 32 else n + 1
            if n == 1 and name == "general" and c == 2:     # the one alignment is not of the simple class: all zeros
                assert _same(R.wrong_inclusive(vals[c], bits), (ref[c], int(ref[3][c])))
                missed.add("inclusive fast_pre")
                continue
            met = _assert_separated(vals[c], bits, (ref[c], int(ref[3][c])), BOUNDS, step, "%s: channel %d, n = %d" % (name, c, n))
            assert ("inclusive" in met) == (n > 0) and "out[n] missing" in met
            assert all(("carry dropped at " + k in met) == (n > at) for k, at in BOUNDS.items())
            assert (c != 1 and n < R.ROUND_ITEMS) or ("32-bit carry" in met) == (n > R.TILE)
        if n:
            assert int(args[0][0]) > 0 and int(ref[1][1]) >= 2 * int(args[0][0])    # matches, and a capacity above 1
            for k, w in enumerate(R.scan3_swapped(ref)):
                differing = sum(not np.array_equal(w[j], ref[j]) for j in range(4))
                if n == 1 and name == "simple" and k == 0:  # one alignment of the simple class: fast_pre is match_off
                    assert differing == 0
                    missed.add("match_off and fast_pre swapped")
                else:
                    assert differing >= 3, (name, k)
        if n > R.ROUND_ITEMS:
            assert all(int(t) >= 1 << 32 for t in ref[3])   # here the 32-bit channels show a 32-bit carry as well
    if n == 1:
        assert not_separated == {"simple": {"match_off and fast_pre swapped"}, "general": {"inclusive fast_pre"}}
    else:
        assert not any(not_separated.values())


def test_the_sizes_reach_every_listed_variant():
    """the tests above apply a variant wherever the size allows it; the sizes allow each of them somewhere"""
    for sizes in (R.SCAN_SIZES, R.SCAN3_SIZES):
        assert all(any(n > at for n in sizes) for at in BOUNDS.values()) and 0 in sizes and 1 in sizes
    assert all(any(b in (n - 1, n) for n in R.SCAN_SIZES) for b in (R.TILE, R.ONE_LAUNCH, R.ROUND_ITEMS))
    assert set(R.ALIGN_SIZES) <= set(R.SCAN_SIZES)


# ---------------------------------------------------------------------------------------------------------------------
# the doubles fail other orders of summation
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", R.WIDTHS)
def test_double_inputs_fail_other_summation_orders(w):
    v = R.wave_doubles(w)
    assert (v > 0).any() and (v < 0).any() and np.abs(v).max() / np.abs(v).min() > 1e12
    down, up, seq = R.butterfly_sum(v, w), R.butterfly_sum(v, w, "up"), R.left_to_right_sum(v, w)
    g = down.reshape(-1, w)
    naive = v.reshape(-1, w).copy()      # the butterfly lane by lane, in Python floats
    for d in [w >> (k + 1) for k in range(w.bit_length() - 1)]:
        naive = np.array([[float(row[i]) + float(row[i ^ d]) for i in range(w)] for row in naive])
    assert np.array_equal(_bits(down), _bits(naive.reshape(-1)))
    assert np.array_equal(_bits(g), _bits(np.repeat(g[:, :1], w, axis=1)))      # every lane holds the same bits
    n_groups = v.size // w
    for name, other in (("d = 1 ... w / 2", up), ("left to right", seq)):
        differing = int((_bits(other).reshape(-1, w)[:, 0] != _bits(g)[:, 0]).sum())
        assert differing >= n_groups // 4, "%s gives the butterfly's bits in all but %d of %d groups" % (name, differing, n_groups)
        assert np.allclose(other, down, rtol=1e-6, atol=1e-6 * np.abs(v).max())   # (the same sum, only rounded otherwise)
