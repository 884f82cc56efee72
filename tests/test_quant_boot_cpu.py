"""--quant-bootstraps without a GPU: the tests' own restatement of the bootstrap definitions in bramble_amd.h (br_quant) --
Philox4x32-10, the draw, the resampled class counts, the summary -- which the GPU tests compare the device against (a replicate's
EM is em_reference of test_quant_cpu.py on the resampled counts); the known answers of the generator; cases worked out by hand;
properties; a statistical sanity check of the restatement on fixed seeds; the ABI without a device and the usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_quant_cpu import em_reference

M32 = np.uint64(0xffffffff)
S32 = np.uint64(32)


# ---- the yardsticks -----------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (or numbers) that hold 32-bit words, key: two 32-bit numbers -> the four output words (uint64 arrays)"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32 for v in ctr]
    k0, k1 = np.uint64(key[0] & 0xffffffff), np.uint64(key[1] & 0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]   # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & M32, (p0 >> S32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def mulhi64(u, n):
    """floor(u n / 2^64) for uint64 arrays u and a number n < 2^32, in uint64 arithmetic: with u = h 2^32 + l, h n + (l n >> 32)
    is below 2^64 and its high half is the answer"""
    assert 0 <= n < (1 << 32)
    n = np.uint64(n)
    return ((u >> S32) * n + (((u & M32) * n) >> S32)) >> S32


def draw_ranks(n, seed, b):
    """the name ranks of replicate b's n draws"""
    seed &= 0xffffffffffffffff
    i = np.arange(n, dtype=np.uint64)
    w = philox4x32_10((i & M32, i >> S32, np.full(n, b, dtype=np.uint64), np.zeros(n, dtype=np.uint64)), (seed & 0xffffffff, seed >> 32))
    return mulhi64(w[0] | (w[1] << S32), n)


def class_of_rank(counts, r):
    """the class c with cum[c] <= r < cum[c + 1], cum the exclusive prefix sums of the counts"""
    cum = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)
    return np.searchsorted(cum, np.asarray(r, dtype=np.uint64), side="right") - 1


def boot_counts(counts, seed, b):
    """n_c^(b): uint32 per class"""
    counts = np.asarray(counts, dtype=np.uint64)
    n = int(counts.sum())
    if n == 0:
        return np.zeros(len(counts), dtype=np.uint32)
    return np.bincount(class_of_rank(counts, draw_ranks(n, seed, b)), minlength=len(counts)).astype(np.uint32)


def boot_em(cl, n_tx, counts_b, lens=None, length_norm=True, **kw):
    """a replicate's EM: em_reference with the counts replaced"""
    return em_reference(dict(cl, counts=[int(v) for v in counts_b]), n_tx, lens, length_norm, **kw)


def boot_summary(theta):
    """theta: [B, T] -> (mean, var), both sums one replicate after the other"""
    n_boot, n_tx = theta.shape
    s = np.zeros(n_tx, dtype=np.float64)
    for b in range(n_boot):
        s = s + theta[b]
    mean = s / np.float64(n_boot)
    v = np.zeros(n_tx, dtype=np.float64)
    for b in range(n_boot):
        d = theta[b] - mean
        v = v + d * d
    return mean, (v / np.float64(n_boot - 1) if n_boot > 1 else np.zeros(n_tx, dtype=np.float64))


# ---- the generator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(w[0]) for w in philox4x32_10(ctr, key)) == out


def test_multiply_high_against_big_integers():
    rng = np.random.RandomState(11)
    u = (rng.randint(0, 1 << 32, size=500).astype(np.uint64) << S32) | rng.randint(0, 1 << 32, size=500).astype(np.uint64)
    u[:3] = [0, 0xffffffffffffffff, 1 << 63]
    for n in (1, 2, 3016, (1 << 20) + 1, (1 << 32) - 1):
        assert [int(v) for v in mulhi64(u, n)] == [(int(v) * n) >> 64 for v in u]
    seed = (1 << 63) + 5
    w = philox4x32_10((7, 0, 3, 0), (seed & 0xffffffff, seed >> 32))
    assert int(draw_ranks(100, seed, 3)[7]) == ((int(w[0][0]) | int(w[1][0]) << 32) * 100) >> 64


# ---- cases worked out by hand -----------------------------------------------------------------------------------------------------
def test_one_class():
    for b in range(4):
        assert boot_counts([7], 0, b).tolist() == [7]


def test_a_draw_on_each_side_of_a_boundary():
    counts = [3, 2, 4]   # cum = 0, 3, 5, 9
    assert class_of_rank(counts, [0, 2, 3, 4, 5, 8]).tolist() == [0, 0, 1, 1, 2, 2]
    assert class_of_rank([3, 0, 4], [2, 3]).tolist() == [0, 2]   # an empty class takes no draw


def test_a_small_class_beside_a_large_one():
    counts = [1, 1 << 20]
    n = sum(counts)
    for b in range(3):
        r = draw_ranks(n, 5, b)
        got = boot_counts(counts, 5, b)
        assert int(r.max()) < n
        assert got.tolist() == [int((r == 0).sum()), int((r > 0).sum())] and int(got.sum()) == n
    assert any(int(boot_counts(counts, 5, b)[0]) != 1 for b in range(8))   # (the rare class is resampled too)


def test_no_names():
    assert boot_counts([], 1, 0).tolist() == [] and boot_counts([0, 0], 1, 0).tolist() == [0, 0]
    mean, var = boot_summary(np.zeros((3, 4)))
    assert not mean.any() and not var.any()


def test_summary_by_hand():
    theta = np.asarray([[1.0, 10.0], [2.0, 10.0], [6.0, 10.0]])
    mean, var = boot_summary(theta)
    assert mean.tolist() == [3.0, 10.0] and var.tolist() == [7.0, 0.0]
    mean, var = boot_summary(theta[:1])
    assert mean.tolist() == [1.0, 10.0] and var.tolist() == [0.0, 0.0]


# ---- properties -----------------------------------------------------------------------------------------------------------------
def test_properties():
    counts = np.random.RandomState(2).randint(1, 9, size=300)
    n = int(counts.sum())
    reps = [boot_counts(counts, 77, b) for b in range(5)]
    assert all(int(r.sum()) == n and r.dtype == np.uint32 for r in reps)
    assert all(not np.array_equal(reps[a], reps[b]) for a in range(5) for b in range(a + 1, 5))
    assert all(np.array_equal(boot_counts(counts, 77, b), reps[b]) for b in range(5))
    assert not np.array_equal(boot_counts(counts, 78, 0), reps[0])
    assert np.array_equal(boot_counts(counts, -1, 1), boot_counts(counts, (1 << 64) - 1, 1))   # the int64's bits are the seed


def test_replicate_em_is_the_point_em_on_resampled_counts():
    cl = {"labels": [(0,), (1,), (0, 1)], "counts": [30, 10, 60]}
    nb = boot_counts(cl["counts"], 3, 0)
    r = boot_em(cl, 2, nb, length_norm=False, max_iters=64, tolerance=0)
    assert abs(float(r["theta"].sum()) - 100.0) < 1e-9
    nb = np.asarray([5, 0, 0], dtype=np.uint32)   # a class the resampling left empty contributes nothing
    r = boot_em(cl, 2, nb, length_norm=False, max_iters=3, tolerance=0)
    assert r["theta"].tolist() == [5.0, 0.0]


# ---- statistical sanity of the restatement, on fixed seeds ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 12345, (1 << 63) + 5])
def test_resampling_is_multinomial(seed):
    counts = np.random.default_rng(1).integers(1, 5, 1204)
    n = int(counts.sum())
    assert n == 3016
    reps = np.asarray([boot_counts(counts, seed, b) for b in range(200)], dtype=np.float64)
    p = counts / n
    z = (reps.mean(axis=0) - n * p) / np.sqrt(n * p * (1 - p) / 200)
    ratio = float(np.mean(reps.var(axis=0, ddof=1) / (n * p * (1 - p))))
    print("seed %d: largest |z| of a class's replicate mean %.2f, mean ratio of sample variance to N p (1 - p) %.3f" % (seed, np.abs(z).max(), ratio))
    assert float(np.abs(z).max()) < 5
    assert 0.97 <= ratio <= 1.03


# ---- ABI and usage errors -------------------------------------------------------------------------------------------------------
def test_boot_abi_without_a_device():
    from bramble_amd import lib
    L = lib.lib()
    names = ("br_quant_bootstrap", "br_quant_boot_counts", "br_quant_boot_theta", "br_quant_boot_summary", "br_quant_boot_stats")
    for name in names:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    L.br_quant_bootstrap.argtypes = [C.c_void_p, C.c_void_p]
    L.br_quant_boot_counts.argtypes = L.br_quant_boot_theta.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.br_quant_boot_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.br_quant_boot_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.br_quant_bootstrap(None, None) == -1
    assert L.br_quant_boot_counts(None, 0, 0, None) == -1 and L.br_quant_boot_theta(None, 0, 0, None) == -1
    assert L.br_quant_boot_summary(None, None, None) == -1 and L.br_quant_boot_stats(None, None, None, None) == -1
    L.br_quant_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    assert L.br_quant_set_param(None, b"bootstraps", 4) == -1


@pytest.mark.parametrize("extra,word", [
    (["--quant-bootstraps", "4"], b"--quant"),
    (["--quant-seed", "7"], b"--quant"),
    (["--quant-boot-out", "b.tsv"], b"--quant"),
    (["--quant", "q.tsv", "--quant-boot-out", "b.tsv"], b"--quant-bootstraps"),
    (["--quant", "q.tsv", "--quant-bootstraps", "0"], b"--quant-bootstraps"),
    (["--quant", "q.tsv", "--quant-bootstraps", "10001"], b"--quant-bootstraps"),
    (["--quant", "q.tsv", "--quant-bootstraps", "many"], b"--quant-bootstraps"),
])
def test_cli_boot_usage_errors(tmp_path, extra, word):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    out = str(tmp_path / "o.bam")
    extra = [str(tmp_path / e) if e.endswith((".txt", ".tsv")) else e for e in extra]
    r = subprocess.run([os.path.join(root, "bramble_amd", "bin", "bramble"), str(tmp_path / "missing.bam"), "-G", str(gtf), "-o", out] + extra,
                       capture_output=True, timeout=60)
    assert r.returncode == 2
    assert word in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]
