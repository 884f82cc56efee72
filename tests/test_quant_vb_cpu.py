"""--quant-vb without a GPU: the restatement of the variational Bayes EM (quant_vb_cases.py) against cases worked out by hand and
against the plain EM; that it is stable -- its six-run spread small -- on every input and parameter set the GPU tests compare the
device with; the ABI without a device; the command line's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import quant_vb_cases as Q
from tests.test_quant_cpu import em_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_psi_series_against_torch():
    g = Q.psi_grid()
    d0 = Q.psi_figure(Q.psi_series(g), Q.psi_torch(g))
    print("the series restatement against torch.special.digamma (float64): worst figure %.3e" % d0)
    assert g.min() == 1e-10 and g.max() == 1e9 and 0 < d0 < 1e-14
    assert abs(Q.psi_series([1.0])[0] + 0.5772156649015329) < 1e-15      # -gamma
    assert abs(Q.psi_series([1.4616321449683623])[0]) < 1e-15             # the root


@pytest.mark.parametrize("prior", [0.0, 1e-2, 1.0, 50.0])
@pytest.mark.parametrize("a,b", [(30, 10), (1, 1000), (7, 7)])
def test_two_transcripts_without_shared_names(a, b, prior):
    # {0}: a, {1}: b, {0, 1}: 0 -- nothing is shared, so alpha = (a, b) whatever the prior
    cl = {"labels": [(0,), (1,), (0, 1)], "counts": [a, b, 0]}
    for psi in (Q.psi_torch, Q.psi_series):
        r = Q.vb_reference(cl, 2, length_norm=False, prior=prior, max_iters=50, tolerance=0, psi=psi)
        assert np.allclose(r["theta"], [a, b], rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", Q.VALUE_CASES, ids=lambda c: "%s-norm%d-prior%g-nt%d" % c)
def test_alpha_keeps_the_names(case):
    which, length_norm, prior, per_nt = case
    tb, cl = getattr(Q, which)(), Q.classes(which)
    n = cl["n_names"] - cl["n_unassigned"]
    sums = []
    Q.vb_reference(cl, tb["n_tx"], tb["lens"], bool(length_norm), prior, bool(per_nt), max_iters=60, tolerance=0, sums=sums)
    assert len(sums) == 60 and all(abs(v - n) <= 1e-9 * n for v in sums)


def test_the_feature_is_observable():
    tb, cl = Q.builder(), Q.classes("builder")
    em = em_reference(cl, tb["n_tx"], tb["lens"], True, max_iters=Q.VALUE_ITERS, tolerance=0)
    vb, _ = Q.spread_of("builder", 1, 1e-2, 0)
    big = Q.vb_reference(cl, tb["n_tx"], tb["lens"], True, prior=1.0, max_iters=Q.VALUE_ITERS, tolerance=0)
    zero = lambda r: int((r["theta"] <= 1e-8).sum())
    diff = float(np.max(np.abs(vb["theta"] - em["theta"])))
    print("at zero: EM %d, VB 1e-2 %d, VB 1.0 %d; max |alpha_vb - theta_em| = %.3f" % (zero(em), zero(vb), zero(big), diff))
    assert zero(big) == 0 and zero(vb) >= zero(em) and diff > 1


@pytest.mark.parametrize("case", Q.VALUE_CASES, ids=lambda c: "%s-norm%d-prior%g-nt%d" % c)
def test_the_restatement_is_stable_where_the_device_is_compared(case):
    _, s = Q.spread_of(*case)
    print("%s: spread over {forward, reversed, shuffled} x {torch psi, series psi} after %d iterations = %.3e" % (case, Q.VALUE_ITERS, s))
    assert 0 < s < 1e-9


def test_the_restatement_stops_at_one_iteration():
    which, length_norm, prior, per_nt = Q.STOP_CASE
    tb, cl = Q.builder(), Q.classes(which)
    runs = [Q.vb_reference(cl, tb["n_tx"], tb["lens"], bool(length_norm), prior, bool(per_nt), order=o, psi=f)
            for f in (Q.psi_torch, Q.psi_series) for o in ("forward", 12345)]
    print("stops after", [r["n_iters"] for r in runs], "at", ["%.3e" % r["rel_change"] for r in runs])
    assert len(set(r["n_iters"] for r in runs)) == 1 and runs[0]["n_iters"] % 16 == 0 and runs[0]["n_iters"] < 10000
    assert all(r["rel_change"] < 0.8e-2 for r in runs)   # not near the tolerance: an ulp does not move the stop


def test_replicates_are_stable_under_the_seed():
    sp = Q.boot_spreads()
    print("replicate spreads:", ["%.2e" % s for _, s in sp])
    assert len(sp) == Q.BOOT_B == 7 and sum(1 for _, s in sp if not 0 < s < 1e-9) <= 1


def test_posteriors_of_by_hand():
    cl = {"labels": [(0,), (0, 2), (1,)], "counts": [1, 1, 1]}
    assert Q.posteriors_of(cl, np.asarray([1.0, 0.0, 3.0])).tolist() == [1.0, 0.25, 0.75, 0.0]


# ---- ABI and usage errors -------------------------------------------------------------------------------------------------------
def test_vb_abi_without_a_device():
    from bramble_amd import lib
    L = lib.lib()
    for name in ("br_quant_set_vb_prior", "br_quant_digamma"):
        assert hasattr(L, name), name
    L.br_quant_set_vb_prior.argtypes = [C.c_void_p, C.c_double]
    L.br_quant_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.br_quant_digamma.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    assert L.br_quant_set_vb_prior(None, 0.5) == -1           # BR_ERR_INVALID_ARG
    assert L.br_quant_set_param(None, b"vb", 1) == -1 and L.br_quant_set_param(None, b"vb_per_nucleotide", 1) == -1
    a, out = np.asarray([1.0, 2.0]), np.zeros(2)
    assert L.br_quant_digamma(4096, a.ctypes.data, 2, out.ctypes.data) == -2   # BR_ERR_NO_DEVICE
    assert L.br_quant_digamma(-1, a.ctypes.data, 2, out.ctypes.data) == -2
    assert L.br_quant_digamma(0, None, 2, out.ctypes.data) == -1 and L.br_quant_digamma(0, a.ctypes.data, -1, out.ctypes.data) == -1
    assert not out.any()
    assert "vb_per_nucleotide" in lib.Quant.__init__.__code__.co_varnames and callable(lib.quant_digamma)


@pytest.mark.parametrize("extra,word", [
    (["--quant-vb"], b"--quant"),
    (["--quant-vb-prior", "0.1"], b"--quant"),
    (["--quant", "q.tsv", "--quant-vb-prior", "0.1"], b"--quant-vb"),
    (["--quant", "q.tsv", "--quant-vb-per-nucleotide"], b"--quant-vb"),
    (["--quant", "q.tsv", "--quant-vb", "--quant-vb-prior", "-1"], b"--quant-vb-prior"),
    (["--quant", "q.tsv", "--quant-vb", "--quant-vb-prior", "nan"], b"--quant-vb-prior"),
    (["--quant", "q.tsv", "--quant-vb", "--quant-vb-prior", "inf"], b"--quant-vb-prior"),
    (["--quant", "q.tsv", "--quant-vb", "--quant-vb-prior", "1e-2x"], b"--quant-vb-prior"),
    (["--quant", "q.tsv", "--quant-vb", "--quant-vb-prior"], b"usage:"),
    (["--quant", "q.tsv", "--quant-vb", "--quant-vb-per-nucleotide", "--lr"], b"length normalisation"),
    (["--quant", "q.tsv", "--quant-vb", "--quant-vb-per-nucleotide", "--quant-no-length-norm"], b"length normalisation"),
])
def test_cli_vb_usage_errors(tmp_path, extra, word):
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    out = str(tmp_path / "o.bam")
    extra = [str(tmp_path / e) if e.endswith(".tsv") else e for e in extra]
    r = subprocess.run([os.path.join(ROOT, "bramble_amd", "bin", "bramble"), str(tmp_path / "missing.bam"), "-G", str(gtf), "-o", out] + extra,
                       capture_output=True, timeout=60)
    assert r.returncode == 2
    assert word in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]
