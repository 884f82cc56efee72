"""bench.py --dump-outputs: the rows the timed path returned in its last step, the same from run to run on the same
arguments, and the same rows the host-side packed entry point gives for that batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_dump(out_dir, warmup):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--pairs", "20000", "--steps", "3", "--warmup",
                        str(warmup), "--no-cpu-baseline", "--no-pcie", "--dump-outputs", str(out_dir)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    files = sorted(os.listdir(out_dir))
    out = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files if f.endswith(".npy")}
    assert len(out) == len(files)
    assert all(v.dtype == np.float64 for v in out.values())
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 << 20
    return out


@pytest.mark.gpu
def test_bench_dumps_the_rows_of_its_last_step(tmp_path):
    from bramble_amd import lib, synth
    first = _bench_dump(tmp_path / "a", 0)
    again = _bench_dump(tmp_path / "b", 2)
    assert sorted(first) == sorted(again)
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    # the batch bench.py projects at rank 0, through the host-side packed entry point
    ann = synth.Annotation("G")
    batch = ann.reads(20000, "pe", seed=synth.SEED ^ 0x51ED)
    idx = lib.Index.from_flat(ann.flat, device=0)
    ctx = lib.Context(idx)
    ctx.set_param("host_detail", 1)
    p = ctx.project_batch_packed(lib.make_config(), batch)
    w = lib.unpack_host_rows(p, batch["l_qseq"])
    ctx.close()
    idx.close()
    n = p["n_rows"]
    assert 0 < n <= 1 << 19   # small enough for the dump to hold every row and every alignment
    assert np.array_equal(first["counts"][:2], [p["n_aln"], n])
    assert np.array_equal(first["row_index"], np.arange(n))
    assert np.array_equal(first["rows_a"], p["a"].astype(np.float64))
    assert np.array_equal(first["cigar_off"], w["cigar_off"].astype(np.float64))
    assert np.array_equal(first["cigar_ops"], w["cigar"].astype(np.float64))
    assert np.array_equal(first["aln_index"], np.arange(p["n_aln"] + 1))
    assert np.array_equal(first["row_off"], p["row_off"].astype(np.float64))


def _bench_line(extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--pairs", "20000", "--steps", "2", "--warmup", "1"]
                       + extra, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_line_is_the_headline_and_full_adds_the_other_legs():
    plain = _bench_line([])
    full = _bench_line(["--full", "--cpu-sample", "1000"])
    for d in (plain, full):
        assert d["unit"] == "alignments/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert abs(d["value"] - d["per_rank_alignments_per_step"][0] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
        assert d["kernel_ms_per_step"]
    assert plain["metric"] == full["metric"]
    assert plain["projected_records_per_step"] == full["projected_records_per_step"] > 0
    assert not {"pcie_inclusive", "roofline", "cpu_baseline"} & set(plain)
    assert full["pcie_inclusive"]["value"] > 0
    assert 0 < full["roofline"]["frac"] <= 1 and full["roofline"]["per_kernel"]
    assert full["cpu_baseline"]["value"] > 0
