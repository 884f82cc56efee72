"""--coverage-bigwig without a GPU: the tests' reader (bigwig_ref.py) against the tests' writer (bigwig_cases.py), both pinned by a
file assembled by hand; what the inputs of the GPU tests hold; the host's pieces of the product (host/bigwig_file.cpp) built with a
probe of their own under the address and undefined-behaviour sanitizers, against the writer; the new ABI without a device; the
command line's usage errors."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bigwig_cases as bc
from tests import bigwig_ref as br
from tests.test_coverage_cpu import coverage_of
from tests.test_quant_fld_cpu import rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {"compress": -1, "items_per_slot": 4, "block_size": 4, "first_reduction": 32, "zoom_levels": 4}


def hand_built():
    _, cov, lens = bc.hand_built()
    return cov, lens


# ---- a file assembled by hand ---------------------------------------------------------------------------------------------------
def test_a_file_assembled_by_hand():
    """Transcripts "b" (10 bases: depth 1 on [2, 5), 3 on [5, 6)) and "a" (8 bases: depth 2 on [0, 8)); S = 2, blockSize 2, one zoom
    level of 4 bases, uncompressed.  "a" is chromosome 0.  642 bytes, every one of them written out here."""
    f32 = lambda *v: struct.pack("<%df" % len(v), *v)   # noqa: E731
    want = b"".join([
        struct.pack("<IHHQQQHHQQIQ", 0x888FFC26, 4, 1, 128, 182, 274, 0, 0, 0, 88, 0, 0),          # header
        struct.pack("<IIQQ", 4, 0, 390, 522),                                                      # zoom header
        struct.pack("<Qdddd", 12, 1.0, 3.0, 22.0, 44.0),                                           # total summary: 8 + 3 + 1 bases
        struct.pack("<IIIIQQ", 0x78CA8C91, 2, 1, 8, 2, 0), b"\x01\x00\x02\x00", b"a", struct.pack("<II", 0, 8), b"b", struct.pack("<II", 1, 10),
        struct.pack("<Q", 2),                                                                      # full data at 182
        struct.pack("<IIIIIBBH", 0, 0, 8, 0, 0, 1, 0, 1), struct.pack("<II", 0, 8), f32(2.0),
        struct.pack("<IIIIIBBH", 1, 2, 6, 0, 0, 1, 0, 2), struct.pack("<II", 2, 5), f32(1.0), struct.pack("<II", 5, 6), f32(3.0),
        struct.pack("<IIQIIIIQII", 0x2468ACE0, 2, 2, 0, 0, 1, 6, 274, 1, 0), b"\x01\x00\x02\x00",  # full index at 274
        struct.pack("<IIIIQQ", 0, 0, 0, 8, 190, 36), struct.pack("<IIIIQQ", 1, 2, 1, 6, 226, 48),
        struct.pack("<I", 4),                                                                      # zoom data at 390
        struct.pack("<IIII", 0, 0, 4, 4), f32(2, 2, 8, 16), struct.pack("<IIII", 0, 4, 8, 4), f32(2, 2, 8, 16),
        struct.pack("<IIII", 1, 0, 4, 2), f32(1, 1, 2, 2), struct.pack("<IIII", 1, 4, 8, 2), f32(1, 3, 4, 10),
        struct.pack("<IIQIIIIQII", 0x2468ACE0, 2, 2, 0, 0, 1, 8, 522, 1, 0), b"\x01\x00\x02\x00",  # zoom index at 522
        struct.pack("<IIIIQQ", 0, 0, 0, 8, 394, 64), struct.pack("<IIIIQQ", 1, 0, 1, 8, 458, 64),
        struct.pack("<I", 0x888FFC26)])
    assert len(want) == 642
    lens = np.asarray([10, 8], dtype=np.int64)
    cov = coverage_of(rows_of([(0, 2, 0, "4M"), (0, 5, 0, "1M"), (0, 5, 0, "1M"), (1, 0, 0, "8M"), (1, 0, 0, "8M")]), lens)
    got, _ = bc.write_bigwig(cov, lens, ["b", "a"], compress=-1, items_per_slot=2, block_size=2, zoom_levels=1, first_reduction=4)
    assert got == want
    r = br.read_all(want, option_bs=2, items_per_slot=2)
    assert r["chroms"] == [(b"a", 0, 8), (b"b", 1, 10)] and not r["compressed"]
    assert [(c, s, e, [tuple(i) for i in it.tolist()]) for c, s, e, it in r["sections"]] == [(0, 0, 8, [(0, 8, 2.0)]), (1, 2, 6, [(2, 5, 1.0), (5, 6, 3.0)])]
    assert r["zooms"][0]["records"].tolist() == [(0, 0, 4, 4, 2, 2, 8, 16), (0, 4, 8, 4, 2, 2, 8, 16), (1, 0, 4, 2, 1, 1, 2, 2), (1, 4, 8, 2, 1, 3, 4, 10)]
    assert r["header"]["summary"] == {"valid": 12, "min": 1.0, "max": 3.0, "sum": 22.0, "sumsq": 44.0}
    assert br.intervals(want, 1, 4, 6) == [(2, 5, 1.0), (5, 6, 3.0)] and br.intervals(want, 0, 8, 9) == [] and br.intervals(want, 1, 0, 2) == []


def test_rounding_to_float32_by_hand():
    assert bc.f32_exact(2 ** 24 + 1, 0) == np.float32(2 ** 24) and bc.f32_exact(2 ** 24 + 3, 0) == np.float32(2 ** 24 + 4)   # ties to even
    assert bc.f32_exact(2 ** 25 - 1, 0) == np.float32(2 ** 25) and bc.f32_exact(3 << 40, 41) == np.float32(1.5)
    assert bc.f32_exact(10 ** 10 * 12, 0) == np.float32(1.2e11) and bc.f32_exact(0, 64) == 0
    assert bc.value_of(1431655765, True) == np.float32(1 / 3) and bc.value_of(100000, False) == np.float32(100000)
    assert bc.ulp_apart(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1


# ---- the reader reads what the writer wrote ------------------------------------------------------------------------------------------
def _assert_same_content(a, b):
    """two read_all results hold the same track: everything but the places and sizes of the compressed streams"""
    assert a["chroms"] == b["chroms"] and a["chrom_tree"] == b["chrom_tree"]
    assert {k: a["header"][k] for k in ("zoom_levels", "uncompress_buf", "summary")} == {k: b["header"][k] for k in ("zoom_levels", "uncompress_buf", "summary")}
    strip = lambda t: {k: t[k] for k in ("block_size", "n", "lo", "hi")}   # noqa: E731
    assert strip(a["full_index"]) == strip(b["full_index"]) and len(a["sections"]) == len(b["sections"])
    for x, y in zip(a["sections"], b["sections"]):
        assert x[:3] == y[:3] and x[3].tobytes() == y[3].tobytes()
    assert len(a["zooms"]) == len(b["zooms"])
    for x, y in zip(a["zooms"], b["zooms"]):
        assert x["reduction"] == y["reduction"] and strip(x["index"]) == strip(y["index"]) and x["block_sizes"] == y["block_sizes"]
        assert x["records"].tobytes() == y["records"].tobytes()


def _assert_track(r, cov, names, lens, wide=False):
    """a read_all result holds the runs of cov, name for name"""
    order = bc.chromosomes(cov["runs"], names)
    assert [(n.decode(), s) for n, _, s in r["chroms"]] == [(names[t], int(lens[t])) for t in order]
    got = sorted((order[c], int(i["start"]), int(i["end"]), float(i["value"])) for c, _, _, items in r["sections"] for i in items)
    assert got == [(int(t), int(s), int(e), float(bc.value_of(d, wide))) for t, s, e, d in zip(*cov["runs"])]


def test_names_case_holds_what_it_is_meant_to_hold():
    cov, lens = hand_built()
    names = bc.NAMES_CASE
    order = bc.chromosomes(cov["runs"], names)
    with_runs = sorted(order)
    assert [names[t] for t in order] == ["A", "T2", "t1", "t10", "t1a", "t2", "t" * 40, "x"] and order != with_runs   # byte order, not @SQ order
    assert {1, 40} <= {len(names[t]) for t in order} and len(names) == len(lens) == len(set(names))
    assert any(a < t < b for t in set(range(len(lens))) - set(order) for a in order for b in order)   # one without runs between two with


@pytest.mark.parametrize("opts", [SMALL, {"block_size": 4}, {"block_size": 2, "items_per_slot": 1, "zoom_levels": -1}, {"zoom_levels": 10, "compress": -1}])
def test_reader_reads_the_writer_hand_built(opts):
    cov, lens = hand_built()
    data, _ = bc.write_bigwig(cov, lens, bc.NAMES_CASE, **opts)
    o = dict(bc.DEFAULTS, **opts)
    r = br.read_all(data, option_bs=o["block_size"], items_per_slot=o["items_per_slot"])
    _assert_track(r, cov, bc.NAMES_CASE, lens)
    assert len(r["zooms"]) == max(o["zoom_levels"], 0) and r["compressed"] == (o["compress"] >= 0)
    if opts is SMALL:   # at least three levels in the full index, partial last sections, windows and nodes
        bs, items = br.levels_of(len(r["sections"]), 4)
        assert len(items) >= 3 and items[0] % 4 and any(len(s[3]) < 4 for s in r["sections"]) and int(lens[7]) % 32
    plain, _ = bc.write_bigwig(cov, lens, bc.NAMES_CASE, **dict(opts, compress=-1))
    packed, _ = bc.write_bigwig(cov, lens, bc.NAMES_CASE, **dict(opts, compress=1))
    ra, rb = br.read_all(plain), br.read_all(packed)
    assert ra["header"]["uncompress_buf"] == 0 and rb["header"]["uncompress_buf"] == max(24 + 12 * o["items_per_slot"], 32 * o["items_per_slot"])
    ra["header"]["uncompress_buf"] = rb["header"]["uncompress_buf"]
    _assert_same_content(ra, rb)
    # queries through the R-tree against brute force over the runs
    rng = np.random.RandomState(3)
    order = bc.chromosomes(cov["runs"], bc.NAMES_CASE)
    for _ in range(20):
        c = int(rng.randint(len(order)))
        s = int(rng.randint(max(int(lens[order[c]]), 1)))
        e = s + 1 + int(rng.randint(200))
        want = [(int(a), int(b), float(np.float32(d))) for t, a, b, d in zip(*cov["runs"]) if t == order[c] and a < e and b > s]
        assert br.intervals(data, c, s, e) == want


def test_sums_of_the_byte_equality_inputs_are_exact():
    """Byte equality needs every zoom sum to round once.  The device sums doubles: exact below 2^53, which every sum here is; and all
    but the windows on the depth-100 000 spot (transcript "t2") are below 2^24, exact in float32 as well."""
    from tests.test_gpu_coverage import T_BULK
    cov, lens = hand_built()
    order = bc.chromosomes(cov["runs"], bc.NAMES_CASE)
    for k in range(4):
        rec, exact = bc.zoom_records(cov["depth"], lens, order, 32 * 4 ** k, False)
        big = [i for i, (s1, s2) in enumerate(exact) if s2 >= 2 ** 24]
        assert all(s2 < 2 ** 53 for _, s2 in exact) and big and all(order[int(rec["chrom"][i])] == T_BULK for i in big)
    for case in (bc.boundary_case(1025, False)[2], bc.zoom_edge_case()[1]):
        assert sum(int(x) ** 2 for d in case["depth"] for x in d) < 2 ** 24


@pytest.mark.parametrize("n_runs", [1024, 1025, 2049])
@pytest.mark.parametrize("random_depth", [False, True])
def test_reader_reads_the_writer_section_boundaries(n_runs, random_depth):
    _, _, cov, lens, wide = bc.boundary_case(n_runs, random_depth)
    assert len(cov["runs"][0]) == n_runs
    data, _ = bc.write_bigwig(cov, lens, ["one"], wide=wide)
    r = br.read_all(data, option_bs=256, items_per_slot=1024)
    assert [len(s[3]) for s in r["sections"]] == [1024] * (n_runs // 1024) + ([n_runs % 1024] if n_runs % 1024 else [])
    _assert_track(r, cov, ["one"], lens, wide)


def test_reader_reads_the_writer_zoom_edges():
    (_, cov, lens), names = bc.zoom_edge_case(), bc.ZOOM_EDGE_NAMES
    for levels in (-1, 4, 10):
        data, _ = bc.write_bigwig(cov, lens, names, zoom_levels=levels, compress=-1)
        r = br.read_all(data)
        assert len(r["zooms"]) == max(levels, 0)
        _assert_track(r, cov, names, lens)
    z = r["zooms"]
    ids = {n: i for i, n in enumerate(sorted(names))}
    assert z[9]["reduction"] == 8388608 and [tuple(x)[:4] for x in z[9]["records"].tolist()] == sorted(
        [(ids["len31"], 0, 31, 1), (ids["len32"], 0, 32, 3), (ids["len33"], 0, 33, 4), (ids["len2049"], 0, 2049, 42), (ids["len5"], 0, 5, 3)])
    lvl0 = [tuple(x)[:4] for x in z[0]["records"].tolist()]
    assert (ids["len31"], 0, 31, 1) in lvl0 and (ids["len32"], 0, 32, 3) in lvl0 and (ids["len33"], 32, 33, 1) in lvl0   # the last base alone
    assert (ids["len2049"], 2048, 2049, 1) in lvl0 and (ids["len2049"], 96, 128, 1) in lvl0 and (ids["len5"], 0, 5, 3) in lvl0
    assert [x[1] for x in lvl0 if x[0] == ids["len2049"]] == [96, 576, 608, 2048]   # windows without coverage are absent


# ---- the host's pieces of the product -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bwprobe") / "probe")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "bigwig_file_probe.cpp"), os.path.join(ROOT, "bramble_amd", "csrc", "host", "bigwig_file.cpp")],
                   check=True, timeout=300)
    return exe


def _probe(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()
    return r.stdout.decode()


@pytest.mark.parametrize("bs", [2, 4])
def test_chromosome_trees_against_the_writer(probe, bs):
    for n in (0, 1, bs, bs + 1, bs * bs + 1):
        enc = [b"c%06d" % i for i in range(n)]
        ks = 7 if n else 0
        hbs, nodes = bc._tree(n, bs, ks + 8, ks + 8, lambda i: enc[i] + struct.pack("<II", i, 100 + i),
                              lambda l, i, child: enc[i * min(bs, max(n, 1)) ** l] + struct.pack("<Q", child), 1000 + 32)
        want = struct.pack("<IIIIQQ", br.CHROM_MAGIC, hbs, ks, 8, n, 0) + nodes
        got = bytes.fromhex(_probe(probe, "tree", bs, n, 1000).strip())
        assert got == want, (bs, n)
        head, chroms, behind = br.chrom_tree(b"\0" * 1000 + got, 1000, bs)
        assert chroms == [(enc[i], i, 100 + i) for i in range(n)] and behind == 1000 + len(got)
        shape = [int(v) for v in _probe(probe, "shape", bs, n).split()]
        assert shape[0] == hbs and shape[1:-1] == br.levels_of(n, bs)[1]
    assert len(br.levels_of(bs * bs + 1, bs)[1]) == 3


def test_name_order_and_refusals(probe):
    assert _probe(probe, "order", "t1a", "t10", "t1", "T2", "x", "t" * 40).split() == ["40", "T2", "t1", "t10", "t1a", "t" * 40, "x"]
    assert _probe(probe, "order").split() == ["0"]
    for bad in (["a", "-"], ["!", "a"], ["b", "a", "b"], ["a", "a"]):
        assert _probe(probe, "order", *bad).startswith("refused: "), bad


def test_headers_against_the_layout(probe):
    head, rt = [bytes.fromhex(l) for l in _probe(probe, "head").split()]
    assert head == struct.pack("<IHHQQQHHQQIQ", br.BIGWIG_MAGIC, 4, 2, 152, 300, 900, 0, 0, 0, 112, 32768, 0) + struct.pack("<IIQQ", 32, 0, 1000, 2000) + \
        struct.pack("<IIQQ", 128, 0, 3000, 2 ** 33) + struct.pack("<Qdddd", 12, 1.0, 3.0, 22.0, 44.0)
    assert rt == struct.pack("<IIQIIIIQII", br.RTREE_MAGIC, 4, 9, 2, 7, 5, 11, 2 ** 32, 1, 0)


# ---- ABI and usage errors ---------------------------------------------------------------------------------------------------------
SYMBOLS = ("br_coverage_bigwig", "br_coverage_bigwig_read", "br_coverage_bigwig_stats", "br_zlib_sections_device")


def test_new_symbols_without_a_device():
    from bramble_amd import lib
    L = lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    L.br_coverage_bigwig.argtypes = [C.c_void_p] * 4
    L.br_coverage_bigwig_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.br_coverage_bigwig_stats.argtypes = [C.c_void_p] * 9
    L.br_zlib_sections_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    n = C.c_uint64()
    assert L.br_coverage_bigwig(None, None, None, C.byref(n)) == -1 and L.br_coverage_bigwig_read(None, 0, 0, None) == -1
    assert L.br_coverage_bigwig_stats(*[None] * 9) == -1
    src = np.zeros(131073, dtype=np.uint8)
    out, out_off = C.c_void_p(), np.zeros(2, dtype=np.uint64)
    off = np.asarray([0, 10], dtype=np.uint64)
    assert L.br_zlib_sections_device(4096, src.ctypes.data, off.ctypes.data, 1, 0, C.byref(out), out_off.ctypes.data) == -2 and not out.value   # BR_ERR_NO_DEVICE
    assert L.br_zlib_sections_device(4096, src.ctypes.data, off.ctypes.data, 1, 2, C.byref(out), out_off.ctypes.data) == -1            # no such mode
    off[1] = 131073
    assert L.br_zlib_sections_device(4096, src.ctypes.data, off.ctypes.data, 1, 0, C.byref(out), out_off.ctypes.data) == -1            # a payload too large
    off[:] = [5, 4]
    assert L.br_zlib_sections_device(4096, src.ctypes.data, off.ctypes.data, 1, 0, C.byref(out), out_off.ctypes.data) == -1            # offsets that descend
    assert L.br_zlib_sections_device(4096, src.ctypes.data, off.ctypes.data, 1, 0, None, out_off.ctypes.data) == -1
    assert C.sizeof(lib.BrBigwigOpts) == 20
    for name in ("bigwig", "bigwig_raw", "bigwig_stats"):
        assert hasattr(lib.Coverage, name), name
    assert callable(lib.zlib_sections)


@pytest.mark.parametrize("extra", [
    ["--coverage-bigwig"],
    ["--coverage-bigwig-zooms", "3"],
    ["--coverage-bigwig-uncompressed", "--coverage", "c.bedgraph"],
    ["--coverage-bigwig", "c.bw", "--coverage-bigwig-zooms", "11"],
    ["--coverage-bigwig", "c.bw", "--coverage-bigwig-zooms", "-1"],
    ["--coverage-bigwig", "c.bw", "--coverage-bigwig-zooms", "four"],
    ["--coverage-bigwig", "c.bw", "--devices", "0,1"],
])
def test_cli_usage_errors(tmp_path, extra):
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    extra = [str(tmp_path / e) if e.endswith((".bw", ".bedgraph")) else e for e in extra]
    r = subprocess.run([os.path.join(ROOT, "bramble_amd", "bin", "bramble"), str(tmp_path / "missing.bam"), "-G", str(gtf), "-o",
                        str(tmp_path / "o.bam")] + extra, capture_output=True, timeout=60)
    assert r.returncode == 2
    assert b"--coverage" in r.stderr and b"usage:" in r.stderr
    assert os.listdir(str(tmp_path)) == ["g.gtf"]


def test_usage_text_names_the_switches():
    r = subprocess.run([os.path.join(ROOT, "bramble_amd", "bin", "bramble"), "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0
    for word in (b"--coverage-bigwig <cov.bw>", b"--coverage-bigwig-zooms", b"--coverage-bigwig-uncompressed", b"[bramble] bigwig: C transcripts"):
        assert word in r.stdout, word
