"""--coverage-bigwig on the GPU: br_coverage_bigwig's file image against the tests' writer (bigwig_cases.py: the definitions of
bramble_amd.h restated) -- to the byte without compression, field for field and stream by decoded stream with it -- through the
tests' reader (bigwig_ref.py), which walks and checks every tree; section boundaries at the default S with the stored fallback;
the edges of the zoom windows; the weighted depth against derived bounds; the zlib codec on its own at its edges; the errors and
the device-memory account; and the command line with the switch against the run without it."""
import os
import struct
import zlib

import numpy as np
import pytest

from bramble_amd import lib
from tests import bamio
from tests import bigwig_cases as bc
from tests import bigwig_ref as br
from tests.test_bigwig_cpu import SMALL, _assert_same_content, _assert_track
from tests.test_coverage_cpu import coverage_of
from tests.test_coverage_weight_cpu import weight_words_nh, weighted_coverage_of
from tests.test_quant_fld_cpu import packed_of, rows_of, wide_rows

pytestmark = pytest.mark.gpu


def _coverage(rows, lens, calls=1, nh=None):
    """a finished Coverage of the rows, added from the host in `calls` adds; nh: the rows' NH and weight nh"""
    a, ref, pool = packed_of(rows)
    c = lib.Coverage(lens)
    if nh is not None:
        a = a.copy()
        a[:, 3] = nh
        c.set_param("weight", 1)
    cuts = [0, len(a)] if calls == 1 else [0, len(a) // 3, len(a) // 3 + 1, len(a)]
    for r0, r1 in zip(cuts, cuts[1:]):
        c.add_rows_host(a, ref, pool, r0, r1)
    c.finish()
    return c


# ---- 1. byte equality, uncompressed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [1, 3])
def test_uncompressed_image_equals_the_writer(calls):
    """The hand-built table under the names case; S = 4, blockSize 4, four levels from 32 bases: three tree levels, partial last
    sections, windows and nodes.  Every byte is compared, the zoom sums of the depth-100 000 spot included: they are above 2^24 but
    below 2^53, so the device's double sums are exact and round once, as the writer's do (test_bigwig_cpu.py asserts both)."""
    rows, cov, lens = bc.hand_built()
    want, _ = bc.write_bigwig(cov, lens, bc.NAMES_CASE, **SMALL)
    c = _coverage(rows, lens, calls)
    got = c.bigwig(bc.NAMES_CASE, **SMALL)
    if got != want:   # say where before failing
        ra, rb = br.read_all(got, 4, 4), br.read_all(want, 4, 4)
        _assert_same_content(ra, rb)
    assert got == want
    st = c.bigwig_stats()
    r = br.read_all(got, 4, 4)
    assert st["chromosomes"] == 8 and st["sections"] == len(r["sections"]) and st["zoom_records"] == [len(z["records"]) for z in r["zooms"]]
    assert st["n_bytes"] == len(got) and st["raw_bytes"] == st["data_bytes"] == sum(24 + 12 * len(s[3]) for s in r["sections"]) + 32 * sum(st["zoom_records"])
    assert len(br.levels_of(st["sections"], 4)[1]) >= 3
    c.close()


# ---- 2. compressed ------------------------------------------------------------------------------------------------------------------
def test_compressed_image_decodes_to_the_writers():
    rows, cov, lens = bc.hand_built()
    want, _ = bc.write_bigwig(cov, lens, bc.NAMES_CASE, block_size=4)
    c = _coverage(rows, lens)
    got = c.bigwig(bc.NAMES_CASE, block_size=4)
    ra, rb = br.read_all(got, option_bs=4, items_per_slot=1024), br.read_all(want, option_bs=4, items_per_slot=1024)
    assert ra["compressed"] and ra["header"]["uncompress_buf"] == 32768
    _assert_same_content(ra, rb)
    _assert_track(ra, cov, bc.NAMES_CASE, lens)
    st = c.bigwig_stats()
    assert st["data_bytes"] < st["raw_bytes"] and st["n_bytes"] == len(got)
    rng = np.random.RandomState(3)
    order = bc.chromosomes(cov["runs"], bc.NAMES_CASE)
    for _ in range(20):
        k = int(rng.randint(len(order)))
        s = int(rng.randint(int(lens[order[k]])))
        e = s + 1 + int(rng.randint(300))
        assert br.intervals(got, k, s, e) == [(int(a), int(b), float(np.float32(d))) for t, a, b, d in zip(*cov["runs"]) if t == order[k] and a < e and b > s]
    assert c.bigwig(bc.NAMES_CASE, block_size=4) == got          # a second call replaces the image with the same bytes
    c2 = _coverage(rows, lens, 3)
    assert c2.bigwig(bc.NAMES_CASE, block_size=4, page=1000) == got   # and so does a second object, read in small pages
    c.close(); c2.close()


# ---- 3. section boundaries at the default S -------------------------------------------------------------------------------------
def _stored(stream):
    return stream[2] & 6 == 0   # BTYPE 00 behind the two bytes of the zlib header


def _streams(data):
    h = br.header(data)
    _, leaves, _ = br.rtree(data, h["full_index"])
    return [bytes(data[off:off + size]) for _, _, off, size in leaves]


@pytest.mark.parametrize("n_runs", [1024, 1025, 2049])
def test_section_boundaries_at_the_default_slot(n_runs):
    stored = 0
    for random_depth in (False, True):
        rows, nh, cov, lens, wide = bc.boundary_case(n_runs, random_depth)
        c = _coverage(rows, lens, nh=nh)
        assert c.n_runs == n_runs
        got = c.bigwig(["one"])
        want, _ = bc.write_bigwig(cov, lens, ["one"], wide=wide)
        ra, rb = br.read_all(got, 256, 1024), br.read_all(want, 256, 1024)
        assert [len(s[3]) for s in ra["sections"]] == [1024] * (n_runs // 1024) + ([n_runs % 1024] if n_runs % 1024 else [])
        for x, y in zip(ra["sections"], rb["sections"]):
            assert x[:3] == y[:3] and x[3].tobytes() == y[3].tobytes()
        if not wide:
            _assert_same_content(ra, rb)
        streams = _streams(got)
        for s, sec in zip(streams, ra["sections"]):
            assert len(s) <= 24 + 12 * len(sec[3]) + 11
        if random_depth:
            stored += sum(_stored(s) for s, sec in zip(streams, ra["sections"]) if len(sec[3]) == 1024)   # (of the full sections)
        else:   # every end is the next start and the values repeat 24 bytes apart: compressed (a last section of one item is not)
            full = [s for s, sec in zip(streams, ra["sections"]) if len(sec[3]) == 1024]
            assert full and not any(_stored(s) for s in full) and all(len(s) < 24 + 12 * 1024 for s in full)
        c.close()
    assert stored >= 1


# ---- 4. zoom edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [-1, 4, 10])
def test_zoom_edges(levels):
    rows, cov, lens = bc.zoom_edge_case()
    c = _coverage(rows, lens)
    for compress in (-1, 1):
        got = c.bigwig(bc.ZOOM_EDGE_NAMES, zoom_levels=levels, compress=compress)
        want, _ = bc.write_bigwig(cov, lens, bc.ZOOM_EDGE_NAMES, zoom_levels=levels, compress=compress)
        if compress < 0:
            assert got == want
        ra = br.read_all(got)
        _assert_same_content(ra, br.read_all(want))
        assert len(ra["zooms"]) == max(levels, 0) == c.bigwig_stats()["zoom_levels"]
    if levels == 10:
        assert ra["zooms"][9]["reduction"] == 8388608 and len(ra["zooms"][9]["records"]) == 5
    c.close()


# ---- 5. weighted ------------------------------------------------------------------------------------------------------------------------
def test_weighted_values_and_zoom_floats():
    """Weight nh with NH 3 and 7.  The items' values are (float) ((double) depth64 * 2^-32) exactly.  A zoom sum: the device adds at
    most 2^23 doubles, relative error at most 2^23 * 2^-53 = 2^-30, far below half a float32 ulp (2^-25), so only the last rounding
    can differ: within 1 ulp of the exact value rounded once.  The total summary's doubles: n covered bases, n * 2^-52 relative."""
    rng = np.random.RandomState(11)
    lens = np.asarray([300, 5000, 64, 0, 1], dtype=np.int64)
    items = [(int(t), int(rng.randint(int(lens[t]))), 0, "%dM%dN%dM" % (1 + rng.randint(60), 1 + rng.randint(9), 1 + rng.randint(60)))
             for t in rng.choice([0, 1, 1, 1, 2, 4], 400)]
    rows = rows_of(items)
    nh = np.where(np.arange(len(items)) % 2, 3, 7)
    cov = weighted_coverage_of(rows, lens, weight_words_nh(nh))
    names = ["w300", "w5000", "w64", "none", "w1"]
    c = _coverage(rows, lens, nh=nh)
    opts = dict(SMALL, items_per_slot=16)
    got = c.bigwig(names, **opts)
    want, extra = bc.write_bigwig(cov, lens, names, wide=True, **opts)
    ra, rb = br.read_all(got, 4, 16), br.read_all(want, 4, 16)
    assert ra["chroms"] == rb["chroms"] and len(ra["sections"]) == len(rb["sections"]) > 8
    for x, y in zip(ra["sections"], rb["sections"]):
        assert x[:3] == y[:3] and x[3].tobytes() == y[3].tobytes()
    assert len({float(i["value"]) for s in ra["sections"] for i in s[3]}) > 20
    for x, y in zip(ra["zooms"], rb["zooms"]):
        a, b = x["records"], y["records"]
        assert len(a) == len(b) > 0
        for f in ("chrom", "start", "end", "valid", "min", "max"):
            assert np.array_equal(a[f], b[f]), f
        for f in ("sum", "sumsq"):
            apart = bc.ulp_apart(a[f], b[f])
            print("zoom R=%d %s: %d of %d records differ from the exact value rounded once, at most %d ulp" % (x["reduction"], f, int((apart > 0).sum()), len(a), int(apart.max())))
            assert apart.max() <= 1, f
    sa, sb = ra["header"]["summary"], rb["header"]["summary"]
    n = sb["valid"]
    assert sa["valid"] == n > 1000 and sa["min"] == sb["min"] and sa["max"] == sb["max"]
    for f in ("sum", "sumsq"):
        print("total %s: relative error %.3g (bound %.3g)" % (f, abs(sa[f] - sb[f]) / sb[f], n * 2.0 ** -52))
        assert abs(sa[f] - sb[f]) <= n * 2.0 ** -52 * sb[f], f
    c.close()


# ---- 6. the codec on its own ---------------------------------------------------------------------------------------------------------
def _payloads():
    rng = np.random.RandomState(6)
    out = []
    for n in (0, 1, 3, 4, 258, 259, 5552, 5553, 16384, 255, 256, 257, 16383, 64 * 256 - 255, 65535, 65536, 70000, 131072):
        out.append(rng.randint(0, 4, n).astype(np.uint8).tobytes())                 # compressible
        out.append(rng.randint(0, 256, n).astype(np.uint8).tobytes())               # not
    out += [b"\xff" * 16384, b"\0" * 16384, b"\xff" * 131072, bytes(range(256)) * 64, b"abc" * 1000 + b"x"]
    return out


def _max_stream(n):
    return n + 6 + 5 * max(-(-n // 65535), 1)   # payload + 11 up to 65535 bytes


def test_zlib_sections_alone():
    payloads = _payloads()
    streams = lib.zlib_sections(0, payloads, 0)
    assert len(streams) == len(payloads) > 4
    n_stored = n_fixed = 0
    for p, s in zip(payloads, streams):
        assert s[:2] == b"\x78\x9c" and zlib.decompress(s) == p, len(p)     # (the Adler-32 is checked by zlib)
        assert len(s) <= _max_stream(len(p)), len(p)
        if _stored(s):
            n_stored += 1
            assert len(s) == _max_stream(len(p))
        else:
            n_fixed += 1
            assert s[2] & 7 == 3 and len(s) - 6 < len(p)                    # one final fixed-Huffman block, smaller than the payload
    assert n_stored >= 10 and n_fixed >= 10
    # one byte repeated: matches of 258 after the first step's literals, a sixteenth of the payload at the very most
    assert len(streams[payloads.index(b"\0" * 16384)]) < 16384 // 16 and len(streams[payloads.index(b"\xff" * 131072)]) < 131072 // 16
    for p, s in zip(payloads, lib.zlib_sections(0, payloads, 1)):           # mode 1: stored
        assert _stored(s) and zlib.decompress(s) == p and len(s) == _max_stream(len(p))
        if len(p) <= 65535:
            assert s[2] == 1 and struct.unpack_from("<HH", s, 3) == (len(p), len(p) ^ 0xffff) and s[7:7 + len(p)] == p


def test_zlib_sections_many_in_one_call():
    rng = np.random.RandomState(7)
    payloads = [(rng.randint(0, 3 + k % 5, 40 + 37 * k).astype(np.uint8).tobytes() if k % 3 else rng.randint(0, 256, 100 + k).astype(np.uint8).tobytes())
                for k in range(70)]
    for mode in (0, 1):
        streams = lib.zlib_sections(0, payloads, mode)
        assert [zlib.decompress(s) for s in streams] == payloads and all(len(s) <= len(p) + 11 for p, s in zip(payloads, streams))
    assert lib.zlib_sections(0, [], 0) == [] and [zlib.decompress(s) for s in lib.zlib_sections(0, [b""], 0)] == [b""]


# ---- 7. errors and memory ---------------------------------------------------------------------------------------------------------
def test_errors_and_held_bytes():
    rows, cov, lens = bc.zoom_edge_case()
    names = bc.ZOOM_EDGE_NAMES
    a, ref, pool = packed_of(rows)
    c = lib.Coverage(lens)
    c.add_rows_host(a, ref, pool)
    assert c.bigwig_raw(names)[0] == -1 and c._raw("bigwig_read", 0, 0, None) == -1 and c._raw("bigwig_stats", *[None] * 8) == -1   # before finish
    c.finish()
    h0 = c.stats()["held_bytes"]
    assert c._raw("bigwig_read", 0, 0, None) == -1 and c._raw("bigwig_stats", *[None] * 8) == -1                  # no image yet
    bad = [{"items_per_slot": 4097}, {"block_size": 1}, {"block_size": 4097}, {"zoom_levels": 11}, {"zoom_levels": -2}, {"compress": 2},
           {"compress": -2}, {"first_reduction": 2 ** 29}, {"first_reduction": 2 ** 13, "zoom_levels": 10}]
    for o in bad:
        assert c.bigwig_raw(names, **o)[0] == -1, o
    for bad_names in ([None] + names[1:], names[:2] + [""] + names[3:], ["same", "same"] + names[2:], []):
        rc = c.bigwig_raw(bad_names + [None] * (len(names) - len(bad_names))) if bad_names else (c._raw("bigwig", None, None, None), 0)
        assert rc[0] == -1, bad_names
    assert c.stats()["held_bytes"] == h0                                                                          # nothing was made
    assert c.bigwig_raw(names, first_reduction=2 ** 12, zoom_levels=10)[0] == 0                                   # 2^12 * 4^9 = 2^30
    first = c.bigwig(names, compress=-1)
    assert c.stats()["held_bytes"] == h0 + len(first) and c.stats()["peak_bytes"] > h0 + len(first)
    second = c.bigwig(names, zoom_levels=-1)
    assert len(second) != len(first) and c.stats()["held_bytes"] == h0 + len(second)                              # the first image went
    for o in bad[:3]:
        assert c.bigwig_raw(names, **o)[0] == -1
    assert c.stats()["held_bytes"] == h0 + len(second) and c.bigwig_stats()["n_bytes"] == len(second)             # a refusal keeps the image
    out = np.zeros(16, dtype=np.uint8)
    n = len(second)
    assert c._raw("bigwig_read", n, 0, out.ctypes.data) == 0 and c._raw("bigwig_read", n - 4, 4, out.ctypes.data) == 0
    assert out[:4].tobytes() == struct.pack("<I", br.BIGWIG_MAGIC)
    assert c._raw("bigwig_read", n - 3, 4, out.ctypes.data) == -1 and c._raw("bigwig_read", n + 1, 0, out.ctypes.data) == -1
    assert c._raw("bigwig_read", 2 ** 64 - 1, 2, out.ctypes.data) == -1 and c._raw("bigwig_read", 0, 4, None) == -1
    # names of transcripts without runs are not read
    rows1 = rows_of([(1, 0, 0, "5M")])
    c1 = _coverage(rows1, lens)
    r = br.read_all(c1.bigwig([None, "only", "", "only", None]))
    assert r["chroms"] == [(b"only", 0, 32)]
    c.close(); c1.close()


def test_an_object_without_runs():
    lens = np.asarray([100, 0, 7], dtype=np.int64)
    c = lib.Coverage(lens)
    assert c.finish() == 0
    for opts in ({}, {"compress": -1, "zoom_levels": -1}, {"block_size": 2, "zoom_levels": 10}):
        data = c.bigwig(["a", "b", "c"], **opts)
        r = br.read_all(data)
        want, _ = bc.write_bigwig(coverage_of(rows_of([]), lens), lens, ["a", "b", "c"], **opts)
        assert r["chroms"] == [] and r["sections"] == [] and r["header"]["summary"]["valid"] == 0 and data == want
    assert c.bigwig_stats()["chromosomes"] == 0 and br.read_all(c.bigwig([])) is not None
    c.close()


# ---- 8. command line ------------------------------------------------------------------------------------------------------------------
def test_cli_coverage_bigwig(tmp_path):
    from tests.test_gpu_collate import _files, _inputs, _report, _run
    from tests.test_gpu_quant import _body
    annd, _, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, _ = _files(tmp_path, annd, stream, "in")
    tb, rows = wide_rows("pe", guide_order=True)   # (the command line numbers the transcripts in guide order)
    names = [t["id"] for t in tb["annd"]["transcripts"]]
    want = coverage_of(rows, tb["lens"])

    def paths(tag):
        return [str(tmp_path / ("%s.%s" % (tag, ext))) for ext in ("out", "bedgraph", "cov.tsv", "bw")]
    o0, bed0, tsv0, _ = paths("plain")
    r0 = _run([in_bam, "-G", gtf, "--coverage", bed0, "--coverage-summary", tsv0], o0)
    o1, bed1, tsv1, bw1 = paths("with")
    r1 = _run([in_bam, "-G", gtf, "--coverage", bed1, "--coverage-summary", tsv1, "--coverage-bigwig", bw1], o1)
    # everything else the run writes is the run's without the switch, to the byte
    for p0, p1 in ((bed0, bed1), (tsv0, tsv1)):
        assert open(p0, "rb").read() == open(p1, "rb").read(), p1
    (h0, s0), (h1, s1) = _body(o0, False), _body(o1, False)   # (the header but for its @PG line, which holds the command line)
    assert h0 == h1 and np.array_equal(s0, s1) and len(s0) > 100000
    out0, out1 = r0.stdout.decode().split("\n"), r1.stdout.decode().split("\n")
    line = [l for l in out1 if l.startswith("[bramble] bigwig: ")]
    assert len(line) == 1 and not any("bigwig" in l for l in out0) and len(out1) == len(out0) + 1 and _report(r1) == _report(r0)
    assert out1[out1.index(line[0]) - 1].startswith("[bramble] coverage: ") and out1.index(line[0]) + 2 == out1.index("[bramble] final report:")
    assert len(_report(r1)) == 5
    # the file is Coverage.bigwig's on the same rows, and its items are the bedGraph's lines
    c = _coverage(rows, tb["lens"])
    data = open(bw1, "rb").read()
    assert data == c.bigwig(names)
    st = c.bigwig_stats()
    r = br.read_all(data, 256, 1024)
    _assert_track(r, want, names, tb["lens"])
    order = bc.chromosomes(want["runs"], names)
    bed = sorted((names[order[cid]], int(i["start"]), int(i["end"]), int(i["value"])) for cid, _, _, items in r["sections"] for i in items)
    assert bed == sorted((f[0], int(f[1]), int(f[2]), int(f[3])) for f in (l.split("\t") for l in open(bed1).read().split("\n")[:-1])) and len(bed) > 10000
    zr = ", ".join(str(v) for v in st["zoom_records"])
    assert line[0].startswith("[bramble] bigwig: %d transcripts, %d sections of %d runs, 4 zoom levels (%s records), %d -> %d bytes (build " % (
        st["chromosomes"], st["sections"], len(want["runs"][0]), zr, st["raw_bytes"], st["data_bytes"])) and line[0].endswith("s)")
    assert not os.path.exists(bw1 + ".tmp-bramble")
    # alone, with its switches; the options reach the file
    o2, bed2, tsv2, bw2 = paths("alone")
    r2 = _run([in_bam, "-G", gtf, "--coverage-bigwig", bw2, "--coverage-bigwig-zooms", "0", "--coverage-bigwig-uncompressed"], o2)
    h2, s2 = _body(o2, False)
    assert h2 == h0 and np.array_equal(s2, s0) and not os.path.exists(bed2) and not os.path.exists(tsv2)
    assert open(bw2, "rb").read() == c.bigwig(names, zoom_levels=-1, compress=-1)
    assert any(l.startswith("[bramble] bigwig: ") and ", 0 zoom levels ( records), " in l for l in r2.stdout.decode().split("\n"))
    c.close()
    # a bad value stops the run before anything is projected
    o3 = str(tmp_path / "bad.out")
    r3 = _run([in_bam, "-G", gtf, "--coverage-bigwig", str(tmp_path / "bad.bw"), "--coverage-bigwig-zooms", "11"], o3, ok=False)
    assert r3.returncode == 2 and b"--coverage-bigwig-zooms" in r3.stderr and not [p for p in os.listdir(str(tmp_path)) if p.startswith("bad")]
    # a path that cannot be written fails the run and leaves nothing
    o4 = str(tmp_path / "fail.out")
    r4 = _run([in_bam, "-G", gtf, "--coverage-bigwig", str(tmp_path / "no_such_dir" / "c.bw")], o4, ok=False)
    assert r4.returncode == 1 and b"c.bw" in r4.stderr and not [p for p in os.listdir(str(tmp_path)) if p.startswith("fail")]
