"""The records that did not project ("keep_unprojected", br_ctx_unprojected_*, --unprojected) against the oracle's complement
(tests/unprojected_cases.py; tests/test_unprojected_cpu.py shows its conditions on the CPU): every records-in / records-out input
in both scopes, the routes of the projection, several calls with a regrowing arena and small pieces, shapes around the kernels'
tiles and the copy's alignment, a record above 64 KiB, and the command line's file, report and failure."""
import os
import struct

import numpy as np
import pytest

from bramble_amd import lib, synth
from tests import alphabet_cases as ac
from tests import bamio, route_cases
from tests import unprojected_cases as uc
from tests.test_cg_tag_cpu import ANN, long_cigar
from tests.test_collate_cpu import collate_order, mapped_records
from tests.test_gpu_collate import _cat, _coordinate_stream, _files, _inputs, _named_records, _run, _strip
from tests.test_sam_cpu import encode_sam

pytestmark = pytest.mark.gpu

BIG = 1 << 40


def _draw(ctx, max_bytes=BIG):
    """every piece until the empty one: (the concatenated stream, its row_off, the pieces' (bytes, rows))"""
    parts, offs, sizes, base = [], [np.zeros(1, np.uint64)], [], 0
    while True:
        s, off = ctx.unprojected_next(max_bytes)
        if off.size == 0:
            break
        assert off[0] == 0 and int(off[-1]) == s.size
        parts.append(s)
        offs.append(off[1:] + np.uint64(base))
        base += s.size
        sizes.append((int(s.size), len(off) - 1))
    s, off = ctx.unprojected_next(max_bytes)   # a draw after the last
    assert s.size == 0 and off.size == 0
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), np.concatenate(offs), sizes


def _stats(ctx):
    st = ctx.unprojected_stats()
    return [st[k] for k in lib.Context.UNPROJECTED_STATS[:6]]


def _assert_result(ctx, want, max_bytes=BIG, tag=""):
    stream, off, stats = want
    got, goff, sizes = _draw(ctx, max_bytes)
    assert _stats(ctx) == stats, (tag, _stats(ctx), stats)
    assert np.array_equal(goff, off), tag
    assert got.size == stream.size and np.array_equal(got, stream), tag
    return sizes


def _context(idx, scope, **params):
    ctx = lib.Context(idx)
    for k, v in params.items():
        ctx.set_param(k, v)
    ctx.set_param("keep_unprojected", uc.SCOPES[scope])
    return ctx


@pytest.mark.parametrize("scope", list(uc.SCOPES))
@pytest.mark.parametrize("case", ac.BAM_CASES, ids=[c.id for c in ac.BAM_CASES])
def test_every_input_in_both_scopes(case, scope):
    ann, stream, ref_map, orc, roff, rlen, recs = uc.case_input(case.id)
    want = uc.yardstick(recs, orc["input_index"], scope)
    assert want[2][1] >= 1
    idx = lib.Index(ann, device=0)
    ctx = _context(idx, scope)
    got, _ = ctx.project_bam_bundle(lib.make_config(**case.flags), stream, roff, rlen, ref_map)
    assert np.array_equal(got, orc["bam_stream"])   # the projected stream of the same call
    _assert_result(ctx, want, tag=case.id)
    ctx.close()
    idx.close()


@pytest.mark.parametrize("case_id,route", [("adv-pe-default-22", r) for r in ("small", "direct", "match_table")] +
                         [("dense-pe-default-25", r) for r in ("direct", "direct_side64", "match_table")])
def test_routes(case_id, route):
    ann, stream, ref_map, orc, roff, rlen, recs = uc.case_input(case_id)
    case = next(c for c in ac.BAM_CASES if c.id == case_id)
    idx = lib.Index(ann, device=0)
    for scope in uc.SCOPES:
        ctx = _context(idx, scope, **route_cases.ROUTES[route])
        ctx.set_profiling(True)
        got, _ = ctx.project_bam_bundle(lib.make_config(**case.flags), stream, roff, rlen, ref_map)
        assert route_cases.route_of(ctx, len(recs)) == route.split("_side")[0]
        if route == "direct_side64":
            assert ctx.direct_diag()["side_attempts"] > 1
        assert np.array_equal(got, orc["bam_stream"])
        _assert_result(ctx, uc.yardstick(recs, orc["input_index"], scope), tag="%s %s %s" % (case_id, route, scope))
        ctx.close()
    idx.close()


def test_several_calls_small_pieces_and_a_regrowing_arena():
    case_id = "adv-pe-default-22"
    ann, stream, ref_map, orc, roff, rlen, recs = uc.case_input(case_id)
    case = next(c for c in ac.BAM_CASES if c.id == case_id)
    cfg = lib.make_config(**case.flags)
    cuts, at = [0], 0
    for a, e in uc.groups_of(recs):   # calls of about 700 records, cut at name boundaries
        if e - cuts[-1] >= 700:
            cuts.append(e)
    if cuts[-1] != len(recs):
        cuts.append(len(recs))
    assert len(cuts) > 5
    idx = lib.Index(ann, device=0)
    for scope in uc.SCOPES:
        want = uc.yardstick(recs, orc["input_index"], scope)
        ctx = _context(idx, scope, unprojected_cap=1024)
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            sub = _cat(recs[lo:hi])
            o, l, _, used = lib.bam_split(sub)
            assert used == sub.size and len(o) == hi - lo
            parts.append(ctx.project_bam_bundle(cfg, sub, o, l, ref_map)[0])
        assert np.array_equal(np.concatenate(parts), orc["bam_stream"])
        st = ctx.unprojected_stats()
        assert st["held_bytes"] >= want[2][2] + 8 * want[2][1] > 1024 and st["peak_bytes"] > st["held_bytes"]   # it grew, the old beside the new
        with pytest.raises(lib.BrambleError):   # not while records are held
            ctx.set_param("keep_unprojected", 0)
        sizes = _assert_result(ctx, want, max_bytes=4096, tag=scope)
        assert len(sizes) > 20 and all(b <= 4096 or r == 1 for b, r in sizes)
        assert max(b for b, _ in sizes) > 4096 - 600   # the pieces are filled
        ctx.unprojected_reset()
        assert ctx.unprojected_stats() == dict.fromkeys(lib.Context.UNPROJECTED_STATS, 0)
        assert _draw(ctx)[0].size == 0
        ctx.set_param("keep_unprojected", 0)
        ctx.project_bam_bundle(cfg, _cat(recs[:cuts[1]]), *lib.bam_split(_cat(recs[:cuts[1]]))[:2], ref_map)
        assert ctx.unprojected_stats() == dict.fromkeys(lib.Context.UNPROJECTED_STATS, 0)   # off: nothing is kept, nothing allocated
        ctx.close()
    idx.close()


def _shaped_records(n):
    """_named_records(n), collated, the names of group g longer by g % 8 bytes: record lengths (and with them source and
    destination alignments) of every residue mod 8"""
    recs = list(_named_records(n))
    recs = [recs[i] for i in collate_order(recs)]
    out, g, prev = [], -1, None
    for r in recs:
        name = r[36:36 + r[12]]
        if name != prev:
            g, prev = g + 1, name
        k = g % 8
        body = r[4:36] + name[:-1] + b"x" * k + b"\0" + r[36 + r[12]:]
        body = body[:8] + bytes([r[12] + k]) + body[9:]
        out.append(struct.pack("<I", len(body)) + body)
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097])
def test_nothing_projects_the_result_is_the_input(n):
    """a reference map of all -1: around the wave (64), a block of groups (256) and two scan tiles (2048)"""
    ann = uc.case_input("adv-pe-default-22")[0]
    recs = _shaped_records(n)
    assert n < 65 or len({len(r) % 8 for r in recs}) == 8
    stream = _cat(recs) if n else np.zeros(0, np.uint8)
    roff, rlen, _, _ = lib.bam_split(stream) if n else (np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0, 0)
    idx = lib.Index(ann, device=0)
    for scope in uc.SCOPES:
        ctx = _context(idx, scope)
        got, cnt = ctx.project_bam_bundle(lib.make_config(), stream, roff, rlen, np.full(3, -1, np.int32))
        assert got.size == 0 and cnt["n_rows"] == 0
        want = uc.yardstick(recs, [], scope)
        assert want[0].size == stream.size
        _assert_result(ctx, want, tag=scope)
        ctx.close()
    idx.close()


def test_everything_projects_the_result_is_empty():
    """the records of the read names that projected whole in the first test's input, as an input of their own"""
    case_id = "adv-pe-default-22"
    ann, stream, ref_map, orc, roff, rlen, recs = uc.case_input(case_id)
    projected = np.zeros(len(recs), bool)
    projected[orc["input_index"]] = True
    sub = [r for a, e in uc.groups_of(recs) if projected[a:e].all() for r in recs[a:e]]
    assert len(sub) > 1000
    sub_stream = _cat(sub)
    flags = next(c for c in ac.BAM_CASES if c.id == case_id).flags
    orc2, o, l = uc.oracle_bam(ann, sub_stream, ref_map, flags)
    want = uc.yardstick(sub, orc2["input_index"], "record")
    assert want[2][1] == 0 and want[2][4] == 0 and want[2][5] == 0   # (the oracle's own complement is empty)
    idx = lib.Index(ann, device=0)
    for scope in uc.SCOPES:
        ctx = _context(idx, scope)
        got, _ = ctx.project_bam_bundle(lib.make_config(**flags), sub_stream, o, l, ref_map)
        assert np.array_equal(got, orc2["bam_stream"])
        _assert_result(ctx, uc.yardstick(sub, orc2["input_index"], scope), tag=scope)
        assert ctx.unprojected_stats()["held_bytes"] == 0
        ctx.close()
    idx.close()


@pytest.mark.parametrize("mapped", [False, True])
def test_a_record_above_64_kib_between_two_short_ones(mapped):
    cig, qlen, _ = long_cigar(17501)   # 70004 ops in a CG:B,I tag: 280 KB of tag, 400 KB in all
    recs = [bamio.bam_record(b"r000", 0, 1300, [(90 << 4) | 0], 90, aux=b"NMC\x01"),
            bamio.bam_record(b"ultra", 0, 1999, cig, qlen, aux=b"NMi" + struct.pack("<i", 5)),
            bamio.bam_record(b"r01", 0, 2400, [(90 << 4) | 0], 90, aux=b"NMC\x01")]
    assert len(recs[1]) > 65536
    framed = uc.split(bamio.frame(recs))
    stream = _cat(framed)
    ref_map = np.array([0 if mapped else -1], np.int32)
    orc, roff, rlen = uc.oracle_bam(ANN, stream, ref_map, {"lr": 1})
    assert (orc["n_rows"] > 0) == mapped
    idx = lib.Index(ANN, device=0)
    for scope in uc.SCOPES:
        ctx = _context(idx, scope)
        got, _ = ctx.project_bam_bundle(lib.make_config(lr=1), stream, roff, rlen, ref_map)
        assert np.array_equal(got, orc["bam_stream"])
        _assert_result(ctx, uc.yardstick(framed, orc["input_index"], scope), tag=scope)
        ctx.close()
    idx.close()


# ---- command line -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """the input of tests/test_gpu_cli_outputs.py (unmapped records every 23rd), its files, and the run without the switch"""
    d = tmp_path_factory.mktemp("in")
    annd, recs, stream = _inputs("pe")
    gtf = str(d / "g.gtf")
    bamio.write_gtf(gtf, annd)
    bam, hdr = _files(d, annd, stream, "in")
    ref_map = np.arange(len(annd["refnames"]), dtype=np.int32)
    plain = str(d / "plain.bam")
    _run([bam, "-G", gtf], plain)
    return {"annd": annd, "recs": recs, "stream": stream, "gtf": gtf, "bam": bam, "hdr": hdr, "ref_map": ref_map, "dir": d,
            "plain": bamio.read_bam(plain), "refs": [(n, 10 ** 7) for n in annd["refnames"]]}


def _want(cli, recs, scope):
    orc, _, _ = uc.oracle_bam(cli["annd"], _cat(recs), cli["ref_map"], {})
    return uc.yardstick(recs, orc["input_index"], scope)


def _assert_file(cli, path, want):
    text, refs, s = bamio.read_bam(path)
    assert text == cli["hdr"] and [tuple(r) for r in refs] == cli["refs"]   # the input's header and nothing else
    assert want[2][1] > 100 and np.array_equal(np.frombuffer(bytes(s), np.uint8), want[0])


def _assert_report(r, want, scope, n_more=0):
    out = r.stdout.decode().split("\n")
    at = out.index("[bramble] final report:")
    line = "[bramble] unprojected: %d of %d records written (%d read names without a projected record, %d partly projected; scope %s)" % (
        want[2][1], want[2][0], want[2][4], want[2][5], scope)
    assert out[at - 1] == "" and out[at - 2] == line, out[at - 2]
    assert sum(1 for l in out if l.startswith("[bramble] unprojected")) == 1
    assert sum(1 for l in out[:at] if l.startswith(("[bramble] sorted ", "[bramble] quantified ", "[bramble] coverage: "))) == n_more


@pytest.mark.parametrize("scope", list(uc.SCOPES))
def test_cli_file_main_output_and_report(tmp_path, cli, scope):
    out, un = str(tmp_path / "out.bam"), str(tmp_path / "un.bam")
    r = _run([cli["bam"], "-G", cli["gtf"], "--unprojected", un] + (["--unprojected-scope", "name"] if scope == "name" else []), out)
    want = _want(cli, cli["recs"], scope)
    _assert_file(cli, un, want)
    text, refs, s = bamio.read_bam(out)
    text0, refs0, s0 = cli["plain"]
    assert _strip(text) == _strip(text0) and refs == refs0 and np.array_equal(s, s0)   # the run without the switch, but for @PG
    _assert_report(r, want, scope)
    assert sorted(os.listdir(tmp_path)) == ["out.bam", "un.bam"]


@pytest.mark.parametrize("how", ["host-reader", "host-deflate", "collate", "sam-stdin", "every-switch"])
def test_cli_other_inputs(tmp_path, cli, how):
    out, un = str(tmp_path / "out.bam"), str(tmp_path / "un.bam")
    args, stdin, recs, n_more = [cli["bam"]], None, cli["recs"], 0
    if how == "host-reader":
        args += ["--host-reader"]
    elif how == "host-deflate":
        args += ["--host-deflate"]
    elif how == "collate":   # the coordinate-sorted file: the yardstick over the tests' collation of its mapped records
        sorted_stream = _coordinate_stream(cli["stream"])
        args = [_files(tmp_path, cli["annd"], sorted_stream, "sorted")[0], "--collate"]
        recs = mapped_records(sorted_stream)
        recs = [recs[i] for i in collate_order(recs)]
    elif how == "sam-stdin":   # the records as the SAM reader makes them of the lines
        names = cli["annd"]["refnames"]
        sam = synth.records_to_sam(cli["stream"], names)
        args, stdin = ["-"], cli["hdr"].encode() + sam
        recs = mapped_records(encode_sam(sam, names)[2])
    else:
        d = str(tmp_path)
        args += ["--sort", "--write-index", "--quant", d + "/quant.tsv", "--coverage", d + "/cov.bedgraph"]
        n_more = 3
    r = _run(args + ["-G", cli["gtf"], "--unprojected", un], out, stdin=stdin)
    want = _want(cli, recs, "record")
    _assert_file(cli, un, want)
    _assert_report(r, want, "record", n_more)
    assert len(bamio.read_bam(out)[2]) > 100000
    if how == "every-switch":
        assert sorted(os.listdir(tmp_path)) == ["cov.bedgraph", "out.bam", "out.bam.bai", "quant.tsv", "un.bam"]


def test_cli_a_file_that_cannot_be_written(tmp_path, cli):
    d = str(tmp_path / "out")
    os.mkdir(d)
    r = _run([cli["bam"], "-G", cli["gtf"], "--unprojected", d + "/no_such_dir/un.bam"], d + "/out.bam", ok=False)
    assert r.returncode == 1 and b"no_such_dir/un.bam" in r.stderr
    assert os.listdir(d) == []
