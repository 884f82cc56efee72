"""--quant-bam on the GPU: br_assign's values (w, ZW, kept) and its rewritten record stream against the tests' restatement of the
definitions (tests/quant_bam_cases.py; tests/test_quant_bam_cpu.py pins it on the CPU), with the posteriors the quantifier itself
hands out as the yardstick's input: on the oracle's rows of the synthetic inputs through every way in, on a hand-built table, on the
records-in inputs in both modes and three piece sizes, on sizes around the kernels' tiles, with a regrowing arena; the errors, the
memory account and the command line."""
import functools
import os
import struct

import numpy as np
import pytest

from bramble_amd import lib
from tests import alphabet_cases as ac
from tests import bamio
from tests import quant_bam_cases as qb
from tests import unprojected_cases as uc
from tests.route_cases import yardstick_rows
from tests.test_cg_tag_cpu import ANN, long_cigar
from tests.test_coverage_weight_cpu import name_classes_of, row_names_of
from tests.test_gpu_collate import _cat, _coordinate_stream, _files, _inputs, _report, _run, _strip
from tests.test_gpu_coverage_weight import _fill_last, _quant, _tables
from tests.test_gpu_unprojected import _shaped_records
from tests.test_quant_cpu import classes_of
from tests.test_quant_fld_cpu import ROW_FIRST, wide_rows

pytestmark = pytest.mark.gpu

BIG = 1 << 30
INVALID, CAPACITY = -1, -5


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def _packed(tids, meta):
    a = np.zeros((len(tids), 4), dtype=np.uint32)
    a[:, 0], a[:, 2], a[:, 3] = tids, meta, 1
    return a


def _cuts(n, calls):
    return [0, n] if calls == 1 else [0, n // 3, n // 3 + 1, n]   # (a call of one name among them)


def _fill(objs, a, row_off, group_off, how, stream=None):
    """the read names into every object of `objs` (Quant or Assign), call by call, from host memory ("host", "host3") or from HBM
    ("dev1", "dev3"); stream: the rows' records (host memory) for the Assign objects, or None"""
    import torch
    ro, go = np.ascontiguousarray(row_off, dtype=np.uint64), np.ascontiguousarray(group_off, dtype=np.uint32)
    cuts = _cuts(len(go) - 1, 3 if how.endswith("3") else 1)
    rec_off = lib.Sorter.row_offsets(stream) if stream is not None else None
    keep = []
    if how.startswith("dev"):
        d_a, d_ro, d_go = (torch.from_numpy(x).cuda() for x in (a.view(np.int32), ro.view(np.int64), go.view(np.int32)))
        recs = None
        if stream is not None:
            d_s, d_off = torch.from_numpy(np.array(stream, dtype=np.uint8)).cuda(), torch.from_numpy(rec_off.view(np.int64)).cuda()
            recs = lib.BrDeviceBam(d_s.data_ptr(), d_s.numel(), d_off.data_ptr(), d_off.numel() - 1)
            keep += [d_s, d_off]
    for g0, g1 in zip(cuts, cuts[1:]):
        for o in objs:
            if isinstance(o, lib.Quant):
                if how.startswith("host"):
                    o.add_host(a, ro, go[g0:g1 + 1])
                else:
                    o.add_device(d_a, d_ro, d_go, g0, g1)
            elif how.startswith("host"):
                o.add_host(a, ro, go[g0:g1 + 1], stream, rec_off)
            else:
                o.add_device(d_a, d_ro, d_go, len(a), recs, g0, g1)
    torch.cuda.synchronize()


def _yardstick(post, tids, meta, row_off, group_off):
    """-> (w float64 per record, placements): everything downstream of the quantifier's own posteriors"""
    cl = classes_of(tids, row_off, group_off)
    pl = qb.placements_of(meta, row_off, group_off)
    w, _ = qb.weights_of(post, cl, name_classes_of(tids, row_off, group_off), row_names_of(len(tids), row_off, group_off), tids, pl)
    return w, pl


def _assert_values(a, w, kept, tag):
    gw, gz, gk = a.values(0, len(w))
    assert gw.dtype == np.float64 and gz.dtype == np.float32 and gk.dtype == np.uint8
    bad = np.flatnonzero(gw.view(np.uint64) != w.view(np.uint64))
    assert bad.size == 0, (tag, bad[:5], gw[bad[:5]], w[bad[:5]])
    assert np.array_equal(gz.view(np.uint32), qb.zw_of(w).view(np.uint32)), tag
    assert np.array_equal(gk, kept), (tag, int(np.count_nonzero(gk != kept)))


def _drain(a, max_bytes):
    """every piece until the empty one: (the concatenated stream, the pieces' (bytes, rows))"""
    parts, sizes = [], []
    for data, off in a.pieces(max_bytes):
        assert off[0] == 0 and int(off[-1]) == data.size and np.all(np.diff(off) > 0)
        parts.append(data)
        sizes.append((int(data.size), len(off) - 1))
    assert a.next_records(max_bytes).n_rows == 0   # a draw after the last
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), sizes


def _em(q):
    q.finish()
    q.em()
    return q.posteriors()


# ---- values on the synthetic inputs --------------------------------------------------------------------------------------------
HOWS = ("host", "host3", "dev1", "dev3", "last")


@pytest.mark.parametrize("vb", [0, 1])
@pytest.mark.parametrize("mode,length_norm,eff_len", [("pe", 1, 0), ("ont", 0, 0), ("pe", 1, 1), ("ont", 1, 0)])
def test_values_match_the_yardstick_whatever_the_way_in(mode, length_norm, eff_len, vb):
    t = _tables(mode)
    tb, rows = t["tb"], t["rows"]
    a_rows = t["pk"][0]
    q = _quant(tb["n_tx"], tb["lens"], length_norm=length_norm, eff_len=eff_len, vb=vb)
    import torch
    d = [torch.from_numpy(x).cuda() for x in (t["pk"][0].view(np.int32), t["pk"][1].view(np.int64), t["pk"][2].view(np.int32),
                                              np.ascontiguousarray(tb["row_off"], np.uint64).view(np.int64), np.ascontiguousarray(tb["group_off"], np.uint32).view(np.int32))]
    q.add_rows_device(*d)
    post = _em(q)
    w, pl = _yardstick(post, rows["tid"], rows["meta"], tb["row_off"], tb["group_off"])
    assert len(set(w.tolist())) > 50 and np.count_nonzero((w > 0) & (w < 1)) > 100
    todo = [(m, s) for m in ("tag", "sample") for s in (0, 1)]
    kept = {(m, s): qb.kept_of(w, pl, m, s) for m, s in todo}
    assert not np.array_equal(kept[("sample", 0)], kept[("sample", 1)]) and int(kept[("sample", 0)].sum()) < len(w)
    named = sum(1 for mine in pl[1] if mine)
    for how in HOWS:
        objs = [lib.Assign(mode=qb.MODES[m], seed=s) for m, s in todo]
        if how == "last":
            _fill_last(objs, tb)
        else:
            _fill(objs, a_rows, tb["row_off"], tb["group_off"], how)
        for (m, s), a in zip(todo, objs):
            n_out, n_named = a.finish(q)
            assert (n_out, n_named) == (int(kept[(m, s)].sum()), named), (how, m, s)
            _assert_values(a, w, kept[(m, s)], (mode, how, m, s))
            assert a._raw("next", 1, lib.C.byref(lib.BrDeviceBam())) == INVALID   # values only: no records
            assert all(v == 0 for k, v in a.stats().items() if k.startswith("bad_"))
            a.close()
    q.close()


# ---- the hand-built table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["host", "host3", "dev1", "dev3"])
def test_hand_built_table(how):
    names, lens = qb.hand_built()
    tids, meta, row_off, group_off = qb.table_of(names)
    a_rows = _packed(tids, meta)
    q = _quant(qb.HAND_N_TX, lens, length_norm=0)
    _fill([q], a_rows, row_off, group_off, "host")
    post = _em(q)
    w, pl = _yardstick(post, tids, meta, row_off, group_off)
    r5 = int(row_off[5])
    assert len(set(w[r5:r5 + 130].tolist())) > 1 and np.count_nonzero((w > 0) & (w < 1)) > 100
    for m in ("tag", "sample"):
        for seed in (0, 1, -7):
            a = lib.Assign(mode=qb.MODES[m], seed=seed)
            _fill([a], a_rows, row_off, group_off, how)
            kept = qb.kept_of(w, pl, m, seed)
            assert a.finish(q) == (int(kept.sum()), sum(1 for nm in names if nm))
            _assert_values(a, w, kept, (how, m, seed))
            w2, z2, k2 = a.values(r5 + 3, 40)   # a window of the values
            assert np.array_equal(w2, w[r5 + 3:r5 + 43]) and np.array_equal(k2, kept[r5 + 3:r5 + 43])
            assert a._raw("values", 0, len(w) + 1, None, None, None) == INVALID and a._raw("values", -1, 1, None, None, None) == INVALID
            a.close()
    q.close()


# ---- records ---------------------------------------------------------------------------------------------------------------------
def _group_off_of(recs):
    return np.asarray([a for a, _ in uc.groups_of(recs)] + [len(recs)], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _records_input(case_id):
    """(annotation, stream, ref_map, the oracle's rows, flags) of a records-in input"""
    if case_id == "pairing-dense":
        from tests import test_gpu_pairing_dense as pd
        ann, flags = pd.annotation(), {}
        stream = pd._bam_stream(pd.paired_dense_records())
        ref_map = np.zeros(1, dtype=np.int32)
    elif case_id == "spilled-cigar":
        cig, qlen, _ = long_cigar(17501)   # 70004 ops: the rewritten CIGAR spills into a CG:B,I tag again
        recs = [bamio.bam_record(b"r000", 0, 1300, [(90 << 4) | 0], 90, aux=b"NMC\x01"),
                bamio.bam_record(b"ultra", 0, 1999, cig, qlen, aux=b"NMi" + struct.pack("<i", 5)),
                bamio.bam_record(b"r01", 0, 2400, [(90 << 4) | 0], 90, aux=b"NMC\x01")]
        ann, flags, stream, ref_map = ANN, {"lr": 1}, bamio.frame(recs), np.zeros(1, dtype=np.int32)
    else:
        ann, stream, ref_map = uc.case_input(case_id)[:3]
        flags = next(c for c in ac.BAM_CASES if c.id == case_id).flags
    orc, roff, rlen = uc.oracle_bam(ann, stream, ref_map, flags)
    return ann, stream, ref_map, orc, roff, rlen, flags


def _device_records(stream, roff, rlen):
    import torch
    recs = lib.BrDeviceRecords()
    d = (torch.from_numpy(np.ascontiguousarray(stream).copy()).cuda(), torch.from_numpy(np.asarray(roff, dtype=np.int64)).cuda(),
         torch.from_numpy(np.asarray(rlen, dtype=np.int32)).cuda())
    recs.blob, recs.rec_off, recs.n_aln, recs.rec_len = d[0].data_ptr(), d[1].data_ptr(), len(rlen), d[2].data_ptr()
    return recs, d


def _assert_sampled(got, projected, kept, pl, long_reads):
    """what mode sample promises, read off the bytes: one placement a name, NH / HI / flag / MAPQ, the rest the input's"""
    out = uc.split(got)
    src = [r for r, k in zip(projected, kept) if k]
    assert len(out) == len(src)
    lead = pl[0][np.flatnonzero(kept)]
    assert len(set(lead.tolist())) == sum(1 for mine in pl[1] if mine)   # one placement a name with records
    for o, s in zip(out, src):
        f, g = bamio.record_fields(o[4:]), bamio.record_fields(s[4:])
        tags = {e[1]: e for e in qb.aux_entries(f["aux"])}
        assert struct.unpack_from("<i", f["aux"], tags[b"NH"][0] + 3)[0] == 1 and struct.unpack_from("<i", f["aux"], tags[b"HI"][0] + 3)[0] == 1
        assert f["flag"] == g["flag"] & ~0x100 and f["mapq"] == (3 if long_reads else 255) and list(tags)[-1] == b"ZW"
        for k in ("ref_id", "pos", "name", "bin", "l_seq", "mtid", "mpos", "tlen", "cigar", "seq", "qual"):
            assert np.array_equal(f[k], g[k]), k
        assert len(f["aux"]) == len(g["aux"]) + 7


RECORD_CASES = [c.id for c in ac.BAM_CASES] + ["pairing-dense", "spilled-cigar"]


@pytest.mark.parametrize("case_id", RECORD_CASES)
def test_records_equal_the_rewrite(case_id):
    ann, stream, ref_map, orc, roff, rlen, flags = _records_input(case_id)
    long_reads = bool(flags.get("lr") or flags.get("lr_hq"))
    in_recs = uc.split(stream)
    group_off = _group_off_of(in_recs)
    rows, row_off, group_off = yardstick_rows(orc, group_off)
    projected = uc.split(orc["bam_stream"])
    assert len(projected) == len(rows["tid"]) >= 1
    idx = lib.Index(ann, device=0)
    ctx = lib.Context(idx)
    recs, held = _device_records(stream, roff, rlen)
    db, cnt = ctx.project_bam_resident_kept(lib.make_config(**flags), recs, ref_map)
    assert cnt["n_rows"] == len(projected)
    q = _quant(idx.num_transcripts(), None, length_norm=0)
    q.add_last(ctx)
    sizes = (BIG, 4096, 1)
    objs = {(m, mb): lib.Assign(mode=qb.MODES[m], seed=1, long_reads=int(long_reads)) for m in ("tag", "sample") for mb in sizes}
    for a in objs.values():
        a.add_last(ctx)
    post = _em(q)
    w, pl = _yardstick(post, rows["tid"], rows["meta"], row_off, group_off)
    for m in ("tag", "sample"):
        kept = qb.kept_of(w, pl, m, 1)
        want = qb.rewrite(projected, qb.zw_of(w), kept, m, long_reads)
        for mb in sizes:
            a = objs[(m, mb)]
            assert a.finish(q)[0] == int(kept.sum())
            _assert_values(a, w, kept, (case_id, m))
            got, pieces = _drain(a, mb)
            assert got.size == want.size and np.array_equal(got, want), (case_id, m, mb)
            assert all(b <= mb or r == 1 for b, r in pieces) and (mb != 1 or len(pieces) == int(kept.sum()))
            st = a.stats()
            assert st["next_s"] > 0 and st["held_bytes"] > orc["bam_stream"].size
            a.close()
        if m == "sample":
            _assert_sampled(want, projected, kept, pl, long_reads)
            assert case_id != "adv-pe-default-22" or int(kept.sum()) < len(kept)
    if case_id == "spilled-cigar":
        assert max(len(r) for r in projected) > 65536 and any(b"CGBI" in r for r in projected)
    q.close()
    ctx.close()
    idx.close()
    del held


def test_add_last_of_a_flat_batch():
    """a flat batch call has no records: an object with records refuses it, one without takes it"""
    from bramble_amd import device
    from tests.test_gpu_quant import _batch_of
    tb = _tables("ont")["tb"]
    ann, stream, ref_map, orc, roff, rlen, flags = _records_input("adv-se-strict-21")
    idx, idx2 = lib.Index(ann, device=0), lib.Index(tb["annd"], device=0)
    ctx, ctx2 = lib.Context(idx), lib.Context(idx2)
    recs, held = _device_records(stream, roff, rlen)
    ctx.project_bam_resident_kept(lib.make_config(**flags), recs, ref_map)
    ctx2.project_batch_device(lib.make_config(**tb["flags"]), device.upload_batch(_batch_of(tb)))
    a = lib.Assign()
    a.add_last(ctx)
    assert a._raw("add_last", ctx2.h) == INVALID
    a.close()
    b = lib.Assign()
    b.add_last(ctx2)
    b.add_last(ctx)     # without records from its first add on: the rows and names only
    assert b._raw("set_param", b"mode", 1) == INVALID   # after the first add
    b.close()
    # the main route: the records are noted when they go home too, not only when they stay in HBM
    ctx.project_bam_bundle(lib.make_config(**flags), stream, roff, rlen, ref_map)
    c = lib.Assign()
    c.add_last(ctx)
    assert c.stats()["held_bytes"] > orc["bam_stream"].size
    c.close()
    for o in (ctx, ctx2, idx, idx2):
        o.close()
    del held


# ---- sizes around the tiles ----------------------------------------------------------------------------------------------------
N_SHAPED_TX = 8


def _tagged(rec, nh, hi):
    """a shaped record with the encoder's two entries behind its aux area"""
    body = rec[4:] + b"NHi" + struct.pack("<i", nh) + b"HIi" + struct.pack("<i", hi)
    return struct.pack("<I", len(body)) + body


def _shaped_table(recs):
    """every record a placement of its own on its name's one transcript"""
    group_off = _group_off_of(recs)
    names = np.repeat(np.arange(len(group_off) - 1), np.diff(group_off.astype(np.int64)))
    tids = (names % N_SHAPED_TX).astype(np.uint32)
    meta = np.full(len(recs), ROW_FIRST, dtype=np.uint32)
    row_off = np.arange(len(recs) + 1, dtype=np.uint64)
    return tids, meta, row_off, group_off


def _run_shaped(recs, how="dev1", seed=3, big_at=None):
    tids, meta, row_off, group_off = _shaped_table(recs)
    a_rows = _packed(tids, meta)
    stream = _cat(recs) if recs else np.zeros(0, np.uint8)
    q = _quant(N_SHAPED_TX, None, length_norm=0)
    objs = {m: lib.Assign(mode=qb.MODES[m], seed=seed) for m in ("tag", "sample")}
    if recs:
        _fill([q] + list(objs.values()), a_rows, row_off, group_off, how, stream)
    else:
        for a in objs.values():
            a.add_host(a_rows, np.zeros(1, np.uint64), np.zeros(1, np.uint32), stream)
    post = _em(q)
    w, pl = _yardstick(post, tids, meta, row_off, group_off)
    assert len(w) == 0 or set(np.round(w * 6).astype(int).tolist()) <= {2, 3, 6}   # a one-label class: 1 / m
    out = {}
    for m, a in objs.items():
        kept = qb.kept_of(w, pl, m, seed)
        assert a.finish(q) == (int(kept.sum()), len(group_off) - 1)
        _assert_values(a, w, kept, (len(recs), m))
        got, _ = _drain(a, BIG)
        want = qb.rewrite(recs, qb.zw_of(w), kept, m)
        assert got.size == want.size and np.array_equal(got, want), (len(recs), m)
        out[m] = kept
        a.close()
    q.close()
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8193, 70000])
def test_sizes_around_the_tiles(n):
    """around the wave (64), a block (256; 16 records of the write kernel's groups), a scan tile (2048) and, at 8 193 and 70 000,
    the three-launch scan; the names of group g are longer by g % 8 bytes, so sources and destinations take every alignment"""
    recs = [_tagged(r, 3, 1 + i % 3) for i, r in enumerate(_shaped_records(n))]
    assert n < 65 or len({len(r) % 8 for r in recs}) == 8
    kept = _run_shaped(recs, how="dev3" if n in (257, 2049) else "host" if n in (63, 8193) else "dev1")
    if n >= 63:
        assert 0 < int(kept["sample"].sum()) < n   # the yardstick drops records under this seed


def test_a_record_above_64_kib_between_two_short_ones():
    short = _shaped_records(6)
    name = b"zz_big\0"
    body = struct.pack("<iiBBHHHiiii", 0, 5, len(name), 9, 4680, 1, 0x100, 20, -1, -1, 0) + name + struct.pack("<I", (20 << 4)) + bytes(10) + bytes(20)
    body += b"XYZ" + b"a" * 70000 + b"\0"
    big = struct.pack("<I", len(body)) + body
    recs = [_tagged(r, 2, 1) for r in short[:3] + [big, big] + short[3:]]
    assert len(recs[3]) > 65536
    for how in ("host", "dev1"):
        kept = _run_shaped(recs, how=how, seed=0)
        assert int(kept["tag"].sum()) == len(recs) and int(kept["sample"][3:5].sum()) == 1   # one of the two large records stays


# ---- a regrowing arena, and the cap --------------------------------------------------------------------------------------------
def test_the_arena_grows_and_the_cap_holds():
    recs = [_tagged(r, 3, 1) for r in _shaped_records(900)]
    tids, meta, row_off, group_off = _shaped_table(recs)
    a_rows, stream = _packed(tids, meta), _cat(recs)
    rec_off = lib.Sorter.row_offsets(stream)
    ng = len(group_off) - 1
    cuts = [0, 2, 40, 300, ng]   # a small first add: the arena grows with every later one
    q = _quant(N_SHAPED_TX, None, length_norm=0)
    q.add_host(a_rows, row_off, group_off)
    a = lib.Assign()
    held = []
    for g0, g1 in zip(cuts, cuts[1:]):
        a.add_host(a_rows, row_off, group_off[g0:g1 + 1], stream, rec_off)
        held.append(a.stats()["held_bytes"])
    assert held[0] < held[1] < held[2] < held[3] and a.stats()["peak_bytes"] > held[3]   # it grew twice and more, the old beside the new
    post = _em(q)
    w, pl = _yardstick(post, tids, meta, row_off, group_off)
    a.finish(q)
    got, _ = _drain(a, 4096)
    assert np.array_equal(got, qb.rewrite(recs, qb.zw_of(w), np.ones(len(recs), np.uint8), "tag"))
    a.close()
    b = lib.Assign(max_bytes=stream.size // 2)
    k = ng // 4
    b.add_host(a_rows, row_off, group_off[:k + 1], stream, rec_off)
    bam = lib.BrDeviceBam(stream.ctypes.data, stream.size, rec_off.ctypes.data, len(rec_off) - 1)
    go = np.ascontiguousarray(group_off[k:], dtype=np.uint32)
    assert b.add_raw(bam, a_rows.ctypes.data, row_off.ctypes.data, len(a_rows), go.ctypes.data, len(go) - 1, False) == CAPACITY
    assert b.stats()["held_bytes"] > 0
    b.close()   # it can still be freed
    q.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    names, lens = qb.hand_built()
    tids, meta, row_off, group_off = qb.table_of(names)
    a_rows = _packed(tids, meta)
    n_tx = qb.HAND_N_TX
    n1, n2 = lib.C.c_int64(), lib.C.c_int64()
    recs = [_tagged(struct.pack("<I", 40) + bytes(8) + bytes([4]) + bytes(23) + b"abc\0" + bytes(4), 1, 1) for _ in range(len(tids))]
    stream = _cat(recs)
    rec_off = lib.Sorter.row_offsets(stream)
    bam = lib.BrDeviceBam(stream.ctypes.data, stream.size, rec_off.ctypes.data, len(rec_off) - 1)

    def raw(a, rows=a_rows, go=group_off, recs=None, ro=row_off):
        return a.add_raw(recs, rows.ctypes.data, ro.ctypes.data, len(rows), go.ctypes.data, len(go) - 1, False)

    def finish(a, q):
        return a._raw("finish", q.h if q is not None else None, lib.C.byref(n1), lib.C.byref(n2))
    a = lib.Assign()
    assert a._raw("set_param", b"mode", 2) == INVALID and a._raw("set_param", b"nothing", 0) == INVALID and a._raw("set_param", b"max_bytes", -1) == INVALID
    # the quantifier: before its finish, before its EM, without keep_names, with another name count, on no device at all
    early = _quant(n_tx, lens, length_norm=0)
    _fill([early], a_rows, row_off, group_off, "host")
    assert raw(a) == 0
    assert finish(a, early) == INVALID
    early.finish()
    assert finish(a, early) == INVALID and finish(a, None) == INVALID
    early.close()
    plain = lib.Quant(n_tx, lens)
    plain.set_param("length_norm", 0)
    _fill([plain], a_rows, row_off, group_off, "host")
    _em(plain)
    assert finish(a, plain) == INVALID
    plain.close()
    fewer = _quant(n_tx, lens, length_norm=0)
    fewer.add_host(a_rows, row_off, group_off[:-1])
    _em(fewer)
    assert finish(a, fewer) == INVALID
    fewer.close()
    assert a._raw("values", 0, 0, None, None, None) == INVALID   # before finish
    # a mix of adds with and without records; another row count; offsets that descend: nothing is added
    assert raw(a, recs=bam) == INVALID
    c = lib.Assign()
    short = lib.BrDeviceBam(stream.ctypes.data, stream.size, rec_off.ctypes.data, len(rec_off) - 2)
    assert raw(c, recs=short) == INVALID
    down = rec_off.copy()
    down[7] = down[9]
    assert raw(c, recs=lib.BrDeviceBam(stream.ctypes.data, stream.size, down.ctypes.data, len(down) - 1)) == INVALID
    bad_go = group_off.copy()
    bad_go[3] = bad_go[5]
    assert raw(c, go=bad_go, recs=bam) == INVALID
    assert raw(c, recs=bam) == 0 and raw(c) == INVALID
    c.close()
    # a PAIRED leader whose mate lies in the next name; a record that belongs to no placement -- from host and from device tables
    import torch
    k = len(names) // 3
    r = int(row_off[k])
    for change in ({r + 1: ROW_FIRST}, {r: int(meta[r]) & ~ROW_FIRST}, {len(meta) - 1: int(meta[len(meta) - 1]) | (1 << 25) | ROW_FIRST}):
        m2 = meta.copy()
        for at, v in change.items():
            m2[at] = v
        with pytest.raises(ValueError):
            qb.placements_of(m2, row_off, group_off)
        rows2 = _packed(tids, m2)
        d = lib.Assign()
        assert raw(d, rows=rows2) == INVALID
        t = [torch.from_numpy(x).cuda() for x in (rows2.view(np.int32), row_off.view(np.int64), group_off.view(np.int32))]
        assert d.add_raw(None, t[0].data_ptr(), t[1].data_ptr(), len(rows2), t[2].data_ptr(), len(group_off) - 1, True) == INVALID
        assert raw(d) == 0   # nothing was added by the refused ones
        d.close()
    d = lib.Assign()                  # the cut between a leader and its mate: the mate lies in the next name
    two = _packed(np.asarray([1, 1], np.uint32), np.asarray([meta[r] | (1 << 25) | ROW_FIRST, 1 << 25], np.uint32))
    assert raw(d, rows=two, go=np.asarray([0, 1, 2], np.uint32), ro=np.asarray([0, 1, 2], np.uint64)) == INVALID
    assert raw(d, rows=two, go=np.asarray([0, 2], np.uint32), ro=np.asarray([0, 2, 2], np.uint64)) == 0
    d.close()
    # the look-up meets tables that do not fit: counted, never looked up, and the object is dead afterwards
    q = _quant(n_tx, lens, length_norm=0)
    _fill([q], a_rows, row_off, group_off, "host")
    _em(q)
    other = tids.copy()
    other[int(row_off[5]) + 2] = 79     # a transcript that is not in its name's class
    other[0] = 0xfffffff0               # ... and one past every table
    e = lib.Assign()
    assert raw(e, rows=_packed(other, meta)) == 0
    assert finish(e, q) == INVALID
    st = e.stats()
    assert st["bad_transcripts"] == 2 and st["bad_names"] == st["bad_classes"] == st["bad_posteriors"] == 0
    assert e._raw("values", 0, 0, None, None, None) == INVALID and finish(e, q) == INVALID and raw(e) == INVALID
    e.close()
    f = lib.Assign()                    # name 10 has no rows in the quantifier: here it takes name 11's first row -- a name without a class
    ro2 = row_off.copy()
    ro2[11] += 1
    assert raw(f, ro=ro2) == 0
    assert finish(f, q) == INVALID and f.stats()["bad_classes"] == 1 and f.stats()["bad_transcripts"] == 0
    f.close()
    # a good object beside them: add after finish
    a.finish(q)
    assert raw(a) == INVALID and finish(a, q) == INVALID
    a.close()
    q.close()


def test_a_kept_record_without_the_encoders_entries():
    """mode sample rewrites NH and HI: a record that does not end in them is refused by next, mode tag does not look"""
    recs = list(_shaped_records(5))
    tids, meta, row_off, group_off = _shaped_table(recs)
    a_rows, stream = _packed(tids, meta), _cat(recs)
    q = _quant(N_SHAPED_TX, None, length_norm=0)
    objs = [lib.Assign(mode=0), lib.Assign(mode=1)]
    _fill([q] + objs, a_rows, row_off, group_off, "host", stream)
    _em(q)
    for a in objs:
        a.finish(q)
    assert _drain(objs[0], BIG)[0].size == stream.size + 7 * len(recs)
    assert objs[1]._raw("next", BIG, lib.C.byref(lib.BrDeviceBam())) == INVALID
    assert objs[1]._raw("values", 0, 1, None, None, None) == INVALID   # dead
    for o in objs + [q]:
        o.close()


# ---- memory ----------------------------------------------------------------------------------------------------------------------
def test_held_bytes_follow_the_device_memory_account():
    """assign.cpp's account, to the byte: the first add makes room for exactly what it brings"""
    recs = [_tagged(r, 3, 1) for r in _shaped_records(500)]
    tids, meta, row_off, group_off = _shaped_table(recs)
    a_rows, stream = _packed(tids, meta), _cat(recs)
    n, R = len(recs), int(stream.size)
    q = _quant(N_SHAPED_TX, None, length_norm=0)
    tag, sample, bare = lib.Assign(mode=0), lib.Assign(mode=1, seed=3), lib.Assign()
    assert tag.stats()["held_bytes"] == 128
    _fill([q, tag, sample], a_rows, row_off, group_off, "host", stream)
    _fill([bare], a_rows, row_off, group_off, "host")
    from_add = 128 + R + 64 + 16 * (n + 1) + 8 * (n + 1)
    assert tag.stats()["held_bytes"] == sample.stats()["held_bytes"] == from_add and bare.stats()["held_bytes"] == 128 + 16 * (n + 1)
    assert tag.stats()["peak_bytes"] >= from_add + 16 * (n + 1) + 8 * (n + 1)   # the uploaded rows and offsets of the host add
    _em(q)
    for a in (tag, sample, bare):
        K = a.finish(q)[0] if a is not bare else 0
        a.finish(q) if a is bare else None
        base = from_add if a is not bare else 128 + 16 * (n + 1)
        assert a.stats()["held_bytes"] == base + 9 * (n + 1) + (12 * (K + 1) if K else 0), a is sample
        assert a.stats()["peak_bytes"] >= a.stats()["held_bytes"] + 20 * (n + 1)
    K = sample.n_out
    assert 0 < K < n
    before = sample.stats()["held_bytes"]
    piece = sample.next_records(BIG)
    assert sample.stats()["held_bytes"] == before + int(piece.n_bytes) + 16 + 8 * (K + 1)
    for o in (tag, sample, bare, q):
        o.close()


# ---- command line ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cli_yardstick(mode, collated, vb, eff_len):
    """(w, placements) of the run of the synthetic input, from a lib.Quant fed the same rows (the command line numbers the
    transcripts in guide order)"""
    tb, rows = wide_rows(mode, guide_order=True, collated=collated)
    q = _quant(tb["n_tx"], tb["lens"], length_norm=0 if mode == "ont" else 1, vb=vb, eff_len=eff_len)
    _fill_last([q], tb)
    post = _em(q)
    w, pl = _yardstick(post, rows["tid"], rows["meta"], tb["row_off"], tb["group_off"])
    q.close()
    return w, pl


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("in")
    out = {"dir": d}
    for mode in ("pe", "ont"):
        annd, recs, stream = _inputs(mode)
        gtf = str(d / ("%s.gtf" % mode))
        bamio.write_gtf(gtf, annd)
        bam, hdr = _files(d, annd, stream, mode)
        base = [bam, "-G", gtf] + (["--lr"] if mode == "ont" else [])
        plain, qt = str(d / ("%s_plain.bam" % mode)), str(d / ("%s_plain.tsv" % mode))
        r = _run(base + ["--quant", qt], plain)
        out[mode] = {"annd": annd, "stream": stream, "gtf": gtf, "bam": bam, "hdr": hdr, "base": base, "plain": bamio.read_bam(plain),
                     "quant": open(qt, "rb").read(), "stdout": r.stdout.decode().split("\n")}
    return out


def _assert_side_file(path, main, w, pl, how, seed, long_reads):
    text, refs, s = bamio.read_bam(path)
    text0, refs0, s0 = main
    assert _strip(text) == _strip(text0) and refs == refs0
    projected = uc.split(s0)
    assert len(projected) == len(w) > 1000
    kept = qb.kept_of(w, pl, how, seed)
    want = qb.rewrite(projected, qb.zw_of(w), kept, how, long_reads)
    got = np.frombuffer(bytes(s), np.uint8)
    assert got.size == want.size and np.array_equal(got, want)
    return kept


def _assert_report(r, plain_stdout, kept, pl, how):
    out = r.stdout.decode().split("\n")
    at = out.index("[bramble] final report:")
    named = sum(1 for mine in pl[1] if mine)
    front = "[bramble] posterior BAM: %d of %d records written for %d read names (mode %s; add " % (int(kept.sum()), len(kept), named, how)
    assert out[at - 1] == "" and out[at - 2].startswith(front) and ", weigh " in out[at - 2], out[at - 2]
    assert sum(1 for l in out if l.startswith("[bramble] posterior BAM")) == 1
    if plain_stdout is not None:
        assert len(out) == len(plain_stdout) + 1 and _report(r) == [l for l in plain_stdout if l.startswith("# ")]


@pytest.mark.parametrize("how", ["tag", "sample"])
@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_cli_file_main_output_and_report(tmp_path, cli, mode, how):
    c = cli[mode]
    out, post, qt = str(tmp_path / "out.bam"), str(tmp_path / "post.bam"), str(tmp_path / "q.tsv")
    def args(post_path, seed):
        return c["base"] + ["--quant", qt, "--quant-bam", post_path] + (["--quant-bam-mode", "sample"] if how == "sample" else []) + ["--quant-seed", str(seed)]
    r = _run(args(post, 5), out)
    text, refs, s = bamio.read_bam(out)
    text0, refs0, s0 = c["plain"]
    assert _strip(text) == _strip(text0) and refs == refs0 and np.array_equal(s, s0)   # the run without the switch, but for @PG
    assert open(qt, "rb").read() == c["quant"]
    w, pl = _cli_yardstick(mode, False, 0, 0)
    kept = _assert_side_file(post, (text, refs, s), w, pl, how, 5, mode == "ont")
    _assert_report(r, c["stdout"], kept, pl, how)
    assert sorted(os.listdir(tmp_path)) == ["out.bam", "post.bam", "q.tsv"]
    # the same seed gives the same bytes; another seed another file in mode sample, the same in mode tag
    post2, post3 = str(tmp_path / "post2.bam"), str(tmp_path / "post3.bam")
    _run(args(post2, 5), str(tmp_path / "out2.bam"))
    assert bytes(bamio.read_bam(post2)[2]) == bytes(bamio.read_bam(post)[2])
    _run(args(post3, 6), str(tmp_path / "out3.bam"))
    assert (bytes(bamio.read_bam(post3)[2]) == bytes(bamio.read_bam(post)[2])) == (how == "tag")


@pytest.mark.parametrize("how", ["sam-stdin", "collate", "sort-index", "host-deflate", "vb", "every-switch"])
def test_cli_other_inputs_and_switches(tmp_path, cli, how):
    from bramble_amd import synth
    c = cli["pe"]
    out, post, qt = str(tmp_path / "out.bam"), str(tmp_path / "post.bam"), str(tmp_path / "q.tsv")
    args, stdin, collated, vb, eff, mode_word, sorted_out = [c["bam"]], None, False, 0, 0, "sample", False
    if how == "sam-stdin":
        args, stdin = ["-"], c["hdr"].encode() + synth.records_to_sam(c["stream"], c["annd"]["refnames"])
    elif how == "collate":
        args, collated = [_files(tmp_path, c["annd"], _coordinate_stream(c["stream"]), "sorted")[0], "--collate"], True
    elif how == "sort-index":
        args, sorted_out = args + ["--sort", "--write-index"], True
    elif how == "host-deflate":
        args, mode_word = args + ["--host-deflate"], "tag"
    elif how == "vb":
        args, vb = args + ["--quant-vb"], 1
    else:
        d = str(tmp_path)
        args += ["--sort", "--write-index", "--quant-vb", "--quant-eff-length", "--coverage", d + "/cov.bedgraph", "--coverage-weight", "em",
                 "--unprojected", d + "/un.bam", "--quant-bootstraps", "2"]
        vb, eff, sorted_out = 1, 1, True
    r = _run(args + ["-G", c["gtf"], "--quant", qt, "--quant-bam", post, "--quant-bam-mode", mode_word, "--quant-seed", "9"], out, stdin=stdin)
    main = bamio.read_bam(out)
    if sorted_out:   # the side file stays in the order of the unsorted output, under its header
        plain = str(tmp_path / "plain.bam")
        _run([a for a in args if a not in ("--sort", "--write-index")] + ["-G", c["gtf"], "--quant", str(tmp_path / "q2.tsv")], plain)
        unsorted = bamio.read_bam(plain)
        assert sorted(uc.split(main[2])) == sorted(uc.split(unsorted[2])) and bytes(main[2]) != bytes(unsorted[2])
        main = (unsorted[0], unsorted[1], unsorted[2])
    w, pl = _cli_yardstick("pe", collated, vb, eff)
    kept = _assert_side_file(post, main, w, pl, mode_word, 9, False)
    _assert_report(r, None, kept, pl, mode_word)
    assert not any(f.endswith(".tmp-bramble") for f in os.listdir(tmp_path))


def test_cli_a_file_that_cannot_be_written(tmp_path, cli):
    d = str(tmp_path / "out")
    os.mkdir(d)
    r = _run(cli["pe"]["base"] + ["--quant", d + "/q.tsv", "--quant-bam", d + "/no_such_dir/post.bam"], d + "/out.bam", ok=False)
    assert r.returncode == 1 and b"no_such_dir/post.bam" in r.stderr
    assert os.listdir(d) == []
