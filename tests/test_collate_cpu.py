"""--collate without a GPU: the tests' restatement of the collation C (groups of equal read names in the order of their first
mapped record, input order inside a group) on hand-made streams, the command line's usage error for several devices, and
br_collator_new without a device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tests import bamio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bramble_amd", "bin", "bramble")


def mapped_records(stream):
    """[block_size][record]... -> the mapped records (flag 0x4 clear), each with its block_size, in stream order."""
    data, out, p = bytes(stream), [], 0
    while p < len(data):
        n = struct.unpack_from("<I", data, p)[0]
        rec = data[p:p + 4 + n]
        if not (struct.unpack_from("<H", rec, 4 + 14)[0] & 0x4):
            out.append(rec)
        p += 4 + n
    return out


def read_name(rec):
    """l_read_name and the read_name bytes (NUL included) of a [block_size][record]."""
    return rec[36:36 + rec[12]]


def collate_order(recs):
    """C: the input index of every output record -- groups of equal names in the order of their first record, stable."""
    groups, first = {}, []
    for i, r in enumerate(recs):
        k = read_name(r)
        if k not in groups:
            groups[k] = []
            first.append(k)
        groups[k].append(i)
    return [i for k in first for i in groups[k]]


def collate_stream(stream):
    recs = mapped_records(stream)
    return np.frombuffer(b"".join(recs[i] for i in collate_order(recs)), dtype=np.uint8)


def coordinate_sorted(recs):
    """stable by (refID, pos), as a coordinate-sorted BAM holds them"""
    return sorted(recs, key=lambda r: struct.unpack_from("<ii", r, 4))


def _rec(name, pos, ref=0, flag=0):
    return bamio.frame([bamio.bam_record(name, ref, pos, [10 << 4], 10, flag=flag)]).tobytes()


def test_restated_collation_interleaved_mates():
    recs = [_rec(b"a", 100), _rec(b"b", 120), _rec(b"a", 300), _rec(b"c", 50), _rec(b"b", 500), _rec(b"a", 900)]
    assert collate_order(recs) == [0, 2, 5, 1, 4, 3]
    # an already collated input comes out unchanged
    again = [recs[i] for i in collate_order(recs)]
    assert collate_order(again) == list(range(len(again)))


def test_restated_collation_names_by_length_and_last_byte():
    recs = [_rec(b"read1", 1), _rec(b"read10", 2), _rec(b"read2", 3), _rec(b"read1", 4), _rec(b"read10", 5), _rec(b"read2", 6)]
    assert collate_order(recs) == [0, 3, 1, 4, 2, 5]
    names = [read_name(recs[i]) for i in collate_order(recs)]
    assert names[0] == names[1] != names[2]


def test_restated_collation_skips_unmapped():
    s = np.frombuffer(b"".join([_rec(b"x", 1), _rec(b"y", 2, flag=4), _rec(b"x", 3), _rec(b"y", 4)]), dtype=np.uint8)
    recs = mapped_records(s)
    assert len(recs) == 3 and collate_order(recs) == [0, 1, 2]


def test_coordinate_sort_is_stable():
    recs = [_rec(b"p", 10), _rec(b"q", 5), _rec(b"r", 10)]
    assert [read_name(r) for r in coordinate_sorted(recs)] == [b"q\0", b"p\0", b"r\0"]


def test_cli_collate_with_several_devices_is_a_usage_error(tmp_path):
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    out = str(tmp_path / "o.bam")
    r = subprocess.run([BIN, str(tmp_path / "missing.bam"), "-G", str(gtf), "-o", out, "--collate", "--devices", "0,0"],
                       capture_output=True, timeout=60)
    assert r.returncode == 2
    assert b"--collate" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp-bramble")


def test_collator_new_without_a_device():
    """BR_ERR_NO_DEVICE for a device that does not exist (every device, on a machine without one)."""
    from bramble_amd import lib
    L = lib.lib()
    L.br_collator_new.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.br_collator_free.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert L.br_collator_new(4096, C.byref(h)) == -2   # BR_ERR_NO_DEVICE
    assert not h.value
    assert L.br_collator_new(-1, C.byref(h)) == -2
