"""The yardstick of --unprojected / "keep_unprojected", shared by tests/test_unprojected_cpu.py and
tests/test_gpu_unprojected.py: the oracle's complement.  Record i of an input stream is unprojected when i is not among the
input indices of the oracle's rows; in scope name, when no record of its read name is.  Nothing here comes from a device run."""
import functools
import struct

import numpy as np

from oracle import oracle_binding as ob
from tests import adversarial as adv
from tests import alphabet_cases as ac

SCOPES = {"record": 1, "name": 2}
# the inputs in which at least 85 read names are partly projected (the table of the feature's issue, from the oracle)
PARTIAL = ("adv-pe-default-22", "adv-mm-fr-23", "adv-near-default-24", "adv-near-rf-24", "adv-pe-override-22", "dense-pe-default-25")


def split(stream):
    """[block_size][record]... -> the records, each with its block_size word"""
    data, out, p = bytes(stream), [], 0
    while p < len(data):
        n = struct.unpack_from("<I", data, p)[0]
        out.append(data[p:p + 4 + n])
        p += 4 + n
    assert p == len(data)
    return out


def name_of(rec):
    return rec[36:36 + rec[12]]


def groups_of(recs):
    """the runs of equal read names of a collated record list: [(first, end)]"""
    out, a = [], 0
    for i in range(1, len(recs) + 1):
        if i == len(recs) or name_of(recs[i]) != name_of(recs[a]):
            out.append((a, i))
            a = i
    return out


def yardstick(recs, input_index, scope):
    """recs: the mapped records of a name-collated stream; input_index: the input record of every row the oracle emitted.
    -> (stream uint8, row_off uint64 [n + 1], stats[0..5] as br_ctx_unprojected_stats counts them)"""
    projected = np.zeros(len(recs), dtype=bool)
    projected[np.asarray(input_index, dtype=np.int64)] = True
    groups = groups_of(recs)
    none = sum(1 for a, e in groups if not projected[a:e].any())
    part = sum(1 for a, e in groups if projected[a:e].any() and not projected[a:e].all())
    keep = ~projected
    if scope == "name":
        for a, e in groups:
            if projected[a:e].any():
                keep[a:e] = False
    chosen = [recs[i] for i in np.nonzero(keep)[0]]
    off = np.zeros(len(chosen) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in chosen], dtype=np.uint64)
    stream = np.frombuffer(b"".join(chosen), dtype=np.uint8)
    return stream, off, [len(recs), len(chosen), int(stream.size), len(groups), none, part]


def oracle_bam(ann, stream, ref_map, flags):
    from bramble_amd import lib
    roff, rlen, _, used = lib.bam_split(stream)
    assert used == stream.size
    orc, _, _, _ = ob.run_bam(ob.OracleIndex(ann), ob.make_flags(**flags), stream, roff, rlen, ref_map)
    return orc, roff, rlen


@functools.lru_cache(maxsize=None)
def case_input(case_id):
    """(annotation, stream, ref_map, oracle rows, rec_off, rec_len, the records) of a tests/alphabet_cases.py BAM input"""
    case = next(c for c in ac.BAM_CASES if c.id == case_id)
    ann = case.annotation()
    stream = adv.bam_stream(case.records())
    ref_map = np.arange(len(ann["refnames"]), dtype=np.int32)
    orc, roff, rlen = oracle_bam(ann, stream, ref_map, case.flags)
    return ann, stream, ref_map, orc, roff, rlen, split(stream)
