"""The inputs of tests/test_gpu_name_windows.py: one table of read names that every accumulator with an add of read names takes --
Quant, Coverage (weight em), Assign, Dedup, Cells -- once as one add and once as three adds that point into the same whole tables,
so that every bias of the adds' shared front end (the names' window of row_off, the rows' window of a and cigar, the records'
window of rec_off and of the bytes) is non-zero in the middle add.  Built with the builders of dedup_cases and cells_cases alone;
tests/test_name_window_cases_cpu.py checks, from the restatements alone, that the table holds what the GPU tests rely on.

  * table(): the run (names with a barcode and a UMI, with a UMI alone, with neither; names without rows; names of 17, 64, 65 and
    200 rows; pooled CIGARs of up to 8 ops), its records, its row tables, the cuts of the three adds and the expectations (a
    record_route_cases.Expect over a stand-in for the oracle's output, made from the run's own description);
  * field_sort_run(): per-cell dedup's own corner: two position groups that hold the same barcodes and UMIs, and names without a UMI
    that the (group, length, bytes) order puts next to each other."""
import functools
import itertools

import numpy as np

from tests import cells_cases as cc
from tests import dedup_cases as dc

SMALL_ROWS = 16      # dedup_kernels.h DD_SMALL_ROWS, quant_kernels.h Q_SMALL_ROWS: above it a name's rows are a wave's work
N_TX = 200
LENS = np.asarray([2600 + 13 * (t % 17) for t in range(N_TX)], dtype=np.int64)


def _with_barcodes(run, seed=11):
    """the names of `run` that carry <name>_<UMI> re-emitted as <name>_<CB>_<UMI> over six cells, every fifth left as it is"""
    rng = np.random.default_rng(seed)
    cells = [cc._bc(rng, 8 + k % 3) for k in range(6)]
    out = []
    for i, nm in enumerate(run):
        at = nm["name"].rfind(b"_")
        name = nm["name"]
        if at >= 0 and i % 5:
            name = name[:at] + b"_" + cells[int(rng.integers(len(cells)))] + name[at:]
        out.append(dc.name_row(name, nm["rows"], nm["aux"]))
    return out


@functools.lru_cache(maxsize=None)
def run_and_cuts():
    """-> (run, (c1, c2)): the names [c1, c2) are the middle add; names c1 and c2 - 1 have no rows"""
    base = dc.base_names()                                   # names of 64, 65, 200, 17 and 16 rows and without rows among them
    mine, cells = _with_barcodes(dc.with_umis(base)), cc.dedup_run()[:90]
    names = [nm for pair in itertools.zip_longest(mine, cells) for nm in pair if nm is not None]   # interleaved: every piece holds both
    third = len(names) // 3
    empty = [dc.name_row(b"norows%d_ACGTACGT_ACGTAC" % k, []) for k in range(2)]
    run = names[:third] + empty[:1] + names[third:2 * third] + empty[1:] + names[2 * third:]
    return run, (third, 2 * third + 2)


class _Table:
    pass


@functools.lru_cache(maxsize=None)
def table():
    from tests import record_route_cases as rr
    t = _Table()
    t.run, t.cuts = run_and_cuts()
    t.groups = dc.records_of(t.run, spill_every=7)
    t.stream = dc.stream_of(t.groups)
    t.tb = dc.tables_of(t.run)
    sizes = np.asarray([len(r) + 4 for g in t.groups for r in g], dtype=np.uint64)
    t.rec_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes, dtype=np.uint64)])
    assert int(t.rec_off[-1]) == t.stream.size and len(t.rec_off) == len(t.tb["a"]) + 1
    for x in (t.stream, t.rec_off, *t.tb.values()):
        x.setflags(write=False)
    t.want = rr.Expect([(stand_in_for_the_oracle(t.run, t.tb, t.stream), t.tb["group_off"])], LENS)
    return t


def stand_in_for_the_oracle(run, tb, stream):
    """what record_route_cases.Expect reads of an oracle call, from the run's description: the rows in name order, their alignment
    (tables_of's) and their ops as the row table holds them (a row on a '-' transcript holds them reversed)"""
    ro = tb["row_off"].astype(np.int64)
    n = len(tb["a"])
    group, ops, cigar_off, minus, primary = [], [], [0], [], []
    for g, nm in enumerate(run):
        for j, (tid, pos, o, flag) in enumerate(nm["rows"]):
            m = dc.minus_row(tid, pos)
            ops += o[::-1] if m else o
            cigar_off.append(len(ops))
            group.append(g)
            minus.append(m)
            primary.append(j == 0)
    assert len(group) == n
    return {"n_rows": n, "group": np.asarray(group, dtype=np.int64), "input_index": np.searchsorted(ro, np.arange(n), side="right") - 1,
            "cigar_off": np.asarray(cigar_off, dtype=np.uint64), "cigar": np.asarray(ops, dtype=np.uint32),
            "strand": np.where(np.asarray(minus, dtype=bool), ord("-"), ord("+")), "is_paired": np.zeros(n, np.uint8),
            "same_transcript": np.zeros(n, np.uint8), "is_first": np.ones(n, np.uint8), "primary": np.asarray(primary, dtype=np.uint8),
            "tid": tb["a"][:, 0].copy(), "pos": tb["a"][:, 1].copy(), "bam_stream": stream}


def windows(t, pieces):
    """the adds as (g0, g1) over the names: the whole table, or the three pieces"""
    n = len(t.run)
    return [(0, n)] if pieces == 1 else [(0, t.cuts[0]), t.cuts, (t.cuts[1], n)]


@functools.lru_cache(maxsize=None)
def field_sort_run():
    """Two position groups (transcript 3 at 500 and at 900) that each hold the same two barcodes with the same two UMIs, twice over;
    in each group and cell two names without a UMI (<name>_<CB>_: the empty field), which the (group, length, bytes) order puts next
    to each other and which are two molecules; two names without a barcode beside them"""
    run = []
    for pos in (500, 900):
        sig = [(3, pos, dc.cig("30M"), 0)]
        for bc in (b"AAAACCCC", b"GGGGTTTT"):
            for umi in (b"ACGTAC", b"TTGGCC"):
                run += [dc.name_row(b"f%d.%d_%s_%s" % (pos, k, bc, umi), sig) for k in range(2)]
            run += [dc.name_row(b"e%d.%d_%s_" % (pos, k, bc), sig) for k in range(2)]
        run += [dc.name_row(b"p%d.%d" % (pos, k), sig) for k in range(2)]
    order = np.random.default_rng(3).permutation(len(run))
    return [run[i] for i in order]
