"""tests/record_route_cases.py without a GPU: its builders against cases worked out by hand, and -- from the oracle's stream and rows
alone -- what tests/test_gpu_record_consumers_routes.py relies on in its inputs: molecules that only the directional method joins,
duplicates above a tenth of the names, names without a UMI and without a barcode, cells with ambiguous names, read names whose
placements weigh differently, alignments of more than 64 rows at the dense locus, a spread of the cells' restatement over its
summation orders that is neither 0 nor loose, and runs of calls whose read names never repeat."""
import struct

import numpy as np
import pytest

from tests import bamio
from tests import record_route_cases as rr
from tests import unprojected_cases as uc


def _framed(names):
    return [struct.pack("<I", len(r)) + r for r in (bamio.bam_record(n, 0, 100 + 10 * i, [(30 << 4)], 30, aux=b"NMC\x01") for i, n in enumerate(names))]


def _names(recs):
    return [bytes(uc.name_of(r)[:-1]) for r in recs]


def test_builders_by_hand():
    recs = _framed([b"a", b"a", b"b_x", b"c", b"c", b"c", b"d"])
    assert rr.group_off_of(recs).tolist() == [0, 2, 3, 6, 7] and rr.group_off_of([]).tolist() == [0]
    assert [len(p) for p in rr.cut(recs, (2, 2, 1))] == [2, 1, 4] and [len(p) for p in rr.cut(recs, (5, 1))] == [3, 4]
    assert _names(rr.prefixed(recs, b"c7."))[:3] == [b"c7.a", b"c7.a", b"c7.b_x"]
    moved = rr.moved_off_the_annotation(recs, 2, keep_every=3)
    assert [struct.unpack_from("<i", r, 4)[0] for r in moved] == [0, 2, 2, 0, 2, 2, 0] and [len(r) for r in moved] == [len(r) for r in recs]
    stream, roff, rlen = rr.split3(recs)
    assert roff.tolist()[:2] == [4, 4 + len(recs[0])] and rlen.tolist() == [len(r) - 4 for r in recs] and rr.split3([])[1].size == 0
    from bramble_amd import lib
    off2, len2, _, used = lib.bam_split(stream)
    assert used == stream.size and np.array_equal(off2, roff) and np.array_equal(len2, rlen) and roff.dtype == np.uint64 and rlen.dtype == np.uint32
    # the decoration: the even names through the UMI plan (a name's '_' becomes '-'), the odd ones through the cells' plan; every
    # new name is one run of records, and a name of the first kind has at most one separator, one of the second two when its cell is named
    out = rr.decorate(recs)
    names = _names(out)
    runs = [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n]
    assert len(runs) == len(set(runs)) and len(out) > len(recs)
    assert [n for n in runs if n.startswith((b"a.", b"c."))] and all(n.count(b"_") <= 1 for n in runs if n.startswith((b"a.", b"c.")))
    assert all(n.count(b"_") in (1, 2) for n in runs if n.startswith((b"b-x.", b"d."))) and any(n.count(b"_") == 2 for n in runs)


@pytest.mark.parametrize("inp", rr.INPUTS, ids=[i.id for i in rr.INPUTS])
def test_inputs_hold_what_the_gpu_tests_rely_on(inp):
    annd, recs, ref_map = inp.data()
    want = inp.want()
    c = want.counts()
    post = want.posteriors(want.em_restated())
    unequal = want.names_with_unequal_weights(post)
    spread = {m: want.cells(m)[1] for m in ("uniform", "em")}
    _, kept, _ = want.assign(post, "sample")
    print("%s: %d records in, %d read names (%d with records), %d rows; molecules %d unique / %d directional, %d duplicates, %d names without UMI, "
          "%d without barcode; %d cells (%d with ambiguous names); %d names of unequal weights, sample keeps %d of %d records; %d alignments of more "
          "than 64 rows; spread uniform %.3e, em %.3e"
          % (inp.id, len(recs), c["names"], c["names_with_records"], c["rows"], c["molecules_unique"], c["molecules_directional"], c["duplicates"],
             c["no_umi"], c["no_barcode"], c["cells"], c["cells_ambiguous"], unequal, int(kept.sum()), len(kept), c["big_alignments"],
             spread["uniform"], spread["em"]))
    assert c["names"] == len(rr.group_off_of(recs)) - 1 and c["records_out"] == c["rows"] > 1000
    assert c["molecules_directional"] < c["molecules_unique"]            # directional joins molecules that unique does not
    assert c["duplicates"] > 0.1 * c["names_with_records"]
    assert c["no_umi"] > 0 and c["no_barcode"] > 0
    assert c["cells_ambiguous"] >= 8                                     # uniform and em differ from unique in at least 8 cells
    assert unequal >= 1 and 0 < int(kept.sum()) < len(kept)             # ZW and the sampled pick are not trivial
    assert all(0 < s < 1e-9 for s in spread.values())                    # the rule of tests/test_gpu_cells.py::_assert_values applies
    print("%s: spread of the quantifier's restated EM over three class orders %.3e" % (inp.id, want.em_spread()[1]))
    assert 0 < want.em_spread()[1] < 1e-9                                # and so does tests/test_gpu_quant.py::_assert_em_to
    u, m = want.cells("unique")[0], want.cells("uniform")[0]
    assert len(m["feature"]) > len(u["feature"]) and int(u["multi"].sum()) > 0
    if inp.id == "dense":
        assert c["big_alignments"] > 50
    # the decorated inputs stay the smallest that still take each route: a GPU case over them lasts a second, not ten
    n_in = len(recs)
    assert {"pairs-default": 2500 <= n_in <= 3500, "pairs-strict": 2500 <= n_in <= 3500, "dense": n_in < 1500,
            "long-ont-lr": 1000 <= n_in <= 1600, "rescue-ont-S": 1800 <= n_in <= 2600}[inp.id], n_in


def test_the_presets_of_the_pairs_differ():
    a, b = rr.BY_ID["pairs-default"].want(), rr.BY_ID["pairs-strict"].want()
    assert a.stream.size != b.stream.size


def test_the_command_lines_input_leaves_the_small_route_and_holds_copies():
    """tests/test_gpu_cli_routes.py's decorated input: one default bundle of more than 65 536 records, copies of 2 000 of its read
    names, and names without a UMI and without a barcode"""
    from tests import cells_cases as cc
    from tests import dedup_cases as dc
    from tests import route_cases as rc
    recs = rr.decorate_lightly(rr.records_of_batch(rc.cli_pairs()[1]))
    groups = [[r[4:] for r in recs[a:e]] for a, e in uc.groups_of(recs)]
    umis, ucnt = dc.umis_of(groups)
    bcs, bcnt = cc.barcodes_of(groups)
    copies = sum(1 for g in groups if b"." in g[0][32:32 + g[0][8]])
    print("%d records, %d read names (%d of them copies' names), %d without UMI, %d without barcode, %d cells"
          % (len(recs), len(groups), copies, ucnt["no_umi"], bcnt["no_barcode"], len({b for b in bcs if b})))
    assert len(recs) > rc.SMALL_N and len(groups) > 40000 and copies > 4000
    assert ucnt["no_umi"] > 100 and bcnt["no_barcode"] > 4000 and len({b for b in bcs if b}) == 12
    assert len({bytes(g[0][32:32 + g[0][8]]) for g in groups}) == len(groups)     # every name is one run of records


@pytest.mark.parametrize("name", ["short_run", "long_run", "staged_run"])
def test_runs_of_calls(name):
    run = getattr(rr, name)()
    names, sizes = set(), []
    for recs, route, params in run.calls:
        mine = set(_names(recs))
        assert not (mine & names)          # read names never repeat across the bundles of a run
        names |= mine
        sizes.append(len(recs))
    calls, lens = run.oracle()
    rows = [int(o["n_rows"]) for o, _ in calls]
    c = run.want().counts()
    print("%s: bundles of %s records, %s rows; %d names, %d molecules (directional), %d duplicates, %d cells" %
          (name, sizes, rows, c["names"], c["molecules_directional"], c["duplicates"], c["cells"]))
    assert c["names"] == sum(len(g) - 1 for _, g in calls) and c["duplicates"] > 0.1 * c["names_with_records"] and c["cells_ambiguous"] >= 8
    assert all(0 < run.want().cells(m)[1] < 1e-9 for m in ("uniform", "em")) and 0 < run.want().em_spread()[1] < 1e-9
    if name == "short_run":
        assert sizes[4] == 0 and len(calls) == 5
    if name == "long_run":
        assert rows[2] * 5 < rows[1]       # far fewer matches per record than the call before it predicts
    if name == "staged_run":
        assert len(sizes) == 5 and all(abs(s - n) <= 12 for s, n in zip(sizes, rr.STAGED_SIZES))
