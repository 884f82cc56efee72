"""tests/name_window_cases.py without a GPU: from the builders' descriptions and the restatements alone, that the table of
tests/test_gpu_name_windows.py holds what the GPU tests rely on -- the middle add of the three starts at a non-zero alignment, row
and record byte and its first and last names have no rows; names above the small-name threshold, pooled CIGARs, UMIs, barcodes and
names without either are there, in every piece where it matters -- and that the field sort's input has two position groups with
the same (barcode, UMI) pairs and names without a UMI that the (group, length, bytes) order makes neighbours."""
import numpy as np

from tests import cells_cases as cc
from tests import dedup_cases as dc
from tests import name_window_cases as nw


def test_the_three_pieces_and_what_the_table_holds():
    t = nw.table()
    n = len(t.run)
    assert 180 <= n <= 220
    go, ro, rec = t.tb["group_off"].astype(np.int64), t.tb["row_off"].astype(np.int64), t.rec_off.astype(np.int64)
    assert len(go) == n + 1 and np.all(np.diff(go) >= 0) and np.all(np.diff(ro) >= 0) and np.all(np.diff(rec) >= 36)
    rows_of = [int(ro[go[g + 1]] - ro[go[g]]) for g in range(n)]
    assert rows_of == [len(nm["rows"]) for nm in t.run] == [len(g) for g in t.groups]
    pieces = nw.windows(t, 3)
    assert [p[0] for p in pieces] == [0, t.cuts[0], t.cuts[1]] and pieces[-1][1] == n and nw.windows(t, 1) == [(0, n)]
    c1, c2 = t.cuts
    # the middle window: a non-zero alignment, row and record byte; its edge names are empty, one of them without an alignment
    assert go[c1] > 0 and ro[go[c1]] > 0 and rec[ro[go[c1]]] > 0
    assert rows_of[c1] == 0 and rows_of[c2 - 1] == 0 and {int(go[c1 + 1] - go[c1]), int(go[c2] - go[c2 - 1])} == {0, 1}
    assert ro[go[c2]] < ro[-1] and rec[ro[go[c2]]] < t.stream.size
    umis, ucnt = dc.umis_of(t.groups)
    bcs, bcnt = cc.barcodes_of(t.groups)
    for g0, g1 in pieces:
        mine = range(g0, g1)
        assert sum(rows_of[g] > 0 for g in mine) > 20
        assert any(rows_of[g] > nw.SMALL_ROWS for g in mine)                             # a wave's name in every piece
        assert any(umis[g] is not None for g in mine) and any(bcs[g] is not None for g in mine)
        assert any(umis[g] is None and rows_of[g] for g in mine)
        r0, r1 = int(ro[go[g0]]), int(ro[go[g1]])
        ncig = t.tb["a"][r0:r1, 2] & 0xffffff
        assert int(ncig.max()) > 2 and int((ncig <= 2).sum()) > 0                       # pooled and inline CIGARs
    assert max(rows_of) == 200 and {17, 64, 65} <= set(rows_of)
    assert ucnt["no_umi"] > 5 and ucnt["too_long"] > 0 and bcnt["no_barcode"] > 20
    # every consumer has work: duplicates, molecules only the directional method joins, more per-cell groups than groups
    want = t.want
    cnt = want.counts()
    assert cnt["duplicates"] > 20 and cnt["molecules_unique"] > cnt["molecules_directional"] and cnt["cells"] >= 6 and cnt["names_multi_tx"] > 30
    plain, cell = want.dedup("directional"), want.dedup("directional", True)
    assert len(set(cell["gf"].tolist())) > len(set(plain["gf"].tolist()))
    assert len(want.placements()[1]) == n and want.stream.size == t.stream.size


def test_the_field_sort_input():
    run = nw.field_sort_run()
    groups = dc.records_of(run)
    umis, _ = dc.umis_of(groups)
    bcs, _ = cc.barcodes_of(groups)
    sigs = dc.signatures_of(groups)
    assert len(set(sigs)) == 2
    per_sig = {}
    for s, b, u in zip(sigs, bcs, umis):
        per_sig.setdefault(s, []).append((b, u))
    a, b = (sorted(v, key=lambda x: (x[0] or b"", x[1] or b"")) for v in per_sig.values())
    assert a == b                                                                        # the two groups hold the same (barcode, UMI) pairs
    assert sum(1 for x in a if x[0] is not None and x[1] is None) == 4 and sum(1 for x in a if x[0] is None) == 2
    # in (group, cell) order by (length, bytes) the names without a UMI are neighbours: two of them in every (group, cell)
    for method in ("unique", "directional"):
        rep, gf = cc.per_cell_molecules(method, groups, umis, bcs)
        assert len(set(gf.tolist())) == 6
        for g in set(gf.tolist()):
            mine = [i for i in range(len(run)) if gf[i] == g]
            empty = [i for i in mine if umis[i] is None]
            assert len(empty) == 2 and all(rep[i] == i for i in empty)                   # a molecule each
            assert len({int(rep[i]) for i in mine}) == (4 if bcs[mine[0]] is not None else 2)   # two UMIs, two names without one
