"""The nearby-contact merging (fithic_amd.combine / csrc/fhx_cni.hip) on the built shapes of tests/cni_shapes.py: the lines must be
the oracle's, and the fields the text does not show - components, largest_component, component_size, first_row, box_cells,
sum_cc, selected - must be the plain model's, straight from the records and the run's info.  Everything is integers, bit
patterns or text: every comparison is exact.  tests/test_cni_shapes_inputs.py checks without a GPU that the oracle gives each
shape's closed-form result, so none of these cases can pass vacuously."""
import gzip

import numpy as np
import pytest

import cni_shapes as cs

pytestmark = pytest.mark.gpu

_oracle, _model = {}, {}


def _table(c, tmp_path):
    path = str(tmp_path / (c.id + ".txt"))
    with open(path, "w") as f:
        f.write(cs.text_of(c.rows))
    return path


def _want_lines(c, path):
    if c.id not in _oracle:
        from oracle import combine_oracle as co
        _oracle[c.id] = tuple(co.combine_lines(path, cs.RES, **c.kw))
    return _oracle[c.id]


def _want_model(c):
    key = (id(c.rows), c.kw.get("conn", 8))
    if key not in _model:
        _model[key] = cs.model(c.rows, c.kw.get("conn", 8))
    return _model[key]


def _run(c, tmp_path):
    from fithic_amd import combine
    path = _table(c, tmp_path)
    names, rec, info = combine.combine_records(combine.read_significances(path, 1), cs.RES, **c.kw)
    return path, names, rec, info


def _check_records(c, names, rec, info):
    cells, summary = _want_model(c)
    assert info.rows == len(c.rows) and info.nodes == summary["nodes"], c.id
    assert info.selected == len(rec), c.id
    if c.kw.get("pct", 100) <= 100:                               # above 100 the run stops before it labels anything
        assert info.components == summary["components"] and info.largest_component == summary["largest"], c.id
    for r in rec:
        cell = (names[int(r["chr"])], int(r["n_lo"]) // cs.RES - 1, int(r["n_hi"]) // cs.RES - 1)
        m = cells[cell]
        box = tuple(int(r[k]) // cs.RES - 1 for k in ("box_min_lo", "box_max_lo", "box_min_hi", "box_max_hi"))
        got = dict(first_row=int(r["first_row"]), cc=int(r["cc"]), p=float(r["p"]), q=float(r["q"]), component_size=int(r["component_size"]),
                   box=box, box_cells=int(r["box_cells"]), sum_cc=int(r["sum_cc"]))
        assert got == m, (c.id, cell)
        assert int(r["n_lo"]) % cs.RES == 0 and int(r["n_hi"]) % cs.RES == 0


@pytest.mark.parametrize("c", cs.cases(), ids=repr)
def test_shape_gives_the_oracles_lines_and_the_models_fields(c, tmp_path):
    from fithic_amd import combine
    path, names, rec, info = _run(c, tmp_path)
    want = _want_lines(c, path)
    got = combine.format_lines(names, rec, cs.RES)
    assert len(got) == len(want) == c.expect.get("lines", len(want)), c.id
    assert tuple(got) == want, c.id
    _check_records(c, names, rec, info)
    e = c.expect
    if "min_pick_rounds" in e:
        print(c.id, "pick_rounds", info.pick_rounds)
        assert info.pick_rounds > 64 and info.pick_rounds >= e["min_pick_rounds"], "the chain must go the serial way"
    if e.get("box_is_full"):
        assert all(int(r["box_cells"]) == int(r["component_size"]) for r in rec)
    if "box" in e:
        lo = [int(rec[0][k]) // cs.RES - 1 for k in ("box_min_lo", "box_max_lo", "box_min_hi", "box_max_hi")]
        assert tuple(lo) == e["box"]
    if e.get("first_copy"):
        assert info.nodes == cs.DUP_CELLS
        assert sorted(int(r["first_row"]) for r in rec) == list(range(cs.DUP_CELLS))
        for r in rec:
            first = c.rows[int(r["first_row"])]
            assert (int(r["cc"]), float(r["p"]), float(r["q"])) == first[3:]
    if "same_lines_as" in e:
        other = cs.case(e["same_lines_as"])
        _, names2, rec2, info2 = _run(other, tmp_path)
        assert names2 == names and rec2.tobytes() == rec.tobytes() and info2.as_dict() == info.as_dict()


def test_lattice_edges_through_load():
    """bins 0 and 2^24 - 1 and chromosome id 65535 are the largest the 64-bit cell key holds (the last cell's key is all ones);
    one step further is refused, and the context takes the next valid load"""
    from fithic_amd import _capi
    chr_ids, n1, n2, cc, p, q = cs.edge_columns()
    cn = _capi.CniContext(0)
    try:
        assert cn.load(chr_ids, n1, n2, cc, p, q, cs.RES) == 4
        rec, info = cn.run(8, 100, 0, 0)
        assert (info.rows, info.nodes, info.components, info.selected, info.largest_component) == (4, 4, 3, 4, 2)
        assert sorted((int(r["n_lo"]) // cs.RES, int(r["n_hi"]) // cs.RES) for r in rec) == sorted(cs.EDGE_CELLS)
        for r in rec:
            assert int(r["chr"]) == cs.EDGE_CHR and int(r["n_lo"]) % cs.RES == 0 and int(r["n_hi"]) % cs.RES == 0      # lattice offset 0
            want = cs.EDGE_EXPECT[(int(r["n_lo"]) // cs.RES, int(r["n_hi"]) // cs.RES)]
            got = dict(component_size=int(r["component_size"]), box_cells=int(r["box_cells"]), sum_cc=int(r["sum_cc"]),
                       first_row=int(r["first_row"]),
                       box=tuple(int(r[k]) // cs.RES for k in ("box_min_lo", "box_max_lo", "box_min_hi", "box_max_hi")))
            assert got == want
        assert [int(r["component_size"]) for r in rec] == [2, 2, 1, 1]           # largest first, then by first row
        # -n 1: the pair's second cell lies within one bin of the first and is dropped; the windows reach past both ends of the lattice
        rec1, info1 = cn.run(8, 100, 1, 0)
        assert sorted(int(r["first_row"]) for r in rec1) == [0, 1, 2] and info1.selected == 3
        for bad_chr, bad_bin in ((cs.EDGE_CHR, cs.TOP + 1), (cs.EDGE_CHR + 1, cs.TOP)):
            with pytest.raises(_capi.FhxError) as err:
                cn.load([0, bad_chr], [0, 0], [cs.RES, bad_bin * cs.RES], [1, 2], [0.5, 0.5], [0.5, 0.5], cs.RES)
            assert err.value.code == _capi.FHX_ERR_UNSUPPORTED
        assert cn.load(chr_ids, n1, n2, cc, p, q, cs.RES) == 4                 # the next valid load works
        again, info2 = cn.run(8, 100, 0, 0)
        assert again.tobytes() == rec.tobytes() and info2.as_dict() == info.as_dict()
    finally:
        cn.close()


@pytest.mark.parametrize("pct", [101, 1000])
def test_percent_above_100_selects_nothing(pct, tmp_path, monkeypatch, capsys):
    """none of the reference's three branches runs (CombineNearbyInteraction.py:421, 470, 608): no record from the context, a
    header-only file from main()"""
    from fithic_amd import _capi, combine
    rows = cs.chain_rows(300)
    cn = _capi.CniContext(0)
    try:
        n = np.array([[r[1] + cs.RES // 2, r[2] + cs.RES // 2] for r in rows], np.int64)
        assert cn.load(np.zeros(len(rows), np.int32), n[:, 0], n[:, 1], [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows],
                       cs.RES) == 300
        rec, info = cn.run(8, pct, 1, 0)
        assert len(rec) == 0 and info.selected == 0 and info.nodes == 300
        rec, info = cn.run(8, 100, 1, 0)                          # the same context still merges at -p 100
        assert info.selected == 150 and info.components == 1
    finally:
        cn.close()
    src, out = str(tmp_path / "sig.txt.gz"), str(tmp_path / "merged.gz")
    with gzip.open(src, "wt") as f:
        f.write(cs.text_of(rows))
    monkeypatch.setattr("sys.argv", ["CombineNearbyInteraction.py", "-i", src, "-o", out, "-r", str(cs.RES), "-p", str(pct), "-n", "1"])
    combine.main()
    with gzip.open(out, "rt") as f:
        assert f.read() == combine.HEADER
