"""The inputs of tests/test_gpu_combine_shapes.py, checked without a GPU: on every shape of tests/cni_shapes.py the oracle
(oracle.combine_oracle, itself pinned to the real script's files by tests/test_combine_oracle.py) must give the closed-form result
the shape states, and the plain model of cells, components and boxes must agree with every field the oracle's text shows - or
the GPU test would compare the engine with an oracle that says nothing about the seam the shape was built for."""
import pytest

import cni_shapes as cs

_lines = {}


def oracle_lines(c, tmp_path_factory):
    if c.id not in _lines:
        from oracle import combine_oracle as co
        path = str(tmp_path_factory.mktemp("cni") / "sig.txt")
        with open(path, "w") as f:
            f.write(cs.text_of(c.rows))
        _lines[c.id] = tuple(co.combine_lines(path, cs.RES, **c.kw))
    return _lines[c.id]


@pytest.mark.parametrize("c", cs.cases(), ids=repr)
def test_oracle_gives_the_closed_form(c, tmp_path_factory):
    lines = oracle_lines(c, tmp_path_factory)
    e = c.expect
    cells, summary = cs.model(c.rows, c.kw.get("conn", 8))
    for k in ("nodes", "components", "largest"):
        if k in e:
            assert summary[k] == e[k], (c.id, k)
    if "lines" in e:
        assert len(lines) == e["lines"], c.id
    parsed = [cs.parse_line(ln) for ln in lines]
    assert len({cell for cell, _ in parsed}) == len(parsed), "a cell is written at most once"
    if "picked" in e:
        assert {cell for cell, _ in parsed} == e["picked"], c.id
    for cell, shown in parsed:                                   # the model against what the text shows
        m = cells[cell]
        assert (shown["cc"], shown["p"], shown["q"]) == (m["cc"], m["p"], m["q"]), (c.id, cell, "not the first row's values")
        assert shown["box"] == m["box"] and shown["sum_cc"] == m["sum_cc"], (c.id, cell)
        area = (m["box"][1] - m["box"][0] + 1) * (m["box"][3] - m["box"][2] + 1)
        assert shown["strong"] == m["box_cells"] / area, (c.id, cell)
        if e.get("box_is_full"):
            assert m["box_cells"] == m["component_size"], (c.id, cell)
        if "box" in e:
            assert m["box"] == e["box"], (c.id, cell)
    if "same_lines_as" in e:
        assert lines == oracle_lines(cs.case(e["same_lines_as"]), tmp_path_factory)
    if e.get("first_copy"):
        assert sorted(cells[cell]["first_row"] for cell, _ in parsed) == list(range(cs.DUP_CELLS))


def test_every_shape_of_the_list_is_there():
    ids = [c.id for c in cs.cases()]
    for stem, count in (("chain_", 2), ("comb_", 2), ("square_", 12), ("orient_", 2), ("diagonal_", 2), ("two_names", 1),
                        ("pct_", len(cs.PCT_LENGTHS) * 2 * len(cs.PCT_VALUES) * 2), ("zero_", 6), ("duplicates", 1), ("above100_", 2)):
        assert sum(1 for i in ids if i.startswith(stem)) == count, stem


def test_the_chain_is_one_dependent_sequence():
    """every cell of the chain but the first lies within one bin of the cell ranked just before it: no pick is known before the
    previous one, which is what sends cn_pick_round through thousands of rounds"""
    rows = cs.chain_rows(4096)
    qs = [r[5] for r in rows]
    assert qs == sorted(qs) and len(set(qs)) == len(qs)
    for a, b in zip(rows, rows[1:]):
        assert b[1] - a[1] == cs.RES and b[2] - a[2] == cs.RES


def test_the_comb_joins_only_through_its_spine():
    rows = cs.comb_rows()
    teeth = [r for r in rows if r[2] != cs.mid(1064)]
    _, summary = cs.model(teeth, 8)
    assert summary == dict(nodes=64 * 64, components=64, largest=64)
    keys = sorted((r[1], r[2]) for r in rows)
    for lo in range(0, 128, 2):                                   # the joining cell is the last key of its lo
        assert [k for k in keys if k[0] == cs.mid(lo)][-1] == (cs.mid(lo), cs.mid(1064))


def test_the_percent_lines_reach_both_branches_and_whole_products():
    index = {(L, p): L * p // 100 for L in cs.PCT_LENGTHS for p in cs.PCT_VALUES if p < 100}
    assert any(v <= 1 for v in index.values()) and any(v > 1 for v in index.values())
    assert any(L * p % 100 == 0 and L * p // 100 > 1 for L, p in index) and any(L * p % 100 != 0 for L, p in index)
    strict = 0
    for L in cs.PCT_LENGTHS:
        qs = cs.line_q(L, True)
        for p in cs.PCT_VALUES:
            idx = L * p // 100
            if p < 100 and idx > 1:
                bound = sorted(qs)[idx]
                strict += sum(1 for q in qs if q == bound) > 1 and cs.percent_selected(qs, p, 0) > idx + 1
    assert strict >= 5, "ties at the bound must add picks beyond the index in several runs"


def test_duplicates_cannot_align_with_the_tiles():
    rows = cs.dup_rows()
    cells, summary = cs.model(rows, 8)
    assert summary == dict(nodes=cs.DUP_CELLS, components=cs.DUP_CELLS, largest=1)
    assert 1024 % 3 and 4096 % 3                                  # sorted runs of three straddle both tile sizes
    for c in range(cs.DUP_CELLS):
        assert rows[c][:3] == rows[c + cs.DUP_CELLS][:3] == rows[c + 2 * cs.DUP_CELLS][:3]
        assert len({rows[c + m * cs.DUP_CELLS][3:] for m in range(3)}) == 3
    assert sorted(v["first_row"] for v in cells.values()) == list(range(cs.DUP_CELLS))
    order = [v["first_row"] for _, v in sorted(cells.items())]
    assert order != sorted(order)                                 # key order is not row order


def test_lattice_edges_by_hand_agree_with_the_model():
    """EDGE_EXPECT is written by hand; the model on the same cells (moved down by one: it names cells by k = bin - 1) agrees.
    Bin 0 has no k, so the model gets the cells shifted up by one bin, which keeps every relation"""
    rows = [cs.row("c", a + 1, b + 1, cc, q) for (a, b), cc, q in zip(cs.EDGE_CELLS, cs.edge_columns()[3], cs.edge_columns()[5])]
    cells, summary = cs.model(rows, 8)
    assert summary == dict(nodes=4, components=3, largest=2)
    for (a, b), want in cs.EDGE_EXPECT.items():
        m = cells[("c", a + 1, b + 1)]
        assert tuple(v - 1 for v in m["box"]) == want["box"]
        assert {k: m[k] for k in ("component_size", "box_cells", "sum_cc", "first_row")} == {k: want[k] for k in
                                                                                             ("component_size", "box_cells", "sum_cc", "first_row")}
    assert cs.make_key_is_all_ones()


def test_golden_built_rows_are_small_and_hold_every_set():
    rows = cs.golden_built_rows()
    assert len(rows) <= 1500 and {r[0] for r in rows} == {"chr2", "chr10", "chrX"}
    assert sum(1 for r in rows if r[1] > r[2]) >= 100             # rows written (hi, lo)
    assert sum(1 for r in rows if r[5] == 0.0) == 9
    cells, summary = cs.model(rows, 8)
    assert summary["largest"] == 300 and summary["nodes"] == len(rows) - 1     # one repeated cell (the diagonal set's)
