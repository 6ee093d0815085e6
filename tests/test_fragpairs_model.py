"""CPU tests of the fragment binning: the plain-Python model (tests/fragpairs_model.py) against expectations written out by hand -
so that a failure of the GPU tests points at the device and not at the model - the model's bed route against its digest route on
the fixtures of tests/golden/digest, and the host half of fithic_amd.fragpairs (the numpy bed parser, the limits, the command
line's arguments) against the model."""
import os

import numpy as np
import pytest

import digest_model as dm
import fragpairs_model as fm
from test_digest_host import DG, RUNS, _gunzip, run_bed, run_fasta

# two contigs cut with BglII and DpnII: `a` has a site at 0 and one site twice, so rows 0 and 2 are empty fragments
GENOME = b">a first\nGATCTTAGATCTGG\n>b\nTTGATCAA\n"
SITES = ["bglii", "dpnii"]
TABLE = [(b"a", [0, 7, 7, 14]), (b"b", [2, 8])]                       # rows 0-3 and 4-5 of the fragments file


def line(n1, p1, n2, p2):
    return b"read\t%s\t%d\t+\t%s\t%d\t-\t100\n" % (n1, p1, n2, p2)


def test_table_of_the_hand_written_genome():
    assert fm.table_of_fasta(GENOME, SITES) == TABLE
    assert fm.table_of_bed(dm.bed(GENOME, SITES)) == TABLE
    assert dm.fragments(GENOME, SITES) == b"chr1\t0\t0\t1\t1\nchr1\t0\t7\t1\t1\nchr1\t0\t7\t1\t1\nchr1\t0\t14\t1\t1\nchr2\t0\t2\t1\t1\nchr2\t0\t8\t1\t1\n"


@pytest.mark.parametrize("name,p,row", [(b"a", 1, 1), (b"a", 7, 1), (b"a", 8, 3), (b"a", 14, 3), (b"b", 1, 4), (b"b", 2, 4), (b"b", 3, 5),
                                        (b"b", 8, 5)])
def test_one_an_end_an_end_plus_one_and_the_length_land_where_the_rule_says(name, p, row):
    other = (b"b", 8, 5) if row != 5 else (b"a", 1, 1)
    kept, _ = fm.pairs(line(name, p, other[0], other[1]), TABLE)
    assert kept == [(min(row, other[2]), max(row, other[2]))]
    assert row not in (0, 2)                                          # an empty fragment is never hit


def test_order_drops_and_counts():
    data = (line(b"a", 1, b"a", 8) +          # (1, 3)
            line(b"a", 14, b"a", 7) +         # given in descending order: swapped to (1, 3)
            line(b"b", 3, b"a", 7) +          # trans with the later contig first: swapped to (1, 5)
            line(b"a", 2, b"a", 7) +          # both in row 1: dropped as same-fragment
            line(b"chrM", 5, b"a", 3) +       # dropped by name
            line(b"a", 8, b"a", 1) +          # (1, 3) a third time
            line(b"b", 1, b"b", 2) +          # both in row 4
            line(b"b", 2, b"b", 8) +          # (4, 5)
            line(b"a", 14, b"b", 1))          # (3, 4)
    kept, counts = fm.pairs(data, TABLE, drop=[b"chrM"])
    assert kept == [(1, 3), (1, 3), (1, 5), (1, 3), (4, 5), (3, 4)]
    got, counts = fm.cells(data, TABLE, drop=[b"chrM"])
    assert got == [(0, 7, 0, 14, 3), (0, 7, 1, 8, 1), (0, 14, 1, 2, 1), (1, 2, 1, 8, 1)]
    assert counts == dict(lines=9, pairs=6, dropped_name=1, same_fragment=2, cells=4)
    assert fm.text(data, TABLE, drop=[b"chrM"]) == b"chr1\t7\tchr1\t14\t3\nchr1\t7\tchr2\t8\t1\nchr1\t14\tchr2\t2\t1\nchr2\t2\tchr2\t8\t1\n"
    assert fm.columns(data, TABLE, drop=[b"chrM"]) == [[0, 0, 0, 1], [7, 7, 14, 2], [0, 1, 1, 1], [14, 8, 2, 8], [3, 1, 1, 1]]


def test_a_dropped_line_is_not_read_further_and_a_dropped_contig_receives_nothing():
    data = line(b"chrM", 5, b"a", 3).replace(b"\t5\t", b"\t-5.0\t") + b"r chrM 1 + nowhere x\n" + line(b"a", 1, b"b", 1) + line(b"a", 1, b"a", 8)
    got, counts = fm.cells(data, TABLE, drop=[b"chrM", b"b"])
    assert got == [(0, 7, 0, 14, 1)] and counts == dict(lines=4, pairs=1, dropped_name=3, same_fragment=0, cells=1)


BAD = {"unknown name": (b"r a 1 + c 1", fm.NAME), "position 0": (b"r a 0 + b 1", fm.RANGE), "above the length": (b"r a 1 + b 9", fm.RANGE),
       "sign": (b"r a +1 + b 1", fm.POSITION), "point": (b"r a 1.0 + b 1", fm.POSITION), "11 digits": (b"r a 1 + b 00000000001", fm.POSITION),
       "5 tokens": (b"r a 1 + b", fm.TOKENS), "empty line": (b"", fm.TOKENS), "control byte": (b"r a 1 + b 1 \x01", fm.BYTES),
       "lone CR": (b"r a 1\r + b 1", fm.BYTES), "4097 bytes": (b"r" * 4082 + b" a 1 + b 1 - 12", fm.LONG_LINE)}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_the_model_refuses_with_the_line_number(kind):
    bad, why = BAD[kind]
    with pytest.raises(fm.Refused) as e:
        fm.pairs(line(b"a", 1, b"b", 1) * 2 + bad + b"\n" + line(b"a", 1, b"b", 1), TABLE)
    assert (e.value.why, e.value.line) == (why, 3)


def test_grammar_at_its_limits_is_taken():
    data = b"r" * 4081 + b" a 1 + b 1 - 12\n" + b"r  a\t 0000000001 +  b 8\r\n" + b"r a 1 + b 1"       # 4096 bytes; \r\n; no last newline
    assert len(data.split(b"\n")[0]) == 4096
    assert fm.cells(data, TABLE)[0] == [(0, 7, 1, 2, 2), (0, 7, 1, 8, 1)]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_bed_route_and_digest_route_give_the_same_table_on_the_fixtures(name):
    run = RUNS[name]
    assert os.path.exists(os.path.join(DG, run["bed"]))
    by_bed, by_digest = fm.table_of_bed(run_bed(run)), fm.table_of_fasta(run_fasta(run), run["sites"])
    assert by_bed == by_digest and sum(len(e) for _, e in by_bed) == run_bed(run).count(b"\n")


# ---- the host half of the module ---------------------------------------------------------------------------------------------------
def _module_table(bed, tmp_path, name="d.bed"):
    from fithic_amd import fragpairs
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(bed)
    t = fragpairs.table_of_bed(path)
    return [(n, t.ends[a:b].tolist()) for n, a, b in zip(t.names, t.first[:-1], t.first[1:])]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_numpy_bed_parser_gives_the_model_s_table(name, tmp_path):
    bed = run_bed(RUNS[name])
    assert _module_table(bed, tmp_path) == fm.table_of_bed(bed)
    with open(os.path.join(DG, RUNS[name]["bed"]), "rb") as f:
        assert _module_table(f.read(), tmp_path, "d.bed.gz") == fm.table_of_bed(bed)     # gzipped
    assert _module_table(dm.bed(GENOME, SITES)[:-1], tmp_path) == TABLE                   # no last newline


BAD_BEDS = {"name comes back": (b"a\t0\t5\tx\nb\t0\t3\tx\na\t5\t9\tx\n", 3), "first start": (b"a\t0\t5\nb\t1\t3\n", 2),
            "gap": (b"a\t0\t5\na\t6\t9\n", 2), "two tokens": (b"a\t0\t5\n\na\t5\t9\n", 2), "sign": (b"a\t0\t5\na\t5\t-9\n", 2),
            "end below start": (b"a\t0\t5\na\t5\t4\n", 2), "end beyond int32": (b"a\t0\t2147483648\n", 1),
            "the smaller line wins": (b"a\t0\t5\na\t4\t9\nb\t2\t3\n", 2)}


@pytest.mark.parametrize("kind", sorted(BAD_BEDS))
def test_bed_refusals_name_file_and_line(kind, tmp_path):
    bed, number = BAD_BEDS[kind]
    with pytest.raises(ValueError, match=r"^line %d: " % number):
        fm.table_of_bed(bed)
    with pytest.raises(ValueError, match=r"d\.bed, line %d: " % number):
        _module_table(bed, tmp_path)


def test_table_limits_are_value_errors():
    from fithic_amd import fragpairs
    fragpairs.check_limits([b"n%d" % k for k in range(4096)], (1 << 31) - 1, [b"x" * 63])
    for names, n, drop in (([b"n%d" % k for k in range(4097)], 5000, []), ([b"x" * 64], 1, []), ([b"a"], 1 << 31, []), ([b"a"], 1, [b"y" * 64])):
        with pytest.raises(ValueError):
            fragpairs.check_limits(names, n, drop)
    with pytest.raises(ValueError):
        fm.check_limits([(b"x" * 64, [1])])
    with pytest.raises(ValueError):
        fm.check_limits([(b"n%d" % k, [1]) for k in range(4097)])


def test_table_of_a_digest_is_fragment_ends():
    from fithic_amd import digest, fragpairs
    want = dm.contigs(GENOME, SITES)
    contig = np.array([c for c, (_, _, cuts) in enumerate(want) for _ in cuts], np.int32)
    position = np.array([p for _, _, cuts in want for p in cuts], np.int32)
    d = digest.Digest([n for n, _, _ in want], np.array([n for _, n, _ in want], np.int64), contig, position, {})
    t = fragpairs.table_of_digest(d)
    assert [(n, t.ends[a:b].tolist()) for n, a, b in zip(t.names, t.first[:-1], t.first[1:])] == TABLE


def test_command_line_wants_exactly_one_table_source():
    from fithic_amd import fragpairs
    for argv in (["vp", "out"], ["vp", "out", "--bed", "b", "--fasta", "f", "--re", "^GATC"], ["vp", "out", "--fasta", "f"],
                 ["vp", "out", "--bed", "b", "--re", "^GATC"]):
        with pytest.raises(SystemExit):
            fragpairs.parse_args(argv)
    args = fragpairs.parse_args(["vp", "out", "--fasta", "f", "--re", "hindiii", "--also", "^GATC", "--drop", "chrM", "--drop", "chrY"])
    assert (args.re, args.also, args.drop, args.bed) == ("hindiii", ["^GATC"], ["chrM", "chrY"], None)
