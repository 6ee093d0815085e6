"""CPU tests of the digest path: the plain-Python model (tests/digest_model.py) gives the outputs written out by hand below and,
for step 2, the bytes the reference's own loop left on the fixtures of tests/golden/digest (made by
tests/golden/make_golden_digest.py); parse_sites takes the four names in any case and refuses everything outside the limits; the
model refuses each reason with the right line; and the library's host writers make the two files of the fixtures."""
import gzip
import json
import os

import numpy as np
import pytest

import digest_model as dm
from conftest import GOLDEN

DG = os.path.join(GOLDEN, "digest")
with open(os.path.join(DG, "cases.json")) as _f:
    CASES = json.load(_f)
RUNS = {r["name"]: r for r in CASES["runs"]}


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def run_fasta(run):
    return _gunzip(os.path.join(DG, run["fasta"]))


def run_bed(run):
    return _gunzip(os.path.join(DG, run["bed"]))


def run_fragments(run):
    return _gunzip(os.path.join(DG, run["fragments"]))


def bed_lines(rows):
    """[(name, start, end, k)] -> the bed file"""
    return "".join("%s\t%d\t%d\tHIC_%s_%d\t0\t+\n" % (n, s, e, n, k) for n, s, e, k in rows).encode()


def frag_lines(rows):
    """[(ctr, end)] -> the fragments file"""
    return "".join("chr%d\t0\t%d\t1\t1\n" % r for r in rows).encode()


# ---- the model against expectations written out by hand --------------------------------------------------------------------------
# (text, sites, bed rows, fragment rows, stdout)
BY_HAND = {
    "hindiii_two_contigs_site_over_a_newline": (
        b">c1 some description\nGGAAG\nCTTAA\n>c2\nAAGCTT\n", ["HindIII"],
        [("c1", 0, 3, 1), ("c1", 3, 10, 2), ("c2", 0, 1, 1), ("c2", 1, 6, 2)],
        [(1, 3), (1, 10), (2, 1), (2, 6)], "Working on c1\nWorking on c2\n"),
    "gatc_site_at_0_and_motif_ending_the_contig": (
        b">a\nGATCTTGATC\n", ["^GATC"],
        [("a", 0, 0, 1), ("a", 0, 6, 2), ("a", 6, 10, 3)],
        [(1, 0), (1, 6), (1, 10)], "Working on a\n"),
    "cut_behind_the_motif_gives_a_site_at_length": (
        b">a\nGATCTTGATC\n", ["GATC^"],
        [("a", 0, 4, 1), ("a", 4, 10, 2), ("a", 10, 10, 3)],
        [(1, 4), (1, 10), (1, 10)], "Working on a\n"),
    "overlaps_all_count": (
        b">r\naaaa\n", ["A^A"],
        [("r", 0, 1, 1), ("r", 1, 2, 2), ("r", 2, 3, 3), ("r", 3, 4, 4)],
        [(1, 1), (1, 2), (1, 3), (1, 4)], "Working on r\n"),
    "n_of_the_site_is_expanded_n_of_the_genome_matches_nothing": (
        b">x\ngaatc\n>y\ngantc\n>z\nGAcTC\n", ["G^ANTC"],
        [("x", 0, 1, 1), ("x", 1, 5, 2), ("y", 0, 5, 1), ("z", 0, 1, 1), ("z", 1, 5, 2)],
        [(1, 1), (1, 5), (2, 5), (3, 1), (3, 5)], "Working on x\nWorking on y\nWorking on z\n"),
    "two_enzymes_one_duplicate": (
        b">d\naagatctt\n", ["bglii", "dpnii"],
        [("d", 0, 2, 1), ("d", 2, 2, 2), ("d", 2, 8, 3)],
        [(1, 2), (1, 2), (1, 8)], "Working on d\n"),
    "empty_contig": (
        b">e\n>f\nacgt\n", ["^GATC"],
        [("e", 0, 0, 1), ("f", 0, 4, 1)],
        [(1, 0), (2, 4)], "Working on e\nWorking on f\n"),
    "text_before_the_first_header": (
        b"GATC\n>a\nGATC\n", ["^GATC"],
        [("a", 0, 0, 1), ("a", 0, 4, 2)],
        [(1, 0), (1, 4)], "Working on a\n"),
    "crlf_line_ends": (
        b">a x\r\nGA\r\nTC\r\n", ["^GATC"],
        [("a", 0, 0, 1), ("a", 0, 4, 2)],
        [(1, 0), (1, 4)], "Working on a\n"),
    "no_final_newline": (
        b">a\nGATCGATC", ["^GATC"],
        [("a", 0, 0, 1), ("a", 0, 4, 2), ("a", 4, 8, 3)],
        [(1, 0), (1, 4), (1, 8)], "Working on a\n"),
}


@pytest.mark.parametrize("case", sorted(BY_HAND))
def test_model_gives_what_was_written_out_by_hand(case):
    text, sites, bed, frags, said = BY_HAND[case]
    assert dm.refusal(text) is None
    assert dm.bed(text, sites) == bed_lines(bed)
    assert dm.fragments(text, sites) == frag_lines(frags)
    assert dm.stdout(text, sites) == said


def test_model_sites_and_lengths():
    assert dm.contigs(b">c1 d\nGGAAG\nCTTAA\n>c2\nAAGCTT\n", ["hindiii"]) == [("c1", 10, [3]), ("c2", 6, [1])]
    assert dm.contigs(b">r\naaaa\n", ["A^A"]) == [("r", 4, [1, 2, 3])]
    assert dm.contigs(b">d\naagatctt\n", ["bglii", "dpnii"]) == [("d", 8, [2, 2])]


# ---- the fixtures: step 2 is the reference's own loop ----------------------------------------------------------------------------
def test_fixtures_cover_the_cases_they_were_made_for():
    q = run_fasta(RUNS["dgq"])
    assert not q.startswith(b">") and b"\r\n" in q and b"\n\n" in q and not q.endswith(b"\n") and b"n" in q and b"N" in q
    assert b">empty\n>two" in q and b">one first contig" in q
    assert b"AAG\nCTT" in run_fasta(RUNS["dga"])                             # a site across a line end
    frags = run_fragments(RUNS["dg2"]).splitlines()
    assert len(frags) != len(set(frags))                                     # equal sites give equal lines
    assert RUNS["dgn"]["sites"] == ["G^ANTC"]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_model_equals_the_reference_s_loop_on_the_fixtures(name):
    run = RUNS[name]
    data = run_fasta(run)
    assert dm.bed(data, run["sites"]) == run_bed(run)
    assert dm.loop(run_bed(run)) == (run_fragments(run), run["stdout"])
    assert dm.fragments(data, run["sites"]) == run_fragments(run) and dm.stdout(data, run["sites"]) == run["stdout"]


# ---- parse_sites ---------------------------------------------------------------------------------------------------------------------
def test_parse_sites_names_in_any_case_and_explicit_sites():
    from fithic_amd.digest import parse_sites
    assert parse_sites(["hindiii"]) == parse_sites(["HindIII"]) == parse_sites(["HINDIII"]) == [("aagctt", 1)]
    assert parse_sites(["MboI"]) == parse_sites(["dpnII"]) == parse_sites(["^gatc"]) == [("gatc", 0)]
    assert parse_sites(["BglII"]) == parse_sites("a^gatct") == [("agatct", 1)]
    assert parse_sites(["GATC^"]) == [("gatc", 4)]
    assert parse_sites(["G^ANTC"]) == [("gaatc", 1), ("gactc", 1), ("gagtc", 1), ("gattc", 1)]
    assert parse_sites(["hindiii", "^GATC"]) == [("aagctt", 1), ("gatc", 0)]
    assert parse_sites(["A" * 16 + "^"]) == [("a" * 16, 16)]
    assert len(parse_sites(["^NNN"])) == 64
    for sites in (["hindiii"], ["G^ANTC", "bglii"], ["^NNA"]):
        assert parse_sites(sites) == dm.motifs_of(sites)


@pytest.mark.parametrize("sites", [[], ["AAGCTT"], ["A^AG^CTT"], ["^"], ["A^" + "C" * 16], ["^NNNN"], ["^NNN", "A^A"], ["A^RGCTT"], ["ecori"],
                                   ["A^AG CTT"], [b"^GATC"], [None], ["^GA-TC"], ["^NNA", "^NNC", "^NNG", "^NNT", "^A"]])
def test_parse_sites_refuses_what_is_outside_the_limits(sites):
    from fithic_amd.digest import parse_sites
    with pytest.raises(ValueError):
        parse_sites(sites)


def test_read_refuses_bad_sites_before_any_file_is_opened():
    from fithic_amd import digest
    with pytest.raises(ValueError, match="cut site"):
        digest.read("/nonexistent/genome.fa", ["^NNNN"])


# ---- the grammar ---------------------------------------------------------------------------------------------------------------------
# name -> (text, line, reason)
BAD = {
    "nul": (b">a\nAC\x00GT\n", 2, dm.BYTES),
    "non_ascii": (b">a\nACGT\n>b\xe9\nAC\n", 3, dm.BYTES),
    "control_byte": (b">a\nACGT\nAC\x07\n", 3, dm.BYTES),
    "del": (b">a\nAC\x7fGT\n", 2, dm.BYTES),
    "cr_inside_a_line": (b">a\nAC\rGT\n", 2, dm.BYTES),
    "cr_at_the_end_of_the_file": (b">a\nACGT\r", 2, dm.BYTES),
    "blank_inside": (b">a\nACGT\nAC GT\n", 3, dm.BLANK),
    "blank_at_the_end": (b">a\nACGT \n", 2, dm.BLANK),
    "tab": (b">a\n\tACGT\n", 2, dm.BLANK),
    "blank_before_the_first_header": (b"AC GT\n>a\nACGT\n", 1, dm.BLANK),
    "long_line": (b">a\n" + b"A" * 4097 + b"\n", 2, dm.LONG_LINE),
    "long_header": (b">a\nAC\n>" + b"b" * 4096 + b"\nAC\n", 3, dm.LONG_LINE),
    "empty_name": (b">a\nAC\n>\nAC\n", 3, dm.EMPTY_NAME),
    "empty_name_blank": (b"> text\nAC\n", 1, dm.EMPTY_NAME),
    "empty_name_crlf": (b">a\r\nAC\r\n>\r\n", 3, dm.EMPTY_NAME),
    "name_star": (b">a\nAC\n>b*\n", 3, dm.NAME_CHARS),
    "name_question": (b">a?b\nAC\n", 1, dm.NAME_CHARS),
    "name_bracket": (b">a\n>b\n>c[1]\n", 3, dm.NAME_CHARS),
    "name_backslash": (b">a\\b\nAC\n", 1, dm.NAME_CHARS),
    "duplicate": (b">a x\nAC\n>b\nAC\n>a y\nAC\n", 5, dm.DUPLICATE),
    "no_header": (b"ACGT\nACGT\n", 1, dm.NO_HEADER),
    "empty_file": (b"", 1, dm.NO_HEADER),
    "name_before_byte": (b">a\n>a\nAC GT\n", 2, dm.DUPLICATE),
    "byte_before_name": (b">a\nAC GT\n>a\n", 2, dm.BLANK),
}
GOOD = {
    "line_of_4096": b">a\n" + b"A" * 4096 + b"\n",
    "line_of_4095_crlf": b">a\r\n" + b"A" * 4095 + b"\r\n",
    "tab_and_blank_in_a_header": b">a\tb c\nAC\n",
    "greater_inside_a_line": b">a\nAC>GT\n",
    "odd_names": b">a|b:c;d.e_f-g{h}~!@#$%^&()+=,'\"\nAC\n",
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_model_refuses_with_line_and_reason(name):
    text, line, why = BAD[name]
    assert dm.refusal(text) == (line, why)


@pytest.mark.parametrize("name", sorted(GOOD))
def test_model_takes_the_regular_text(name):
    assert dm.refusal(GOOD[name]) is None


# ---- the host writers of the library --------------------------------------------------------------------------------------------------
def _columns(found):
    contig = np.array([c for c, (_, _, cuts) in enumerate(found) for _ in cuts], np.int32)
    position = np.array([p for _, _, cuts in found for p in cuts], np.int32)
    return [n.encode() for n, _, _ in found], np.array([n for _, n, _ in found], np.int64), contig, position


@pytest.mark.parametrize("name", sorted(RUNS))
def test_host_writers_make_the_files_of_the_fixtures(name, tmp_path):
    from fithic_amd import _capi
    run = RUNS[name]
    names, lengths, contig, position = _columns(dm.contigs(run_fasta(run), run["sites"]))
    frags, bed = str(tmp_path / "f.gz"), str(tmp_path / "f.bed")
    _capi.dg_write_fragments(frags, lengths, contig, position)
    _capi.dg_write_bed(bed, names, lengths, contig, position)
    assert _gunzip(frags) == run_fragments(run)
    with open(bed, "rb") as f:
        assert f.read() == run_bed(run)


def test_host_writers_across_their_blocks_of_rows(tmp_path):
    """more rows than one block of 2^18, contigs without sites between contigs with many"""
    from fithic_amd import _capi
    rng = np.random.default_rng(5)
    found = []
    for c in range(40):
        k = 0 if c % 3 == 1 else int(rng.integers(1, 30000))
        found.append(("ctg%d" % c, 10 ** 6, sorted(int(v) for v in rng.integers(0, 10 ** 6 + 1, k))))
    names, lengths, contig, position = _columns(found)
    assert len(contig) + len(found) > (1 << 18)
    frags, bed = str(tmp_path / "f.gz"), str(tmp_path / "f.bed")
    _capi.dg_write_fragments(frags, lengths, contig, position, threads=4)
    _capi.dg_write_bed(bed, names, lengths, contig, position, threads=4)
    want_bed = "".join("%s\t%d\t%d\tHIC_%s_%d\t0\t+\n" % (n, s, e, n, k + 1) for n, length, cuts in found
                       for k, (s, e) in enumerate(zip([0] + cuts, cuts + [length]))).encode()
    with open(bed, "rb") as f:
        assert f.read() == want_bed
    assert _gunzip(frags) == dm.loop(want_bed)[0]
