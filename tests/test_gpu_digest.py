"""GPU tests of the digest path (fithic_amd.digest, csrc/fhx_digest.hip): the written files equal the fixtures of
tests/golden/digest - step 2 made by the reference's own loop - through read() and through the command line; the bed and the
fragments equal the model's (tests/digest_model.py) byte for byte on texts built around the 16 KB blocks, around line ends inside a
motif, around headers and around batch edges, on many contigs and on dense sites; every refusal names the right line and leaves
nothing written; two runs give the same bytes; and Digest.fragments() feeds an Engine what the written file does."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import digest_model as dm
from batch_env import batch_bytes
from conftest import ROOT, bits_equal
from test_digest_host import BAD, GOOD, RUNS, _gunzip, run_bed, run_fasta, run_fragments

pytestmark = pytest.mark.gpu

BLOCK = 16384
MOTIF6 = b"AAGCTT"
MOTIF16 = b"ACGGTCATTGCAAGTC"


def gpu_files(data, sites, tmp_path, batch=None, name="genome.fa"):
    """(bed bytes, fragments bytes, Digest) of read() on the FASTA text `data`"""
    from fithic_amd import digest
    src, bed, out = str(tmp_path / name), str(tmp_path / "out.bed"), str(tmp_path / "out.gz")
    with open(src, "wb") as f:
        f.write(data)
    with batch_bytes("FHX_DG_BATCH_BYTES", batch):
        d = digest.read(src, sites)
    d.write_bed(bed)
    d.write(out)
    with open(bed, "rb") as f:
        return f.read(), _gunzip(out), d


def same_as_model(data, sites, tmp_path, batch=None):
    assert dm.refusal(data) is None
    bed, frags, d = gpu_files(data, sites, tmp_path, batch)
    want = dm.contigs(data, sites)
    assert d.names == [n for n, _, _ in want] and d.lengths.tolist() == [n for _, n, _ in want]
    contig, position = d.sites()
    assert position.tolist() == [p for _, _, cuts in want for p in cuts]
    assert contig.tolist() == [c for c, (_, _, cuts) in enumerate(want) for _ in cuts]
    assert bed == dm.bed(data, sites) and frags == dm.fragments(data, sites)
    return d


# ---- 1. goldens --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RUNS))
def test_read_writes_the_files_of_the_fixtures(name, tmp_path):
    run = RUNS[name]
    bed, frags, d = gpu_files(run_fasta(run), run["sites"], tmp_path)
    assert bed == run_bed(run) and frags == run_fragments(run)
    assert "".join("Working on %s\n" % n for n in d.names) == run["stdout"]
    assert set(d.stage_seconds()) == {"read_upload", "newline_scan", "class_pass", "sites", "sort", "fetch", "write"}


def test_command_line_writes_outfile_gz_and_prints_the_working_on_lines(tmp_path):
    run = RUNS["dg2"]
    src, out, bed = str(tmp_path / "g.fa"), str(tmp_path / "frags"), str(tmp_path / "g.bed")
    with open(src, "wb") as f:
        f.write(run_fasta(run))
    argv = [out, run["sites"][0], src, "--also", run["sites"][1], "--bed", bed]
    r = subprocess.run([sys.executable, "-m", "fithic_amd.digest"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == run["stdout"]
    assert not os.path.exists(out) and _gunzip(out + ".gz") == run_fragments(run)
    with open(bed, "rb") as f:
        assert f.read() == run_bed(run)


def test_gzipped_fasta_gives_the_plain_one_s_output(tmp_path):
    run = RUNS["dga"]
    data = gzip.compress(run_fasta(run))
    bed, frags, _ = gpu_files(data, run["sites"], tmp_path, name="genome.fa.gz")
    assert bed == run_bed(run) and frags == run_fragments(run)


# ---- 2. block and line edges -------------------------------------------------------------------------------------------------------
def _filler(n, seed=1):
    """n bases without any A: no motif of the tests lies in it"""
    rng = np.random.default_rng(seed)
    return bytes(b"CGT"[k] for k in rng.integers(0, 3, n))


def _wrap(seq, width=60, eol=b"\n"):
    return b"".join(seq[k:k + width] + eol for k in range(0, len(seq), width))


def text_with_motif_at(edge, k, inside=b"", eol=b"\n", motif=MOTIF6):
    """A FASTA whose byte offset `edge` falls behind the first k bases of a motif; `inside` (line ends) lies behind those k bases
    as well, so the edge is followed by it.  Further copies of the motif lie inside lines before and after."""
    head = b">ctg one" + eol
    body = _wrap(_filler(edge - 1200) + motif + _filler(100, 2), 60, eol)
    pad = edge - k - len(head) - len(body)                                  # one last line brings the motif to the edge
    assert len(eol) < pad < 2000
    text = head + body + _filler(pad - len(eol), 3) + eol + motif[:k]
    assert len(text) == edge
    return text + inside + motif[k:] + _filler(37, 4) + eol + _wrap(_filler(300, 5) + motif + _filler(50, 6), 60, eol)


@pytest.mark.parametrize("inside", [b"", b"\n", b"\r\n", b"\n\n\n\n"], ids=["plain", "newline", "crlf", "three_empty_lines"])
def test_motif_across_a_block_edge_at_every_split(inside, tmp_path):
    eol = b"\r\n" if inside == b"\r\n" else b"\n"
    for k in range(1, 6):
        data = text_with_motif_at(BLOCK, k, inside, eol)
        assert data[BLOCK - k:BLOCK] == MOTIF6[:k] and data[BLOCK:].startswith(inside + MOTIF6[k:])
        d = same_as_model(data, ["hindiii"], tmp_path)
        assert len(d.sites()[1]) == 3


def _header_text(where):
    """a second header that begins exactly at a block start, lies across the block edge, or ends the block (its newline is the
    block's last byte)"""
    header = b">second contig of the text\n"
    start = {"begins": BLOCK, "straddles": BLOCK - 9, "ends": BLOCK - len(header)}[where]
    first = b">first\n" + _wrap(_filler(start - 300) + MOTIF6)
    last = _filler(start - len(first) - 1, 2)[:-3] + b"AAG"                 # half a site before the header ...
    text = first + last + b"\n"
    assert len(text) == start
    return text + header + b"CTT" + _filler(50, 3) + b"\n" + _wrap(MOTIF6 + _filler(200, 4) + MOTIF6)      # ... and half behind it


@pytest.mark.parametrize("where", ["begins", "straddles", "ends"])
def test_header_at_a_block_edge_and_no_site_across_a_contig_boundary(where, tmp_path):
    data = _header_text(where)
    assert b"AAG\n>second contig of the text\nCTT" in data
    d = same_as_model(data, ["hindiii"], tmp_path)
    assert d.names == ["first", "second"] and np.bincount(d.sites()[0]).tolist() == [1, 2]


def test_contig_boundary_inside_what_would_be_a_site(tmp_path):
    data = b">a\nGGAAG\n>b\nCTTGG\n>c\nGGAAG\nCTTGG\n"
    d = same_as_model(data, ["hindiii"], tmp_path)
    assert d.sites()[0].tolist() == [2] and d.sites()[1].tolist() == [3]


def test_sixteen_bases_with_fifteen_of_forward_reach_over_short_lines(tmp_path):
    m = MOTIF16
    site = (m[:5] + b"^" + m[5:]).decode()
    data = (b">a\nTT" + m[:1] + b"\n" + m[1:8] + b"\n" + m[8:] + b"TT\n"     # 1 base, then 15 over two short lines
            b">b\n" + m[:1] + b"\n" + m[1:2] + b"\n\n" + m[2:9] + b"\r\n" + m[9:15] + b"\n" + m[15:] + b"\n"
            b">c\n" + m[:15] + b"\n>d\n" + m[15:] + b"\n>e\n" + m + m + b"\n")
    d = same_as_model(data, [site], tmp_path)
    assert d.sites()[0].tolist() == [0, 1, 4, 4] and d.sites()[1].tolist() == [7, 5, 5, 21]


# ---- 3. batch edges ------------------------------------------------------------------------------------------------------------------
def _batch_cut(data, batch):
    """where the first batch of `batch` bytes ends: behind its last newline"""
    return data.rindex(b"\n", 0, batch) + 1


@pytest.mark.parametrize("inside", [b"\n", b"\r\n", b"\n\n\n\n"], ids=["newline", "crlf", "three_empty_lines"])
def test_motif_across_a_batch_edge_at_every_split(inside, tmp_path):
    eol = b"\r\n" if inside == b"\r\n" else b"\n"
    for k in range(1, 6):
        # the batch is cut behind the newline that follows the motif's first k bases
        data = text_with_motif_at(8192 - len(eol), k, inside, eol)
        cut = _batch_cut(data, 8192)
        assert data[:cut].endswith(MOTIF6[:k] + eol) and data[cut:].lstrip(b"\r\n").startswith(MOTIF6[k:])
        d = same_as_model(data, ["hindiii"], tmp_path, batch=8192)
        assert len(d.sites()[1]) == 3


def test_sixteen_bases_across_a_batch_edge_at_every_split(tmp_path):
    site = (MOTIF16[:9] + b"^" + MOTIF16[9:]).decode()
    for k in range(1, 16):
        data = text_with_motif_at(8191, k, b"\n", b"\n", MOTIF16)
        assert data[:_batch_cut(data, 8192)].endswith(MOTIF16[:k] + b"\n")
        same_as_model(data, [site, "hindiii"], tmp_path, batch=8192)


def test_contig_over_five_batches_and_header_first_in_a_batch(tmp_path):
    rng = np.random.default_rng(9)
    seq = bytes(b"ACGT"[k] for k in rng.integers(0, 4, 5 * 8192))
    first = b">long\n" + _wrap(seq)
    # the next header is the first line of a batch: batches are cut behind the last newline before 8192 more bytes
    at, cuts = 0, []
    while len(first) - at > 8192:
        at = first.rindex(b"\n", at, at + 8192) + 1
        cuts.append(at)
    assert len(cuts) >= 5
    pad = at + 8192 - len(first)                                            # fill the last batch of the contig to its end
    first += _wrap(_filler(pad))[:pad - 1] + b"\n"
    assert len(first) == at + 8192
    data = first + b">next contig\n" + _wrap(seq[:3000]) + b">third\nGATC"
    d = same_as_model(data, ["^GATC", "A^AGCTT"], tmp_path, batch=8192)
    assert len(d.sites()[1]) > 150 and d.names == ["long", "next", "third"]
    again = same_as_model(data, ["^GATC", "A^AGCTT"], tmp_path)            # one batch
    assert np.array_equal(d.sites()[1], again.sites()[1])


def test_edge_files_in_batches(tmp_path):
    for where in ("begins", "straddles", "ends"):
        same_as_model(_header_text(where), ["hindiii"], tmp_path, batch=8192)
    for name in sorted(RUNS):
        same_as_model(run_fasta(RUNS[name]), RUNS[name]["sites"], tmp_path, batch=8192)


# ---- 4. volume and order -------------------------------------------------------------------------------------------------------------
def test_seventy_thousand_one_line_contigs(tmp_path):
    rng = np.random.default_rng(3)
    pieces = [b"GATC", b"AC", b"GGATCC", b"T", b"CTAG", b"gatcgatc"]
    pick = rng.integers(0, len(pieces), 70000)
    data = b"".join(b">c%d\n%s\n" % (k, pieces[p]) for k, p in enumerate(pick))
    bed, frags, d = gpu_files(data, ["^GATC"], tmp_path, batch=1 << 18)     # a few batches
    assert len(d.names) == 70000 and d.names[69999] == "c69999"
    assert bed == dm.bed(data, ["^GATC"]) and frags == dm.fragments(data, ["^GATC"])


def test_one_contig_of_gatc_repeated(tmp_path):
    data = b">dense\n" + _wrap(b"GATC" * 75000)
    d = same_as_model(data, ["^GATC"], tmp_path)
    assert len(d.sites()[1]) == 75000 and d.lengths.tolist() == [300000]


def test_mixed_case_n_in_the_genome_and_the_expanded_motif(tmp_path):
    rng = np.random.default_rng(4)
    seq = bytes(b"ACGTacgtNn"[k] for k in rng.integers(0, 10, 40000))
    data = b">m1\n" + _wrap(seq[:25000], 70) + b">m2 x\n" + _wrap(seq[25000:], 61, b"\r\n")
    d = same_as_model(data, ["G^ANTC"], tmp_path)
    assert len(d.sites()[1]) > 20
    same_as_model(data, ["^NNN"], tmp_path)                                  # 64 motifs, a site at nearly every base


def test_two_enzymes_with_duplicates_and_sites_at_0_and_at_length(tmp_path):
    data = b">a\nGATC" + b"ccAGATCTcc" * 30 + b"\nAGATC\n>b\n" + _wrap(b"AGATCTGATC" * 500, 57) + b">c\nGATC\n"
    d = same_as_model(data, ["bglii", "dpnii", "GATC^"], tmp_path)
    contig, position = d.sites()
    a = position[contig == 0]
    assert a[0] == 0 and a[-1] == d.lengths[0] and len(a) != len(set(a.tolist()))
    assert position[contig == 2].tolist() == [0, 4] and d.lengths[2] == 4


# ---- 5. refusals and reproducibility ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BAD))
def test_refusals_name_the_line_and_leave_nothing_written(name, tmp_path):
    from fithic_amd import _capi, digest
    text, line, why = BAD[name]
    src, out = str(tmp_path / "bad.fa"), str(tmp_path / "frags")
    with open(src, "wb") as f:
        f.write(text)
    dg = _capi.DgContext(0)
    try:
        with pytest.raises(_capi.DgRefused) as e:
            dg.digest_file(src, [("gatc", 0)])
        assert (e.value.line, e.value.why) == (line, why)
        assert dg.counts() == dict(lines=0, contigs=0, bases=0, sites=0)
    finally:
        dg.close()
    with pytest.raises(ValueError, match=r"bad\.fa, line %d: " % line):
        digest.main([out, "^GATC", src, "--bed", str(tmp_path / "bad.bed")])
    assert sorted(os.listdir(str(tmp_path))) == ["bad.fa"]


@pytest.mark.parametrize("name", sorted(GOOD))
def test_regular_text_at_the_limits_is_taken(name, tmp_path):
    same_as_model(GOOD[name], ["^A", "C^"], tmp_path)


def test_smallest_bad_line_wins_across_blocks_and_batches(tmp_path):
    from fithic_amd import _capi
    good = b">a\n" + _wrap(_filler(3 * BLOCK))
    lines = good.split(b"\n")[:-1]
    n = len(lines)
    cases = []
    for first, second, why in ((n // 5, n - 3, dm.BLANK), (n // 2, n // 2 + 400, dm.BYTES)):
        bad = list(lines)
        bad[second] = b">a"                                                  # a duplicate name, in a later block
        bad[first] = bad[first][:10] + (b" " if why == dm.BLANK else b"\x01") + bad[first][10:]
        cases.append((b"\n".join(bad) + b"\n", first + 1, why))
    bad = list(lines)
    bad[n // 3], bad[n - 2] = b">a", b"AC GT"                               # the name first, the byte in a later block
    cases.append((b"\n".join(bad) + b"\n", n // 3 + 1, dm.DUPLICATE))
    for text, line, why in cases:
        assert dm.refusal(text) == (line, why)
        src = str(tmp_path / "bad.fa")
        with open(src, "wb") as f:
            f.write(text)
        for batch in (None, 8192):
            dg = _capi.DgContext(0)
            try:
                with batch_bytes("FHX_DG_BATCH_BYTES", batch), pytest.raises(_capi.DgRefused) as e:
                    dg.digest_file(src, [("gatc", 0)])
                assert (e.value.line, e.value.why) == (line, why)
            finally:
                dg.close()


def test_two_runs_give_the_same_bytes(tmp_path):
    rng = np.random.default_rng(8)
    data = b"".join(b">k%d\n" % c + _wrap(bytes(b"ACGT"[k] for k in rng.integers(0, 4, 30000))) for c in range(4))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    one = gpu_files(data, ["^GATC", "hindiii"], tmp_path / "a")
    two = gpu_files(data, ["^GATC", "hindiii"], tmp_path / "b", batch=8192)
    assert one[0] == two[0] == dm.bed(data, ["^GATC", "hindiii"]) and one[1] == two[1]
    with open(str(tmp_path / "a" / "out.gz"), "rb") as f, open(str(tmp_path / "b" / "out.gz"), "rb") as g:
        assert f.read() == g.read()                                          # the compressed bytes too


# ---- 6. the direct path ----------------------------------------------------------------------------------------------------------------
def _one_pass(load):
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    eng = Engine(0)
    try:
        eng.configure(0, 0, None, n_bins=10, mapp_thres=1, mode="All", bias_low=0.5, bias_up=2.0)
        load(eng, tables.ChromIndex())
        eng.run_pass()
        v = eng.fetch()
        return v["p"].copy(), v["q"].copy()
    finally:
        eng.close()


def test_fragments_feed_an_engine_what_the_written_file_does(tmp_path):
    from fithic_amd import digest, tables
    rng = np.random.default_rng(12)
    data = b"".join(b">%s\n" % n + _wrap(bytes(b"ACGT"[k] for k in rng.integers(0, 4, size)))
                    for n, size in ((b"II", 90000), (b"I", 60000), (b"X", 75000)))
    src, frag_path = str(tmp_path / "g.fa"), str(tmp_path / "frags.gz")
    with open(src, "wb") as f:
        f.write(data)
    d = digest.read(src, ["^GATC"])
    d.write(frag_path)
    contig, end = d.fragment_ends()
    keep = np.flatnonzero(np.r_[True, (contig[1:] != contig[:-1]) | (end[1:] != end[:-1])])      # one locus per distinct end
    contig, end = contig[keep], end[keep]
    assert len(end) > 600 and len(d.names) == 3
    a, b = rng.integers(0, len(end), 6000), rng.integers(0, len(end), 6000)
    pairs = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    a, b = pairs[:, 0], pairs[:, 1]
    near = np.where(contig[a] == contig[b], 1 + 40000 // (1 + np.abs(end[a] - end[b]) // 50), 1)
    count = (near * rng.integers(1, 4, len(a))).astype(np.int32)

    def contacts(chroms):
        chr_id = np.array([chroms.intern("chr%d" % (k + 1)) for k in range(3)], np.int32)
        return chr_id[contig[a]], end[a], chr_id[contig[b]], end[b], count

    def from_file(eng, chroms):
        eng.load_fragments(*tables.read_fragments(frag_path, chroms), chroms.sort_rank())
        eng.load_contacts(*contacts(chroms))

    def direct(eng, chroms):
        eng.load_fragments(*d.fragments(chroms), chroms.sort_rank())
        eng.load_contacts(*contacts(chroms))

    (wp, wq), (gp, gq) = _one_pass(from_file), _one_pass(direct)
    assert len(wp) == len(a) and np.isfinite(wp).any() and (wp < 1).any()
    assert bits_equal(gp, wp) and bits_equal(gq, wq)
    chroms = tables.ChromIndex()
    for g, w in zip(d.fragments(chroms), tables.read_fragments(frag_path, tables.ChromIndex())):
        assert g.dtype == w.dtype == np.int32 and np.array_equal(g, w)
    assert chroms.names == ["chr1", "chr2", "chr3"]
