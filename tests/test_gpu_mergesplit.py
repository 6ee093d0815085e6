"""GPU tests of the per-chromosome merge-filter path (fithic_amd.mergefilter_parallel, csrc/fhx_sigsplit.inc): the tree equals the
real script's after decompression (tests/golden/mergesplit), job files byte for byte; the subsets equal the model's
(tests/mergesplit_model.py) on texts built round the 16 KB scan blocks, round batch edges and round the 256-record rounds of
the gather, with names that come and go between batches, at 0 % and 100 % kept, with one name and with 4096; every refusal names
the right line; two runs give the same bytes; the subsets are the one-file selection told apart by chromosome; and the handle
still makes the selection's and the track's golden bytes after a split."""
import gzip
import os
import subprocess
import sys

import pytest

import mergefilter_model as mm
import mergesplit_model as sm
from batch_env import batch_bytes
from conftest import ROOT
from test_gpu_mergefilter import BLOCK
from test_mergesplit_host import GOOD, HEADER, MODEL_REFUSALS, RUNS, run_input, run_tree

pytestmark = pytest.mark.gpu

KEPT, DROPPED = b"1.000000e-03", b"9.000000e-01"                      # at fdr = 0.05
STAGES = ["read_upload", "newline_scan", "names_select", "sort_gather", "copy_out"]


def row(name, k, q=KEPT, pad=0, other=None):
    """one row of chromosome `name` (field 3: `other` or the same) whose field 7 is q; `pad` more bytes in the trailing column"""
    sep = [b"\t", b" ", b" \t"][k % 3]
    return name + b"\t" + sep.join([b"%d" % (5000 * (k % 900) + 2500), other or name, b"%d" % (5000 * (k % 900 + k % 7 + 3) + 2500), b"%d" % (5 + k % 90),
                                    b"1.000000e-09", q, b"1.000000", b"2.5" + b"0" * pad]) + b"\n"


def gpu_split(data, fdr, tmp_path, batch=None):
    """{name: subset} as the device path makes it for `data`, after checking its counts"""
    from fithic_amd import mergefilter_parallel as mp
    src = str(tmp_path / "sig.txt")
    with open(src, "wb") as f:
        f.write(data)
    with batch_bytes("FHX_MS_BATCH_BYTES", batch):
        got = mp.split(src, fdr)
    plain = gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data
    assert got.n_lines == len(mm.lines_of(plain)) and list(got.stage_seconds()) == STAGES
    assert got.chromosomes == [c.decode("latin-1") for c in sm.chromosomes(plain)]
    out = {}
    for c in got.chromosomes:
        text = got.subset_text(c)
        assert isinstance(text, bytes) and got.n_kept(c) == text.count(b"\n") == got.selection(c).n_kept
        out[c.encode("latin-1")] = text
    return out


def check(data, fdr, tmp_path, batch=None):
    """device == model; -> the subsets"""
    want = sm.split(data, fdr)
    got = gpu_split(data, fdr, tmp_path, batch)
    assert sorted(got) == sorted(want)
    for c in want:
        assert got[c] == want[c], c
    return got


# ---- 1. goldens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RUNS))
def test_device_path_makes_the_script_s_subsets_and_merged_files(name, tmp_path):
    from fithic_amd import combine, mergefilter_parallel as mp
    run, tree = RUNS[name], run_tree(RUNS[name])
    src = str(tmp_path / "sig.txt")
    with open(src, "wb") as f:
        f.write(run_input(run))
    got = mp.split(src, run["fdr"])
    assert got.chromosomes == [c.decode() for c in sorted(tree)]
    for c, t in tree.items():
        one = got.selection(c.decode())
        assert got.subset_text(c.decode()) == t["subset"] == one.subset_text()
        out = str(tmp_path / ("merged_%s.gz" % c.decode()))
        combine.write_merged(out, *one.merged(run["res"]), run["res"])
        with gzip.open(out, "rb") as f:
            assert f.read() == t["merged"], c


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("name", sorted(RUNS))
def test_command_line_writes_the_script_s_tree(name, merge, tmp_path):
    run, tree = RUNS[name], run_tree(RUNS[name])
    gzipped = name in ("msa", "msu_5")
    src = "sig.gz" if gzipped else "sig.txt"
    with open(str(tmp_path / src), "wb") as f:
        f.write(gzip.compress(run_input(run)) if gzipped else run_input(run))
    argv = [src, str(run["res"]), run["outdir"], run["fdr"], run["utilityfolder"]] + (["--merge"] if merge else [])
    r = subprocess.run([sys.executable, "-m", "fithic_amd.mergefilter_parallel"] + argv, cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path / run["outdir"]
    assert sorted(os.listdir(out)) == sorted(c.decode() for c in tree)                      # chromosomes.used is not left behind
    for c, t in tree.items():
        c = c.decode()
        files = ["fithic_%s.job" % c, "subset_fithic_%s.gz" % c] + (["postmerged_fithic_%s.gz" % c] if merge else [])
        assert sorted(os.listdir(out / c)) == sorted(files)
        with gzip.open(str(out / c / ("subset_fithic_%s.gz" % c)), "rb") as f:
            assert f.read() == t["subset"]
        with open(str(out / c / ("fithic_%s.job" % c)), "rb") as f:
            assert f.read() == t["job"].encode()
        if merge:
            with gzip.open(str(out / c / ("postmerged_fithic_%s.gz" % c)), "rb") as f:
                assert f.read() == t["merged"]


# ---- 2. block and batch edges, names that come and go --------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 9, -1])
def test_the_chromosome_changes_at_a_16_kb_edge(at, tmp_path):
    """at every 16 KB edge a line of a NEW chromosome starts at the edge, straddles it, or starts one byte behind it (the newline
    before it is the block's first byte); kept and dropped lines alternate round it"""
    buf = HEADER
    for k in range(1, 5):
        edge, name, new = k * BLOCK, b"chr%d" % k, b"chr%d" % (k + 1)
        n = 0
        while len(buf) < edge - 600:
            buf += row(name, n, KEPT if n % 3 else DROPPED)
            n += 1
        line = row(new, k)
        buf += row(name, n, DROPPED if k % 2 else KEPT, pad=edge - at - len(buf) - len(row(name, n))) + line
        assert buf[edge - at:].startswith(line)                       # byte `at` of the line is the first byte of the block
    got = check(buf + row(b"chr5", 1) * 3, "0.05", tmp_path)
    assert all(got[b"chr%d" % k] for k in range(1, 6))


def names_text():
    """batches of 8192 bytes: chrA only in the first, with its last line ending exactly at byte 8192; chrB first seen in the second,
    at its first byte; chrC in the first and the third; chrD only in trans rows of the second"""
    buf, n = HEADER, 0
    while len(buf) < 8192 - 400:
        buf += row(b"chrC" if n % 5 == 0 else b"chrA", n, KEPT if n % 2 else DROPPED)
        n += 1
    buf += row(b"chrA", n, KEPT, pad=8192 - len(buf) - len(row(b"chrA", n)))
    assert len(buf) == 8192
    k = 0
    while len(buf) < 2 * 8192 - 400:
        buf += row(b"chrB", k, DROPPED if k % 4 == 0 else KEPT)
        if k % 9 == 0:
            buf += row(b"chrD", k, KEPT, other=b"chrB")
        k += 1
    buf += row(b"chrB", 1, pad=2 * 8192 - len(buf) - len(row(b"chrB", 1)))
    return buf + b"".join(row(b"chrC" if k % 2 else b"chrB", k) for k in range(40))


def test_names_first_seen_in_a_later_batch_and_seen_only_in_an_earlier_one(tmp_path):
    data = names_text()
    assert data[8192 - 1:8192 + 5] == b"\nchrB\t" and data[2 * 8192 - 1:2 * 8192] == b"\n" and len(data) > 2 * 8192 + 2000
    got = check(data, "0.05", tmp_path, 8192)
    assert got[b"chrA"] and got[b"chrB"] and got[b"chrC"] and got[b"chrD"] == b"" == got[b"chr1"]
    assert got == check(data, "0.05", tmp_path) == check(data, "0.05", tmp_path, 2 * BLOCK - 100)


def test_a_gzipped_input_goes_through_the_host_inflate(tmp_path):
    data = names_text()
    assert gpu_split(gzip.compress(data), "0.05", tmp_path, 8192) == sm.split(data, "0.05")


# ---- 3. keep patterns and name patterns -------------------------------------------------------------------------------------
def test_nothing_kept_everything_kept_only_a_header_and_no_text(tmp_path):
    body = b"".join(row(b"chr%d" % (1 + k % 3), k, b"%d.000000e-%02d" % (1 + k % 9, 1 + k % 5)) for k in range(700))     # three blocks
    got = check(HEADER + body, "0", tmp_path)
    assert got == {b"chr1": b"", b"chr2": b"", b"chr3": b""}
    got = check(HEADER + body, "5", tmp_path)
    assert sum(len(v) for v in got.values()) == len(body)
    assert check(HEADER + body[:-1], "5", tmp_path, 8192) == got                             # the newline the last line lacked
    assert check(HEADER, "0.05", tmp_path) == {b"chr1": b""} == check(HEADER[:6], "0.05", tmp_path)
    assert check(b"", "0.05", tmp_path) == {}


def test_30000_lines_interleaved_line_by_line(tmp_path):
    """24 chromosomes in turn: every record is its own run before the sort, and every wave holds every name"""
    names = [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"chrY"]
    data = HEADER + b"".join(row(names[k % 24], k, KEPT if k % 7 else DROPPED) for k in range(30000))
    got = check(data, "0.05", tmp_path)
    assert len(got) == 24 and min(v.count(b"\n") for v in got.values()) > 1000


def test_one_chromosome_on_every_line(tmp_path):
    data = b"".join(row(b"chr7", k, KEPT if k % 3 else DROPPED) for k in range(20000))
    got = check(data, "0.05", tmp_path)
    assert list(got) == [b"chr7"] and got[b"chr7"].count(b"\n") > 13000


@pytest.mark.parametrize("lead", [0, 1, 37])
def test_64_consecutive_lines_bring_64_new_names(lead, tmp_path):
    """one wave meets 64 names it has to post one by one (`lead` lines shift them across the waves)"""
    data = row(b"old", 0) * lead + b"".join(row(b"n%d_x" % k, k) for k in range(64)) + row(b"old", 1) * 200 + b"".join(row(b"n%d_x" % k, k + 1) for k in range(64))
    got = check(data, "0.05", tmp_path)
    assert len(got) == 65 and all(v.count(b"\n") == 2 for c, v in got.items() if c not in (b"old", b"n0_x" if not lead else b""))


def many_names(n):
    return b"".join(b"n%d\t1 n%d 2 3 4 %s\n" % (k, k, KEPT if k % 2 else DROPPED) for k in range(n))


def test_4096_names_are_taken_and_one_more_is_refused_without_a_line_number(tmp_path):
    from fithic_amd import _capi
    got = check(many_names(4096) + many_names(4096), "0.05", tmp_path)
    assert len(got) == 4096 and got[b"n4095"] == b"n4095\t1 n4095 2 3 4 %s\n" % KEPT * 2 and got[b"n0"] == b""
    assert check(many_names(4096), "0.05", tmp_path, 8192) == {c: v[:len(v) // 2] for c, v in got.items()}
    for batch in (None, 8192):
        assert refusal_of(many_names(4097), tmp_path, batch) == (_capi.MS_NAMES, 0)
        # a bad line is reported with its number although the table is full before it, and although it comes batches later
        assert refusal_of(many_names(4200) + b"x 1 2 3 4 5 6 7\n" + many_names(10), tmp_path, batch) == (_capi.MS_NAME_TAB, 4201)
    with pytest.raises(mm.Refused) as e:
        sm.split(many_names(4200) + b"x 1 2 3 4 5 6 7\n", "0.05")
    assert (e.value.why, e.value.line) == (sm.NAME_TAB, 4201)


def test_sorted_runs_cross_the_256_record_rounds(tmp_path):
    """kept lines per chromosome 255, 257, 1, 511, 256: the runs of the sorted records start and end inside, at and across the
    rounds of the gather, from interleaved lines"""
    want = {b"a": 255, b"b": 257, b"c": 1, b"d": 511, b"e": 256}
    left, lines, k = dict(want), [], 0
    while any(left.values()):
        for c in sorted(left):
            if left[c]:
                left[c] -= 1
                lines.append(row(c, k))
                if k % 3 == 0:
                    lines.append(row(c, k, DROPPED))
                k += 1
    got = check(HEADER + b"".join(lines), "0.05", tmp_path)
    assert {c: got[c].count(b"\n") for c in want} == want
    assert check(HEADER + b"".join(lines), "0.05", tmp_path, 8192) == got


def test_the_longest_line_beside_the_shortest_in_one_round(tmp_path):
    shortest = b"a\t1 a 2 3 4 %s\n" % KEPT
    longest = b"a\t1 a 2 3 4 %s " % KEPT + b"x" * (4096 - 25) + b"\n"
    assert len(longest) == 4097 and len(shortest) == 25
    data = HEADER + (shortest * 3 + longest + shortest) * 40 + b"b\t1 b 2 3 4 %s\n" % KEPT + longest[:-1]
    got = check(data, "0.05", tmp_path)
    assert got[b"a"].count(b"\n") == 201 and got[b"a"].endswith(longest) and len(got[b"b"]) == 25
    assert check(data, "0.05", tmp_path, 3 * 4097) == got


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def refusal_of(data, tmp_path, batch=None):
    from fithic_amd import _capi, mergefilter as mf
    src = str(tmp_path / "bad.txt")
    with open(src, "wb") as f:
        f.write(data)
    ms = _capi.MsContext(0)
    try:
        with batch_bytes("FHX_MS_BATCH_BYTES", batch), pytest.raises(_capi.MsRefused) as e:
            ms.split_file(src, b"0.05", mf.key_bound("0.05"), True)
        assert ms.split_counts() == dict(lines=0, kept=[], bytes=[]) and ms.split_names() == []
        return e.value.why, e.value.line
    finally:
        ms.close()


@pytest.mark.parametrize("kind", sorted(MODEL_REFUSALS))
def test_a_bad_line_is_refused_with_its_line_number(kind, tmp_path):
    bad, why = MODEL_REFUSALS[kind]
    data = HEADER + GOOD * 400 + bad + b"\n" + GOOD * 50 + b"chr1 x\n"   # line 402 lies in the second 16 KB block; a later bad line
    assert len(HEADER + GOOD * 400) > BLOCK
    with pytest.raises(mm.Refused) as e:
        sm.split(data, "0.05")
    assert (e.value.why, e.value.line) == (why, 402)
    assert refusal_of(data, tmp_path) == (why, 402)


def test_line_1_is_held_to_the_rules_for_token_1_only(tmp_path):
    assert check(b"chr7\tany | thing, at all\n" + GOOD, "0.05", tmp_path) == {b"chr7": b"", b"chr1": GOOD}
    assert check(b"chr7\t\n" + GOOD[:-1], "0.05", tmp_path) == {b"chr7": b"", b"chr1": GOOD}
    for first, why in ((b"chr7 x", sm.NAME_TAB), (b"", sm.NAME_TAB), (b"chr7", sm.NAME_TAB), (b"01\tx", sm.NAME_NUMERIC), (b"a/b\tx", sm.NAME_BYTES),
                       (b"c" * 64 + b"\tx", sm.NAME), (b"chr7\t\x01", mm.BYTES), (b"c\t" + b"h" * 4095, mm.LONG_LINE)):
        assert refusal_of(first + b"\n" + GOOD, tmp_path) == (why, 1), first
    assert refusal_of(b"chr7", tmp_path) == (sm.NAME_TAB, 1)


def test_a_refusal_in_the_second_batch_leaves_nothing(tmp_path):
    from fithic_amd import mergefilter_parallel as mp
    data = HEADER + GOOD * 200 + b"chr1\t5 01 7 3 4 1.000000e-03\n" + GOOD * 5
    assert len(HEADER + GOOD * 200) > 8192 and sm.split(HEADER + GOOD * 100, "0.05")[b"chr1"]
    assert refusal_of(data, tmp_path, 8192) == (sm.NAME_NUMERIC, 202)
    src, out = str(tmp_path / "bad.txt"), tmp_path / "out"
    with batch_bytes("FHX_MS_BATCH_BYTES", 8192):
        with pytest.raises(ValueError, match="line 202.*compare as a number.*The reference accepts this"):
            mp.split(src, "0.05")
        with pytest.raises(ValueError, match="line 202"):
            mp.main([src, "5000", str(out), "0.05", "--merge"])
    with pytest.raises(ValueError, match="fdr"):
        mp.main([src, "5000", str(out), "5%"])
    assert not out.exists()


# ---- 5. the same bytes, and the same rows as the one-file path ----------------------------------------------------------------
def test_two_runs_give_the_same_bytes(tmp_path):
    data = run_input(RUNS["msu_5"]) + names_text()[len(HEADER):]
    first = gpu_split(data, "5", tmp_path)
    assert first == gpu_split(data, "5", tmp_path) == gpu_split(data, "5", tmp_path, 8192) == sm.split(data, "5")


def test_the_subsets_are_the_one_file_selection_told_apart_by_chromosome(tmp_path):
    from fithic_amd import mergefilter
    names = [b"chr1", b"chr2", b"chrX", b"2L"]
    data = HEADER + b"".join(b"\t".join(row(names[(k * 7) % 4], k, KEPT if k % 5 else DROPPED).split()) + b"\n" for k in range(3000))
    src = str(tmp_path / "sig.txt")
    got = gpu_split(data, "0.05", tmp_path)
    whole = mergefilter.select(src, "0.05").subset_text().splitlines(keepends=True)
    assert sorted(b"".join(got.values()).splitlines(keepends=True)) == sorted(whole) and len(whole) == 2400
    for c in names:
        assert got[c] == b"".join(line for line in whole if line.split(b"\t")[0] == c)


def test_a_split_leaves_the_selection_and_the_track_of_the_same_handle_as_they_were(tmp_path):
    from fithic_amd import _capi, mergefilter as mf
    import test_mergefilter_host as mfh
    import test_ucsc_host as uch
    mf_run, uc_run = mfh.RUNS["mfa"], uch.RUNS["uca"]
    paths = {}
    for key, data in (("split", run_input(RUNS["msu_5"])), ("select", mfh.run_input(mf_run)), ("track", uch.run_input(uc_run))):
        paths[key] = str(tmp_path / (key + ".txt"))
        with open(paths[key], "wb") as f:
            f.write(data)
    ms = _capi.MsContext(0)
    try:
        for _ in range(2):
            assert ms.split_file(paths["split"], b"5", mf.key_bound("5"), True) == 9
            ms.select_file(paths["select"], mf_run["fdr"].encode(), mf.key_bound(mf_run["fdr"]), True)
            assert ms.subset() == mfh._gunzip(os.path.join(mfh.MF, mf_run["subset"]))
            q = uc_run["qval"]
            ms.track_file(paths["track"], q.encode(), mf.key_bound(q, True), 0 < float(q))
            assert ms.track() == uch.run_track(uc_run)
            names = ms.split_names()                                   # and the split is still there
            tree = run_tree(RUNS["msu_5"])
            assert sorted(names) == sorted(tree)
            counts = ms.split_counts()
            for k, c in enumerate(names):
                assert ms.split_text(k, counts["bytes"][k]) == tree[c]["subset"] and counts["kept"][k] == tree[c]["subset"].count(b"\n")
    finally:
        ms.close()
