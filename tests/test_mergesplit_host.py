"""CPU tests of the per-chromosome merge-filter path: the plain-Python model (tests/mergesplit_model.py) equals the real script's
tree on the fixtures of tests/golden/mergesplit (made by tests/golden/make_golden_mergesplit.py) and the installed mawk on random
lines, the name grammar's claim - between two accepted names awk's `$1==c` is byte equality - holds against mawk itself, every
refused form is refused by the Python-side check, and the job text and the command line's argument handling are the script's."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import mergefilter_model as mm
import mergesplit_model as sm
from conftest import GOLDEN
from test_mergefilter_host import BOUNDARY_FIELDS, THRESHOLDS, _gunzip, _mawk

MS = os.path.join(GOLDEN, "mergesplit")
with open(os.path.join(MS, "cases.json")) as _f:
    CASES = json.load(_f)
RUNS = {r["name"]: r for r in CASES["runs"]}
MERGED_HEADER = "chr1\tmid1\tchr2\tmid2\tCC\tp\tfdr\tbin1_low\tbin1_high\tbin2_low\tbin2_high\tsumCC\tStrongConn"

# the pools of the issue
ACCEPTED = [b"1", b"10", b"2L", b"2R", b"10_random", b"nan", b"NaN", b"inf", b"INF", b"infinity", b"e5", b"x1", b"_1", b"chr1",
            b"123456789012345", b"123456789012346", b"999999999999999", b"100000000000000"]
REFUSED = [b"01", b"1.0", b"1e0", b"0x1", b"2a", b"1234567890123456"]


def run_input(run):
    return _gunzip(os.path.join(MS, run["input"]))


def run_tree(run):
    """{name: {"subset", "job", "merged"}} with the texts as bytes (merged: None when the job left no file)"""
    with open(os.path.join(MS, run["tree"])) as f:
        tree = json.load(f)
    return {name.encode("latin-1"): dict(subset=t["subset"].encode("latin-1"), job=t["job"],
                                         merged=None if t["merged"] is None else t["merged"].encode("latin-1")) for name, t in tree.items()}


def test_fixtures_were_made_by_the_pinned_tools_and_cover_the_cases_of_the_issue():
    assert CASES["awk"].startswith("mawk 1.3.4") and CASES["locale"] == "LC_ALL=C"
    assert sorted(RUNS) == ["msa", "mse", "msn", "msu_1e-5", "msu_5"]
    assert all(r["left_in_outdir"] == [] for r in RUNS.values())                  # chromosomes.used is not left behind
    a, u, n = (run_input(RUNS[k]) for k in ("msa", "msu_5", "msn"))
    # msa: a header, three sorted chromosomes, a tab after token 1 and mixed separators behind it, trans rows, rows round fdr
    firsts = [line.split(b"\t")[0] for line in a.splitlines()[1:]]
    assert a.startswith(b"chr1\tfragmentMid1") and firsts == sorted(firsts) and set(firsts) == {b"chr1", b"chr2", b"chrX"}
    assert b"  " in a and b" \t" in a and any(line.split()[0] != line.split()[2] for line in a.splitlines()[1:])
    tree = run_tree(RUNS["msa"])
    subsets = b"".join(t["subset"] for t in tree.values())
    assert b"5.000000e-02" in subsets and b"4.999999e-02" in subsets and b"5.000001e-02" not in subsets and b"5.000001e-02" in a
    assert all(line.split()[0] == line.split()[2] for line in subsets.splitlines())
    # msu: interleaved line by line, the names of the issue, Y only in trans rows, the header's chr1 in no data row, mfq's quirks
    rows = u.splitlines()[1:]
    assert all(x.split()[0] != y.split()[0] for x, y in zip(rows, rows[1:]))
    assert RUNS["msu_5"]["input"] == RUNS["msu_1e-5"]["input"] and (RUNS["msu_1e-5"]["fdr"], RUNS["msu_5"]["fdr"]) == ("1e-5", "5")
    for run in (RUNS["msu_5"], RUNS["msu_1e-5"]):
        tree = run_tree(run)
        assert sorted(tree) == sorted([b"1", b"2", b"X", b"2L", b"10_random", b"nan", b"NAN", b"Y", b"chr1"])
        assert tree[b"Y"]["subset"] == b"" == tree[b"chr1"]["subset"] and all(tree[c]["subset"] for c in tree if c not in (b"Y", b"chr1"))
    for needle in (b"1.000000e-320", b"2.225074e-308", b"2.225073e-308", b"1.000000e+309"):
        assert needle in u
    lo, hi = (b"".join(t["subset"] for t in run_tree(RUNS[k]).values()) for k in ("msu_1e-5", "msu_5"))
    assert b"1.000000e-320" in lo and b"1.000000e-320" in hi and b"2.225073e-308" not in lo and b"2.225073e-308" in hi
    # msn: line 1 is a data row whose chromosome occurs nowhere else; no final newline, and the last line is kept with one
    assert n.splitlines()[0].startswith(b"chr9\t") and not any(line.startswith(b"chr9") for line in n.splitlines()[1:])
    tree = run_tree(RUNS["msn"])
    assert tree[b"chr9"]["subset"] == b"" and not n.endswith(b"\n") and tree[b"chr6"]["subset"].endswith(n.splitlines()[-1] + b"\n")
    # mse: no row passes; what the real Combine leaves for an empty subset is its header line without a newline
    tree = run_tree(RUNS["mse"])
    assert all(t["subset"] == b"" and t["merged"] == MERGED_HEADER.encode() for t in tree.values()) and len(tree) == 3
    assert all(len(run_input(r).splitlines()) <= 400 for r in RUNS.values())


@pytest.mark.parametrize("name", sorted(RUNS))
def test_model_reproduces_the_script_s_tree(name):
    run = RUNS[name]
    tree, data = run_tree(run), run_input(run)
    got = sm.split(data, run["fdr"])
    assert sorted(got) == sorted(tree) == sm.chromosomes(data)
    for c in tree:
        assert got[c] == tree[c]["subset"], c
        assert sm.job_text(run["outdir"], c.decode(), str(run["res"]), run["utilityfolder"]) == tree[c]["job"]
    # the subsets are the one-file model's selection, told apart by chromosome, trans rows left out
    cis = [line + b"\n" for line in mm.select(data, run["fdr"]).splitlines() if line.split()[0] == line.split()[2]]
    assert sorted(cis) == sorted(line + b"\n" for t in tree.values() for line in t["subset"].splitlines())


# ---- the installed awk ------------------------------------------------------------------------------------------------------
NAMES_OF_RANDOM_LINES = [b"1", b"10", b"2L", b"nan", b"NAN", b"chr1", b"X", b"10_random", b"inf", b"e5"]


def random_lines(seed, n=2000):
    rng = np.random.default_rng(100 + seed)
    fields = list(BOUNDARY_FIELDS)
    while len(fields) < n:
        ex = int([rng.integers(-12, 2), rng.integers(-330, -300), rng.choice([-400, -309, -308, -307, 306, 307, 309, 310, 400]),
                  rng.integers(-307, 308)][int(rng.integers(0, 4))])
        fields.append("%d.%06de%s%02d" % (rng.integers(1, 10), rng.integers(0, 1000000), "-" if ex < 0 else "+", abs(ex)))
    order = rng.permutation(len(fields))
    seps = [b"\t", b" ", b"  ", b" \t"]
    lines = []
    for k, i in enumerate(order):
        c1 = NAMES_OF_RANDOM_LINES[int(rng.integers(0, len(NAMES_OF_RANDOM_LINES)))]
        c3 = c1 if rng.integers(0, 6) else NAMES_OF_RANDOM_LINES[int(rng.integers(0, len(NAMES_OF_RANDOM_LINES)))]
        lines.append(c1 + b"\t" + seps[k % 4].join([b"%d" % (5000 * k + 2500), c3, b"%d" % (5000 * k + 52500), b"9", b"1.000000e-09",
                                                     fields[i].encode(), b"x"]) + b"\n")
    return b"".join(lines)


@pytest.mark.skipif(not _mawk(), reason="the installed awk is not mawk 1.3.4")
@pytest.mark.parametrize("fdr", THRESHOLDS)
def test_model_equals_the_installed_awk_on_random_lines(fdr, tmp_path):
    data = random_lines(THRESHOLDS.index(fdr))
    src = str(tmp_path / "lines.txt")
    with open(src, "wb") as f:
        f.write(data)
    env = dict(os.environ, LC_ALL="C")
    listed = subprocess.run("cat %s | cut -f1 | sort | uniq" % src, shell=True, env=env, capture_output=True, check=True).stdout.split(b"\n")[:-1]
    got = sm.split(data, fdr)
    assert listed == sm.chromosomes(data) == sorted(got) and len(listed) == len(NAMES_OF_RANDOM_LINES)
    total = 0
    for c in listed:
        script = subprocess.run("cat %s | awk '{if(NR!=1){print $0}}'| awk -v c=\"%s\" '{if($1==c && $3==c){print $0}}' | "
                                "awk -v q=\"%s\" '{if($7<=q){print $0}}'" % (src, c.decode(), fdr), shell=True, env=env, capture_output=True,
                                check=True).stdout
        assert got[c] == script, c
        total += script.count(b"\n")
    assert fdr == "0" or 0 < total < data.count(b"\n") - 1


def pairs_of(pool, n, seed):
    rng = np.random.default_rng(seed)
    return [(pool[int(rng.integers(0, len(pool)))], pool[int(rng.integers(0, len(pool)))]) for _ in range(n)]


@pytest.mark.skipif(not _mawk(), reason="the installed awk is not mawk 1.3.4")
def test_between_accepted_names_awk_s_equality_is_byte_equality(tmp_path):
    """2 000 random pairs (A, B) of the adversarial pool: `mawk -v c=A '$1==c'` prints the line B exactly when A == B bytewise.  One
    mawk per distinct A, over the Bs it is paired with."""
    from fithic_amd import mergefilter_parallel as mp
    assert all(sm.name_reason(name) == 0 == mp.name_refusal(name) for name in ACCEPTED)
    pairs = pairs_of(ACCEPTED, 2000, 7)
    assert len(set(pairs)) > 250 and sum(a == b for a, b in pairs) > 50
    env = dict(os.environ, LC_ALL="C")
    checked = 0
    for a in ACCEPTED:
        others = [b for x, b in pairs if x == a]
        src = str(tmp_path / "names.txt")
        with open(src, "wb") as f:
            f.write(b"".join(b + b"\tk\n" for b in others))
        said = subprocess.run(["awk", "-v", "c=" + a.decode(), "$1==c", src], env=env, capture_output=True, check=True).stdout
        assert said == b"".join(b + b"\tk\n" for b in others if b == a), a
        checked += len(others)
    assert checked == 2000


@pytest.mark.skipif(not _mawk(), reason="the installed awk is not mawk 1.3.4")
def test_the_refused_forms_are_the_ones_awk_compares_as_numbers(tmp_path):
    """why they are refused: mawk takes 1, 01, 1.0, 1e0 and 0x1 for one number (2a and the 16-digit integer are refused as forms
    strtod might consume, whatever this awk does with them)"""
    src = str(tmp_path / "names.txt")
    with open(src, "wb") as f:
        f.write(b"1\tk\n01\tk\n1.0\tk\n1e0\tk\n0x1\tk\n2a\tk\n")
    said = subprocess.run(["awk", "-v", "c=1", "$1==c", src], env=dict(os.environ, LC_ALL="C"), capture_output=True, check=True).stdout
    assert said.startswith(b"1\tk\n01\tk\n1.0\tk\n1e0\tk\n") and b"2a" not in said


def test_every_refused_name_is_refused_by_the_python_side_check_and_the_model():
    from fithic_amd import _capi, mergefilter_parallel as mp
    for name in REFUSED + [b"1.5", b"1e3", b"00", b"1-2", b"9.", b"1p3", b"0X1F"]:
        assert mp.name_refusal(name) == _capi.MS_NAME_NUMERIC == sm.NAME_NUMERIC == sm.name_reason(name), name
    for name in [b"", b".1", b"-1", b"+1", b"chr/1", b"chr 1", b"chr$1", b"a\xe9", b"a,b"]:
        assert mp.name_refusal(name) == _capi.MS_NAME_BYTES == sm.NAME_BYTES == sm.name_reason(name), name
    assert mp.name_refusal(b"c" * 64) == _capi.MS_NAME == sm.NAME == sm.name_reason(b"c" * 64)
    for name in ACCEPTED + [b"0", b"c" * 63, b"2L.v1-x", b"9_", b"1g", b"chrUn_KI270742v1", b"X", b"MT", b"a.b-c"]:
        assert mp.name_refusal(name) == 0 == sm.name_reason(name), name
    assert (sm.NAME_TAB, sm.NAMES, sm.MAX_NAMES) == (_capi.MS_NAME_TAB, _capi.MS_NAMES, _capi.MS_SPLIT_NAMES)
    # the two restatements agree on random names over the bytes that matter
    rng = np.random.default_rng(3)
    alphabet = b"0123456789abefxpgzAEXPL_.-+ /"
    for _ in range(4000):
        name = bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(rng.integers(1, 6))))
        assert mp.name_refusal(name) == sm.name_reason(name), name


MODEL_REFUSALS = {"no tab after token 1": (b"chr1 5 chr1 7 3 4 1.000000e-03 x", sm.NAME_TAB), "leading blank": (b" chr1\t5 chr1 7 3 4 1.000000e-03", sm.NAME_TAB),
                  "leading tab": (b"\tchr1\t5 chr1 7 3 4 1.000000e-03", sm.NAME_TAB), "blank then tab": (b"chr1 \t5 chr1 7 3 4 1.000000e-03", sm.NAME_TAB),
                  "bad byte in token 1": (b"chr/1\t5 chr/1 7 3 4 1.000000e-03", sm.NAME_BYTES), "bad byte in token 3": (b"chr1\t5 chr,1 7 3 4 1.000000e-03", sm.NAME_BYTES),
                  "dot first": (b".chr1\t5 chr1 7 3 4 1.000000e-03", sm.NAME_BYTES), "64 bytes in token 1": (b"c" * 64 + b"\t5 c 7 3 4 1.000000e-03", sm.NAME),
                  "64 bytes in token 3": (b"c\t5 " + b"c" * 64 + b" 7 3 4 1.000000e-03", sm.NAME), "six tokens": (b"chr1\t5 chr1 7 3 4", mm.TOKENS),
                  "empty line": (b"", mm.TOKENS), "field 7": (b"chr1\t5 chr1 7 3 4 0.05", mm.FIELD), "CR": (b"chr1\t5 chr1 7 3 4 1.000000e-03\r", mm.BYTES),
                  "long line": (b"chr1\t5 chr1 7 3 4 1.000000e-03 " + b"x" * 4070, mm.LONG_LINE)}
for _k, _name in enumerate(REFUSED):
    MODEL_REFUSALS["%s in token 1" % _name.decode()] = (_name + b"\t5 " + _name + b" 7 3 4 1.000000e-03", sm.NAME_NUMERIC)
    MODEL_REFUSALS["%s in token 3" % _name.decode()] = (b"chr1\t5 " + _name + b" 7 3 4 1.000000e-03", sm.NAME_NUMERIC)
GOOD = b"chr1\t2500\tchr1\t52500\t9\t1.000000e-09\t1.000000e-03\t1.0\t1.0\t2.5\n"
HEADER = b"chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC\n"


@pytest.mark.parametrize("kind", sorted(MODEL_REFUSALS))
def test_the_model_refuses_a_bad_line_with_its_line_number(kind):
    bad, why = MODEL_REFUSALS[kind]
    with pytest.raises(mm.Refused) as e:
        sm.split(HEADER + GOOD * 3 + bad + b"\n" + GOOD + b"chr1 x\n", "0.05")
    assert (e.value.why, e.value.line) == (why, 5)


def test_the_model_holds_line_1_to_the_rules_for_token_1_only():
    assert sm.split(b"chr7\tany | thing, at all\n" + GOOD, "0.05") == {b"chr7": b"", b"chr1": GOOD}
    assert sm.split(b"chr7\t\n" + GOOD[:-1], "0.05") == {b"chr7": b"", b"chr1": GOOD}
    for first, why in ((b"chr7 x", sm.NAME_TAB), (b"", sm.NAME_TAB), (b"chr7", sm.NAME_TAB), (b"01\tx", sm.NAME_NUMERIC), (b"a/b\tx", sm.NAME_BYTES),
                       (b"c" * 64 + b"\tx", sm.NAME), (b"chr7\t\x01", mm.BYTES)):
        with pytest.raises(mm.Refused) as e:
            sm.split(first + b"\n" + GOOD, "0.05")
        assert (e.value.why, e.value.line) == (why, 1), first
    names = [b"n%d\t1 n%d 2 3 4 9.000000e-01\n" % (k, k) for k in range(sm.MAX_NAMES + 1)]
    assert len(sm.split(b"".join(names[:-1]), "0.05")) == sm.MAX_NAMES
    with pytest.raises(mm.Refused) as e:
        sm.split(b"".join(names), "0.05")
    assert (e.value.why, e.value.line) == (sm.NAMES, 0)


# ---- the job text and the command line --------------------------------------------------------------------------------------
def test_job_text_is_the_script_s_line():
    from fithic_amd import mergefilter_parallel as mp
    for run in RUNS.values():
        for c, t in run_tree(run).items():
            assert mp.job_text(run["outdir"], c.decode(), str(run["res"]), run["utilityfolder"]) == t["job"]
    assert mp.job_text("o/", "X", "010", "") == "python3 CombineNearbyInteraction.py -i o//X/subset_fithic_X.gz -H 0 -r 010 -o o//X/postmerged_fithic_X.gz\n"
    assert mp.job_text("/a/b", "2L", "5000", "../u") == sm.job_text("/a/b", "2L", "5000", "../u")
    assert "python3 ../uCombineNearbyInteraction.py " in mp.job_text("/a/b", "2L", "5000", "../u")   # the script pastes, it does not join


def test_command_line_arguments():
    from fithic_amd import mergefilter_parallel as mp
    assert mp.parse_args(["in.gz", "5000", "out", "0.05"]) == ("in.gz", "5000", "out", "0.05", "", False, 0)
    assert mp.parse_args(["in.gz", "5000", "out", "0.05", "u/"]) == ("in.gz", "5000", "out", "0.05", "u/", False, 0)
    assert mp.parse_args(["--merge", "in.gz", "5000", "--device", "3", "out", "1e-5", "u/"]) == ("in.gz", "5000", "out", "1e-5", "u/", True, 3)
    assert mp.parse_args(["in.gz", "5000", "out", "0.05", "--device=2"])[5:] == (False, 2)
    for argv in ([], ["in.gz", "5000", "out"], ["in.gz", "5000", "out", "0.05", "u/", "more"], ["in.gz", "5k", "out", "0.05"],
                 ["in.gz", "5000", "out", "0.05", "--device"], ["in.gz", "5000", "out", "0.05", "--device", "x"],
                 ["in.gz", "5000", "out", "0.05", "--strict"]):
        with pytest.raises(SystemExit) as e:
            mp.parse_args(argv)
        assert "usage: python -m fithic_amd.mergefilter_parallel" in str(e.value.code)


def test_write_tree_makes_the_script_s_tree_without_a_device(tmp_path):
    """the host side alone, on subsets the golden holds: directories, gzip subsets, job lines appended as >> does"""
    from fithic_amd import mergefilter_parallel as mp
    run = RUNS["msn"]
    tree = run_tree(run)
    chosen = mp.Split({c: t["subset"] for c, t in tree.items()}, {c: t["subset"].count(b"\n") for c, t in tree.items()}, 101, {}, 0)
    assert chosen.chromosomes == ["chr4", "chr5", "chr6", "chr9"] and chosen.n_kept("chr9") == 0 and chosen.n_lines == 101
    assert chosen.selection("chr6").subset_text() == tree[b"chr6"]["subset"] == chosen.subset_text(b"chr6")
    with pytest.raises(KeyError):
        chosen.subset_text("chr1")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        for _ in range(2):
            mp.write_tree(chosen, run["outdir"], str(run["res"]), run["utilityfolder"])
    finally:
        os.chdir(cwd)
    out = tmp_path / run["outdir"]
    assert sorted(os.listdir(out)) == ["chr4", "chr5", "chr6", "chr9"]
    for c, t in tree.items():
        name = c.decode()
        assert sorted(os.listdir(out / name)) == ["fithic_%s.job" % name, "subset_fithic_%s.gz" % name]
        assert _gunzip(str(out / name / ("subset_fithic_%s.gz" % name))) == t["subset"]
        assert (out / name / ("fithic_%s.job" % name)).read_text() == t["job"] * 2              # appended, as >> does
    with gzip.open(str(out / "chr9" / "subset_fithic_chr9.gz"), "rb") as f:
        assert f.read() == b""


def test_entry_points_raise_without_a_usable_device(tmp_path):
    from fithic_amd import _capi, mergefilter_parallel as mp
    path = str(tmp_path / "sig.txt")
    open(path, "w").close()
    with pytest.raises(_capi.FhxError):
        mp.split(path, "0.05", device=1 << 20)
    with pytest.raises(ValueError, match="fdr"):
        mp.split(path, "5%", device=1 << 20)                              # refused before a device is asked for
    with pytest.raises(_capi.FhxError):
        mp.main([path, "5000", str(tmp_path / "out"), "0.05", "--device", str(1 << 20)])
    assert not (tmp_path / "out").exists()
    for name in ("fhx_ms_split_file", "fhx_ms_split_counts", "fhx_ms_split_names", "fhx_ms_split_stage_seconds", "fhx_ms_copy_split"):
        assert hasattr(_capi.lib(), name)


def test_refusals_become_the_documented_exceptions(tmp_path):
    from fithic_amd import _capi, mergefilter_parallel as mp
    path = str(tmp_path / "sig.txt")
    with open(path, "wb") as f:
        f.write(b"header\n01\t1 01 2 3 1e-3 1.000000e-02\nchr1 1 chr1\n")
    for why, needle in ((_capi.MS_NAME_NUMERIC, "compare as a number"), (_capi.MS_NAME_TAB, "ended by a tab"), (_capi.MS_NAME_BYTES, "A-Za-z0-9_.-"),
                        (_capi.MS_NAME, "more than 63 bytes")):
        e = mp._refusal(path, _capi.MsRefused(-4, "x", why, 2))
        assert isinstance(e, ValueError) and "line 2" in str(e) and needle in str(e) and "'01\\t1 01" in str(e)
        assert "The reference accepts this" in str(e)
    e = mp._refusal(path, _capi.MsRefused(-4, "x", _capi.MS_NAMES, 0))
    assert isinstance(e, ValueError) and "4096 distinct names" in str(e) and "line" not in str(e)
    e = mp._refusal(path, _capi.MsRefused(-4, "x", _capi.MS_TOKENS, 3))                     # mergefilter's own
    assert "line 3" in str(e) and "3 token(s)" in str(e)
