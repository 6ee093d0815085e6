"""`fithic --significant FDR --significant-track --significant-split`: what is decided before any engine call (no GPU needed), the
fhx_significant_track / fhx_significant_split symbols in the header and in the binding's table, and the words of a refusal: the
resident routes (Engine.track, Engine.split) raise what the file routes raise for the file of the pass."""
import gzip
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")
CON = os.path.join(DATA, "quirk.contacts.gz")
FRG = os.path.join(DATA, "quirk.frags.gz")
NEW = {"fhx_significant_track": 13,               # ctx, names, n_names, fdr, len, key, zero_kept, 4 counts, why, line
       "fhx_significant_copy_track": 3,
       "fhx_significant_split": 11,               # ctx, names, n_names, fdr, len, key, zero_kept, emitted, listed, why, line
       "fhx_significant_split_counts": 4,
       "fhx_significant_split_names": 3,
       "fhx_significant_copy_split": 4}


def _refused(argv, tmp_path, capsys, monkeypatch):
    """exit status and stderr of a command line that must end before an engine exists"""
    from fithic_amd import cli, fithic as F

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")
    monkeypatch.setattr(F._Session, "ensure_engine", no_engine)
    monkeypatch.setattr(F, "read_Interactions", no_engine)
    out_dir = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", CON, "-f", FRG, "-o", str(out_dir), "-r", "10000"] + argv)
    assert not out_dir.exists()                       # not even the banner ran
    return e.value.code, capsys.readouterr().err


@pytest.mark.parametrize("flag", ["--significant-track", "--significant-split"])
def test_the_modifiers_need_significant(flag, tmp_path, capsys, monkeypatch):
    code, err = _refused([flag], tmp_path, capsys, monkeypatch)
    assert code == 2 and flag + " needs --significant" in err
    code, err = _refused([flag, "--significant-only"], tmp_path, capsys, monkeypatch)
    assert code == 2 and "needs --significant" in err


def test_accepted_forms_parse():
    from fithic_amd import cli
    base = ["-i", CON, "-f", FRG, "-o", "x", "-r", "10000"]
    a = cli.parse_args(base + ["--significant", "0.05"])
    assert a.significant_track is False and a.significant_split is False
    a = cli.parse_args(base + ["--significant", "1e-20", "--significant-track", "--significant-split", "--significant-only"])
    assert a.significant_track is True and a.significant_split is True and a.significant_only is True
    a = cli.parse_args(base + ["--significant", ".05", "--significant-track", "--gpus", "2"])      # the file route: allowed
    assert a.significant_track is True and a.gpus == 2


def test_new_symbols_are_declared_and_bound():
    from fithic_amd import _capi
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "fithic_mi355x.h")).read()
    declared = set(re.findall(r"\b(fhx_[a-z0-9_]+)\s*\(", hdr))
    for name, n_args in NEW.items():
        assert name in declared, name
        assert name in _capi.SYMBOLS, name
        assert len(_capi.SYMBOLS[name][1]) == n_args, name
    for method in ("significant_track", "significant_split"):
        assert callable(getattr(_capi.Context, method))
    from fithic_amd.engine import Engine
    assert callable(Engine.track) and callable(Engine.split)


def _gz(tmp_path):
    path = str(tmp_path / "sig.gz")
    with gzip.open(path, "wb") as f:
        f.write(b"x\n" * 9)
    return path


class _E:
    def __init__(self, why, line):
        self.why, self.line = why, line


def test_track_refusals_are_the_file_routes(tmp_path):
    """ucsc._refusal_at gives, for a line that was never written, the words ucsc._refusal gives for the gzipped file of the pass"""
    from fithic_amd import _capi, ucsc
    path = _gz(tmp_path)
    for why, words in ((_capi.MS_MIDPOINT, "1 to 9 digits"), (_capi.MS_NAME, "more than 63 bytes"), (_capi.MS_FIELD, "field 7")):
        want = ucsc._refusal(path, _E(why, 7))
        got = ucsc._refusal_at("%s, line %d" % (path, 7), why, "")
        assert type(want) is ValueError and type(got) is ValueError and str(want) == str(got), why
        assert ", line 7: " in str(got) and words in str(got) and "fithic_amd.ucsc" in str(got) and "fithic_amd.mergefilter" not in str(got)
    assert str(ucsc._refusal(path, _E(_capi.MS_KEPT, 0))) == str(ucsc._refusal_kept(path))


def test_split_refusals_are_the_file_routes(tmp_path):
    from fithic_amd import _capi, mergefilter, mergefilter_parallel as mp
    path = _gz(tmp_path)
    for why, words in ((_capi.MS_NAME, "more than 63 bytes"), (_capi.MS_NAME_BYTES, "[A-Za-z0-9_.-]"), (_capi.MS_NAME_NUMERIC, "as a number"),
                       (_capi.MS_NAME_TAB, "ended by a tab"), (_capi.MS_FIELD, "field 7")):
        want = mp._refusal(path, _E(why, 4))
        got = mp._refusal_at("%s, line %d" % (path, 4), why, "")
        assert type(want) is ValueError and type(got) is ValueError and str(want) == str(got), why
        assert ", line 4: " in str(got) and words in str(got)
    assert str(mp._refusal_at("f, line 4", _capi.MS_FIELD, "")) == str(mergefilter._refusal_at("f, line 4", _capi.MS_FIELD, ""))
    assert str(mp._refusal(path, _E(_capi.MS_NAMES, 0))) == str(mp._refusal_names(path))


def test_the_name_rule_of_the_host_is_the_modules():
    """fhx_significant_split decides the reason per chromosome id on the host with the kernels' name_grammar (csrc/fhx_namerule.hpp);
    mergefilter_parallel.name_refusal is its statement in Python and tests/mergesplit_model.py the model's: the latter two agree on
    the names the GPU tests use"""
    import mergesplit_model as sm
    from fithic_amd import mergefilter_parallel as mp
    for name in (b"chr1", b"chr10", b"01", b"1.5", b"2a", b"2L", b"10_random", b"chr.1", b".chr", b"-chr", b"chr+1", b"c" * 63, b"c" * 64,
                 b"1" * 15, b"1" * 16, b"0", b"_x", b"1e3", b"0x1"):
        assert mp.name_refusal(name) == sm.name_reason(name), name
