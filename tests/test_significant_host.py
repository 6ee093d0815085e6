"""`fithic --significant FDR [--significant-only]`: what is decided before any engine call (no GPU needed), and the three
fhx_significant_* symbols in the binding's table."""
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")
CON = os.path.join(DATA, "quirk.contacts.gz")
FRG = os.path.join(DATA, "quirk.frags.gz")
NEW = ("fhx_significant_select", "fhx_significant_copy_text", "fhx_significant_copy_rows")


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


@pytest.mark.parametrize("fdr", ["1e", "-0.05", "0." + "0" * 30 + "5"], ids=["no_exponent_digits", "sign", "33_bytes"])
def test_fdr_outside_the_grammar_ends_before_the_engine(fdr, tmp_path, capsys, monkeypatch):
    assert len("0." + "0" * 30 + "5") == 33
    code, err = _refused(["--significant", fdr], tmp_path, capsys, monkeypatch)
    assert code == 2 and "--significant" in err and "fdr" in err


def test_significant_only_needs_significant(tmp_path, capsys, monkeypatch):
    code, err = _refused(["--significant-only"], tmp_path, capsys, monkeypatch)
    assert code == 2 and "--significant-only needs --significant" in err


def test_significant_only_is_refused_with_several_gpus(tmp_path, capsys, monkeypatch):
    code, err = _refused(["--significant", "0.05", "--significant-only", "--gpus", "2"], tmp_path, capsys, monkeypatch)
    assert code == 2 and "--gpus" in err


def test_accepted_forms_parse():
    from fithic_amd import cli
    base = ["-i", CON, "-f", FRG, "-o", "x", "-r", "10000"]
    a = cli.parse_args(base)
    assert a.significant is None and a.significant_only is False
    a = cli.parse_args(base + ["--significant", "1e-20", "--significant-only"])
    assert a.significant == "1e-20" and a.significant_only is True
    a = cli.parse_args(base + ["--significant", ".05", "--gpus", "2"])            # the fallback route: allowed
    assert a.significant == ".05" and a.gpus == 2


def test_new_symbols_are_declared_and_bound():
    from fithic_amd import _capi
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "fithic_mi355x.h")).read()
    declared = set(re.findall(r"\b(fhx_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in _capi.SYMBOLS, name
    res, args = _capi.SYMBOLS["fhx_significant_select"]
    assert len(args) == 13                            # ctx, names, n_names, fdr, len, key, zero_kept, strict, 3 counts, why, line


def test_refusal_message_is_the_file_routes():
    """Engine.significant raises what mergefilter raises for the gzipped file of the pass: same builder, same words"""
    from fithic_amd import _capi, mergefilter

    class E:
        why, line = _capi.MS_FIELD, 7
    import gzip
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sig.gz")
        with gzip.open(path, "wb") as f:
            f.write(b"x\n" * 9)
        want = mergefilter._refusal(path, E)
        got = mergefilter._refusal_at("%s, line %d" % (path, 7), _capi.MS_FIELD, "")
    assert type(want) is ValueError and str(want) == str(got) and ", line 7: field 7" in str(got)
