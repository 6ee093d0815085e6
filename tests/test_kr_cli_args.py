"""`fithic --kr` before any GPU is touched: what the parser refuses, the new C entry in the header and in the built library, and
the loud failure of Engine.kr_bias without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DATA = os.path.join(HERE, "golden", "data")
BASE = ["-i", os.path.join(DATA, "quirk.contacts.gz"), "-f", os.path.join(DATA, "quirk.frags.gz"), "-o", "unused", "-r", "10000"]


def _error(argv, capsys):
    from fithic_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(BASE + argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_parser_errors(capsys):
    assert "--kr computes the biases: it cannot be combined with -t BIASFILE" in _error(["--kr", "-t", "x"], capsys)
    assert "--kr is not available with --gpus above 1: each rank holds a part of the rows" in _error(["--kr", "--gpus", "2"], capsys)
    assert "--kr-percent needs --kr" in _error(["--kr-percent", "0.1"], capsys)
    assert "--kr-output needs --kr" in _error(["--kr-output", "bias.gz"], capsys)
    assert "--kr-percent needs --kr" in _error(["--kr-percent", "0.05"], capsys)      # the default value, spelled out, still needs it


def test_parser_accepts_the_flags_with_their_defaults():
    from fithic_amd import cli
    a = cli.parse_args(BASE + ["--kr"])
    assert a.kr and a.kr_percent == 0.05 and a.kr_output is None and a.biasfile is None
    a = cli.parse_args(BASE + ["--kr", "--kr-percent", "0.12", "--kr-output", "b.gz", "-p", "2", "-x", "All", "-v", "--significant", "0.05",
                               "--totals", "wide", "-tL", "0.4", "-tU", "3"])
    assert a.kr_percent == 0.12 and a.kr_output == "b.gz" and a.noOfPasses == 2 and a.significant == "0.05"
    assert not cli.parse_args(BASE).kr


def test_header_declares_and_library_exports_the_entry():
    from fithic_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "fithic_mi355x.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int fhx_kr_load_pairs_resident\(fhx_kr\* kr, fhx_ctx\* ctx, int64_t\* first_unknown_row\);", hdr, re.S)
    assert m, "the header does not declare fhx_kr_load_pairs_resident"
    assert "HiCKRy.py:18-54" in m.group(1)
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "fhx_kr_load_pairs_resident")
    assert "fhx_kr_load_pairs_resident" in _capi.SYMBOLS
    _capi.lib()                                        # binds every declared symbol


def test_kr_bias_fails_loudly_without_a_device():
    from fithic_amd import _capi
    from fithic_amd.engine import Engine
    eng = Engine(-1)                                   # a host-only context: no GPU behind it
    try:
        with pytest.raises(_capi.FhxError) as e:
            eng.kr_bias(np.zeros(3, np.int32), np.array([5, 15, 25], np.int32))
        assert e.value.code == _capi.FHX_ERR_NO_DEVICE
    finally:
        eng.close()


def test_the_stage_function_needs_the_contacts_first():
    from fithic_amd import fithic as F
    F.reset_session()
    with pytest.raises(ValueError, match="read_Interactions first"):
        F.kr_biases(os.path.join(DATA, "quirk.frags.gz"), 0.05)
