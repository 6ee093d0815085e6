"""Host side of the HiC-Pro converter (fithic_amd.hicpro; reference: fithic/utils/HiCPro2FitHiC.py) without a GPU: the model of
tests/hicpro_model.py is pinned to the real reference's outputs (tests/golden/hicpro, written by make_golden_hicpro.py), and
the module's bed reader, fragments writer and bias conversion reproduce the reference's files byte for byte."""
import pytest

import hicpro_model as hm

CASE_NAMES = ["hp1", "hp2_r0", "hp2_r10000", "hp3"]


@pytest.fixture(scope="module")
def models():
    out = {}
    for name in CASE_NAMES:
        case = hm.CASES[name]
        out[name] = hm.Model(hm.fixture_bytes(case["bed"]), hm.fixture_bytes(case["matrix"]),
                             hm.fixture_bytes(case["bias"]) if case["bias"] else None, case["res"])
    return out


def test_fixtures_cover_the_cases_of_the_issue():
    assert sorted(hm.CASES) == sorted(CASE_NAMES)
    hp2 = hm.fixture_bytes("hp2.matrix.gz")
    assert len(hp2) > 30 * 16384 and hp2.count(b"\n") == 40000
    hp3 = hm.fixture_bytes("hp3.matrix.gz")
    assert b"\r\n" in hp3 and not hp3.endswith(b"\n") and b"\t" in hp3 and hp3.startswith(b"7 8")
    assert b"nan" in hm.fixture_bytes("hp1.bias.gz") and b"7.0" in hm.fixture_bytes("hp1.matrix.gz")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_model_reproduces_the_reference_outputs(name, models):
    contacts, fragments, bias = hm.case_outputs(hm.CASES[name])
    m = models[name]
    assert m.contacts_text().encode() == contacts
    assert m.fragments_text().encode() == fragments
    if bias is None:
        assert m.bias_values is None
    else:
        assert m.bias_text().encode() == bias


def test_the_example_of_the_issue(models):
    m = models["hp1"]
    assert m.contacts_text().split("\n")[:3] == ["chr1\t500\tchr1\t500\t4", "chr1\t500\tchr1\t1500\t7", "chr1\t1500\tchr2\t500\t3"]
    assert m.totals[1 - m.index_base] == 15


@pytest.mark.parametrize("name", CASE_NAMES)
def test_bed_reader_fragments_writer_and_bias_conversion_equal_the_reference(name, models, tmp_path):
    from fithic_amd import hicpro
    case = hm.CASES[name]
    bed_path, _, bias_path = hm.case_inputs(case, tmp_path)
    _, fragments, bias = hm.case_outputs(case)
    m = models[name]
    bed = hicpro.read_bed(bed_path, case["res"])
    assert (bed.res, bed.index_base, bed.n_slots, bed.chroms.names) == (m.res, m.index_base, m.n_slots, m.names)
    for index, (c, start, mid) in m.frag.items():
        assert bed.frag[index] == (c, start, mid)
        assert (bed.chr_id[index - bed.index_base], bed.mid[index - bed.index_base]) == (c, mid)
    absent = [s for s in range(bed.n_slots) if s + bed.index_base not in m.frag]
    assert all(bed.chr_id[s] == -1 for s in absent) and (name != "hp3" or absent)
    assert "".join(hicpro.fragments_lines(bed, m.totals)).encode() == fragments
    if bias is not None:
        values = hicpro.convert_bias(bias_path)
        assert "".join(hicpro.bias_lines(bed, values)).encode() == bias


def test_a_repeated_bed_index_keeps_the_later_line(tmp_path):
    from fithic_amd import hicpro
    bed = hicpro.read_bed(hm.case_inputs(hm.CASES["hp3"], tmp_path)[0])
    assert bed.frag[9] == (0, "99000", 101500) and bed.indices == [7, 8, 9, 12, 13]


def test_bias_errors_are_the_reference_s(tmp_path):
    from fithic_amd import hicpro
    bed = hicpro.read_bed(hm.case_inputs(hm.CASES["hp1"], tmp_path)[0])
    all_nan = tmp_path / "nan.bias"
    all_nan.write_text("nan\nnan\n")
    with pytest.raises(ZeroDivisionError):
        hicpro.convert_bias(str(all_nan))
    long_bias = tmp_path / "long.bias"
    long_bias.write_text("1.0\n" * 6)                                # five bins in the bed
    with pytest.raises(KeyError) as e:
        hicpro.bias_lines(bed, hicpro.convert_bias(str(long_bias)))
    assert e.value.args == (6,)


def test_bed_range_and_midpoint_refusals(tmp_path):
    from fithic_amd import hicpro
    wide = tmp_path / "wide.bed"
    wide.write_text("chr1\t0\t1000\t1\nchr1\t1000\t2000\t%d\n" % (2 + (1 << 27)))
    with pytest.raises(ValueError, match="2\\^27"):
        hicpro.read_bed(str(wide))
    far = tmp_path / "far.bed"
    far.write_text("chr1\t0\t1000\t1\nchr1\t%d\t%d\t2\n" % ((1 << 31) - 200, (1 << 31) + 800))
    with pytest.raises(ValueError, match="int32"):
        hicpro.read_bed(str(far))


def test_refused_lines_become_the_documented_exceptions(tmp_path):
    """the mapping from the native refusal (reason, line, index) to the exception, on a file the message quotes from"""
    from fithic_amd import _capi, hicpro
    path = tmp_path / "m.matrix"
    path.write_text("1 2 3\n1 2 2.5\n1 2\n1 2 x\n1 2 1e2\n")

    def refusal(why, line, index=0):
        return hicpro._refusal(str(path), _capi.HpRefused(_capi.FHX_ERR_UNSUPPORTED, "", why, line, index))
    e = refusal(_capi.HP_ABSENT, 1, 77)
    assert isinstance(e, KeyError) and e.args == (77,)
    for why, line in ((_capi.HP_FRACTION, 2), (_capi.HP_COUNT, 5)):
        e = refusal(why, line)
        assert isinstance(e, ValueError) and "line %d" % line in str(e) and "raw (integer) HiC-Pro matrix" in str(e)
    for why, line in ((_capi.HP_TOKENS, 3), (_capi.HP_COUNT, 4)):
        e = refusal(why, line)
        assert isinstance(e, ValueError) and "line %d" % line in str(e) and "raw (integer)" not in str(e)


def test_command_line_takes_the_reference_s_flags():
    from fithic_amd import hicpro
    a = hicpro.parse_args(["-i", "m", "-b", "b"])
    assert (a.matrix, a.bed, a.bias, a.output, a.resolution) == ("m", "b", None, ".", 0)
    a = hicpro.parse_args(["--matrix", "m", "--bed", "b", "--bias", "s", "--output", "o", "--resolution", "5000"])
    assert (a.bias, a.output, a.resolution) == ("s", "o", 5000)
