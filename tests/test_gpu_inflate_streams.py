"""The device gzip decoder (csrc/fhx_inflate.inc) on valid deflate that zlib's encoder never writes.

tests/test_gpu_inflate.py feeds gz_inflate what zlib compresses; bgzip on libdeflate, pigz, zopfli, 7-zip and igzip may write
the rest of RFC 1951.  tests/deflate_writer.py builds it token by token - matches at distances 32 507 to 32 768 and across the
16 KB flush seams, every (length, distance) shape of the two copy branches, 14- and 15-bit codes on either alphabet and
symbols of the full 48 bits, a 1-bit literal code, length 258 as 284 + 31, one distance code, none, a block of end-of-block
alone, stored blocks after every number of leftover bits - and states the text by a byte-by-byte copy of its own
(tests/test_deflate_writer_inputs.py holds both to zlib without a GPU).  Everything here is byte equality.  Streams zlib refuses
must come back as FHX_ERR_UNSUPPORTED, from the exit that reading the kernel says they take, and never as text."""
import random

import pytest

import deflate_writer as dw

pytestmark = pytest.mark.gpu

# fhx::gzdev's E_* as device_inflate words them
REASON = {dw.E_STORED: "stored block length", dw.E_TABLE: "Huffman table", dw.E_SYMBOL: "symbol", dw.E_DISTANCE: "distance beyond the start",
          dw.E_OUTPUT: "more text than ISIZE"}


@pytest.fixture(scope="module")
def ctx():
    from fithic_amd import _capi
    c = _capi.Context(0)
    yield c
    c.close()


def _device_text(ctx, tmp_path, blob, cap, name="m.gz"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(blob)
    return ctx.debug_inflate_file(path, cap)


def test_all_valid_members_in_one_file(ctx, tmp_path):
    blob = b"".join(dw.fh_member_raw(body, text) for _, body, text, _ in dw.CATALOGUE)
    want = b"".join(c[2] for c in dw.CATALOGUE)
    assert _device_text(ctx, tmp_path, blob, len(want) + 16) == want
    # and in another order: other members begin unaligned, other texts land on other addresses
    order = list(dw.CATALOGUE)
    random.Random(3).shuffle(order)
    blob = b"".join(dw.fh_member_raw(body, text) for _, body, text, _ in order)
    assert _device_text(ctx, tmp_path, blob, len(want) + 16, "shuffled.gz") == b"".join(c[2] for c in order)


@pytest.mark.parametrize("name", [c[0] for c in dw.CATALOGUE])
def test_each_valid_member_alone(ctx, tmp_path, name):
    _, body, text, _ = dw.BY_NAME[name]
    got = _device_text(ctx, tmp_path, dw.fh_member_raw(body, text), len(text) + 16)
    assert len(got) == len(text)
    assert got == text, next(i for i in range(len(text)) if got[i] != text[i])


def test_bgzf_subset(ctx, tmp_path):
    members = [dw.BY_NAME[name] for name in dw.BGZF_SUBSET]
    blob = b"".join(dw.bgzf_member_raw(body, text) for _, body, text, _ in members)
    want = b"".join(m[2] for m in members)
    assert _device_text(ctx, tmp_path, blob, len(want) + 16) == want
    for name, body, text, _ in members:
        assert _device_text(ctx, tmp_path, dw.bgzf_member_raw(body, text), len(text) + 16, name + ".gz") == text, name


@pytest.mark.parametrize("name", [r[0] for r in dw.REFUSALS])
def test_refusal_between_two_good_members(ctx, tmp_path, name):
    from fithic_amd import _capi
    _, body, text, code, _ = next(r for r in dw.REFUSALS if r[0] == name)
    good = [dw.BY_NAME[n] for n in ("copy_len65", "table_seams_10_11_8_9")]
    blob = dw.fh_member_raw(*good[0][1:3]) + dw.fh_member_raw(body, text) + dw.fh_member_raw(*good[1][1:3])
    with pytest.raises(_capi.FhxError) as e:
        _device_text(ctx, tmp_path, blob, len(good[0][2]) + len(text) + len(good[1][2]) + 4096)
    assert e.value.code == _capi.FHX_ERR_UNSUPPORTED
    assert "gzip member 1: %s (device decoder)" % REASON[code] in str(e.value)
    # the context is as good as before
    assert _device_text(ctx, tmp_path, dw.fh_member_raw(*good[0][1:3]), len(good[0][2]) + 16, "after.gz") == good[0][2]


def test_literal_only_contacts_file_is_inflated_on_the_device(tmp_path):
    """a contacts file whose blocks hold literals only and no distance code (RFC 1951 3.2.7: HDIST = 1 with that one length 0)
    goes through the device inflate and the device parser, not back to the host"""
    from fithic_amd.engine import Engine
    rng = random.Random(4)
    rows = []
    for _ in range(3000):
        c = rng.randrange(1, 23)
        rows.append("chr%d\t%d\tchr%d\t%d\t%d\n" % (c, rng.randrange(1, 50000) * 5000 + 2500, c, rng.randrange(1, 50000) * 5000 + 2500, rng.randrange(1, 500)))
    members = []
    for at in range(0, len(rows), 1000):
        text = "".join(rows[at:at + 1000]).encode()
        w = dw.Writer()
        w.dynamic(list(text[:10_000]), dw.flat(sorted(set(text)) + [256]), [0], last=False, rle="runs")
        w.dynamic(list(text[10_000:]), dw.flat([256] + sorted(set(text))), [0] * 30, last=True, rle="runs")
        assert dw.walk(w.getvalue())["no_dist_code_blocks"] == 2
        members.append(dw.fh_member_raw(w.getvalue(), text))
    path = str(tmp_path / "literal_only.gz")
    with open(path, "wb") as f:
        f.write(b"".join(members))
    eng = Engine(0)
    eng.configure(5000, 0, None, n_bins=10, mapp_thres=1, mode="All", bias_low=0.5, bias_up=2.0)
    k, seen = eng.ctx.ingest_contacts_file(path)                      # raises with .refused = 1 if the decoder sends the file back
    assert k == len(rows) and sorted(seen) == sorted({r.split("\t")[0] for r in rows})
    eng.close()
