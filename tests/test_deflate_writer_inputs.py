"""The inputs of tests/test_gpu_inflate_streams.py, checked without a GPU: every stream of tests/deflate_writer.py is held to zlib
(the judge the device decoder falls back to) and to the facts it is there for, so that a case which loses its edge - as the
"largest distance" members of tests/test_gpu_inflate.py silently did - fails here."""
import gzip
import random
import zlib

import pytest

import deflate_writer as dw


def _inflate_raw(body):
    d = zlib.decompressobj(-15)
    out = d.decompress(body)
    assert d.eof and d.unused_data == b""
    return out


@pytest.mark.parametrize("name", [c[0] for c in dw.CATALOGUE])
def test_valid_stream_is_what_zlib_reads_and_has_its_facts(name):
    _, body, text, required = dw.BY_NAME[name]
    assert _inflate_raw(body) == text
    assert gzip.decompress(dw.fh_member_raw(body, text)) == text
    facts = dw.walk(body)
    assert facts["bits"] > 8 * (len(body) - 1)                       # the walker reached the last byte
    assert dw.holds(facts, required) == []
    if name in dw.BGZF_SUBSET:
        assert gzip.decompress(dw.bgzf_member_raw(body, text)) == text


def test_the_catalogue_as_a_whole():
    names = [c[0] for c in dw.CATALOGUE]
    assert len(set(names)) == len(names) and set(dw.BGZF_SUBSET) <= set(names) and len(dw.BGZF_SUBSET) >= 10
    assert max(len(c[2]) for c in dw.CATALOGUE) <= 100_000
    blob = b"".join(dw.fh_member_raw(b, t) for _, b, t, _ in dw.CATALOGUE)
    assert gzip.decompress(blob) == b"".join(c[2] for c in dw.CATALOGUE)
    # the copy matrix: every length with its nine distances (1, 2, 3, len - 1, len, len + 1, 63, 64, 65)
    for n in dw.LEN_SET:
        assert dw.BY_NAME["copy_len%d" % n][3]["matches"] == ("==", 9)
    # across the catalogue: every edge once more, as one statement
    facts = [dw.walk(c[1]) for c in dw.CATALOGUE]
    assert max(f["max_lit_code"] for f in facts) == 15 and max(f["max_dist_code"] for f in facts) == 15
    assert max(f["max_span"] for f in facts) == 48 and max(f["max_cl_code"] for f in facts) == 7
    assert max(f["max_distance"] for f in facts) == 32768 and min(f["text_len"] for f in facts) == 0
    assert set().union(*(f["hclen"] for f in facts)) >= {5, 19} and set().union(*(f["cl_cross"] for f in facts)) == {16, 18}


@pytest.mark.parametrize("name", [r[0] for r in dw.REFUSALS])
def test_refusal_is_an_error_under_zlib(name):
    _, body, text, code, raw = next(r for r in dw.REFUSALS if r[0] == name)
    assert code in (dw.E_STORED, dw.E_TABLE, dw.E_SYMBOL, dw.E_DISTANCE, dw.E_OUTPUT)
    if raw:
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(body)
        with pytest.raises(dw.DeflateError):
            dw.walk(body)
    else:
        assert len(_inflate_raw(body)) != len(text)                  # a sound stream under a trailer that disagrees
    with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
        gzip.decompress(dw.fh_member_raw(body, text))
    good = dw.fh_member_raw(*dw.BY_NAME["copy_len65"][1:3])
    with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
        gzip.decompress(good + dw.fh_member_raw(body, text) + good)


def test_the_writer_refuses_what_it_must():
    with pytest.raises(ValueError):
        dw.canonical_codes([1, 1, 1])
    with pytest.raises(ValueError):
        dw.Writer().dynamic([65], {65: 1, 256: 1, 257: 1}, {0: 1}, last=True)               # over-subscribed
    with pytest.raises(ValueError):
        dw.Writer().dynamic([65], {65: 2, 256: 2}, {0: 1}, last=True)                       # incomplete, two codes
    with pytest.raises(ValueError):
        dw.Writer().dynamic([66], {65: 1, 256: 1}, {0: 1}, last=True)                       # a symbol without a code
    with pytest.raises(ValueError):
        dw.Writer().dynamic([65], {65: 1, 256: 1}, {0: 1}, last=True, rle=[1, 1])           # lengths that spell something else
    with pytest.raises(ValueError):
        dw.Writer().dynamic([65], {65: 1, 256: 1}, {0: 1}, last=True, cl_lengths={0: 1, 1: 2})
    with pytest.raises(ValueError):
        dw.expand([65, (3, 2)])
    assert dw.canonical_codes([2, 1, 3, 3]) == [0b10, 0b0, 0b110, 0b111]                  # RFC 1951 3.2.2's example shape
    assert dw.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]     # RFC 1951 3.2.2, ABCDEFGH
    # HCLEN 4..19 come out as asked: 255 literals and end-of-block at 8 bits need the code-length symbols 0 and 8 alone
    lit = [8] * 255 + [0, 8]
    for hclen in range(5, 20):
        cl = dw.flat(sorted({0, 8, 16, 17, 18, dw.CL_ORDER[hclen - 1]}))
        w = dw.Writer()
        w.dynamic([65] * 5, lit, [0], last=True, cl_lengths=cl, rle="runs")
        assert dw.walk(w.getvalue())["hclen"] == {hclen}
        assert _inflate_raw(w.getvalue()) == b"A" * 5
    w = dw.Writer()                                                 # 16, 17, 18 and 0 alone can spell no end-of-block code
    w.dynamic([], [0] * 257, [0], last=True, cl_lengths={0: 1, 18: 2, 17: 3, 16: 3}, rle="runs", eob=False, strict=False)
    with pytest.raises(dw.DeflateError):
        dw.walk(w.getvalue())
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(w.getvalue())


def test_walk_agrees_with_zlib_on_zlib_streams():
    rng = random.Random(5)
    text = b"".join(b"chr%d\t%d\t%d\n" % (rng.randrange(1, 23), rng.randrange(10 ** 6), rng.randrange(500)) for _ in range(5000))
    for level, strategy in ((0, 0), (1, 0), (6, 0), (9, 0), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        body = co.compress(text) + co.flush()
        f = dw.walk(body)
        assert f["text_len"] == len(text) and -(-f["bits"] // 8) == len(body)
        assert (f["matches"] == 0) == (level == 0 or strategy == zlib.Z_HUFFMAN_ONLY)


# ---- what tests/test_gpu_inflate.py's streams do not reach: its members rebuilt here as test_every_block_type_strategy_and_level
# builds them (same generator, same seed, same zlib parameters)
def _old_members(prefix=None):
    from test_gpu_inflate import _rows
    rng = random.Random(1)
    text = _rows(rng, 60_000)
    noise = bytes(rng.getrandbits(8) for _ in range(200_000))
    block = bytes(rng.getrandbits(8) for _ in range(32768))
    if prefix:
        text = text[:prefix]
    out = {}

    def add(name, data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flushes=()):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
        body, at = b"", 0
        for cut, mode in flushes:
            body += co.compress(data[at:cut]) + co.flush(mode)
            at = cut
        out[name] = body + co.compress(data[at:]) + co.flush()
    for level in (0, 1, 2, 4, 6, 9):
        add("level%d" % level, text, level=level)
    for strategy in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
        add("strategy%d" % strategy, text[:400_000], strategy=strategy)
    add("mem_level1", text[:300_000], mem_level=1)
    add("noise", noise)
    add("noise0", noise, level=0)
    add("empty", b"")
    add("x", b"x")
    add("zeros", b"\0" * 1_000_000)
    add("block6", block * 6, level=9)
    add("block5", (block[:32767] + b"!") * 5 + block[:100], level=9)
    add("flushes", text[:500_000], flushes=[(1000, zlib.Z_SYNC_FLUSH), (70_000, zlib.Z_FULL_FLUSH), (70_001, zlib.Z_SYNC_FLUSH)])
    add("fname", text[:10_000])
    add("bytes_fixed", bytes(range(256)) * 50, strategy=zlib.Z_FIXED)
    return out


def test_what_the_zlib_made_members_do_not_reach():
    """Recorded, not wished for: zlib's encoder never looks further back than 32768 - 262, and on these inputs its codes stay
    short.  tests/test_gpu_inflate_streams.py is where the window's far edge and the 14- and 15-bit codes are tested."""
    members = _old_members()
    # random 32 KB repeated: zlib finds no match at all.  `block * 6` is twelve stored blocks; its sibling ten, and its last
    # 100 bytes one fixed block of literals
    f6, f5 = dw.walk(members["block6"]), dw.walk(members["block5"])
    assert f6["blocks"] == [12, 0, 0] and f6["matches"] == 0 and f6["max_distance"] == 0
    assert f5["blocks"] == [10, 1, 0] and f5["matches"] == 0 and f5["max_distance"] == 0
    facts = {name: dw.walk(body) for name, body in members.items()}
    assert max(f["max_distance"] for f in facts.values()) <= 32768 - 262
    assert max(f["max_lit_code"] for f in facts.values()) <= 13
    # one block of the 1.8 MB level-9 member holds a 14-bit distance code; nothing holds a 15-bit one, a full-span symbol,
    # 284 + 31, a block without or with one distance code, or a 7-bit code-length code
    assert {n for n, f in facts.items() if f["max_dist_code"] > 13} <= {"level9"}
    assert max(f["max_dist_code"] for f in facts.values()) <= 14 and max(f["max_span"] for f in facts.values()) < 48
    assert all(f["len258_by_284"] == 0 and f["no_dist_code_blocks"] == 0 and f["max_cl_code"] < 7 for f in facts.values())
    # on the 200 000-byte prefix of the rows no code of either alphabet is longer than 13 bits
    facts = [dw.walk(body) for body in _old_members(200_000).values()]
    assert max(max(f["max_lit_code"], f["max_dist_code"]) for f in facts) <= 13
    assert max(f["max_distance"] for f in facts) <= 32768 - 262
