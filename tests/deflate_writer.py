"""TEST INFRASTRUCTURE - an RFC 1951 writer and walker for tests/test_gpu_inflate_streams.py, no GPU needed
(tests/test_deflate_writer_inputs.py holds every stream built here to zlib and to the facts it is there for).

Every stream tests/test_gpu_inflate.py feeds the device decoder (csrc/fhx_inflate.inc) comes out of zlib's own encoder, and
that encoder never writes a distance above 32 506 (MAX_DIST = 32 768 - 262), a code of 14 or 15 bits on these inputs, length
258 as code 284 + 31, a block without distance codes...  All of it is legal deflate that other encoders may write.  Here the
caller chooses every token and every code length:

  Writer        bits into an integer accumulator; stored(), fixed() and dynamic() blocks
  expand        the text of a token list by a byte-by-byte LZ77 copy - the expected output, independent of zlib
  walk          a puff-style reader that returns facts about a stream (longest code in use, largest distance, ...), so that
                a case that loses its edge is noticed
  CATALOGUE     (name, body, text, required facts) of valid streams; BGZF_SUBSET names those also wrapped as BGZF
  REFUSALS      (name, body, text, the decoder's error code, raw) of streams zlib refuses; raw = the deflate layer itself
                is in error (otherwise the gzip trailer is)

A token is a literal byte (int) or a match (length, distance); (258, distance, True) writes length 258 as code 284 with extra
bits 31.  For the refusals there are raw tokens: ("lit", symbol) and ("dist", symbol) write one codeword without extra bits,
("bits", value, n) writes n bits as they are."""
import random
import struct
import zlib

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_BITS = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_BITS = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
WIN = 32768
FLUSH = 16384                       # the device decoder's window leaves for HBM in pieces of this size

# the decoder's status codes (fhx::gzdev in csrc/fhx_inflate.inc)
E_STORED, E_TABLE, E_SYMBOL, E_DISTANCE, E_OUTPUT = 2, 3, 4, 5, 6


# ------------------------------------------------------------------------------------------------------------- codes
def code_space_left(lengths):
    """the code space a set of lengths leaves: 0 complete, > 0 incomplete, < 0 over-subscribed (in units of 2^-15)"""
    return (1 << 15) - sum(1 << (15 - l) for l in lengths if l)


def canonical_codes(lengths, strict=True):
    """the canonical Huffman code of RFC 1951 3.2.2: codes[s] for every symbol of length > 0 (None otherwise), most
    significant bit first.  An over-subscribed set is an error of the caller unless strict is False."""
    if any(l < 0 or l > 15 for l in lengths):
        raise ValueError("a code length outside 0..15")
    if strict and code_space_left(lengths) < 0:
        raise ValueError("over-subscribed set of code lengths")
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * 16
    code = 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = []
    for l in lengths:
        if l:
            codes.append(nxt[l])
            nxt[l] += 1
        else:
            codes.append(None)
    return codes


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def _as_list(lengths, low, what):
    """a dict {symbol: length} becomes the shortest list RFC 1951 allows (HLIT >= 257, HDIST >= 1); a list is taken as it is"""
    if isinstance(lengths, dict):
        n = max([low] + [s + 1 for s, l in lengths.items() if l])
        out = [0] * n
        for s, l in lengths.items():
            out[s] = l
        return out
    return list(lengths)


def flat(symbols):
    """a complete code over the symbols with two neighbouring lengths (one symbol: length 1)"""
    symbols = list(symbols)
    n = len(symbols)
    if n == 1:
        return {symbols[0]: 1}
    k = n.bit_length() - 1
    short = (2 << k) - n                                            # symbols of k bits, the other n - short of k + 1
    return {s: (k if i < short else k + 1) for i, s in enumerate(symbols)}


def ladder(short, long_):
    """lengths 1, 2, ..., k for the k symbols of `short`, and the 2^j symbols of `long_` share what is left at k + j bits"""
    k, j = len(short), len(long_).bit_length() - 1
    assert len(long_) == 1 << j and k + j <= 15
    out = {s: i + 1 for i, s in enumerate(short)}
    out.update({s: k + j for s in long_})
    return out


def length_symbol(length, by_284=False):
    """(symbol, extra bits, extra value) of a match length"""
    if length == 258:
        return (284, 5, 31) if by_284 else (285, 0, 0)
    if not 3 <= length <= 257 or by_284:
        raise ValueError("match length %r" % (length,))
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, LEN_BITS[i], length - LEN_BASE[i]


def distance_symbol(distance):
    if not 1 <= distance <= 32768:
        raise ValueError("match distance %r" % (distance,))
    i = max(k for k in range(30) if DIST_BASE[k] <= distance)
    return i, DIST_BITS[i], distance - DIST_BASE[i]


_LEN_SYM = {n: length_symbol(n) for n in range(3, 259)}
_DIST_SYM = {}


# ------------------------------------------------------------------------------------------------------------ writer
class Writer:
    """a deflate stream under construction: bits go into an integer accumulator, least significant bit first"""

    def __init__(self):
        self._acc = 0
        self._n = 0
        self._out = bytearray()

    def bits(self, value, n):
        if not 0 <= value < (1 << n):
            raise ValueError("%r does not fit %d bits" % (value, n))
        self._acc |= value << self._n
        self._n += n
        if self._n >= 256:
            self._spill()

    def _spill(self):
        k = self._n >> 3
        self._out += (self._acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self._acc >>= 8 * k
        self._n -= 8 * k

    def bit_length(self):
        return 8 * len(self._out) + self._n

    def align(self):
        """zero bits up to the next byte boundary; returns how many"""
        pad = -self._n % 8
        self.bits(0, pad)
        return pad

    def getvalue(self):
        self.align()
        self._spill()
        return bytes(self._out)

    # -- blocks
    def stored(self, data, last, nlen=None):
        if len(data) > 65535:
            raise ValueError("a stored block holds at most 65535 bytes")
        self.bits(1 if last else 0, 1)
        self.bits(0, 2)
        self.align()
        self.bits(len(data), 16)
        self.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        self._spill()
        assert self._n == 0
        self._out += data

    def fixed(self, tokens, last, eob=True):
        self.bits(1 if last else 0, 1)
        self.bits(1, 2)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST, eob, True)

    def dynamic(self, tokens, lit_lengths, dist_lengths, last, cl_lengths=None, rle=None, hclen=None, eob=True, strict=True):
        """lit_lengths / dist_lengths: {symbol: length} (written with the smallest HLIT / HDIST) or the full list.
        rle: None = every length written as itself; "runs" = 16/17/18 wherever they fit; or the list of code-length symbols
        itself, an int 0..15 or (16 | 17 | 18, repeat count), which must expand to the two lists unless strict is False.
        cl_lengths: {code-length symbol: length} (default: 4 bits for 0..12, 5 bits for 13..18); hclen: how many of them are
        written (default: the fewest).  strict=False lets wrong tables through, for the refusals."""
        lit = _as_list(lit_lengths, 257, "literal/length")
        dist = _as_list(dist_lengths, 1, "distance")
        if strict:
            if not 257 <= len(lit) <= 286 or not 1 <= len(dist) <= 30:
                raise ValueError("HLIT / HDIST out of range")
            if eob and not lit[256]:
                raise ValueError("no end-of-block code")
            for what, ls in (("literal/length", lit), ("distance", dist)):
                left, used = code_space_left(ls), [l for l in ls if l]
                if left < 0 or (left > 0 and not (used == [1] or (what == "distance" and not used))):
                    raise ValueError("%s set neither complete nor a single 1-bit code: %d left" % (what, left))
        both = lit + dist
        if rle is None:
            ops = list(both)
        elif rle == "runs":
            ops = run_length_ops(both)
        else:
            ops = list(rle)
            if strict and expand_ops(ops) != both:
                raise ValueError("the code-length symbols do not spell the two sets of lengths")
        if cl_lengths is None:
            cl_lengths = {s: (4 if s < 13 else 5) for s in range(19)}
        cl = [cl_lengths.get(s, 0) for s in range(19)]
        if strict and code_space_left(cl) != 0:
            raise ValueError("the code-length code must be complete")
        if any(l > 7 for l in cl):
            raise ValueError("a code-length code length above 7")
        n_cl = max([4] + [k + 1 for k in range(19) if cl[CL_ORDER[k]]])
        if hclen is not None:
            if not n_cl <= hclen <= 19:
                raise ValueError("HCLEN %r cannot hold these lengths" % (hclen,))
            n_cl = hclen
        self.bits(1 if last else 0, 1)
        self.bits(2, 2)
        self.bits(len(lit) - 257, 5)
        self.bits(len(dist) - 1, 5)
        self.bits(n_cl - 4, 4)
        for k in range(n_cl):
            self.bits(cl[CL_ORDER[k]], 3)
        cl_codes = canonical_codes(cl, strict)
        for op in ops:
            s, rep = (op, 0) if isinstance(op, int) else op
            if not cl[s]:
                raise ValueError("code-length symbol %d has no code" % s)
            self.bits(_rev(cl_codes[s], cl[s]), cl[s])
            if s == 16:
                self.bits(rep - 3, 2)
            elif s == 17:
                self.bits(rep - 3, 3)
            elif s == 18:
                self.bits(rep - 11, 7)
        self._tokens(tokens, lit + [0] * (288 - len(lit)), dist + [0] * (32 - len(dist)), eob, strict)

    def _tokens(self, tokens, lit, dist, eob, strict):
        lit_codes, dist_codes = canonical_codes(lit, strict), canonical_codes(dist, strict)
        lw = [None if c is None else (_rev(c, l), l) for c, l in zip(lit_codes, lit)]
        dw = [None if c is None else (_rev(c, l), l) for c, l in zip(dist_codes, dist)]
        acc, n = self._acc, self._n

        def need(table, s, what):
            if table[s] is None:
                raise ValueError("%s symbol %d has no code" % (what, s))
            return table[s]
        for t in tokens:
            if isinstance(t, int):
                w = lw[t] or need(lw, t, "literal")
                acc |= w[0] << n
                n += w[1]
            elif isinstance(t[0], str):
                if t[0] == "bits":
                    v, k = t[1] & ((1 << t[2]) - 1), t[2]
                else:
                    v, k = need(lw if t[0] == "lit" else dw, t[1], t[0])
                acc |= v << n
                n += k
            else:
                s, xb, xv = length_symbol(t[0], True) if len(t) > 2 and t[2] else _LEN_SYM[t[0]]
                w = lw[s] or need(lw, s, "length")
                acc |= (w[0] | (xv << w[1])) << n
                n += w[1] + xb
                d = _DIST_SYM.get(t[1])
                if d is None:
                    d = _DIST_SYM[t[1]] = distance_symbol(t[1])
                s, xb, xv = d
                w = dw[s] or need(dw, s, "distance")
                acc |= (w[0] | (xv << w[1])) << n
                n += w[1] + xb
            if n >= 512:
                self._acc, self._n = acc, n
                self._spill()
                acc, n = self._acc, self._n
        self._acc, self._n = acc, n
        if eob:
            w = need(lw, 256, "end-of-block")
            self.bits(w[0], w[1])


def run_length_ops(lengths):
    """a plain greedy 16/17/18 encoding of a sequence of code lengths"""
    ops, i, n = [], 0, len(lengths)
    while i < n:
        v = lengths[i]
        j = i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            rep = min(run, 138)
            ops.append((18, rep) if rep >= 11 else (17, rep))
            i += rep
        elif v != 0 and run >= 4:
            ops.append(v)
            rep = min(run - 1, 6)
            ops.append((16, rep))
            i += 1 + rep
        else:
            ops.append(v)
            i += 1
    return ops


def expand_ops(ops):
    out = []
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        elif op[0] == 16:
            out += [out[-1]] * op[1]
        else:
            out += [0] * op[1]
    return out


def expand(tokens):
    """the text of a token list: literals as they come, matches copied byte by byte"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, distance = t[0], t[1]
            if not (3 <= length <= 258 and 1 <= distance <= len(out)):
                raise ValueError("match %r at position %d" % (t, len(out)))
            for _ in range(length):
                out.append(out[-distance])
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------ walker
class DeflateError(ValueError):
    pass


def _lookup(lengths, what):
    """15-bit lookup: entry = length << 9 | symbol, 0 where no code begins.  zlib's rules: over-subscribed never; incomplete
    only as a single 1-bit code, or as no code at all for the distances"""
    left = code_space_left(lengths)
    used = [l for l in lengths if l]
    if left < 0:
        raise DeflateError("over-subscribed %s set" % what)
    if left > 0 and not (used == [1] or (what == "distance" and not used)) or (what == "code-length" and left):
        raise DeflateError("incomplete %s set" % what)
    codes = canonical_codes(lengths)
    table = [0] * 32768
    for s, l in enumerate(lengths):
        if l:
            table[_rev(codes[s], l)::1 << l] = [(l << 9) | s] * (1 << (15 - l))
    return table


_FIXED_TABLES = []


def walk(raw):
    """reads a deflate stream as puff.c would, keeps no text, and returns what it met:
      blocks            [stored, fixed, dynamic] block counts
      max_lit_code      longest literal/length code decoded        max_dist_code     longest distance code decoded
      lit_over_10       literal/length symbols decoded through more than 10 bits (the decoder's one-read table ends there)
      dist_over_8       distance symbols decoded through more than 8 bits
      max_distance      largest match distance                     matches           number of matches
      len258_by_284 / len258_by_285                                 matches of length 258 by either code
      one_dist_code_blocks / no_dist_code_blocks                    dynamic blocks with one / with no distance code
      max_span / span48 largest symbol (code + extra + code + extra) in bits / symbols of the full 48 bits
      max_cl_code       longest code-length code decoded           hclen             set of HCLEN values (4..19)
      cl_cross          16-, 17- or 18-runs that begin in the literal/length lengths and end in the distance lengths
      stored_pads       set of padding bit counts before stored LENs; stored_lens: set of stored LENs
      empty_blocks      fixed or dynamic blocks that hold end-of-block alone
      eob_over_10       end-of-block symbols decoded through more than 10 bits
      text_len, bits    bytes of text, bits of the stream consumed
    Raises DeflateError on anything zlib would refuse."""
    f = dict(blocks=[0, 0, 0], max_lit_code=0, max_dist_code=0, lit_over_10=0, dist_over_8=0, max_distance=0, matches=0,
             len258_by_284=0, len258_by_285=0, one_dist_code_blocks=0, no_dist_code_blocks=0, max_span=0, span48=0, max_cl_code=0,
             hclen=set(), cl_cross=set(), stored_pads=set(), stored_lens=set(), empty_blocks=0, eob_over_10=0, text_len=0, bits=0)
    if not _FIXED_TABLES:
        _FIXED_TABLES.extend([_lookup(FIXED_LIT, "literal/length"), _lookup(FIXED_DIST, "distance")])
    data = bytes(raw) + bytes(16)
    n_bits = 8 * len(raw)
    at = 0                                                          # next byte of data
    buf = cnt = 0
    pos = 0
    max_l = max_d = over10 = over8 = max_dist = matches = by284 = by285 = max_span = span48 = 0
    last = False
    while not last:
        if cnt < 48:
            buf |= int.from_bytes(data[at:at + 8], "little") << cnt
            at += 8
            cnt += 64
        last = bool(buf & 1)
        kind = (buf >> 1) & 3
        buf >>= 3
        cnt -= 3
        if 8 * at - cnt > n_bits:
            raise DeflateError("stream ends early")
        if kind == 3:
            raise DeflateError("reserved block type")
        if kind == 0:
            pad = cnt & 7
            buf >>= pad
            cnt -= pad
            f["stored_pads"].add(pad)
            start = at - cnt // 8
            if start + 4 > len(raw):
                raise DeflateError("stream ends early")
            length, nlen = struct.unpack_from("<HH", data, start)
            if length ^ 0xffff != nlen:
                raise DeflateError("stored block length")
            if start + 4 + length > len(raw):
                raise DeflateError("stream ends early")
            f["stored_lens"].add(length)
            f["blocks"][0] += 1
            pos += length
            at = start + 4 + length
            buf = cnt = 0
            continue
        if kind == 1:
            lt, dt = _FIXED_TABLES
            f["blocks"][1] += 1
        else:
            f["blocks"][2] += 1
            if cnt < 48:
                buf |= int.from_bytes(data[at:at + 8], "little") << cnt
                at += 8
                cnt += 64
            n_lit, n_dist, n_cl = (buf & 31) + 257, ((buf >> 5) & 31) + 1, ((buf >> 10) & 15) + 4
            buf >>= 14
            cnt -= 14
            if n_lit > 286 or n_dist > 30:
                raise DeflateError("too many length or distance symbols")
            f["hclen"].add(n_cl)
            cl = [0] * 19
            for k in range(n_cl):
                if cnt < 48:
                    buf |= int.from_bytes(data[at:at + 8], "little") << cnt
                    at += 8
                    cnt += 64
                cl[CL_ORDER[k]] = buf & 7
                buf >>= 3
                cnt -= 3
            ct = _lookup(cl, "code-length")
            lens = []
            total = n_lit + n_dist
            while len(lens) < total:
                if cnt < 48:
                    buf |= int.from_bytes(data[at:at + 8], "little") << cnt
                    at += 8
                    cnt += 64
                e = ct[buf & 32767]
                if not e:
                    raise DeflateError("invalid code-length code")
                l, s = e >> 9, e & 511
                buf >>= l
                cnt -= l
                f["max_cl_code"] = max(f["max_cl_code"], l)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise DeflateError("a repeat with no length before it")
                    v, rep, xb = lens[-1], 3 + (buf & 3), 2
                elif s == 17:
                    v, rep, xb = 0, 3 + (buf & 7), 3
                else:
                    v, rep, xb = 0, 11 + (buf & 127), 7
                buf >>= xb
                cnt -= xb
                if len(lens) + rep > total:
                    raise DeflateError("a repeat past the last length")
                if len(lens) < n_lit < len(lens) + rep:
                    f["cl_cross"].add(s)
                lens += [v] * rep
            if not lens[256]:
                raise DeflateError("no end-of-block code")
            lt = _lookup(lens[:n_lit], "literal/length")
            dt = _lookup(lens[n_lit:], "distance")
            used = sum(1 for l in lens[n_lit:] if l)
            f["one_dist_code_blocks"] += used == 1
            f["no_dist_code_blocks"] += used == 0
        first = True
        while True:
            if cnt < 48:
                buf |= int.from_bytes(data[at:at + 8], "little") << cnt
                at += 8
                cnt += 64
            e = lt[buf & 32767]
            if not e:
                raise DeflateError("invalid literal/length code")
            l = e >> 9
            s = e & 511
            if l > max_l:
                max_l = l
            if l > 10:
                over10 += 1
            if s < 256:
                buf >>= l
                cnt -= l
                pos += 1
                first = False
                continue
            if s == 256:
                buf >>= l
                cnt -= l
                f["empty_blocks"] += first
                f["eob_over_10"] += l > 10
                break
            first = False
            if s > 285:
                raise DeflateError("invalid literal/length symbol")
            xb = LEN_BITS[s - 257]
            length = LEN_BASE[s - 257] + ((buf >> l) & ((1 << xb) - 1))
            buf >>= l + xb
            e = dt[buf & 32767]
            if not e:
                raise DeflateError("invalid distance code")
            dl = e >> 9
            ds = e & 511
            if ds > 29:
                raise DeflateError("invalid distance symbol")
            yb = DIST_BITS[ds]
            dist = DIST_BASE[ds] + ((buf >> dl) & ((1 << yb) - 1))
            buf >>= dl + yb
            span = l + xb + dl + yb
            cnt -= span
            if dist > pos:
                raise DeflateError("distance too far back")
            if dl > max_d:
                max_d = dl
            if dl > 8:
                over8 += 1
            if dist > max_dist:
                max_dist = dist
            if span > max_span:
                max_span = span
            if span == 48:
                span48 += 1
            if length == 258:
                if s == 284:
                    by284 += 1
                else:
                    by285 += 1
            matches += 1
            pos += length
        if 8 * at - cnt > n_bits:
            raise DeflateError("stream ends early")
    f.update(max_lit_code=max_l, max_dist_code=max_d, lit_over_10=over10, dist_over_8=over8, max_distance=max_dist, matches=matches,
             len258_by_284=by284, len258_by_285=by285, max_span=max(max_span, max_l), span48=span48, text_len=pos, bits=8 * at - cnt)
    return f


def holds(facts, required):
    """the required facts a stream does not have: {name: (op, value)} with ==, >=, <=, or `has` for the set-valued ones"""
    missing = []
    for name, (op, value) in required.items():
        got = facts[name]
        ok = {"==": lambda: got == value, ">=": lambda: got >= value, "<=": lambda: got <= value,
              "has": lambda: set(value) <= set(got)}[op]()
        if not ok:
            missing.append((name, op, value, got))
    return missing


# -------------------------------------------------------------------------------------------------------- containers
def fh_member_raw(body, text):
    """tests/test_gpu_inflate.py's fh_member around a deflate stream made elsewhere: a gzip member whose "FH" extra subfield
    holds its own size; CRC-32 and ISIZE are those of `text`"""
    size = 10 + 2 + 12 + len(body) + 8
    hdr = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 12) + b"FH" + struct.pack("<HQ", 8, size)
    return hdr + body + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


def bgzf_member_raw(body, text):
    """a BGZF block (the "BC" subfield holds the block size - 1, so at most 64 KB) around a deflate stream made elsewhere"""
    size = 10 + 2 + 6 + len(body) + 8
    if size > 65536:
        raise ValueError("a BGZF block holds at most 65536 bytes")
    hdr = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, size - 1)
    return hdr + body + struct.pack("<II", zlib.crc32(text), len(text))


# --------------------------------------------------------------------------------------------------------- catalogue
CATALOGUE = []                      # (name, body, text, required facts)
BGZF_SUBSET = []                    # names
REFUSALS = []                       # (name, body, text, E_*, raw)

LEN_SET = (3, 63, 64, 65, 128, 129, 257, 258)


def _noise(seed, n):
    return list(random.Random(seed).randbytes(n))


def _one(name, tokens, required, block="fixed", bgzf=False, **kw):
    """a member of one block"""
    w = Writer()
    if block == "fixed":
        w.fixed(tokens, True)
    else:
        w.dynamic(tokens, last=True, **kw)
    _add(name, w, expand(tokens), required, bgzf)


def _add(name, w, text, required, bgzf=False):
    assert name not in [c[0] for c in CATALOGUE]
    required = dict(required)
    required.setdefault("text_len", ("==", len(text)))
    CATALOGUE.append((name, w.getvalue(), text, required))
    if bgzf:
        BGZF_SUBSET.append(name)


def _all_literals():
    """every byte and end-of-block: 257 symbols, 255 of 8 bits and two of 9"""
    return flat(list(range(256)) + [256])


def _window():
    hist = _noise(11, WIN)
    # the window's far edge: 32768 literals, then the match that reads all the way back - dist == pos at pos 32768
    _one("win_258_at_32768", hist + [(258, WIN)], dict(max_distance=("==", WIN), len258_by_285=("==", 1), matches=("==", 1)),
         bgzf=True)
    # the distances zlib's encoder never writes (above 32768 - 262), each with lengths on both sides of the 64-lane copy
    for d in (32507, 32767, 32768):
        for n in (3, 64, 65, 258):
            _one("win_d%d_len%d" % (d, n), hist + [7, 8, 9] + [(n, d)] + [1, 2, 3], dict(max_distance=("==", d), matches=("==", 1)),
                 block="dynamic" if n in (3, 65) else "fixed", lit_lengths=flat(list(range(257)) + [length_symbol(n)[0]]),
                 dist_lengths=flat([29, 28]))
    # dist == pos at pos 1
    _one("dist_eq_pos_at_1", [65, (258, 1), 66, (3, 1)], dict(max_distance=("==", 1), matches=("==", 2)), bgzf=True)
    # matches that straddle the seams at which the window is flushed: k bytes of the match lie before the seam
    for k in (0, 1, 129, 257, 258):
        tokens, at = [], 0
        rng = random.Random(20 + k)
        for seam, d in ((FLUSH, 5000), (WIN, 32767 - k), (WIN + FLUSH, 32768)):
            fill = seam - k - at
            tokens += list(rng.randbytes(fill)) + [(258, d)]
            at += fill + 258
        tokens += list(rng.randbytes(40))
        _one("seams_%d_before" % k, tokens, dict(matches=("==", 3), max_distance=("==", 32768)))
    # texts that end on a seam, 1 byte and 257 bytes after one: the last flush and the tail copy
    for end in (FLUSH, FLUSH + 1, FLUSH + 257, WIN, WIN + 1, WIN + 257):
        rng = random.Random(end)
        tokens, at = list(rng.randbytes(1500)), 1500
        while end - at > 300:
            tokens.append((258, rng.randrange(1, 1500)))
            at += 258
        if end - at > 258:                                          # 42 < end - at <= 300 here
            tokens.append((end - at - 200, 77))
            at = end - 200
        tokens.append((end - at, 1499))
        _one("ends_at_%d" % end, tokens, dict(text_len=("==", end), matches=(">=", 50)), bgzf=end in (FLUSH + 1, WIN + 257))


def _copies():
    # the two copy branches: len <= 64 and dist >= len in one go, everything else in slices of 64 with i % dist
    for n in LEN_SET:
        rng = random.Random(100 + n)
        tokens = list(rng.randbytes(300))
        dists = []
        for d in (1, 2, 3, n - 1, n, n + 1, 63, 64, 65):
            tokens += [(n, d)] + list(rng.randbytes(5))
            dists.append(d)
        _one("copy_len%d" % n, tokens, dict(matches=("==", 9), max_distance=("==", max(dists))), bgzf=n in (65, 258))


def _long_codes():
    rng = random.Random(7)
    # literal/length ladder 1, 2, ..., 14, 15, 15 - the 15-bit codes on two literals
    short = [256] + list(range(32, 45))
    tokens = [rng.choice([200, 201, 201, 201, 33, 40, 44]) for _ in range(4000)]
    _one("ladder_lit15", tokens, dict(max_lit_code=("==", 15), lit_over_10=(">=", 2000), no_dist_code_blocks=("==", 0)), block="dynamic",
         lit_lengths=ladder(short, [200, 201]), dist_lengths={0: 1, 1: 1}, bgzf=True)
    # ... on length codes 277-284 (12 short codes, eight of 15 bits)
    short = [256, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 285]
    tokens = list(rng.choice(short[1:11]) for _ in range(400))
    for k in range(600):
        tokens += [(rng.randrange(67, 258), rng.randrange(1, 400)), rng.choice(short[1:11])]
    _one("ladder_len15", tokens, dict(max_lit_code=("==", 15), lit_over_10=(">=", 600)), block="dynamic",
         lit_lengths=ladder(short, list(range(277, 285))), dist_lengths=flat(range(18)))
    # ... and on end-of-block, in a run of blocks
    w, toks = Writer(), []
    lens = ladder(list(range(97, 111)), [256, 111])
    for k in range(6):
        t = [rng.choice([97, 98, 99, 110, 111]) for _ in range(50 * k)]
        w.dynamic(t, lens, {0: 1, 1: 1}, last=k == 5)
        toks += t
    _add("ladder_eob15", w, expand(toks), dict(eob_over_10=("==", 6), max_lit_code=("==", 15), empty_blocks=("==", 1)))
    # the same ladder on the distance alphabet, codes 28 and 29 at 15 bits
    hist = _noise(12, WIN)
    tokens = list(hist)
    for k in range(800):
        tokens += [(rng.randrange(3, 40), rng.choice([rng.randrange(16385, 32769), rng.randrange(16385, 32769), rng.randrange(1, 129)])),
                   rng.randrange(256)]
    tokens += [(10, 32768), (39, 16385), (3, 128)]
    dl = ladder([0, 2, 4, 6, 8, 10, 12, 1, 3, 5, 7, 9, 11, 13], [28, 29])
    _one("ladder_dist15", tokens, dict(max_dist_code=("==", 15), dist_over_8=(">=", 400), max_distance=(">=", 32507)), block="dynamic",
         lit_lengths=flat(list(range(257)) + list(range(257, 280))), dist_lengths=dl)
    # a block made only of full-span symbols, 15 + 5 + 15 + 13 bits, back to back
    w = Writer()
    w.fixed(hist, False)
    tokens = [(rng.randrange(131, 258), rng.randrange(16385, 32769)) for _ in range(300)]
    w.dynamic(tokens, ladder([256] + list(range(12)), [281, 282, 283, 284]), dl, last=True)
    _add("full_span_only", w, expand(hist + tokens), dict(max_span=("==", 48), span48=("==", 300), lit_over_10=("==", 300),
                                                          dist_over_8=("==", 300), matches=("==", 300)))
    # full-span symbols behind literals of 2 to 13 bits: a 48-bit symbol begins at every bit offset of the walk's 64-bit views,
    # also where exactly 48 valid bits are left (`p + 48 <= B.cnt`) - back to back they begin at multiples of 48 only
    w = Writer()
    w.fixed(hist, False)
    tokens = []
    for k in range(300):
        tokens += [rng.randrange(1, 12) for _ in range(rng.randrange(4))] + [(rng.randrange(131, 258), rng.randrange(16385, 32769))]
    w.dynamic(tokens, ladder([256] + list(range(12)), [281, 282, 283, 284]), dl, last=True)
    _add("full_span_after_literals", w, expand(hist + tokens), dict(max_span=("==", 48), span48=("==", 300), lit_over_10=(">=", 300)))
    # the seams of the one-read tables: literal/length codes of exactly 10 and 11 bits, distance codes of 8 and 9 bits
    ll = {256: 1, 257: 2, 258: 3, 270: 4}
    ll.update({s: 10 for s in range(48, 80)})
    ll.update({s: 11 for s in range(80, 144)})
    dd = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 8, 7: 8, 8: 9, 9: 9, 10: 9, 11: 9}
    tokens = [rng.randrange(48, 144) for _ in range(300)]
    for k in range(1500):
        tokens += [rng.randrange(48, 144), (rng.choice([3, 4, 23, 24, 25, 26]), rng.randrange(1, 65) if k % 3 else rng.randrange(9, 65))]
    _one("table_seams_10_11_8_9", tokens, dict(max_lit_code=("==", 11), lit_over_10=(">=", 500), max_dist_code=("==", 9), dist_over_8=(">=", 300)),
         block="dynamic", lit_lengths=ll, dist_lengths=dd, bgzf=True)
    # a 7-bit code-length code: lengths 1..6 and 7, 7 over the eight code-length symbols the header uses
    ll = {s: 8 for s in range(254)}
    ll.update({254: 9, 255: 9, 256: 9, 257: 9})                     # 254/256 + 4/512 = 1
    tokens = _noise(13, 3000) + [(3, 1)]
    cl = {8: 1, 9: 2, 18: 3, 5: 4, 0: 5, 17: 6, 16: 7, 4: 7}
    dl5 = {0: 5, 1: 5, 2: 4, 3: 4, 4: 4, 5: 4, 6: 4, 7: 4, 8: 4, 9: 4, 10: 4, 11: 4, 12: 4, 13: 4, 14: 4, 15: 4, 16: 4}
    _one("cl_code_7_bits", tokens, dict(max_cl_code=("==", 7)), block="dynamic", lit_lengths=ll, dist_lengths=dl5, cl_lengths=cl, rle="runs")


def _short_codes():
    # 'a' and end-of-block at one bit each: 64 symbols in every 64-bit view of the symbol walk
    _one("one_bit_literals", [97] * 100_000, dict(max_lit_code=("==", 1), max_span=("==", 1), no_dist_code_blocks=("==", 0)), block="dynamic",
         lit_lengths={97: 1, 256: 1}, dist_lengths={0: 1, 1: 1})


def _forms():
    rng = random.Random(9)
    text = list(rng.randbytes(400))
    # length 258 as code 284 with extra bits 31
    tokens = text + [(258, 300, True), 1, (258, 1, True), (258, 399), (257, 2)]
    _one("len258_by_284_fixed", tokens, dict(len258_by_284=("==", 2), len258_by_285=("==", 1)), bgzf=True)
    _one("len258_by_284_dynamic", tokens, dict(len258_by_284=("==", 2), len258_by_285=("==", 1)), block="dynamic",
         lit_lengths=flat(list(range(256)) + [256, 284, 285]), dist_lengths=flat([0, 1, 16, 17]), rle="runs")
    # one distance code of length 1: in use (distances 5 and 6), and present but unused
    tokens = text + [(9, 5), 3, (70, 6), 4, (258, 5)]
    _one("one_dist_code_used", tokens, dict(one_dist_code_blocks=("==", 1), matches=("==", 3)), block="dynamic",
         lit_lengths=flat(list(range(256)) + [256, 263, 277, 285]), dist_lengths={4: 1}, bgzf=True)
    _one("one_dist_code_unused", text, dict(one_dist_code_blocks=("==", 1), matches=("==", 0)), block="dynamic",
         lit_lengths=_all_literals(), dist_lengths={0: 1})
    # no distance code at all (RFC 1951 3.2.7): HDIST = 1 with that one length 0, and 30 lengths all 0
    _one("no_dist_code_hdist1", text, dict(no_dist_code_blocks=("==", 1), matches=("==", 0)), block="dynamic",
         lit_lengths=_all_literals(), dist_lengths=[0], bgzf=True)
    _one("no_dist_code_hdist30", text, dict(no_dist_code_blocks=("==", 1), matches=("==", 0)), block="dynamic",
         lit_lengths=_all_literals(), dist_lengths=[0] * 30, rle="runs")
    # a dynamic block that holds end-of-block alone (a single 1-bit code), between two blocks with text
    w = Writer()
    w.fixed(text[:100], False)
    w.dynamic([], {256: 1}, {0: 1, 1: 1}, last=False, rle="runs")
    w.dynamic([], {256: 1}, [0], last=False, rle="runs")
    w.fixed(text[100:] + [(30, 350)], True)
    _add("eob_alone_dynamic", w, expand(text + [(30, 350)]), dict(empty_blocks=("==", 2), blocks=("==", [0, 2, 2]), no_dist_code_blocks=("==", 1)),
         bgzf=True)
    # an empty fixed block between blocks
    w = Writer()
    w.fixed(text[:123], False)
    w.fixed([], False)
    w.stored(bytes(text[123:200]), False)
    w.fixed([], False)
    w.fixed(text[200:] + [(100, 400)], True)
    _add("empty_fixed_between", w, expand(text + [(100, 400)]), dict(empty_blocks=("==", 2), blocks=("==", [1, 4, 0])), bgzf=True)
    # stored blocks of 0, 1 and 65535 bytes after every number of leftover bits.  A fixed block of only 9-bit literals
    # (bytes >= 144) moves the bit position by 3 + 9 k + 7, so k = 0..7 gives every position
    w, out, pads = Writer(), bytearray(), set()
    for k in range(8):
        for n in (0, 1):
            lits = [200 + k] * ((k + n) % 8)
            w.fixed(lits, False)
            pads.add(-(w.bit_length() + 3) % 8)
            data = bytes(rng.randbytes(n))
            w.stored(data, False)
            out += bytes(lits) + data
    w.fixed([1], True)
    assert pads == set(range(8))
    _add("stored_after_bits", w, bytes(out) + b"\1", dict(stored_pads=("==", set(range(8))), stored_lens=("==", {0, 1})), bgzf=True)
    for pad in range(1, 8):
        k = next(k for k in range(8) if -(13 + 9 * k) % 8 == pad)
        data = bytes(rng.randbytes(65535))
        w = Writer()
        w.fixed([200 + k] * k, False)
        w.stored(data, False)
        w.fixed([(258, 1)], True)
        _add("stored_65535_after_%d_bits" % pad, w, bytes([200 + k] * k) + data + data[-1:] * 258,
             dict(stored_pads=("==", {pad}), stored_lens=("==", {65535}), blocks=("==", [1, 2, 0])))
    # stored -> fixed -> dynamic -> stored, none of them byte-aligned, every match reaching back across a boundary
    w = Writer()
    w.fixed([201], False)                                           # 19 bits before the first stored block
    a = bytes(rng.randbytes(700))
    w.stored(a, False)
    f_tok = [(200, 700), 202, (258, 650), (5, 1)]
    w.fixed(f_tok, False)
    d_tok = [(100, 1164), 66, (258, 600), (64, 64), 65, 65]
    w.dynamic(d_tok, flat([65, 66, 256, 276, 279, 285]), flat([11, 18, 19, 20]), last=False, rle="runs")
    b = bytes(rng.randbytes(301))
    w.stored(b, False)
    tail = [(258, 301), (258, 2000), (3, 302)]
    w.fixed(tail, True)
    text = expand([201] + list(a) + f_tok + d_tok + list(b) + tail)
    _add("mixed_blocks_unaligned", w, text, dict(blocks=("==", [2, 3, 1]), matches=("==", 9), max_distance=("==", 2000)), bgzf=True)
    # HCLEN at its ends: 5 (only 16, 17, 18, 0 and 8 have a code: 255 literals and end-of-block at 8 bits) and 19
    ll = {s: 8 for s in range(255)}
    ll[256] = 8
    tokens = [b for b in rng.randbytes(500) if b != 255]
    _one("hclen_5", tokens, dict(hclen=("==", {5})), block="dynamic", lit_lengths=ll, dist_lengths=[0],
         cl_lengths={8: 1, 0: 2, 18: 3, 17: 4, 16: 4}, rle=[8, (16, 6)] * 36 + [8, 8, 8] + [0, 8, 0])
    _one("hclen_19", tokens, dict(hclen=("==", {19})), block="dynamic", lit_lengths=ll, dist_lengths={0: 15, 1: 15, 2: 14, 3: 13, 4: 12, 5: 11, 6: 10,
         7: 9, 8: 8, 9: 7, 10: 6, 11: 5, 12: 4, 13: 3, 14: 2, 15: 1})
    # a 16-run and an 18-run that begin in the literal/length lengths and end in the distance lengths
    lit = [10] * 256 + [2, 2, 2]                                    # 256/1024 + 3/4 = 1: HLIT = 259 ends in 2, 2, 2
    _one("run16_crosses", tokens, dict(cl_cross=("==", {16})), block="dynamic", lit_lengths=lit, dist_lengths=[2, 2, 2, 2],
         rle=[10, (16, 6)] * 36 + [10, (16, 3)] + [2, 2, (16, 5)])
    lit = [9] * 256 + [1] + [0] * 29                                # 256/512 + 1/2 = 1: HLIT = 286 ends in 29 lengths of 0
    _one("run18_crosses", tokens, dict(cl_cross=("==", {18})), block="dynamic", lit_lengths=lit, dist_lengths=[0] * 20 + [1, 1],
         rle=[9, (16, 6)] * 36 + [9, (16, 3)] + [1, (18, 49), 1, 1])


def _containers():
    # member texts as stored blocks; odd sizes make the members after them begin unaligned
    for n in (0, 1, 15, 16, 17, 31, 33, 4095, 4096, 4097):
        data = bytes(random.Random(300 + n).randbytes(n))
        w = Writer()
        w.stored(data, True)
        _add("stored_text_%d" % n, w, data, dict(blocks=("==", [1, 0, 0])), bgzf=n in (0, 1, 17, 4097))


def _refusals():
    text = list(random.Random(17).randbytes(50))

    def add(name, w, expected, code, raw=True):
        REFUSALS.append((name, w.getvalue(), bytes(expected), code, raw))

    def fixed(tokens, **kw):
        w = Writer()
        w.fixed(tokens, True, **kw)
        return w

    def broken(tokens=(), lit=None, dist=None, eob=True, **kw):
        w = Writer()
        w.fixed(text, False)
        w.dynamic(list(tokens), _all_literals() if lit is None else lit, {0: 1, 1: 1} if dist is None else dist, last=True, eob=eob, strict=False, **kw)
        return w
    # match copy, fhx_inflate.inc `if (dist > pos) err = E_DISTANCE`
    ds, xb, xv = distance_symbol(len(text) + 1)
    add("distance_one_beyond_pos", fixed(text + [("lit", 257), ("dist", ds), ("bits", xv, xb)]), text, E_DISTANCE)
    # `if (len > out_len - pos) err = E_OUTPUT`: the stream is sound, the trailer says 5 bytes less
    add("match_past_isize", fixed(text + [(30, 20)]), expand(text + [(30, 20)])[:-5], E_OUTPUT, raw=False)
    # construct() < 0 -> E_TABLE
    lit = _all_literals()
    lit[0] = 7
    add("oversubscribed_literals", broken(lit=lit), text, E_TABLE)
    add("oversubscribed_distances", broken(dist={0: 1, 1: 1, 2: 1}), text, E_TABLE)
    # construct() > 0 with two codes -> E_TABLE
    add("incomplete_two_literal_codes", broken(lit={65: 2, 256: 2}), text, E_TABLE)
    add("incomplete_two_distance_codes", broken(dist={0: 2, 1: 2}), text, E_TABLE)
    # entry_of() gives kind 3 to 286, 287, 30 and 31 -> E_SYMBOL on either path
    for s in (286, 287):
        add("fixed_symbol_%d" % s, fixed(text + [("lit", s)]), text, E_SYMBOL)
    for s in (30, 31):
        add("fixed_distance_%d" % s, fixed(text + [("lit", 257), ("dist", s)]), text, E_SYMBOL)
    # one distance code '0': '1' is in neither dist_fast nor decode_slow's walk -> E_SYMBOL
    lit = flat(list(range(256)) + [256, 257])
    w = broken(tokens=text[:10] + [("lit", 257), ("bits", 1, 1), ("bits", 0, 20)], lit=lit, dist={3: 1})
    add("unused_word_of_one_distance_code", w, text + text[:10], E_SYMBOL)
    # a length symbol in a block without distance codes: the same exit
    w = broken(tokens=text[:10] + [("lit", 257), ("bits", 0, 20)], lit=lit, dist=[0])
    add("length_without_distance_codes", w, text + text[:10], E_SYMBOL)
    # `(len ^ 0xffff) != nlen` -> E_STORED
    w = Writer()
    w.fixed(text, False)
    w.stored(b"abc", True, nlen=0xfffd)
    add("len_nlen_mismatch", w, bytes(text) + b"abc", E_STORED)
    # `s == 16 && at == 0` -> E_TABLE;  `at + rep > total` -> E_TABLE;  `lens[256] == 0` -> E_TABLE
    add("run16_is_the_first_length", broken(rle=[(16, 3)] + [8] * 254), text, E_TABLE)
    ll = _as_list(_all_literals(), 257, "")
    add("run_past_the_last_length", broken(lit=ll, dist=[1, 1], rle=ll + [1, (16, 3)]), text, E_TABLE)
    add("run18_past_the_last_length", broken(lit=ll, dist=[1, 1], rle=ll[:250] + [(18, 138)]), text, E_TABLE)
    lit = flat(range(256))
    add("no_end_of_block_code", broken(lit=_as_list(lit, 257, ""), eob=False), text, E_TABLE)


def _build():
    _window()
    _copies()
    _long_codes()
    _short_codes()
    _forms()
    _containers()
    _refusals()


_build()
BY_NAME = {c[0]: c for c in CATALOGUE}
