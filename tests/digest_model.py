"""Plain-Python model of fithic_amd.digest (reference: fithic/utils/createFitHiCFragments-nonfixedsize.sh).  Step 1 restates HiC-Pro's
digest_genome.py as the module's docstring states it - a look-ahead regex over each contig's joined, lower-cased sequence - and
step 2 restates the script's loop over the bed file (:18-33).  refusal() restates the grammar of the regular text.  Not a test."""
import itertools
import re

ENZYMES = {"hindiii": "A^AGCTT", "mboi": "^GATC", "dpnii": "^GATC", "bglii": "A^GATCT"}
(OK, BYTES, BLANK, LONG_LINE, CONTIG_LENGTH, EMPTY_NAME, NAME_CHARS, DUPLICATE, NO_HEADER) = range(9)
MAX_LINE = 4096


def motifs_of(sites):
    """[(lower-case motif, offset)] with every N expanded, in the order given"""
    out = []
    for site in sites:
        site = ENZYMES.get(site.lower(), site).upper()
        offset = site.index("^")
        for letters in itertools.product(*[("ACGT" if c == "N" else c) for c in site.replace("^", "")]):
            out.append(("".join(letters).lower(), offset))
    return out


def lines_of(data):
    """the lines of a file as `for line in f` gives them, without their \\n"""
    lines = data.decode("latin-1").split("\n")
    return lines[:-1] if lines[-1] == "" else lines


def contigs(data, sites):
    """[(name, length, [sorted sites])] in file order"""
    found, current = [], None
    for line in lines_of(data):
        if line.startswith(">"):
            current = (line.split()[0][1:], [])
            found.append(current)
        elif current is not None:
            current[1].append(line.lower().strip())
    out = []
    for name, parts in found:
        seq = "".join(parts)
        cuts = sorted(m.start() + offset for motif, offset in motifs_of(sites) for m in re.finditer("(?=%s)" % motif, seq))
        out.append((name, len(seq), cuts))
    return out


def bed(data, sites):
    out = []
    for name, length, cuts in contigs(data, sites):
        for k, (start, end) in enumerate(zip([0] + cuts, cuts + [length])):
            out.append("%s\t%d\t%d\tHIC_%s_%d\t0\t+\n" % (name, start, end, name, k + 1))
    return "".join(out).encode("latin-1")


def loop(bed_bytes):
    """createFitHiCFragments-nonfixedsize.sh:18-33 on a bed file -> (what $outfile holds, stdout)"""
    rows = [p.split() for p in bed_bytes.decode("latin-1").splitlines()]
    curr, ctr, out, said = rows[0][0], 1, [], []
    for line in rows:
        if curr != line[0]:
            said.append("Working on %s\n" % curr)
            ctr += 1
            curr = line[0]
        out.append("chr%d\t0\t%s\t1\t1\n" % (ctr, line[2]))
    said.append("Working on %s\n" % curr)
    return "".join(out).encode("latin-1"), "".join(said)


def fragments(data, sites):
    return loop(bed(data, sites))[0]


def stdout(data, sites):
    return loop(bed(data, sites))[1]


def refusal(data):
    """None, or (1-based line, reason) of the smallest refused line; on one line the first refused byte decides, before the name"""
    seen, any_header = set(), False
    raw = data.split(b"\n")
    if raw[-1] == b"":
        raw.pop()
        ends = [True] * len(raw)
    else:
        ends = [True] * (len(raw) - 1) + [False]
    for number, (line, newline) in enumerate(zip(raw, ends), 1):
        header = line.startswith(b">")
        for k, c in enumerate(line):
            if k >= MAX_LINE:
                return number, LONG_LINE
            if c == 13:
                if not (k == len(line) - 1 and newline):
                    return number, BYTES
            elif c in (32, 9):
                if not header:
                    return number, BLANK
            elif c < 32 or c >= 127:
                return number, BYTES
        if header:
            any_header = True
            name = line.decode("latin-1").split()[0][1:]
            if name == "":
                return number, EMPTY_NAME
            if any(c in name for c in "*?[\\"):
                return number, NAME_CHARS
            if name in seen:
                return number, DUPLICATE
            seen.add(name)
    return None if any_header else (1, NO_HEADER)
