"""merge-filter-parallelized.sh restated in plain Python on top of tests/mergefilter_model.py (reference:
fithic/utils/merge-filter-parallelized.sh:21-25 run with mawk 1.3.4 under LC_ALL=C): what fithic_amd.mergefilter_parallel and
csrc/fhx_sigsplit.inc must give, byte for byte.  Pinned to the real script by tests/golden/mergesplit and to the installed awk by
tests/test_mergesplit_host.py.

The list of chromosomes is field 1 of every line, line 1 included, split at tabs (`cut -f1 | sort | uniq`); a row after line 1
goes to chromosome c when `$1==c && $3==c && $7<=fdr`.  The `$7` decision is mergefilter_model's.  awk compares `$1==c` as numbers
when both sides look numeric, so the grammar takes only names for which that equality is byte equality (name_reason) and the
model may compare bytes.  Everything the grammar leaves out is refused with the smallest offending 1-based line number; the order of
the checks on one line is the kernel's: bytes, length, token count, the tab after token 1, token 1, token 3, field 7.
"""
import re

import mergefilter_model as mm

NAME, NAME_TAB, NAME_BYTES, NAME_NUMERIC, NAMES = 8, 10, 11, 12, 13
MAX_NAMES = 4096
MAX_NAME = 63
_NAME = re.compile(rb"[A-Za-z0-9_][A-Za-z0-9_.-]*\Z")
_CERTAIN = set(b"_ghijklmnoqrstuvwyzGHIJKLMNOQRSTUVWYZ")                # strtod cannot run past one of these


def name_reason(name):
    """0 for a name that is taken, else why it is not"""
    if len(name) > MAX_NAME:
        return NAME
    if not _NAME.match(name):
        return NAME_BYTES
    if not 0x30 <= name[0] <= 0x39:
        return 0
    if name.isdigit():
        return 0 if len(name) <= 15 and (name == b"0" or name[0] != 0x30) else NAME_NUMERIC
    return 0 if _CERTAIN & set(name) else NAME_NUMERIC


def split(data, fdr):
    """-> {name: subset} for every name of `cut -f1 | sort | uniq`; the kept lines verbatim, in order, each ending in a newline"""
    fdr = mm.check_fdr(fdr)
    out = {}
    for number, line in enumerate(mm.lines_of(data), 1):
        bad = mm._BAD_BYTE.search(line)
        if bad and bad.start() < mm.MAX_LINE:
            raise mm.Refused(mm.BYTES, number)
        if len(line) > mm.MAX_LINE:
            raise mm.Refused(mm.LONG_LINE, number)
        tokens = line.replace(b"\t", b" ").split()
        if number != 1 and len(tokens) < 7:
            raise mm.Refused(mm.TOKENS, number)
        first = line.split(b"\t", 1)[0]                                   # cut's field 1
        if b"\t" not in line or not tokens or first != tokens[0]:         # ... is awk's $1
            raise mm.Refused(NAME_TAB, number)
        for name in tokens[0:1] if number == 1 else (tokens[0], tokens[2]):
            if name_reason(name):
                raise mm.Refused(name_reason(name), number)
        out.setdefault(first, [])
        if number == 1:
            continue
        if mm.classify(tokens[6]) is None:
            raise mm.Refused(mm.FIELD, number)
        if tokens[2] == first and mm.keeps(tokens[6], fdr):
            out[first].append(line + b"\n")
    if len(out) > MAX_NAMES:
        raise mm.Refused(NAMES, 0)
    return {name: b"".join(lines) for name, lines in out.items()}


def chromosomes(data):
    """`cut -f1 | sort | uniq` under LC_ALL=C over every line"""
    return sorted(set(line.split(b"\t", 1)[0] for line in mm.lines_of(data)))


def job_text(outdir, name, resolution, utilityfolder=""):
    """the line `echo "python3 $script -i ... -o ..." >> $jobFile` appends"""
    script = utilityfolder + "CombineNearbyInteraction.py"
    return ("python3 " + script + " -i " + outdir + "/" + name + "/subset_fithic_" + name + ".gz -H 0 -r " + resolution + " -o " + outdir + "/" +
            name + "/postmerged_fithic_" + name + ".gz\n")
