"""merge-filter-parallelized.sh on the MI355X engine: one FDR subset and one job file per chromosome of a significances file
(reference: fithic/utils/merge-filter-parallelized.sh), same positional arguments, same tree.

    python -m fithic_amd.mergefilter_parallel INPUT RESOLUTION OUTDIR FDR [UTILITYFOLDER] [--merge] [--device N]

The script lists the chromosomes with `zcat INPUT | cut -f1 | sort | uniq` - field 1 of EVERY line, line 1 included, split at
tabs only - and then, once per listed name c, pipes the whole file through `awk 'NR!=1' | awk '$1==c && $3==c' | awk '$7<=fdr'`
into OUTDIR/c/subset_fithic_c.gz and appends one line to OUTDIR/c/fithic_c.job: the CombineNearbyInteraction.py call that would
merge that subset (-H 0 -r RESOLUTION) into OUTDIR/c/postmerged_fithic_c.gz.  This module reads the file ONCE: the kernels of
csrc/fhx_sigsplit.inc make mergefilter's `$7` decision on every row, intern the names of field 1, sort the kept rows by (name,
file offset) and hand back one run of bytes per chromosome.  What is written:

  * for every name c of the list, in bytewise order, OUTDIR/c/subset_fithic_c.gz (decompressed: the script's bytes) and
    OUTDIR/c/fithic_c.job (the script's line, byte for byte, APPENDED as `>>` does; paths as typed, the script path is
    UTILITYFOLDER + "CombineNearbyInteraction.py");
  * a name with no passing row - the `chr1` of a header fithic wrote, a chromosome seen only in trans rows - still gets its
    directory, an empty gzip subset and its job file; chromosomes.used is not left behind;
  * with --merge (an engine option, like --device) also OUTDIR/c/postmerged_fithic_c.gz, the file the job line would produce,
    through fithic_amd.combine as fithic_amd.mergefilter makes it for the one-file case.  For an empty subset the reference's
    Combine writes only its header line (no newline after it), and so does this module.

Line 1 is dropped from every subset whatever it holds; trans rows go nowhere.

Known deviations: nothing is approximated, so a file outside the device grammar is refused with a ValueError that names the
first such line, and nothing is written, not even OUTDIR.  Beyond what fithic_amd.mergefilter refuses: mawk compares `$1==c` as
NUMBERS when both sides look numeric (with 1, 01, 1.0, 1e0, 0x1 and +1 in one file each of the six directories receives all
such rows), so only names for which awk's equality is byte equality are taken.  On every line (on line 1: token 1 only) token 1
starts in column 0 and is ended by a tab (cut's field 1 and awk's $1 are then the same bytes); tokens 1 and 3 are 1 to 63 bytes
of [A-Za-z0-9_.-] starting with a letter, a digit or `_` (each becomes a directory name in an unquoted shell word); a name that
starts with a digit is a decimal integer of at most 15 digits without a leading zero, or holds `_` or a letter other than
a-f, x, p in either case (2L, 3R, 10_random: strtod cannot consume it whole) - 01, 1.5, 1e3, 0x1, 2a are refused.  At most 4096
distinct names.  There is no CPU implementation here: without the library or a GPU the entry points raise.

`fithic --significant FDR --significant-split` and Engine.split make the same tree straight from a pass's resident q-values
(csrc/fhx_sigresident_split.inc), without the significances file being written or read back.
"""
import os
import re
import sys

from . import _capi
from . import mergefilter
from .hicpro import _line_of

_ACCEPTS = ".  The reference accepts this; fithic_amd.mergefilter_parallel does not take it."
_NAME = re.compile(rb"[A-Za-z0-9_][A-Za-z0-9_.-]*\Z")
_CERTAIN = re.compile(rb"[_g-oq-wyzG-OQ-WYZ]")                       # strtod stops there at the latest
MAX_NAME = _capi.MS_SPLIT_NAME_BYTES - 1
USAGE = "usage: python -m fithic_amd.mergefilter_parallel INPUT RESOLUTION OUTDIR FDR [UTILITYFOLDER] [--merge] [--device N]"


def name_refusal(name):
    """0 for a name the device grammar takes, else the reason (_capi.MS_NAME, MS_NAME_BYTES, MS_NAME_NUMERIC): what the kernel decides
    for tokens 1 and 3"""
    name = bytes(name)
    if len(name) > MAX_NAME:
        return _capi.MS_NAME
    if not _NAME.match(name):
        return _capi.MS_NAME_BYTES
    if not name[:1].isdigit():
        return 0
    if name.isdigit():
        return 0 if len(name) <= 15 and (len(name) == 1 or name[:1] != b"0") else _capi.MS_NAME_NUMERIC
    return 0 if _CERTAIN.search(name) else _capi.MS_NAME_NUMERIC


def job_text(outdir, name, resolution, utilityfolder=""):
    """the line the script appends to OUTDIR/name/fithic_name.job, with its newline; every argument as typed"""
    return "python3 %sCombineNearbyInteraction.py -i %s/%s/subset_fithic_%s.gz -H 0 -r %s -o %s/%s/postmerged_fithic_%s.gz\n" % (
        utilityfolder, outdir, name, name, resolution, outdir, name, name)


def _refusal_names(path):
    return ValueError("%s: more than %d distinct names in field 1" % (path, _capi.MS_SPLIT_NAMES) + _ACCEPTS)


def _refusal(path, e):
    """the exception a refused file is reported with (module docstring, `Known deviations`)"""
    if e.why == _capi.MS_NAMES:
        return _refusal_names(path)
    if e.why not in (_capi.MS_NAME, _capi.MS_NAME_TAB, _capi.MS_NAME_BYTES, _capi.MS_NAME_NUMERIC):
        return mergefilter._refusal(path, e)
    with open(path, "rb") as f:
        gzipped = f.read(2) == b"\x1f\x8b"
    text = _line_of(path, e.line).decode("latin-1") if not gzipped else ""
    return _refusal_at("%s, line %d" % (path, e.line), e.why, text)


def _refusal_at(where, why, text):
    """the ValueError for reason `why` at `where` ("<file>, line <n>"), `text` being the line when it is at hand ("" for a gzipped
    file and for a line that was never written: Engine.split)"""
    if why not in (_capi.MS_NAME, _capi.MS_NAME_TAB, _capi.MS_NAME_BYTES, _capi.MS_NAME_NUMERIC):
        return mergefilter._refusal_at(where, why, text)
    if why == _capi.MS_NAME_TAB:
        return ValueError("%s: the chromosome name must start in column 0 and be ended by a tab: %r" % (where, text[:80]) + _ACCEPTS)
    if why == _capi.MS_NAME:
        return ValueError("%s: a chromosome name of more than %d bytes: %r" % (where, MAX_NAME, text[:80]) + _ACCEPTS)
    if why == _capi.MS_NAME_BYTES:
        return ValueError("%s: a chromosome name is 1 to %d bytes of [A-Za-z0-9_.-] and starts with a letter, a digit or _: %r"
                          % (where, MAX_NAME, text[:80]) + _ACCEPTS)
    return ValueError("%s: a chromosome name that starts with a digit and that awk would, or might, compare as a number (01, 1.5, 1e3, "
                      "0x1, 2a; 1, 2L and 10_random are taken): %r" % (where, text[:80]) + _ACCEPTS)


class Split:
    """The per-chromosome FDR subsets of one significances file: for every name of field 1, its kept lines verbatim and in file
    order."""

    def __init__(self, texts, kept, n_lines, seconds, device):
        self._texts, self._kept, self.n_lines, self._seconds, self.device = texts, kept, n_lines, seconds, device
        # `sort | uniq` under LC_ALL=C: bytewise
        self.chromosomes = [name.decode("latin-1") for name in sorted(texts)]

    def _key(self, name):
        key = name.encode("latin-1") if isinstance(name, str) else bytes(name)
        if key not in self._texts:
            raise KeyError(name)
        return key

    def subset_text(self, name):
        return self._texts[self._key(name)]

    def n_kept(self, name):
        return self._kept[self._key(name)]

    def selection(self, name):
        """the subset of one chromosome as a mergefilter.Selection: write_subset, combine and merged are its own"""
        key = self._key(name)
        return mergefilter.Selection(self._texts[key], self.n_lines, self._kept[key], self._seconds, self.device)

    def stage_seconds(self):
        return dict(self._seconds)


def split(path, fdr, device=0):
    """For every name c of field 1 of `path` (plain or gzipped; every line counts, line 1 too) the rows after line 1 with
    field 1 == field 3 == c and field 7 <= fdr as mawk decides it, made in one read on GPU `device`; `fdr` is text, the way the
    shell passes it."""
    text = mergefilter.fdr_text(fdr)
    bound = mergefilter.key_bound(text)
    ms = _capi.MsContext(device)
    try:
        try:
            ms.split_file(path, text, bound, 0 <= float(text))
        except _capi.MsRefused as e:
            raise _refusal(path, e) from None
        counts = ms.split_counts()
        names = ms.split_names()
        texts = {name: ms.split_text(k, counts["bytes"][k]) for k, name in enumerate(names)}
        kept = {name: counts["kept"][k] for k, name in enumerate(names)}
        if len(texts) != len(names):
            raise _capi.FhxError(_capi.FHX_ERR_INTERNAL, "a name was interned twice")
        return Split(texts, kept, counts["lines"], ms.split_stage_seconds(), device)
    finally:
        ms.close()


def parse_args(argv):
    """-> (input, resolution text, outdir, fdr, utilityfolder, merge, device); SystemExit with the usage line otherwise"""
    positional, merge, device = [], False, 0
    k = 0
    while k < len(argv):
        a = argv[k]
        if a == "--merge":
            merge = True
        elif a == "--device" or a.startswith("--device="):
            value = a[len("--device="):] if a.startswith("--device=") else (argv[k + 1] if k + 1 < len(argv) else "")
            k += 0 if a.startswith("--device=") else 1
            if not re.match(r"[0-9]+\Z", value):
                sys.exit(USAGE)
            device = int(value)
        elif a.startswith("--"):
            sys.exit(USAGE)
        else:
            positional.append(a)
        k += 1
    if len(positional) not in (4, 5) or not re.match(r"[0-9]+\Z", positional[1]):
        sys.exit(USAGE)
    path, resolution, outdir, fdr = positional[:4]
    return path, resolution, outdir, fdr, positional[4] if len(positional) == 5 else "", merge, device


def write_tree(chosen, outdir, resolution, utilityfolder="", merge=False):
    """the script's tree for a Split: per chromosome its directory, its gzipped subset, its job line appended, and with `merge` the
    file that job would write"""
    from . import combine
    os.makedirs(outdir, exist_ok=True)
    for name in chosen.chromosomes:
        folder = "%s/%s" % (outdir, name)
        os.makedirs(folder, exist_ok=True)
        one = chosen.selection(name)
        one.write_subset("%s/subset_fithic_%s.gz" % (folder, name))
        with open("%s/fithic_%s.job" % (folder, name), "a") as f:
            f.write(job_text(outdir, name, resolution, utilityfolder))
        if merge:
            names, rec = one.merged(int(resolution))
            combine.write_merged("%s/postmerged_fithic_%s.gz" % (folder, name), names, rec, int(resolution))


def main(argv=None):
    path, resolution, outdir, fdr, utilityfolder, merge, device = parse_args(sys.argv[1:] if argv is None else argv)
    chosen = split(path, fdr, device=device)                         # a refused file leaves nothing behind, not even OUTDIR
    write_tree(chosen, outdir, resolution, utilityfolder, merge)


if __name__ == "__main__":
    main()
