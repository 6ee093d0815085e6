"""Host driver of one Fit-Hi-C run on one GPU: the body of the reference's main() after argument parsing
(fithic/fithic.py:317-370) expressed over the C ABI of libfithic_mi355x.so.

    pass_stats  (K1)   <- read_Interactions                       fithic/fithic.py:389-454
    fit         (host) <- makeBinsFromInteractions, generate_FragPairs, calculateProbabilities,
                          fit_Spline's spline + table             fithic/fithic.py:463-689, 843-918, 936-968
    pvalues     (K2)   <- fit_Spline's per-pair loop + bdtrc      fithic/fithic.py:1017-1124
    bh          (K3)   <- benjamini_hochberg_correction           fithic/myStats.py:24-48
    next_pass          <- outlier collection                      fithic/fithic.py:1215-1217

There is no CPU implementation behind this class: without the built library or without a GPU it raises.
"""
import os
import time

import numpy as np

from . import _capi

MODES = {"intraOnly": _capi.MODE_INTRA_ONLY, "interOnly": _capi.MODE_INTER_ONLY, "All": _capi.MODE_ALL}
# what bdtrc is given for a total of counts at or above 2^31: "reference" = narrowed to a C int, as scipy does with the Python ints
# of fithic.py:1070 / :1101 (p = q = nan for 2^31 <= total < 2^32, a wrong small n above) - the drop-in answer and the default;
# "wide" = the true total (what the formula means; no reference computes it)
TOTALS = {"reference": _capi.TOTALS_REFERENCE, "wide": _capi.TOTALS_WIDE}


def totals_notice(info):
    """One line for stderr when a total of this pass reached 2^31 (info = fhx_fit_info as a dict), else None."""
    bits = info.get("totals_narrowed", 0)
    if not bits:
        return None
    which = " and ".join(w for b, w in ((1, "observedIntraInRangeSum"), (2, "observedInterAllSum")) if bits & b)
    if info["totals"] == _capi.TOTALS_WIDE:
        return ("fithic-mi355x: %s >= 2^31: p-values computed with the true total(s) (--totals wide). The reference (scipy's bdtrc "
                "takes a C int) would have used n = %d (intra) / %d (inter) there and written nan wherever that is below "
                "count - 1; --totals reference reproduces that." % (which, _narrow(info["bdtrc_n_intra"]), _narrow(info["bdtrc_n_inter"])))
    return ("fithic-mi355x: %s >= 2^31: scipy's bdtrc narrows n to a C int, so the reference computes these p-values with n = %d "
            "(intra) / %d (inter) - nan wherever n < count - 1 - and so does this run (--totals reference, the default: output "
            "identical to fithic.py). --totals wide uses the true totals instead." % (which, info["bdtrc_n_intra"], info["bdtrc_n_inter"]))


def _narrow(n):
    return ((int(n) + 2 ** 31) % 2 ** 32) - 2 ** 31


class PassOutput:
    """Everything one spline pass produced (host copies of the small arrays; p/q stay on the GPU until fetched)."""

    def __init__(self):
        self.stats = None       # dict of fhx_stats
        self.info = None        # dict of fhx_fit_info
        self.arrays = {}


class Engine:
    def __init__(self, device=0):
        self.ctx = _capi.Context(device)
        self.device = device
        self.n_rows = 0
        self.mode = "intraOnly"
        self.pass_no = 0
        # FHX_CALL_TIMES=1 (measurements): host seconds inside pass_stats / fit / pvalues / bh summed over run_pass calls, then the
        # number of calls - where a small pass's wall time goes that its kernels do not explain
        self.call_seconds = [0.0, 0.0, 0.0, 0.0, 0] if os.environ.get("FHX_CALL_TIMES") else None

    def close(self):
        self.ctx.close()

    def configure(self, resolution, dist_low=0, dist_up=float("inf"), n_bins=100, mapp_thres=1, mode="intraOnly",
                  bias_low=0.5, bias_up=2.0, totals="reference"):
        if mode not in MODES:
            raise ValueError("Invalid Option. Only options are 'All', 'interOnly', or 'intraOnly'")
        if totals not in TOTALS:
            raise ValueError("totals must be 'reference' or 'wide'")
        self.mode = mode
        self.resolution = int(resolution)
        self.dist_low, self.dist_up = dist_low, dist_up
        self.totals = totals
        self.ctx.set_params(resolution, dist_low, dist_up, n_bins, mapp_thres, MODES[mode], bias_low, bias_up, TOTALS[totals])

    def load_fragments(self, chr_ids, mids, hits, chr_sort_rank):
        self.ctx.load_fragments(chr_ids, mids, hits, chr_sort_rank)

    def load_bias(self, chr_ids, mids, bias):
        self.ctx.load_bias(chr_ids, mids, bias)

    def load_contacts(self, chr1, mid1, chr2, mid2, count):
        self.ctx.load_pairs(chr1, mid1, chr2, mid2, count)
        self.n_rows = len(mid1)
        self.pass_no = 0

    def commit_contacts_text(self, ids, n):
        """second half of the device-side ingest (tables.load_contacts): ids of the names ctx.ingest_contacts_text returned"""
        self.ctx.ingest_contacts_commit(ids)
        self.n_rows = int(n)
        self.pass_no = 0

    def load_contacts_device(self, ptrs, n, stream=None):
        self.ctx.load_pairs_device(ptrs, n, stream)
        self.n_rows = int(n)
        self.pass_no = 0

    # ---- the four steps of a pass; run_pass() strings them together ----
    def pass_stats(self):
        return self.ctx.pass_stats()

    def fit(self):
        return self.ctx.fit()

    def run_pass(self, collect=True):
        """K1 -> host fit -> K2 -> K3, all on this context's stream.  Returns a PassOutput."""
        out = PassOutput()
        if self.call_seconds is None:
            st, info = self.ctx.run_pass()      # the four calls below as one C call: no interpreter between K1 and K2
        else:                                   # measurements: host wall time of each of the four calls, summed
            t = [time.perf_counter()]
            st = self.ctx.pass_stats()
            t.append(time.perf_counter())
            info = self.ctx.fit()
            t.append(time.perf_counter())
            self.ctx.pvalues()
            t.append(time.perf_counter())
            self.ctx.bh(info.bh_total_tests)
            t.append(time.perf_counter())
            for k in range(4):
                self.call_seconds[k] += t[k + 1] - t[k]
            self.call_seconds[4] += 1
        out.stats, out.info = st.as_dict(), info.as_dict()
        if collect:
            self.ctx.sync()
            A = _capi
            names = dict(hist_sumcc=A.A_HIST_SUMCC, hist_npairs=A.A_HIST_NPAIRS, bin_lb=A.A_BIN_LB, bin_ub=A.A_BIN_UB,
                         bin_poss=A.A_BIN_POSS, bin_poss0=A.A_BIN_POSS0, bin_sumcc=A.A_BIN_SUMCC, bin_sumdist=A.A_BIN_SUMDIST,
                         bin_poss7=A.A_BIN_POSS7, x=A.A_X, y=A.A_Y)
            dist_keys = self.ctx.get_array(A.A_DIST_KEYS)
            if self.resolution == 0 or len(dist_keys):      # -r 0, or -r N on loci off the grid
                out.arrays["dist_keys"] = dist_keys
            if self.mode != "interOnly":
                names.update(knots=A.A_KNOTS, coeffs=A.A_COEFFS, table_x=A.A_TABLE_X, table_y0=A.A_TABLE_Y0, table_y=A.A_TABLE_Y)
            for k, w in names.items():
                out.arrays[k] = self.ctx.get_array(w)
        self.pass_no += 1
        return out

    def fetch(self, p=True, q=True, expcc=False, bias=False):
        return self.ctx.fetch(self.n_rows, p=p, q=q, expcc=expcc, bias=bias)

    def fdr_counts(self):
        return self.ctx.get_array(_capi.A_FDR_COUNTS)

    def significant(self, fdr, names, strict=False, path=None):
        """The FDR subset of this pass from its resident q (csrc/fhx_sigresident.hip), between run_pass / bh and next_pass:
        the mergefilter.Selection that mergefilter.select(file, fdr, strict) returns for the file this pass writes - same text,
        same n_lines (the header counted), same n_kept - without writing it.  `fdr` is text, as the shell passes it; `names` are
        the chromosome names the writer is given.  A q outside the grammar raises the ValueError mergefilter raises for that file,
        with the line the row would have in it (`path` only names the file in that message); a kept row the device formatter does
        not cover raises _capi.FhxError with code FHX_ERR_UNSUPPORTED - select from the written file then."""
        from . import mergefilter
        text = mergefilter.fdr_text(fdr)
        bound = mergefilter.key_bound(text, strict)
        zero_kept = 0 < float(text) if strict else 0 <= float(text)
        t0 = time.perf_counter()
        try:
            emitted, kept, subset, _ = self.ctx.significant_select(names, text, bound, zero_kept, strict)
        except _capi.MsRefused as e:
            if e.why in (_capi.MS_INTERNAL, _capi.MS_FDR):
                raise
            raise mergefilter._refusal_at("%s, line %d" % (path or "the significances of this pass", e.line), e.why, "") from None
        return mergefilter.Selection(subset, emitted + 1, kept, {"significant_select": time.perf_counter() - t0}, self.device)

    def track(self, qval, names, path=None):
        """The UCSC interact track of this pass from its resident q (csrc/fhx_sigresident_track.inc), between run_pass / bh and
        next_pass: the ucsc.Track that ucsc.track(file, qval) returns for the file this pass writes - same text, same n_lines (the
        header counted), n_kept and n_deferred - without writing it.  Arguments, refusals and the FHX_ERR_UNSUPPORTED case as for
        significant(); the track's rules for midpoints and names hold for every row the writer would print."""
        from . import mergefilter, ucsc
        text = mergefilter.fdr_text(qval)
        bound = mergefilter.key_bound(text, strict=True)
        t0 = time.perf_counter()
        try:
            emitted, kept, deferred, track = self.ctx.significant_track(names, text, bound, 0 < float(text))
        except _capi.MsRefused as e:
            if e.why in (_capi.MS_INTERNAL, _capi.MS_FDR):
                raise
            where = path or "the significances of this pass"
            if e.why == _capi.MS_KEPT:
                raise ucsc._refusal_kept(where) from None
            raise ucsc._refusal_at("%s, line %d" % (where, e.line), e.why, "") from None
        return ucsc.Track(track, dict(lines=emitted + 1, kept=kept, deferred=deferred), {"significant_track": time.perf_counter() - t0},
                          self.device)

    def split(self, fdr, names, path=None):
        """The per-chromosome FDR subsets of this pass from its resident q (csrc/fhx_sigresident_split.inc), between run_pass / bh
        and next_pass: the mergefilter_parallel.Split that mergefilter_parallel.split(file, fdr) returns for the file this pass
        writes - same chromosomes, same subsets, same n_lines - without writing it, so that mergefilter_parallel.write_tree takes
        it as it is.  Arguments, refusals and the FHX_ERR_UNSUPPORTED case as for significant(); the split's name rules hold for
        both names of every row the writer would print."""
        from . import mergefilter, mergefilter_parallel
        text = mergefilter.fdr_text(fdr)
        bound = mergefilter.key_bound(text)
        t0 = time.perf_counter()
        try:
            emitted, parts = self.ctx.significant_split(names, text, bound, 0 <= float(text))
        except _capi.MsRefused as e:
            if e.why in (_capi.MS_INTERNAL, _capi.MS_FDR):
                raise
            where = path or "the significances of this pass"
            if e.why == _capi.MS_NAMES:
                raise mergefilter_parallel._refusal_names(where) from None
            raise mergefilter_parallel._refusal_at("%s, line %d" % (where, e.line), e.why, "") from None
        return mergefilter_parallel.Split({name: sub for name, _, sub in parts}, {name: kept for name, kept, _ in parts}, emitted + 1,
                                          {"significant_split": time.perf_counter() - t0}, self.device)

    def kr_bias(self, frag_chr, frag_mid, perc=0.05, tol=1e-6, echo=False):
        """The Knight-Ruiz bias vector of HiCKRy (fithic/utils/HiCKRy.py) from the contact rows resident in this engine
        (csrc/fhx_kr_resident.inc): what hickry.loadfastfithicInteractions + returnBias give for the file the rows came from,
        bit for bit, without reading it again.  frag_chr, frag_mid: the fragment lines, chromosome ids as the rows were loaded
        with.  Returns (bias, one value per fragment line with -1 at the removed rows; the fhx_kr_info as a dict).  Every
        loaded row counts whatever the passes have skipped; the rows and the pass state are left as they are.  `echo`: print
        HiCKRy's lines.  KeyError(row) for a row whose locus is no fragment line; _capi.FhxError with code
        FHX_ERR_UNSUPPORTED when a count of the contacts text was not an integer as written - the matrix is then the file's
        (hickry.loadfastfithicInteractions)."""
        import contextlib
        import io
        from . import hickry
        t0 = time.time()
        kr = _capi.KrContext(self.device)
        try:
            kr.load_loci(frag_chr, frag_mid)
            kr.load_pairs_resident(self.ctx)
            with contextlib.nullcontext() if echo else contextlib.redirect_stdout(io.StringIO()):
                print("Creating sparse matrix...")                  # (said once it exists: a refusal leaves the lines to the file route)
                print("Sparse matrix creation took %s seconds" % (time.time() - t0))
                bias, info = hickry._bias_and_info(hickry.DeviceMatrix(kr), perc, tol)
            return bias.reshape(-1), info
        finally:
            kr.close()

    def next_pass(self):
        """Fold this pass's outliers (p < 1/N) into the skip mask and the outlier-distance multiset."""
        return self.ctx.next_pass()

    def reset_passes(self):
        """Start over at pass 1 on the loaded tables (the reference: a fresh main() on the same files)."""
        self.ctx.reset_passes()
        self.pass_no = 0

    def kernel_seconds(self):
        return self.ctx.kernel_seconds()
