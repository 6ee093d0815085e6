/*
 * oracle/cephes_libm_nudge.c - TEST INFRASTRUCTURE ONLY.
 *
 * cephes_oracle.c with a libm that is one ulp off: every log(), exp() and pow() it calls returns the next double above
 * (-DFHO_NUDGE=+1) or below (-DFHO_NUDGE=-1) what this machine's libm returns; NaN, +-inf and 0 pass through unchanged.
 * Cephes' lgam, lbeta, beta, Gamma, log1p and expm1 are restated in that file in terms of these three calls, so they move
 * with them.  How far bdtrc moves between the three builds is how far two faithful libms may legitimately differ on a row:
 * oracle/fithic_oracle.py: bdtrc_libm_spread() measures it, tests/p_relative.py turns it into a per-row bar.
 *
 * The engine's route has no further function to nudge: fhx_bdtrc.hpp calls log, exp and pow (the device's) and its per-count
 * tables are built on the host by fhx_host.cpp's cephes_lgam / cephes_lbeta / cephes_beta with std::log, std::exp and
 * std::pow - no lgamma(), no libm log1p().
 */
#include <math.h>

#ifndef FHO_NUDGE
#error "build with -DFHO_NUDGE=+1 or -DFHO_NUDGE=-1"
#endif

static double fho_nudged(double r)
{
    if (isnan(r) || isinf(r) || r == 0.0)
        return r;
    return nextafter(r, (FHO_NUDGE) > 0 ? INFINITY : -INFINITY);
}

static double fho_nudged_log(double x) { return fho_nudged(log(x)); }
static double fho_nudged_exp(double x) { return fho_nudged(exp(x)); }
static double fho_nudged_pow(double x, double y) { return fho_nudged(pow(x, y)); }

/* <math.h> is read above and guarded, so the include inside cephes_oracle.c declares nothing again: from here on the three
 * names are the wrappers. */
#define log(x) fho_nudged_log(x)
#define exp(x) fho_nudged_exp(x)
#define pow(x, y) fho_nudged_pow(x, y)

#include "cephes_oracle.c"
