// fhx_bdtrc.hpp - device-side binomial survival function, bit-faithful to Cephes bdtrc/incbet as shipped
// in scipy.special (the reference calls scipy.special.bdtrc(count-1, n, prior) at fithic/fithic.py:1070,1101).
//
// Rules:
//   * every recurrence is written as separate IEEE multiply / add / divide in Cephes' association and the
//     translation unit is compiled with -ffp-contract=off, so hipcc cannot fuse a*b+c into v_fma_f64;
//   * the continued fractions keep Cephes' 300-iteration cap and its big/biginv rescaling - in the
//     "observed < expected" branch the fraction does NOT converge and the truncated value IS the answer;
//   * lbeta(count, n-count+1) and 1/beta(...) come from host-built tables (glibc log, Cephes lgam): one ulp
//     of lgam(n) is 1.5e-8 relative on every p-value, so they are never recomputed with the device's log;
//   * `1.0 - xx` is a rounded subtraction followed by log(), exactly as Cephes does (no log1p "improvement").
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fhx {
namespace dev {

constexpr double kMachEp = 1.11022302462515654042E-16;
constexpr double kMaxLog = 7.09782712893383996732E2;
constexpr double kMinLog = -7.451332191019412076235E2;
constexpr double kMaxGam = 171.624376956302725;
constexpr double kBig = 4.503599627370496e15;
constexpr double kBigInv = 2.22044604925031308085e-16;

// per-(pass, n) constants of one binomial: n = total contacts, tables indexed by count
struct BinomTables {
    const double* lbeta;      // lbeta(count, n-count+1)
    const double* inv_beta;   // 1/beta(count, n-count+1), used only when n + 1 < MAXGAM
    double n;
    int small_n;              // n + 1 < MAXGAM
};

// ---- Cephes unity.c log1p / expm1 (scipy's bdtrc uses these for k == 0) ---------------------------
__device__ __forceinline__ double cephes_log1p(double x) {
    double z = 1.0 + x;
    if (z < 0.70710678118654752440 || z > 1.41421356237309504880) return log(z);
    z = x * x;
    double num = 4.5270000862445199635215E-5;
    num = num * x + 4.9854102823193375972212E-1;
    num = num * x + 6.5787325942061044846969E0;
    num = num * x + 2.9911919328553073277375E1;
    num = num * x + 6.0949667980987787057556E1;
    num = num * x + 5.7112963590585538103336E1;
    num = num * x + 2.0039553499201281259648E1;
    double den = x + 1.5062909083469192043167E1;
    den = den * x + 8.3047565967967209469434E1;
    den = den * x + 2.2176239823732856465394E2;
    den = den * x + 3.0909872225312059774938E2;
    den = den * x + 2.1642788614495947685003E2;
    den = den * x + 6.0118660497603843919306E1;
    z = -0.5 * z + x * (z * num / den);
    return x + z;
}

__device__ __forceinline__ double cephes_expm1(double x) {
    if (!isfinite(x)) {
        if (isnan(x) || x > 0) return x;
        return -1.0;
    }
    if (x < -0.5 || x > 0.5) return exp(x) - 1.0;
    const double xx = x * x;
    double ep = 1.2617719307481059087798E-4;
    ep = ep * xx + 3.0299440770744196129956E-2;
    ep = ep * xx + 9.9999999999999999991025E-1;
    double r = x * ep;
    double eq = 3.0019850513866445504159E-6;
    eq = eq * xx + 2.5244834034968410419224E-3;
    eq = eq * xx + 2.2726554820815502876593E-1;
    eq = eq * xx + 2.0000000000000000000897E0;
    r = r / (eq - r);
    return r + r;
}

// ---- power series for small b*x (incbet.c pseries) ------------------------------------------------
// SMALL_N (here and below): the binomial total is so small (n + 1 < MAXGAM = 171.6) that Cephes multiplies powers instead of
// exponentiating a sum of logarithms.  No Hi-C run gets there, but pow() costs ~90 VGPRs wherever it is compiled in: the class
// kernels exist in both forms and the host launches the one the pass's totals call for (false: the pow statements are not
// compiled; their condition (a + b) < MAXGAM is false for such totals anyway).
//
// LEAN (the pass's class kernels only; bdtrc_count keeps the statements as Cephes has them): the same divisions as lean_div does
// them (lean_rcp, lean_quot: defined below), their reciprocals read from rtab (div_table_build<false>, kPsTabJ entries of lean_rcp(j)) where the divisor is
// a small integer - the term number n, and a + n when a is the contact count.  hipcc's `/` is the same v_rcp_f64, Newton steps,
// quotient and fused residual step inside v_div_scale / v_div_fmas / v_div_fixup, which only act on extreme exponents; lean_div
// equals it bit for bit for divisors in (1e-200, 1e200) and numerators that are 0 or in that window.  The window, under the
// predicate checked at entry (b an integer, 1 <= a, b < 4.5e15, 1e-150 < x, b x <= 1 and x <= 0.95 as for every caller):
//   * divisors: a, a + 1, n and a + n are in [1, 2^53 + 2^53) - n counts terms, every term is at most 0.95 times the last or
//     below 1 / n of it, so the loop ends long before n reaches 2^53;
//   * 1 / a: the numerator is 1;
//   * (1 - b) x and (n - b) x: b and n are integers, so 1 - b and n - b are exact and either 0 - then the numerator is +0 in both
//     forms, and so are the quotient, t and every later v: the loop ends - or at least 1 in magnitude: |numerator| in [1e-150, 4.5e15];
//   * t: |u| <= max(x, b x / n) <= 1 in every term, so |t| <= |(1 - b) x| <= 1; and the loop goes on only while
//     |v| = |t / (a + n)| > MACHEP / a, i.e. |t| > 1.1e-16, so the next t = t u is 0 or above 1.1e-16 x / n > 1e-182.
//   A zero quotient: the only zero numerator is +0 over a positive divisor, +0 both ways (lean_quot keeps a zero's sign in any
//   case) - and the sign would be unobservable anyway (t *= u; s += v with s = +0 or nonzero).
__device__ __forceinline__ double lean_rcp(double d);
__device__ __forceinline__ double lean_quot(double n, double d, double y);
constexpr int kPsTabJ = 512;
template <bool SMALL_N = true, bool LEAN = false>
__device__ __forceinline__ double pseries(double a, double b, double x, double lbeta_ab, double inv_beta_ab, const double* rtab = nullptr) {
    double ai, t1, s = 0.0;
    if (LEAN && x > 1e-150 && x <= 0.95 && b * x <= 1.0 && a >= 1.0 && a < 4.5e15 && b >= 1.0 && b < 4.5e15 && b == __builtin_rint(b)) {
        // ja: a as a table index when it is a small integer, else kPsTabJ ("compute"): ja + ni < kPsTabJ fails from then on
        int ja = kPsTabJ;
        if (a < (double)kPsTabJ) {
            const int ia = (int)a;
            if ((double)ia == a) ja = ia;
        }
        const double a1 = a + 1.0;
        ai = lean_quot(1.0, a, ja < kPsTabJ ? rtab[ja] : lean_rcp(a));
        double u = (1.0 - b) * x;
        double v = lean_quot(u, a1, ja + 1 < kPsTabJ ? rtab[ja + 1] : lean_rcp(a1));
        t1 = v;
        double t = u;
        double n = 2.0;
        int ni = 2;                                       // n as an integer: the same in every lane that is still in the loop
        const double z = kMachEp * ai;
        while (fabs(v) > z) {
            u = lean_quot((n - b) * x, n, ni < kPsTabJ ? rtab[ni] : lean_rcp(n));
            t *= u;
            const double an = a + n;
            v = lean_quot(t, an, ja + ni < kPsTabJ ? rtab[ja + ni] : lean_rcp(an));
            s += v;
            n += 1.0;
            ni += 1;
        }
    } else {
        ai = 1.0 / a;
        double u = (1.0 - b) * x;
        double v = u / (a + 1.0);
        t1 = v;
        double t = u;
        double n = 2.0;
        const double z = kMachEp * ai;
        while (fabs(v) > z) {
            u = (n - b) * x / n;
            t *= u;
            v = t / (a + n);
            s += v;
            n += 1.0;
        }
    }
    double u, t;
    s += t1;
    s += ai;
    u = a * log(x);
    if (SMALL_N && (a + b) < kMaxGam && fabs(u) < kMaxLog) {
        t = inv_beta_ab;
        s = s * t * pow(x, a);
    } else {
        t = -lbeta_ab + u + log(s);
        s = (t < kMinLog) ? 0.0 : exp(t);
    }
    return s;
}

// ---- continued fractions (incbet.c incbcf / incbd); kind 0 = incbcf, 1 = incbd ----------------------
template <int KIND>
__device__ __forceinline__ double contfrac(double a, double b, double x) {
    double k1, k2, k3, k4, k5, k6, k7, k8, arg;
    if (KIND == 0) {
        arg = x;
        k1 = a; k2 = a + b; k3 = a; k4 = a + 1.0; k5 = 1.0; k6 = b - 1.0; k7 = k4; k8 = a + 2.0;
    } else {
        arg = x / (1.0 - x);
        k1 = a; k2 = b - 1.0; k3 = a; k4 = a + 1.0; k5 = 1.0; k6 = a + b; k7 = a + 1.0; k8 = a + 2.0;
    }
    double pkm2 = 0.0, qkm2 = 1.0, pkm1 = 1.0, qkm1 = 1.0, ans = 1.0, r = 1.0;
    const double thresh = 3.0 * kMachEp;
    int n = 0;
    do {
        double xk = -(arg * k1 * k2) / (k3 * k4);
        double pk = pkm1 + pkm2 * xk;
        double qk = qkm1 + qkm2 * xk;
        pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;

        xk = (arg * k5 * k6) / (k7 * k8);
        pk = pkm1 + pkm2 * xk;
        qk = qkm1 + qkm2 * xk;
        pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;

        double t;
        if (qk != 0) r = pk / qk;
        if (r != 0) {
            t = fabs((ans - r) / r);
            ans = r;
        } else {
            t = 1.0;
        }
        if (t < thresh) break;

        k1 += 1.0;
        k2 += (KIND == 0) ? 1.0 : -1.0;
        k3 += 2.0;
        k4 += 2.0;
        k5 += 1.0;
        k6 += (KIND == 0) ? -1.0 : 1.0;
        k7 += 2.0;
        k8 += 2.0;

        if ((fabs(qk) + fabs(pk)) > kBig) {
            pkm2 *= kBigInv; pkm1 *= kBigInv; qkm2 *= kBigInv; qkm1 *= kBigInv;
        }
        if ((fabs(qk) < kBigInv) || (fabs(pk) < kBigInv)) {
            pkm2 *= kBig; pkm1 *= kBig; qkm2 *= kBig; qkm1 *= kBig;
        }
    } while (++n < 300);
    return ans;
}

// Same continued fraction, same result bit for bit, without the two IEEE divisions of Cephes' convergence test in the
// iterations where the test cannot succeed.  Cephes does, after each double step,
//       if (qk != 0) r = pk/qk;   if (r != 0) { t = |(ans - r)/r|; ans = r; } else t = 1;   if (t < 3*MACHEP) break;
// `ans` is only ever USED (a) in the next test and (b) as the return value.  We keep it as an unevaluated ratio rp/rq
// and decide the test by cross-multiplication: |rp*qk - pk*rq| > 1e-13*|pk*rq| implies t > 1e-13 - 5e-16 > 3*MACHEP
// (each product carries a relative rounding error <= 2^-53, and so does each of the two quotients Cephes would have
// formed), so the loop provably does not break and nothing else depends on t.  Whenever that cheap test is
// inconclusive (and on every unusual input: zero / tiny / huge pk or qk) the pending quotient is materialised with a
// real IEEE division and Cephes' statements run literally.  On Hi-C data the swapped fraction sits on a rounding-noise
// plateau of t ~ 1e-11 for all 300 iterations, so ~99.9 % of iterations take the cheap path.
// IEEE-754 division for operands that cannot overflow / underflow on the way: the reciprocal refinement and the final
// residual correction that hipcc's own expansion of `/` performs (v_rcp_f64, two Newton steps, quotient, one fused
// residual step), without the v_div_scale / v_div_fmas / v_div_fixup scaffolding that only matters for extreme
// exponents and non-finite inputs.  Bit-identical to `n / d` for finite d with 1e-200 < |d| < 1e200 and |n| = 0 or in the
// same window (checked on 10^8 random operand pairs by tests/test_gpu_parity.py::test_lean_division_matches_ieee);
// the sign of a zero quotient may differ, which no caller below can observe.
__device__ __forceinline__ double lean_rcp(double d) {                  // the refined reciprocal: v_rcp_f64, two Newton steps
    const double y0 = __builtin_amdgcn_rcp(d);
    const double e0 = __builtin_fma(-d, y0, 1.0);
    const double y1 = __builtin_fma(y0, e0, y0);
    const double e1 = __builtin_fma(-d, y1, 1.0);
    return __builtin_fma(y1, e1, y1);
}
__device__ __forceinline__ double lean_div(double n, double d) {
    const double y2 = lean_rcp(d);
    const double q0 = n * y2;
    const double r0 = __builtin_fma(-d, q0, n);
    return __builtin_fma(r0, y2, q0);
}
// lean_div's quotient and fused residual step for a reciprocal y = lean_rcp(d) that the caller holds (the tables below).  The
// residual is formed as -(d q0 - n) instead of (-d) q0 + n: one rounding of the same exact value, negated - the same bits whenever
// it is not zero - and a quotient of zero keeps the numerator's sign as `/` does (n = -0: q0 = -0, d q0 - n = -0 + 0 = +0,
// -(+0) y + (-0) = -0; with (-d) q0 + n the residual is +0 and the sum +0).  Both negations are operand modifiers.
__device__ __forceinline__ double lean_quot(double n, double d, double y) {
    const double q0 = n * y;
    const double r0 = __builtin_fma(d, q0, -n);
    return __builtin_fma(-r0, y, q0);
}

// Reciprocal tables by integer, in LDS, for the pass's per-lane loops.  lean_rcp(d) is a pure function of d, and the divisors of
// those loops are small exact integers whenever the row's a is its contact count: D = j (j + 1) with j = a + 2 i (then j + 1) in
// the continued fractions, the term number n and a + n in the power series.  Every workgroup tabulates lean_rcp of them once, with
// the statements above, so lean_quot(n, D, table[j]) is lean_div(n, D) with the same reciprocal, product and two fused steps: the
// v_rcp_f64 and the four Newton fma per division leave the loop, the quotient's three instructions stay.  Entry 0 is never read.
//   kCfTabJ: 448 doubles are what the LDS of k2_queue_by_count leaves at four workgroups per CU (16 KB tile, 16 KB histogram, 4 KB
//            queue prefix: 37 152 of 40 960 bytes).  A row uses the table while j + 1 < kCfTabJ, i.e. up to count 400 for 23
//            iterations; Hi-C counts of the converging classes are far below that.  Past the table a lane computes lean_rcp itself.
//   kPsTabJ (above, at pseries): the power-series kernel holds no tile: 512.
constexpr int kCfTabJ = 448;
template <bool PRODUCT>          // true: lean_rcp(j (j + 1)), false: lean_rcp(j); all threads of the workgroup, the caller synchronises
__device__ __forceinline__ void div_table_build(double* tab, int len) {
    for (int j = (int)threadIdx.x; j < len; j += (int)blockDim.x) {
        const double fj = (double)j;
        tab[j] = j == 0 ? 0.0 : lean_rcp(PRODUCT ? fj * (fj + 1.0) : fj);
    }
}

// Division modes of the continued-fraction loop: 0 = hipcc's `/`, 1 = lean_div, 2 / 3 = lean_div whose reciprocal seed is
// the previous denominator's refined reciprocal instead of v_rcp_f64.  The denominators of both fractions form ONE
// sequence D_m = (a+m)(a+m+1), m = 0, 1, 2, ... (k3*k4 is D_2n, k7*k8 is D_2n+1), so 1/D_m is within 2/(a+m) of 1/D_m-1;
// for a >= 1e6 two Newton steps from that seed land on the same reciprocal quality as v_rcp_f64 + two steps
// (error e -> e^2: 2e-6 -> 4e-12 -> 2e-23, i.e. rounding-limited), and the final fused residual step is identical.
// MODE 3, for a >= 2e8: consecutive denominators differ by <= 1e-8 relative, so ONE Newton step from the previous
// reciprocal leaves (1e-8)^2 = 1e-16 + one rounding - as good as the two-step value for the residual-corrected quotient
// (its correction term is < 1 ulp and inherits only the reciprocal's RELATIVE error): two fma less per division.
// (Tried on top and rejected: one wave-uniform branch around all rare statements instead of per-lane exec masking -
// the ballot -> scalar branch dependency made the heavy launch 14 % slower; chunks of 20 iterations without the exact
// statements plus checkpoint / repeat when a lane needed them - bit-exact, but 6 % slower even with < 1 % repeats:
// Cephes' rescaling fires every 2.4 iterations per lane, so the per-lane masking stays, and the VALU is ~80 % busy;
// deferring that (exact, power-of-two) rescaling to 2^480 and doing nine steps at once - bit-exact too - changed nothing.)
template <int MODE>
__device__ __forceinline__ double cf_div(double n, double d, double& y) {
    if (MODE == 0) return n / d;
    if (MODE == 1) return lean_div(n, d);
    double e = __builtin_fma(-d, y, 1.0);
    y = __builtin_fma(y, e, y);
    if (MODE == 2) {                     // MODE 3 (a >= 2e8): the seed is within 1e-8, ONE step is already rounding-limited
        e = __builtin_fma(-d, y, 1.0);
        y = __builtin_fma(y, e, y);
    }
    const double q0 = n * y;
    const double r0 = __builtin_fma(-d, q0, n);
    return __builtin_fma(r0, y, q0);
}

// TAB (MODE 1 only, the pass's class kernels): the reciprocals of both denominators come from ytab (div_table_build<true>,
// kCfTabJ entries) while the lane's j = a + 2 i is an integer with j + 1 < kCfTabJ.  Decided per lane and iteration: a lane that
// leaves the table, or whose a is no integer, computes lean_rcp as MODE 1 does - the same value either way, so the quotients are
// MODE 1's bit for bit.  The address does not depend on the recurrence: the pair of the NEXT iteration is requested before this
// one's divisions, one LDS instruction for both half steps.
//
// LEAN (MODE 1 to 3, the pass's class kernels; LEAN with MODE 1 is TAB): the divisions of the exact block by lean_div.  A wave runs
// that block in several of its iterations - its lanes converge at different steps, and each passes through 1e-13 > t > 3 MACHEP
// on the way - so its three `/` are not rare in a wave's instruction stream.  Window: LEAN narrows the fast test's window from
// 1e-100 / 1e100 to 1e-30 / 1e30 (Cephes' own rescaling keeps |pk| + |qk| below 2^52 times one iteration's growth and both above
// 2^-52 over it, so this sends nothing on Hi-C rows to the exact block that did not go there; and which iterations run the exact
// statements never changes a bit).  Inside the block `win` says pk, qk are in (1e-30, 1e30); `lean_live` says every exact block so far
// took the lean form, so the pending (rp, rq) is (1, 1), a (pk, qk) that passed the fast test - same window - or (ans, 1) with
// ans = r of a lean block, a quotient of two such values: in (1e-60, 1e60).  Then rp / rq and pk / qk have operands in lean_div's
// window and values in (1e-60, 1e60), both nonzero - Cephes' `qk != 0` and `r != 0` hold - and ans - r is 0 or at least 2^-53 of
// 1e-60, over r: 0 or within (1e-136, 1e120).  Anything else (win false, fast_ok false) runs Cephes' statements with `/`, and clears lean_live.
// x / 1.0 is x: the pending quotient is not divided when rq is 1 (every block after a lane's first, and the loop's exit).
template <int KIND, int MODE, bool LEAN = false>
__device__ __forceinline__ double contfrac_lazy_impl(double a, double b, double arg, const double* ytab = nullptr) {
    static_assert(!LEAN || MODE >= 1, "MODE 0 is the loop for operands outside lean_div's window");
    constexpr bool TAB = LEAN && MODE == 1;
    constexpr double kWinLo = LEAN ? 1e-30 : 1e-100, kWinHi = LEAN ? 1e30 : 1e100;
    bool lean_live = true;
    double k1, k2, k3, k4, k5, k6, k8;
    if (KIND == 0) {
        k1 = a; k2 = a + b; k3 = a; k4 = a + 1.0; k5 = 1.0; k6 = b - 1.0; k8 = a + 2.0;
    } else {
        k1 = a; k2 = b - 1.0; k3 = a; k4 = a + 1.0; k5 = 1.0; k6 = a + b; k8 = a + 2.0;
    }
    // k7 == k4 in both fractions (a + 1 + 2n): one variable serves both
    double pkm2 = 0.0, qkm2 = 1.0, pkm1 = 1.0, qkm1 = 1.0;
    double rp = 1.0, rq = 1.0;          // Cephes' ans (== r while fast_ok) as an unevaluated ratio; exact when rq == 1
    double ans = 1.0, r = 1.0;          // only used once the invariant ans == r is broken (some r was exactly 0)
    bool fast_ok = true;
    const double thresh = 3.0 * kMachEp;
    double yrec = 0.0;                  // running reciprocal of the denominator sequence (MODE 2 only)
    if (MODE >= 2) {
        const double d0 = k3 * k4;
        yrec = __builtin_amdgcn_rcp(d0);
        double e0 = __builtin_fma(-d0, yrec, 1.0);
        yrec = __builtin_fma(yrec, e0, yrec);
        if (MODE == 3) {                 // fully refined before the loop: the loop itself refines once per denominator
            e0 = __builtin_fma(-d0, yrec, 1.0);
            yrec = __builtin_fma(yrec, e0, yrec);
        }
    }
    // TAB: the lane's j = k3 as an int while it can read the table (tj <= kCfTabJ - 2: entries j and j + 1 exist); any value above
    // that means "compute".  It steps by 2 with k3 either way: at most kCfTabJ + 600, no wrap.  ty0 / ty1: the requested pair.
    int tj = kCfTabJ;
    double ty0 = 0.0, ty1 = 0.0;
    if (TAB) {
        if (a < (double)(kCfTabJ - 1)) {                 // a >= 1 (contfrac_lazy): the conversion is in range
            const int ia = (int)a;
            if ((double)ia == a) tj = ia;
        }
        const int jc = tj < kCfTabJ - 2 ? tj : kCfTabJ - 2;
        ty0 = ytab[jc];
        ty1 = ytab[jc + 1];
    }
    int n = 0;
    do {
        double y0 = ty0, y1 = ty1;
        double xk;
        if (TAB) {
            const double d0 = k3 * k4;
            if (__builtin_expect(tj > kCfTabJ - 2, 0)) {
                y0 = lean_rcp(d0);
                y1 = lean_rcp(k4 * k8);
            }
            tj += 2;
            const int jc = tj < kCfTabJ - 2 ? tj : kCfTabJ - 2;      // clamped: a lane outside reads an entry it does not use
            ty0 = ytab[jc];
            ty1 = ytab[jc + 1];
            xk = -lean_quot(arg * k1 * k2, d0, y0);
        } else {
            xk = -cf_div<MODE>(arg * k1 * k2, k3 * k4, yrec);
        }
        double pk = pkm1 + pkm2 * xk;
        double qk = qkm1 + qkm2 * xk;
        pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;

        xk = TAB ? lean_quot(arg * k5 * k6, k4 * k8, y1) : cf_div<MODE>(arg * k5 * k6, k4 * k8, yrec);
        pk = pkm1 + pkm2 * xk;
        qk = qkm1 + qkm2 * xk;
        pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;

        const double apk = fabs(pk), aqk = fabs(qk);
        const double mag_sum = aqk + apk;
        const double mag_min = fmin(apk, aqk);
        bool exact = true;
        const bool win = fast_ok && mag_min > kWinLo && mag_sum < kWinHi;
        if (__builtin_expect(win, 1)) {
            const double c1 = rp * qk;
            const double c2 = pk * rq;
            if (__builtin_expect(fabs(c1 - c2) > 1e-13 * fabs(c2), 1)) {        // certainly t > thresh: Cephes would set ans = r = pk/qk and go on
                rp = pk;
                rq = qk;
                exact = false;
            }
        }
        if (__builtin_expect(exact, 0)) {
            double t;
            if (LEAN && win && lean_live) {                  // Cephes' statements with qk != 0 and r != 0 known (above)
                ans = rp;
                if (rq != 1.0) ans = lean_div(rp, rq);
                r = lean_div(pk, qk);
                t = fabs(lean_div(ans - r, r));
                ans = r;
            } else {
                lean_live = false;
                if (fast_ok) {
                    ans = rp / rq;                           // materialise the pending quotient (x / 1.0 is exact)
                    r = ans;
                }
                if (qk != 0) r = pk / qk;
                if (r != 0) {
                    t = fabs((ans - r) / r);
                    ans = r;
                } else {
                    t = 1.0;
                }
                if (ans != r) fast_ok = false;
            }
            rp = ans;
            rq = 1.0;
            if (t < thresh) break;
        }

        k1 += 1.0;
        k2 += (KIND == 0) ? 1.0 : -1.0;
        k3 += 2.0;
        k4 += 2.0;
        k5 += 1.0;
        k6 += (KIND == 0) ? -1.0 : 1.0;
        k8 += 2.0;

        if (__builtin_expect(mag_sum > kBig, 0)) {
            pkm2 *= kBigInv; pkm1 *= kBigInv; qkm2 *= kBigInv; qkm1 *= kBigInv;
        }
        if (__builtin_expect(mag_min < kBigInv, 0)) {
            pkm2 *= kBig; pkm1 *= kBig; qkm2 *= kBig; qkm1 *= kBig;
        }
    } while (++n < 300);
    if (LEAN && fast_ok) {
        if (rq == 1.0) return rp;
        if (lean_live) return lean_div(rp, rq);
    }
    return fast_ok ? rp / rq : ans;
}

template <int KIND, bool LEAN = false>
__device__ __forceinline__ double contfrac_lazy(double a, double b, double x, const double* ytab = nullptr) {
    const double arg = (KIND == 0) ? x : x / (1.0 - x);
    // operand window of lean_div: denominators are (a+2n)(a+2n+1) with 1 <= a < 2^53 (exact integers), numerators are
    // arg * k * k' with |k k'| < 1e20, so |arg| in [1e-150, 1e150] keeps every operand inside [1e-200, 1e200] or exactly 0
    const double aa = fabs(arg);
    if (aa > 1e-150 && aa < 1e150 && a >= 1.0 && a < 4.5e15 && b < 4.5e15) {
        if (a >= 2e8) return contfrac_lazy_impl<KIND, 3, LEAN>(a, b, arg);
        if (a >= 1e6) return contfrac_lazy_impl<KIND, 2, LEAN>(a, b, arg);
        return contfrac_lazy_impl<KIND, 1, LEAN>(a, b, arg, ytab);
    }
    return contfrac_lazy_impl<KIND, 0>(a, b, arg);
}

// ---- swapped incbcf with WAVE-UNIFORM iteration constants --------------------------------------------------------
// In the swapped orientation (the "observed < expected" rows: 20 % of the rows and > 90 % of all iterations on Hi-C data)
// a = n - count + 1 and b = count, so every k1..k8 of incbcf, both denominators D_2i = k3*k4, D_2i+1 = k7*k8 and their
// reciprocals depend on (n, count) ONLY - never on the row's prior.  When all 64 lanes of a wave hold rows of one
// (binomial, count), those values come from a table row per iteration (built once per pass by k2h_offsets_and_tables with the
// same fp64 statements Cephes uses) through scalar loads into SGPR operands, and the lanes execute only what depends
// on their own x = 1 - prior: 2 products + 3-instruction division + 4 recurrence instructions per half step.
//
// Two more statements of Cephes' loop disappear without changing a result bit:
//   * the big/biginv rescaling multiplies all four recurrence values by 2^-52 or 2^52.  A power-of-two scaling of
//     (pkm2, pkm1, qkm2, qkm1) commutes with every rounding of the recurrence (no overflow, no subnormals), the value
//     r = pk/qk and the convergence test are scale-free, so ANY rescaling schedule that keeps the values in range gives
//     the same bits as Cephes' data-dependent one.  Here every lane renormalises at the same iterations (every 8th, by
//     the exponent of the largest of its four values): no per-lane exec masking in the loop.
//     Range proof: x < 1, b <= a  =>  |xk| <= 2 in the first half step and <= 1 in the second, so the largest value grows
//     by at most 4x per iteration: from < 1 after a renormalisation to <= 2^16 before the next, products <= 2^32.
//     The renormalisation cannot be made rarer: on Hi-C rows (x = 1 - prior ~ 1 - 1e-8, a ~ 1e9) every step cancels
//     pk = pkm1 - ~pkm2 and the values SHRINK by 2^-24..2^-30 per iteration (Cephes multiplies by 2^52 every ~2.4 iterations);
//     eight iterations stay inside the 2^-300 window of the exact statements, sixteen do not (tried: every row came back
//     irregular and went through the per-lane loop - correct results, twice the time).
//     Smallness is checked where it matters (below).
//   * the lazy convergence test of contfrac_lazy_impl (cross-multiplication instead of two divisions) needs Cephes'
//     previous r = ans.  In the common case that is the pair (pkm1, qkm1) the iteration started with - still live for
//     the second half step - so no register copy is kept for it.
// Lanes with unusual inputs or states (b > a, x outside (0, 1), pk or qk zero or tiny, r == 0) are reported through
// `irregular` and the caller evaluates them with contfrac_lazy (the per-lane loop above).
struct CfRow {          // one iteration's constants, 64 bytes = one scalar-cache line
    double k1, k2, k5, k6, d0, y0, d1, y1;
};
constexpr int kCfIters = 300;
constexpr double kCfLazyT = 1e-15;          // cf_swapped_step: |d| > kCfLazyT |c2| proves Cephes' t >= 3 MACHEP (derivation there)

typedef const CfRow __attribute__((address_space(4))) * CfRowConstPtr;      // constant address space: s_load

typedef double cf_d8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ CfRow cf_load_row(CfRowConstPtr p0) {
    const volatile cf_d8 __attribute__((address_space(4))) * p = (const volatile cf_d8 __attribute__((address_space(4))) *)p0;
    const cf_d8 v = *p;
    CfRow r;
    r.k1 = v[0]; r.k2 = v[1]; r.k5 = v[2]; r.k6 = v[3];
    r.d0 = v[4]; r.y0 = v[5]; r.d1 = v[6]; r.y1 = v[7];
    __builtin_amdgcn_sched_barrier(0);
    return r;
}

// table of one (n_total, count): the values Cephes' loop would hold at iteration i, and lean_div's reciprocals.  Cephes
// reaches them by repeated k += 1 or 2 from integer-valued doubles below 2^53 - exact additions - so row i can be written
// down directly (k1 = a + i, k3 = a + 2i, ...) and the 300 rows of a table are built by 300 threads instead of one.
__device__ __forceinline__ CfRow cf_swapped_row(double n_total, int count, int i) {
    const double fk = (double)count - 1.0;
    const double a = n_total - fk, b = fk + 1.0;            // swapped: a = bb, b = aa of incbet
    const double di = (double)i, d2 = 2.0 * di;
    const double k1 = a + di, k2 = (a + b) + di, k3 = a + d2, k4 = (a + 1.0) + d2, k5 = 1.0 + di, k6 = (b - 1.0) - di, k8 = (a + 2.0) + d2;
    CfRow r;
    r.k1 = k1; r.k2 = k2; r.k5 = k5; r.k6 = k6;
    r.d0 = k3 * k4;
    r.d1 = k4 * k8;
    double d = r.d0;
    double y = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-d, y, 1.0);
    r.y0 = __builtin_fma(y, e, y);
    d = r.d1;
    y = __builtin_amdgcn_rcp(d);
    e = __builtin_fma(-d, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-d, y, 1.0);
    r.y1 = __builtin_fma(y, e, y);
    return r;
}
// which rows cf_swapped_uniform may evaluate (the rest go through contfrac_lazy): the operand window of lean_div
// (see contfrac_lazy) and the premises of the range proof above
__device__ __forceinline__ bool cf_swapped_regular(double a, double b, double x) {
    return x > 1e-150 && x < 1.0 && a >= 1.0 && a < 4.5e15 && b >= 1.0 && b <= a;
}

// incbcf(a, b, x) for R rows per lane of one wave, all rows of the wave sharing (a, b); `rows` must be wave-uniform.
// R > 1: the R recurrences of a lane are independent instruction streams (plus the two divisions each): a dependent fp64
// instruction issues ~32 cycles behind its producer on this chip and eight waves per SIMD of single-row lanes do not hide
// that (profiles/fp64_rate.hip: one chain per lane tops out at 41 % of the issue rate whatever the occupancy, eight chains
// reach 85-93 % from two waves per SIMD up) - more rows per lane, not more waves, is what fills the fp64 pipe.  The scalar
// loads, the loop control and the wave-uniform exactness branch are shared by the R rows.
// Returns Cephes' value for the rows it leaves regular; rows that come back irregular must be recomputed.
template <int R>
struct CfState {
    double pm[R], qm[R], p0[R], q0[R];        // pkm2, qkm2, pkm1, qkm1
    double result[R];
    // lane masks, wave-uniform (SGPR pairs): which lanes are finished (converged or given up - they go on iterating, as copies
    // of a lane that is not, and are ignored) and which must be recomputed by the caller
    unsigned long long done[R], irregular[R];
};

__device__ __forceinline__ bool cf_lane_bit(unsigned long long m) {
    return (m >> (threadIdx.x & 63)) & 1ull;
}

// v of lane `src` (wave-uniform) for the lanes with `take`, the lane's own v for the others
__device__ __forceinline__ double cf_copy_lane(bool take, double v, int src) {
    const double w = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
    return take ? w : v;
}

// the folded convergence test of cf_swapped_step: true for a lane one of whose e[r], |c2[r]| is not above 2^-600 (by the high
// words; derivation in cf_swapped_step).  R minima and one compare.
template <int R>
__device__ __forceinline__ bool cf_fold_fails(const double (&e)[R], const double (&c2)[R]) {
    static_assert(R == 1 || R == 2 || R == 4, "one minimum tree per row count");
    // one asm statement per row count, as in cf_swapped_renorm: the compiler separates asm statements by a wait state each
    unsigned int m, t;
    if constexpr (R == 4) {
        asm("v_min3_f32 %0, %2, %3, %4\n\tv_min3_f32 %1, |%6|, |%7|, |%8|\n\tv_min3_f32 %0, %0, %1, %5\n\tv_min_f32 %0, %0, |%9|"
            : "=&v"(m), "=&v"(t)
            : "v"(__double2hiint(e[0])), "v"(__double2hiint(e[1])), "v"(__double2hiint(e[2])), "v"(__double2hiint(e[3])),
              "v"(__double2hiint(c2[0])), "v"(__double2hiint(c2[1])), "v"(__double2hiint(c2[2])), "v"(__double2hiint(c2[3])));
    } else if constexpr (R == 2) {
        asm("v_min3_f32 %0, %1, %2, |%3|\n\tv_min_f32 %0, %0, |%4|"
            : "=&v"(m)
            : "v"(__double2hiint(e[0])), "v"(__double2hiint(e[1])), "v"(__double2hiint(c2[0])), "v"(__double2hiint(c2[1])));
    } else {
        asm("v_min_f32 %0, %1, |%2|" : "=v"(m) : "v"(__double2hiint(e[0])), "v"(__double2hiint(c2[0])));
    }
    (void)t;
    return !(__builtin_bit_cast(float, m) > __builtin_bit_cast(float, 0x1A700000u));        // high word of 2^-600
}

template <int R>
__device__ __forceinline__ void cf_swapped_step(CfState<R>& S, const CfRow c, double (&arg)[R]) {
    // Written stage by stage ACROSS the rows (and across the two divisions of a row, which do not depend on each other): the
    // compiler keeps this order, so every instruction sits 2R (the divisions) or R (the recurrence, the test) instructions
    // behind its producer instead of right behind it.
    double p1[R], q1[R], p2[R], q2[R];
    double na[R], nb[R], ta[R], tb[R];
    // xk_a = -(x*k1*k2)/(k3*k4), xk_b = (x*k5*k6)/(k7*k8): lean_div with the tabulated reciprocals
#pragma unroll
    for (int r = 0; r < R; ++r) {
        na[r] = arg[r] * c.k1;
        nb[r] = arg[r] * c.k5;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        na[r] = na[r] * c.k2;
        nb[r] = nb[r] * c.k6;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        ta[r] = na[r] * c.y0;
        tb[r] = nb[r] * c.y1;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        na[r] = __builtin_fma(-c.d0, ta[r], na[r]);
        nb[r] = __builtin_fma(-c.d1, tb[r], nb[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        ta[r] = __builtin_fma(na[r], c.y0, ta[r]);          // xk_a (sign folded into the subtraction below)
        tb[r] = __builtin_fma(nb[r], c.y1, tb[r]);          // xk_b
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        na[r] = S.pm[r] * ta[r];
        nb[r] = S.qm[r] * ta[r];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        p1[r] = S.p0[r] - na[r];
        q1[r] = S.q0[r] - nb[r];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        na[r] = S.p0[r] * tb[r];
        nb[r] = S.q0[r] * tb[r];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        p2[r] = p1[r] + na[r];
        q2[r] = q1[r] + nb[r];
    }
    // Lazy convergence test.  Cephes' ans is the r of the previous iteration, fl(pk/qk) of the pair this iteration started
    // with (1.0 = 1/1 before the first) - for every lane that is still regular, because those never met pk == 0 or qk == 0.
    // With u = 2^-53, C = p2*q0 and E = p0*q2 - C (exact values):  c2 = C(1 + e1), d = fl(p0*q2 - c2) = (E - C e1)(1 + e2)
    // (one fused rounding), so |d| > T |c2| gives |E/C| > T(1 - 2u) - u.  Cephes forms ans = fl(p0/q0) = (p0/q0)(1 + a1),
    // r = fl(p2/q2) = (p2/q2)(1 + a2), the difference ans - r exactly (Sterbenz: the two are within a factor 1 + 1e-10 of
    // each other here) and t = |fl((ans - r)/r)| = |ans/r - 1|(1 + a3) with ans/r - 1 = E/C + (a1 - a2)(1 + E/C) + O(u^2):
    // t > (|E/C| - 2u(1 + |E/C|))(1 - u) > T - 3.4e-16.  Cephes goes on iff t >= 3 MACHEP = 3.33e-16, so any T >= 6.8e-16 proves
    // it; T = kCfLazyT = 1e-15 leaves 3.2e-16 (one more 3u) of margin.  (Round 2 used 1e-13: a hundred times more rows than
    // necessary fell through to the exact statements - a wave-uniform branch of three IEEE divisions, 55 instructions, that a
    // single lane of the wave triggers; at 2e-15 that branch was still taken in 2 % of the wave-row-iterations = 1.2 of the
    // 26.1 VALU instructions per row-iteration.)
    // c2 must not have lost bits to underflow and p2, q0 must not be zero: |c2| > 2^-600 (values are <= 2^17).  q2 == 0
    // shows up as q0 == 0 one iteration later - or in the caller's final check - and sends the row to the per-lane loop like
    // every other unusual state.
    //
    // ONE compare per wave step.  What the loop needs from the test is one bit per wave - does any lane, for any of its R
    // rows, fail the proof? - and the per-row lane masks only inside the exact block (about 1 % of the wave steps).  So:
    //   e = fma(-T, |c2|, |d|)   one rounding of the exact |d| - T |c2|: e > 0 IS the premise above (rounding is monotone, a
    //                            value <= 0 never rounds to one > 0), where fl(T |c2|) had a rounding of its own;
    //   m = min over the lane's 2R values e[r], |c2[r]|, taken on their HIGH WORDS read as binary32 (cf_swapped_renorm's
    //       trick: for finite doubles below 2^1017 the high word orders like the double, negative ones included);
    //   m > hi(2^-600) as binary32, i.e. every e[r] and every |c2[r]| >= 2^-600 (1 + 2^-20): both premises for every row.
    // A lane that fails sends the wave to the exact block, which first forms the per-row masks with the statements every step
    // used to run and then decides as before: a false alarm costs time, never a bit.  The other way round, a row that passes here has
    // |d| > T |c2| exactly; fl(T |c2|) may lie half an ulp above T |c2|, so |d| == fl(T |c2|) passes here and did not pass the
    // two-rounding compare - the proof above needs the exact premise only, the exact block would have found t >= 3 MACHEP.
    // That is 5R - 3 instructions (c2, d, e per row; R minima; one compare) where the per-row compares took 5R.
    // NaN and infinity: v_min*_f32 skips a quiet NaN operand, and the high word of a double infinity or NaN (and of anything
    // from 2^1017 up) reads as a binary32 NaN, so the folded compare does not see a non-finite e or c2 unless all 2R are.
    //   * An infinity cannot arise for rows inside cf_swapped_regular: the range proof above (growth <= 4x per iteration,
    //     renormalised every 8th) keeps every value below 2^17 and every product below 2^34; with finite operands e, c2 and d
    //     are finite, and without an infinity no NaN is born (inf - inf and 0 * inf are its only sources here).
    //   * If a NaN did stand in p (or q) it would stay: p1 = p0 - pm * xk and p2 = p1 + p0 * xk are NaN when pm or p0 is, so
    //     both values of the next state are; ldexp keeps it.  Such a row never converges here.  Either some lane sends the
    //     wave to the exact block - there the per-row compares are false for it, the window check fails and it is handed back
    //     at once - or it runs to the cap and cf_swapped_uniform's final check fabs(p0) > 2^-300 && fabs(q0) > 2^-300 is false
    //     for it: handed back to the per-lane loop either way, as the two-rounding compare would have done at the first NaN.
    // One compare has no `& ~done[r]` term, so a lane without a live row of its own would send its wave to the exact block at
    // every remaining step once its state has converged or degenerated.  Such lanes therefore run COPIES of live rows: a
    // lane that is marked done takes arg and the four recurrence values of the first lane of its slot r that is not done
    // (v_readlane, in the exact block only) and from then on computes, bit for bit, what that lane computes - it fails the
    // compare exactly when a live lane does.  Every done lane of the slot is re-seeded whenever one more finishes, because the
    // lane they copy may be the one that finished.  result[r], done[r] and irregular[r] are not touched, nothing of a done
    // lane is read again.  A slot with no unfinished lane keeps its state: the block is entered, finds nothing and leaves.
#pragma unroll
    for (int r = 0; r < R; ++r) na[r] = p2[r] * S.q0[r];                                  // c2
#pragma unroll
    for (int r = 0; r < R; ++r) nb[r] = __builtin_fma(S.p0[r], q2[r], -na[r]);            // d
#pragma unroll
    for (int r = 0; r < R; ++r) ta[r] = __builtin_fma(-kCfLazyT, fabs(na[r]), fabs(nb[r]));   // e
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(cf_fold_fails<R>(ta, na)) != 0ull, 0)) {     // wave-uniform branch
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // the per-row masks, by the statements every step used to run
            const double tc = kCfLazyT * fabs(na[r]);
            const unsigned long long differ = __builtin_amdgcn_ballot_w64(fabs(nb[r]) > tc) & __builtin_amdgcn_ballot_w64(fabs(na[r]) > 0x1p-600);
            const unsigned long long exact = ~(differ | S.done[r]);
            if (exact == 0ull) continue;                                // wave-uniform
            // Cephes' statements, literally
            const bool mine = cf_lane_bit(exact);
            const bool window = fabs(S.p0[r]) > 0x1p-300 && fabs(S.q0[r]) > 0x1p-300 && fabs(p2[r]) > 0x1p-300 && fabs(q2[r]) > 0x1p-300;
            const bool go = mine && window;
            // inside the window every operand is in lean_div's (2^-300 < |p|, |q| <= 2^17; ans - rr is 0 or >= 2^-370)
            const double ans = go ? lean_div(S.p0[r], S.q0[r]) : 1.0;   // the pending quotient
            const double rr = go ? lean_div(p2[r], q2[r]) : 1.0;        // != 0 inside the window
            const double t = fabs(lean_div(ans - rr, rr));
            const unsigned long long fin = __builtin_amdgcn_ballot_w64(go && t < 3.0 * kMachEp);
            const unsigned long long bad = __builtin_amdgcn_ballot_w64(mine && !window);
            if (cf_lane_bit(fin)) S.result[r] = rr;
            S.done[r] |= fin | bad;
            S.irregular[r] |= bad;
            const unsigned long long running = ~S.done[r];
            if ((fin | bad) != 0ull && running != 0ull) {               // wave-uniform: done lanes become copies of a running one
                const int src = __builtin_ctzll(running);
                const bool idle = cf_lane_bit(S.done[r]);
                arg[r] = cf_copy_lane(idle, arg[r], src);
                p1[r] = cf_copy_lane(idle, p1[r], src);
                q1[r] = cf_copy_lane(idle, q1[r], src);
                p2[r] = cf_copy_lane(idle, p2[r], src);
                q2[r] = cf_copy_lane(idle, q2[r], src);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        S.pm[r] = p1[r];
        S.qm[r] = q1[r];
        S.p0[r] = p2[r];
        S.q0[r] = q2[r];
    }
}

template <int R>
__device__ __forceinline__ void cf_swapped_renorm(CfState<R>& S) {      // same iterations for every lane: no exec masking
#pragma unroll
    for (int r = 0; r < R; ++r) {
        // exponent of the largest of the four magnitudes from the HIGH WORDS alone: for finite doubles below 2^1017 a high word
        // without its sign, read as binary32, is an ordinary number and orders like the double (ties differ in the low word
        // only: same exponent), so two f32 maxima with |.| operand modifiers replace seven v_max_f64 (hipcc canonicalises
        // every fabs() operand of fmax with a v_max_f64 x, x of its own).  Any power of two is a correct scale (above).
        unsigned int top;
        asm("v_max3_f32 %0, |%1|, |%2|, |%3|\n\tv_max_f32 %0, %0, |%4|"
            : "=&v"(top)
            : "v"(__double2hiint(S.pm[r])), "v"(__double2hiint(S.p0[r])), "v"(__double2hiint(S.qm[r])), "v"(__double2hiint(S.q0[r])));
        const int e = 1022 - (int)((top >> 20) & 0x7ffu);            // -frexp_exp(largest) for normal numbers
        S.pm[r] = __builtin_amdgcn_ldexp(S.pm[r], e);
        S.p0[r] = __builtin_amdgcn_ldexp(S.p0[r], e);
        S.qm[r] = __builtin_amdgcn_ldexp(S.qm[r], e);
        S.q0[r] = __builtin_amdgcn_ldexp(S.q0[r], e);
    }
}

// arg[r] = x of row r, overwritten (a lane that is done goes on with a copy of a running lane's row, see cf_swapped_step);
// irregular[r]: in = rows outside cf_swapped_regular, out = rows that must be recomputed by the per-lane loop; result[r] =
// Cephes' incbcf value for the other rows.  A lane without a row of its own must be given a copy of a row of the same (a, b):
// to the loop it is a row like any other, and the caller ignores what comes back for it.
template <int R>
__device__ __forceinline__ void cf_swapped_uniform(CfRowConstPtr rows, double (&arg)[R], bool (&irregular)[R], double (&result)[R]) {
    CfState<R> S;
    unsigned long long all_done = ~0ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        S.pm[r] = 0.0;
        S.qm[r] = 1.0;
        S.p0[r] = 1.0;
        S.q0[r] = 1.0;
        S.result[r] = 1.0;
        S.irregular[r] = __builtin_amdgcn_ballot_w64(irregular[r]);
        S.done[r] = S.irregular[r];
        // rows irregular on input are done from the start: they run a regular lane's x (if the slot has none they keep theirs -
        // whatever their values become, the exact block finds no lane of theirs to decide about)
        const unsigned long long running = ~S.done[r];
        if (S.done[r] != 0ull && running != 0ull) arg[r] = cf_copy_lane(irregular[r], arg[r], __builtin_ctzll(running));
    }
    static_assert(kCfIters % 8 == 4, "blocks of 8 iterations, then one of 4");
    int i = 0;
    // Scalar loads return out of order, so the only wait is "all of them": each iteration first waits for its own row (the
    // empty asm is a use), then requests the next one, then computes - the request has a whole iteration to complete.
#define FHX_CF_NEXT(cur, nxt, idx)            \
    asm volatile("" ::"s"(cur.k1));           \
    const CfRow nxt = cf_load_row(rows + (idx)); \
    cf_swapped_step<R>(S, cur, arg);
#pragma unroll 1
    for (; i + 8 <= kCfIters; i += 8) {
        const CfRow c0 = cf_load_row(rows + i);
        FHX_CF_NEXT(c0, c1, i + 1)
        FHX_CF_NEXT(c1, c2, i + 2)
        FHX_CF_NEXT(c2, c3, i + 3)
        FHX_CF_NEXT(c3, c4, i + 4)
        FHX_CF_NEXT(c4, c5, i + 5)
        FHX_CF_NEXT(c5, c6, i + 6)
        FHX_CF_NEXT(c6, c7, i + 7)
        cf_swapped_step<R>(S, c7, arg);
        cf_swapped_renorm<R>(S);
        all_done = ~0ull;
#pragma unroll
        for (int r = 0; r < R; ++r) all_done &= S.done[r];
        if (all_done == ~0ull) break;
    }
    if (i + 8 > kCfIters) {
        const CfRow c0 = cf_load_row(rows + i);
        FHX_CF_NEXT(c0, c1, i + 1)
        FHX_CF_NEXT(c1, c2, i + 2)
        FHX_CF_NEXT(c2, c3, i + 3)
        cf_swapped_step<R>(S, c3, arg);
    }
#undef FHX_CF_NEXT
#pragma unroll
    for (int r = 0; r < R; ++r) {
        irregular[r] = cf_lane_bit(S.irregular[r]);
        // the loop ran to the cap: Cephes returns the last r = pk/qk
        if (!cf_lane_bit(S.done[r])) {
            if (!(fabs(S.p0[r]) > 0x1p-300 && fabs(S.q0[r]) > 0x1p-300)) irregular[r] = true;     // a zero in the last iteration
            S.result[r] = S.p0[r] / S.q0[r];
        }
        result[r] = S.result[r];
    }
}

// branch classes of one incbet evaluation (used to run branch-homogeneous waves)
enum BranchClass : int {
    BC_TRIVIAL = 0,        // NaN / 0 / 1 / closed form k == 0: no loop at all
    BC_PSERIES = 1,        // power series (either orientation): ~15 iterations
    BC_CF_BCF = 2,         // incbcf, not swapped: converges in ~9 iterations
    BC_CF_BD = 3,          // incbd (either orientation): converges in ~9 iterations
    BC_CF_SWAPPED = 4,     // swapped incbcf ("observed < expected"): runs to (or near) the 300 cap
    BC_COUNT = 5
};

// incbet(aa, bb, xx) with aa = count, bb = n - count + 1 and the two table values for that count
__device__ __forceinline__ double incbet(double aa, double bb, double xx, double lbeta_ab, double inv_beta_ab) {
    if (xx <= 0.0 || xx >= 1.0) {
        if (xx == 0.0) return 0.0;
        if (xx == 1.0) return 1.0;
        return __builtin_nan("");
    }
    if (bb * xx <= 1.0 && xx <= 0.95) return pseries(aa, bb, xx, lbeta_ab, inv_beta_ab);
    double w = 1.0 - xx;
    double a, b, x, xc, t, y;
    int flag;
    if (xx > aa / (aa + bb)) {
        flag = 1; a = bb; b = aa; xc = xx; x = w;
    } else {
        flag = 0; a = aa; b = bb; xc = w; x = xx;
    }
    if (flag == 1 && b * x <= 1.0 && x <= 0.95) {
        t = pseries(a, b, x, lbeta_ab, inv_beta_ab);
    } else {
        y = x * (a + b - 2.0) - (a - 1.0);
        if (y < 0.0)
            w = contfrac<0>(a, b, x);
        else
            w = contfrac<1>(a, b, x) / xc;
        y = a * log(x);
        t = b * log(xc);
        if ((a + b) < kMaxGam && fabs(y) < kMaxLog && fabs(t) < kMaxLog) {
            t = pow(xc, b);
            t *= pow(x, a);
            t /= a;
            t *= w;
            t *= inv_beta_ab;
        } else {
            y += t - lbeta_ab;
            y += log(w / a);
            t = (y < kMinLog) ? 0.0 : exp(y);
        }
    }
    if (flag == 1) {
        if (t <= kMachEp)
            t = 1.0 - kMachEp;
        else
            t = 1.0 - t;
    }
    return t;
}

// scipy.special.bdtrc(count - 1, n, p) for an integer count
__device__ __forceinline__ double bdtrc_count(int count, const BinomTables& T, double p) {
    if (isnan(p)) return p;
    const double fk = (double)count - 1.0;
    if (p < 0.0 || p > 1.0 || T.n < fk) return __builtin_nan("");
    if (fk < 0) return 1.0;
    if (fk == T.n) return 0.0;
    const double dn = T.n - fk;
    if (count == 1) {
        if (p < 0.01) return -cephes_expm1(dn * cephes_log1p(-p));
        return 1.0 - pow(1.0 - p, dn);
    }
    return incbet(fk + 1.0, dn, p, T.lbeta[count], T.small_n ? T.inv_beta[count] : 0.0);
}

// bdtrc_count restricted to the inputs bdtrc_class() below calls BC_TRIVIAL: the same statements minus incbet's loops.
// (Calling the generic function from the classify kernel inlined the whole of incbet four times: 7 900 fp64 instructions
// and 154 VGPRs of dead code.)
__device__ __forceinline__ double bdtrc_count_trivial(int count, const BinomTables& T, double p) {
    if (isnan(p)) return p;
    const double fk = (double)count - 1.0;
    if (p < 0.0 || p > 1.0 || T.n < fk) return __builtin_nan("");
    if (fk < 0) return 1.0;
    if (fk == T.n) return 0.0;
    const double dn = T.n - fk;
    if (count == 1) {
        if (p < 0.01) return -cephes_expm1(dn * cephes_log1p(-p));
        return 1.0 - pow(1.0 - p, dn);
    }
    return p <= 0.0 ? 0.0 : 1.0;              // incbet's domain edges: xx == 0 -> 0, xx == 1 -> 1 (no other p is trivial)
}

// The one trivial case that costs transcendentals: count == 1 with a proper probability and n > 0, where scipy's bdtrc takes
// the closed form -expm1(n * log1p(-p)) or 1 - pow(1 - p, n).  bdtrc_count_trivial(1, T, p) == bdtrc_closed_form(T.n, p) there.
__device__ __forceinline__ bool bdtrc_is_closed_form(int count, double n_total, double p) {
    return count == 1 && p >= 0.0 && p <= 1.0 && n_total > 0.0;          // false for NaN
}
__device__ __forceinline__ double bdtrc_closed_form(double n_total, double p) {
    if (p < 0.01) return -cephes_expm1(n_total * cephes_log1p(-p));     // dn = n - (count - 1) = n
    return 1.0 - pow(1.0 - p, n_total);
}

// bdtrc_count_trivial for the inputs that are BC_TRIVIAL and NOT bdtrc_is_closed_form: with count == 1 those are NaN, p outside
// [0, 1], or n <= 0, all of which return above the count == 1 statement - so the statement (and its log1p / expm1 / pow, which
// would set the caller's register budget) is left out.  Same values as bdtrc_count_trivial on that domain.
__device__ __forceinline__ double bdtrc_count_trivial_open(int count, const BinomTables& T, double p) {
    if (isnan(p)) return p;
    const double fk = (double)count - 1.0;
    if (p < 0.0 || p > 1.0 || T.n < fk) return __builtin_nan("");
    if (fk < 0) return 1.0;
    if (fk == T.n) return 0.0;
    return p <= 0.0 ? 0.0 : 1.0;
}

// cheap classification of which loop bdtrc_count(count, T, p) will run (same predicates as incbet, same rounding)
__device__ __forceinline__ int bdtrc_class(int count, double n_total, double p) {
    if (isnan(p)) return BC_TRIVIAL;
    const double fk = (double)count - 1.0;
    if (p < 0.0 || p > 1.0 || n_total < fk || fk < 0 || fk == n_total || count == 1) return BC_TRIVIAL;
    const double aa = fk + 1.0, bb = n_total - fk, xx = p;
    if (xx <= 0.0 || xx >= 1.0) return BC_TRIVIAL;
    if (bb * xx <= 1.0 && xx <= 0.95) return BC_PSERIES;
    const double w = 1.0 - xx;
    double a, b, x;
    bool swapped;
    if (xx > aa / (aa + bb)) {
        swapped = true; a = bb; b = aa; x = w;
        if (b * x <= 1.0 && x <= 0.95) return BC_PSERIES;
    } else {
        swapped = false; a = aa; b = bb; x = xx;
    }
    const double y = x * (a + b - 2.0) - (a - 1.0);
    if (y < 0.0) return swapped ? BC_CF_SWAPPED : BC_CF_BCF;
    return BC_CF_BD;
}

// bdtrc_class as a table: for one (n_total, count) every predicate of the classification is a monotone function of the prior
// (IEEE multiplication by a positive constant, 1 - x and the subtraction of a constant are monotone; a rounded difference has the
// sign of the exact one), so each is ONE threshold on the prior - found by bisection over the bit patterns of the doubles in
// [0, 1) with the very statements of bdtrc_class, on the device, once per pass and count:
//   tA  largest  x with  bb*x <= 1 && x <= 0.95                                  (power series, direct orientation)
//   tB  = aa / (aa + bb): x > tB is the swapped orientation
//   tC  smallest x with  aa*(1-x) <= 1 && (1-x) <= 0.95                          (power series, swapped)
//   tD  smallest x with  (1-x)*(bb+aa-2) - (bb-1) < 0                            (swapped: incbcf, else incbd)
//   tE  largest  x with  x*(aa+bb-2) - (aa-1) < 0                                (direct: incbcf, else incbd)
// "none" is -1 for the "largest" kind and 2 for the "smallest" kind.  The classify kernel then needs one 64-byte row and
// four comparisons per contact instead of a division and five multiplications (tests: fhx_debug_classify against bdtrc_class
// on random priors and on the neighbours of every threshold).
struct ClsRow {
    double tA, tB, tC, tD, tE, pad0, pad1, pad2;
};

__device__ __forceinline__ bool cls_pred(int which, double aa, double bb, double xx) {
    const double w = 1.0 - xx;
    switch (which) {
        case 0: return bb * xx <= 1.0 && xx <= 0.95;
        case 2: return aa * w <= 1.0 && w <= 0.95;
        case 3: return w * (bb + aa - 2.0) - (bb - 1.0) < 0.0;
        default: return xx * (aa + bb - 2.0) - (aa - 1.0) < 0.0;
    }
}

__device__ __forceinline__ ClsRow cls_row(double n_total, int count) {
    const double fk = (double)count - 1.0;
    const double aa = fk + 1.0, bb = n_total - fk;
    ClsRow r;
    r.pad0 = r.pad1 = r.pad2 = 0.0;
    r.tB = aa / (aa + bb);
    const long long one = 0x3FF0000000000000ll;                 // bits of 1.0: the candidates are the patterns below it
    auto largest_true = [&](int which) -> double {              // predicate true on an initial segment of [0, 1)
        if (!cls_pred(which, aa, bb, 0.0)) return -1.0;
        long long lo = 0, hi = one;                             // P(lo) true, P(hi) treated as false
        while (hi - lo > 1) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (cls_pred(which, aa, bb, __longlong_as_double(mid)))
                lo = mid;
            else
                hi = mid;
        }
        return __longlong_as_double(lo);
    };
    auto smallest_true = [&](int which) -> double {             // predicate true on a final segment of [0, 1)
        if (!cls_pred(which, aa, bb, __longlong_as_double(one - 1))) return 2.0;
        long long lo = -1, hi = one - 1;                        // P(hi) true, P(lo) treated as false
        while (hi - lo > 1) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (cls_pred(which, aa, bb, __longlong_as_double(mid)))
                hi = mid;
            else
                lo = mid;
        }
        return __longlong_as_double(hi);
    };
    r.tA = largest_true(0);
    r.tC = smallest_true(2);
    r.tD = smallest_true(3);
    r.tE = largest_true(4);
    return r;
}

// bdtrc_class(count, n_total, p) for a proper probability 0 < p < 1 and 2 <= count <= n_total (everything else is BC_TRIVIAL)
__device__ __forceinline__ int cls_lookup(const ClsRow& r, double xx) {
    if (xx <= r.tA) return BC_PSERIES;
    if (xx > r.tB) {
        if (xx >= r.tC) return BC_PSERIES;
        return xx >= r.tD ? BC_CF_SWAPPED : BC_CF_BD;
    }
    return xx <= r.tE ? BC_CF_BCF : BC_CF_BD;
}
__device__ __forceinline__ bool cls_is_trivial(int count, double n_total, double p) {
    return !(p > 0.0 && p < 1.0) || count < 2 || (double)count - 1.0 >= n_total;
}

// bdtrc_class with the one division of the classification - the orientation threshold aa / (aa + bb) - read from the count's
// table row (ClsRow::tB holds exactly that quotient) instead of being computed per contact
__device__ __forceinline__ int bdtrc_class_tb(int count, double n_total, double p, double tB) {
    if (cls_is_trivial(count, n_total, p)) return BC_TRIVIAL;
    const double fk = (double)count - 1.0;
    const double aa = fk + 1.0, bb = n_total - fk, xx = p;
    if (bb * xx <= 1.0 && xx <= 0.95) return BC_PSERIES;
    const double w = 1.0 - xx;
    if (xx > tB) {
        if (aa * w <= 1.0 && w <= 0.95) return BC_PSERIES;
        return w * (bb + aa - 2.0) - (bb - 1.0) < 0.0 ? BC_CF_SWAPPED : BC_CF_BD;
    }
    return xx * (aa + bb - 2.0) - (aa - 1.0) < 0.0 ? BC_CF_BCF : BC_CF_BD;
}

// Multiply the continued fraction / series value by x^a (1-x)^b / (a B(a,b)) and undo the swap (incbet.c tail).
template <bool SMALL_N = true>
__device__ __forceinline__ double incbet_finish(double a, double b, double x, double xc, double w, int flag,
                                                double lbeta_ab, double inv_beta_ab) {
    double y = a * log(x);
    double t = b * log(xc);
    if (SMALL_N && (a + b) < kMaxGam && fabs(y) < kMaxLog && fabs(t) < kMaxLog) {
        t = pow(xc, b);
        t *= pow(x, a);
        t /= a;
        t *= w;
        t *= inv_beta_ab;
    } else {
        y += t - lbeta_ab;
        y += log(w / a);
        t = (y < kMinLog) ? 0.0 : exp(y);
    }
    if (flag == 1) {
        if (t <= kMachEp)
            t = 1.0 - kMachEp;
        else
            t = 1.0 - t;
    }
    return t;
}

// bdtrc_count for a row whose class (bdtrc_class) is known at compile time: only that class's code path is
// instantiated, so the long-running kernels carry neither the other loops' registers nor their branches.
// Same operations in the same order as incbet() above.
// LEAN (the pass's class kernels): `tab` is the workgroup's LDS table of reciprocals by integer - div_table_build<false> for
// BC_PSERIES (pseries<.., true>), div_table_build<true> for BC_CF_BCF and BC_CF_BD (contfrac_lazy<.., true>).  Same bits.
template <int CLS, bool SMALL_N = true, bool LEAN = false>
__device__ __forceinline__ double bdtrc_count_class(int count, const BinomTables& T, double p, const double* tab = nullptr) {
    static_assert(!LEAN || CLS == BC_PSERIES || CLS == BC_CF_BCF || CLS == BC_CF_BD, "the swapped class has no small divisors");
    const double fk = (double)count - 1.0;
    const double aa = fk + 1.0, bb = T.n - fk, xx = p;
    const double lb = T.lbeta[count];
    const double ib = (SMALL_N && T.small_n) ? T.inv_beta[count] : 0.0;
    if (CLS == BC_PSERIES) {
        if (LEAN) {                                       // one inlined series for both orientations: a wave that mixes them runs one loop
            const bool direct = bb * xx <= 1.0 && xx <= 0.95;
            const double w = 1.0 - xx;
            const double t = pseries<SMALL_N, true>(direct ? aa : bb, direct ? bb : aa, direct ? xx : w, lb, ib, tab);
            if (direct) return t;
            return (t <= kMachEp) ? 1.0 - kMachEp : 1.0 - t;
        }
        if (bb * xx <= 1.0 && xx <= 0.95) return pseries<SMALL_N, LEAN>(aa, bb, xx, lb, ib, tab);
        const double w = 1.0 - xx;                       // otherwise the swapped orientation (flag = 1)
        double t = pseries<SMALL_N, LEAN>(bb, aa, w, lb, ib, tab);
        return (t <= kMachEp) ? 1.0 - kMachEp : 1.0 - t;
    }
    const double w1 = 1.0 - xx;
    if (CLS == BC_CF_BCF) return incbet_finish<SMALL_N>(aa, bb, xx, w1, contfrac_lazy<0, LEAN>(aa, bb, xx, tab), 0, lb, ib);
    if (CLS == BC_CF_SWAPPED) return incbet_finish<SMALL_N>(bb, aa, w1, xx, contfrac_lazy<0>(bb, aa, w1), 1, lb, ib);
    // BC_CF_BD: either orientation
    const int flag = (xx > aa / (aa + bb)) ? 1 : 0;
    const double a = flag ? bb : aa, b = flag ? aa : bb, x = flag ? w1 : xx, xc = flag ? xx : w1;
    return incbet_finish<SMALL_N>(a, b, x, xc, contfrac_lazy<1, LEAN>(a, b, x, tab) / xc, flag, lb, ib);
}

}  // namespace dev
}  // namespace fhx
