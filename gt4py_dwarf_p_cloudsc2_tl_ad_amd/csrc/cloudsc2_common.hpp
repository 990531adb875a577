// Shared device-side definitions for the CLOUDSC2 HIP kernels (gfx950 / CDNA4 only).
//
// Execution model used by every column kernel in this directory:
//   * one lane = one atmospheric column, one wave64 = 64 adjacent columns, workgroup = 4 waves (kColBlock = 256
//     threads: one wave per SIMD of a CU);
//   * fields are [level][column], so every per-level access of a wave is one fully coalesced
//     512-B (fp64) / 256-B (fp32) request;
//   * the vertical loop is sequential per lane; the loop-carried precipitation state lives in
//     registers, level-only quantities (eta, scalm) live in a small LDS table built per workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "../../include/cloudsc2_hip.h"

namespace cs2 {

constexpr int kWave = 64;  // CDNA wavefront
// Workgroup of the column kernels: 4 waves = one per SIMD of a CU.  One-wave workgroups are placed
// SIMD by SIMD by the dispatcher, and after a kernel with a very large grid (e.g. `saturation`) ~10 % of
// them double up on a SIMD while other SIMDs stay empty (profiles/census_placement.hip), which cost
// cloudsc2_nl +65 us in the driver loop; the 4 waves of a 256-thread workgroup always go to the 4
// different SIMDs of their CU.
constexpr int kColBlock = 256;

// XCD-aware workgroup -> column-block mapping.  Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8
// share one, MI355X_MICROARCH.md "Workgroup dispatch"); with the identity mapping every XCD's L2 and fabric port sees
// every eighth 2-KB piece of each field row.  Remapped, the workgroups of one XCD own one contiguous eighth of the
// columns.  Measured on cloudsc2_nl (profiles/r02/ab_xcd_remap.txt, one process): neutral at 65 536 fp64 columns (one
// workgroup per CU, everything in lockstep), -1.4 .. -2.2 % at 262 144 fp64 / 524 288 fp32 columns.  Grids that are not
// a multiple of 8 keep the identity mapping (every block index must stay below gridDim.x).
__device__ __forceinline__ int xcd_block() {
    const int b = blockIdx.x, n = gridDim.x;
    if ((n & 7) == 0) return (b & 7) * (n >> 3) + (b >> 3);
    return b;
}

// Ensemble launches (the *_ens_kernel families; C ABI cloudsc2_*_ens_*): a one-dimensional grid of nmem * bpm workgroups,
// bpm = ceil(nx / kColBlock) column blocks per member.  The remapped block index of xcd_block() - a permutation of
// [0, gridDim.x) for every grid size - is split as member * bpm + column block, so every (member, column block) pair is
// served by exactly one workgroup, and with the remap active the workgroups of one XCD own one contiguous eighth of that
// order: whole members, or one contiguous run of a member's columns.  Both values are workgroup-uniform and are held in
// SGPRs (readfirstlane states it).  Returns the column block.
__device__ __forceinline__ int ens_block(int bpm, int& member) {
    const uint32_t v = uint32_t(xcd_block()), m = v / uint32_t(bpm);
    member = __builtin_amdgcn_readfirstlane(int(m));
    return __builtin_amdgcn_readfirstlane(int(v - m * uint32_t(bpm)));
}
// What an ensemble kernel takes beside the arguments of its single form: the member stride in elements (one per call, for
// every field) and the column blocks per member.  The launchers check nmem * bpm against the grid limit.
struct EnsGeom {
    int64_t ms;
    int bpm;
};
constexpr int64_t kMaxGrid = 0x7FFFFFFF;   // workgroups of a one-dimensional grid

// Ensembles that SHARE part of their state (the *_enss_kernel families; C ABI cloudsc2_*_enss_*): EnsGeom plus
//   shared   bit i: state input i (NL_IN_*) is ONE field, the call's pointer, read by every member - its base is 0 instead of
//            member * ms.  The select is wave-uniform (a scalar compare and select where the pointer is formed); the lanes'
//            offsets do not change;
//   eta_ms   0: one `eta` for all members; otherwise member m's level vector starts m * eta_ms elements behind `eta`.  A
//            workgroup serves one member and builds its level table from that member's vector;
//   order    how the remapped block index is split (enss_block): kMemberMajor as ens_block (member * bpm + column block),
//            kColumnMajor as column block * nmem + member - the nmem workgroups that read one column block of a shared
//            field are then neighbours in dispatch order.
// A kernel templated on its geometry G compiles the shared form where G is EnssGeom; with EnsGeom nothing of it exists.
enum EnsOrder : int { kMemberMajor = 0, kColumnMajor = 1 };
constexpr int kEnssDefaultOrder = kMemberMajor;   // docs/TUNING_LOG.md 3.27
struct EnssGeom : EnsGeom {
    uint32_t shared;
    int nmem;
    int order;
    int64_t eta_ms;
};
template <typename G>
constexpr bool kSharedGeom = std::is_same<G, EnssGeom>::value;
__device__ __forceinline__ int enss_block(const EnssGeom& g, int& member) {
    if (g.order == kMemberMajor) return ens_block(g.bpm, member);
    const uint32_t v = uint32_t(xcd_block()), cb = v / uint32_t(g.nmem);
    member = __builtin_amdgcn_readfirstlane(int(v - cb * uint32_t(g.nmem)));
    return __builtin_amdgcn_readfirstlane(int(cb));
}

// ---- math in the working precision --------------------------------------------------------
template <typename T> __device__ __forceinline__ T rexp(T x);
template <> __device__ __forceinline__ double rexp<double>(double x) { return exp(x); }
template <> __device__ __forceinline__ float rexp<float>(float x) { return expf(x); }
template <typename T> __device__ __forceinline__ T rtanh(T x);
template <> __device__ __forceinline__ double rtanh<double>(double x) { return tanh(x); }
template <> __device__ __forceinline__ float rtanh<float>(float x) { return tanhf(x); }
template <typename T> __device__ __forceinline__ T rcosh(T x);
template <> __device__ __forceinline__ double rcosh<double>(double x) { return cosh(x); }
template <> __device__ __forceinline__ float rcosh<float>(float x) { return coshf(x); }
template <typename T> __device__ __forceinline__ T rsqrt_(T x);
template <> __device__ __forceinline__ double rsqrt_<double>(double x) { return sqrt(x); }
template <> __device__ __forceinline__ float rsqrt_<float>(float x) { return sqrtf(x); }
template <typename T> __device__ __forceinline__ T rpow(T x, T y);
template <> __device__ __forceinline__ double rpow<double>(double x, double y) { return pow(x, y); }
template <> __device__ __forceinline__ float rpow<float>(float x, float y) { return powf(x, y); }
// Reciprocal by hardware seed + Newton steps (v_rcp_f64 + 4 fma; v_rcp_f32 + 2 fma), about
// half the instructions of the IEEE-correct division sequence hipcc emits for `a / b`.  The column
// kernels are VALU-issue-bound in fp64 (profiles/), so divisions are expressed as x * frcp(y) and
// reciprocals shared between the expressions that divide by the same quantity.
// Accuracy, for normal x with normal 1/x: at most 1 ulp (faithful; the last step rounds r (2 - x r) =
// 1/x (1 - d^2) once, d the relative error before it); measured: worst 0.50 ulp over 5 M arguments per precision
// (tests/test_math_primitives.py).  Outside that range the Newton step meets inf * 0 and frcp is NOT the IEEE
// quotient (measured on gfx950; v_rcp_f32 takes a subnormal for 0 and flushes a subnormal result):
//         x                      1 / x (IEEE)         frcp(x)
//         +-0                    +-inf                NaN
//         +-inf                  +-0                  NaN
//         subnormal              finite or +-inf      fp64: NaN where 1/x overflows, else <= 1 ulp;  fp32: NaN
//         2^1022 < |x| <= max    subnormal            fp64: <= 1 ulp (subnormal spacing);  fp32: +-0
//         NaN                    NaN                  NaN
// No level loop may use frcp of a divisor that can be 0 or inf for finite inputs without a guard: the call
// sites are listed with their guards in docs/TUNING_LOG.md 3.14.
template <typename T> __device__ __forceinline__ T frcp(T x);
template <> __device__ __forceinline__ double frcp<double>(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
template <> __device__ __forceinline__ float frcp<float>(float x) {
    float r = __builtin_amdgcn_rcpf(x);
    r = fmaf(fmaf(-x, r, 1.0f), r, r);
    return r;
}
// exp() for the level loops.  ocml's exp re-materialises its 11 polynomial coefficients into VGPRs
// on every call (destructive v_fmac form: 2 v_mov per coefficient, ~42 VALU per call); here the
// coefficients travel as kernel arguments (`ExpK`), stay in registers across the loop and the
// evaluation is 19 VALU: n = rint(x log2 e), r = x - n ln2 (two-term Cody-Waite), degree-12 polynomial
// in Horner form on |r| <= ln2/2, ldexp.  The polynomial is 1 + r + r^2/2 + r^3 g(r) with g fitted, not
// truncated: the Taylor coefficients 1/3! .. 1/12! leave r^13/13! = 2.4e-16 of exp(r) at the interval
// ends and measured 2.32 ulp; the fit's own error is 1e-18, so what remains is the rounding of the last
// Horner steps.  Measured against a 50-digit reference (tests/test_math_primitives.py, table in
// docs/TUNING_LOG.md 3.14): worst 0.86 ulp, ocml's exp 0.87 ulp on the same arguments.  The argument is
// clamped to [-746, 710] first (exp(-746) = 0, exp(710) = inf in double): the autoconversion terms
// exp(-(cld/crit)^2) reach arguments of -1e20, where the Cody-Waite reduction would lose all bits.
// NaN stays NaN, -inf gives 0, +inf gives inf, results below 2^-1022 are subnormal (ldexp rounds them).
template <typename T>
struct ExpK {
    T l2e, ln2h, ln2l, c12, c11, c10, c9, c8, c7, c6, c5, c4, c3;
};
template <typename T>
inline ExpK<T> make_expk() {
    ExpK<T> k;
    k.l2e = T(1.4426950408889634);
    k.ln2h = T(6.93147180369123816490e-01);
    k.ln2l = T(1.90821492927058770002e-10);
    // c3 .. c12: profiles/fit_exp_poly.py (Chebyshev fit of (exp(r) - 1 - r - r^2/2) / r^3 on |r| <= ln2/2)
    k.c3 = T(1.66666666666666685e-01);
    k.c4 = T(4.16666666666666644e-02);
    k.c5 = T(8.33333333333006500e-03);
    k.c6 = T(1.38888888888865540e-03);
    k.c7 = T(1.98412698630405450e-04);
    k.c8 = T(2.48015873171351639e-05);
    k.c9 = T(2.75572684803100238e-06);
    k.c10 = T(2.75572829840558774e-07);
    k.c11 = T(2.51003758325613201e-08);
    k.c12 = T(2.09112297297586281e-09);
    return k;
}
template <typename T> __device__ __forceinline__ T fexp(const ExpK<T>& k, T x);
template <> __device__ __forceinline__ double fexp<double>(const ExpK<double>& k, double x) {
    {
        // clamp; a NaN argument must stay NaN (v_max / v_min return their non-NaN operand, which would turn exp(NaN)
        // into exp(-746) = 0 where the reference propagates the NaN): its high word is patched back in - 2 VALU
        const double xc = __builtin_fmin(__builtin_fmax(x, -746.0), 710.0);
        int hi = __double2hiint(xc);
        if (x != x) hi = 0x7FF80000;
        x = __hiloint2double(hi, __double2loint(xc));
    }
    const double n = __builtin_rint(x * k.l2e);
    double r = __builtin_fma(-n, k.ln2h, x);
    r = __builtin_fma(-n, k.ln2l, r);
    double p = __builtin_fma(k.c12, r, k.c11);
    p = __builtin_fma(p, r, k.c10);
    p = __builtin_fma(p, r, k.c9);
    p = __builtin_fma(p, r, k.c8);
    p = __builtin_fma(p, r, k.c7);
    p = __builtin_fma(p, r, k.c6);
    p = __builtin_fma(p, r, k.c5);
    p = __builtin_fma(p, r, k.c4);
    p = __builtin_fma(p, r, k.c3);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, static_cast<int>(n));
}
template <> __device__ __forceinline__ float fexp<float>(const ExpK<float>&, float x) { return expf(x); }
// A product that is ROUNDED as a product, whatever consumes it: contraction is switched off for this multiply, so the
// backend cannot fold it into a following add / subtract as an fma.  The kernels that fuse `state_increment` in
// (x_i = f * x formed in registers instead of loaded) use it to reproduce the stored products bit for bit.
template <typename T>
__device__ __forceinline__ T rounded_product(T f, T x) {
#pragma clang fp contract(off)
    return f * x;
}
template <typename T> __device__ __forceinline__ T rmin(T a, T b) { return a < b ? a : b; }
template <typename T> __device__ __forceinline__ T rmax(T a, T b) { return a > b ? a : b; }
template <typename T> __device__ __forceinline__ T sq(T x) { return x * x; }
template <typename T> __device__ __forceinline__ T cube(T x) { return x * x * x; }

// The logistic forms of the mixed-phase weight (nonlinear/_stencils/cloudsc2.py:147, and its derivative in the TL / AD
// stencils).  With u = 0.17 (t - RLPTRC), ex = exp(-2u) and rr = 1 / (1 + ex) - `fw2` is 2 * 0.17 (make_nlk):
//     0.545 (tanh u + 1) = 1.09 rr          1 / cosh(u)^2 = 4 ex rr^2
// one exponential and one reciprocal instead of tanh and cosh, and no cancellation in tanh(u) + 1 for cold t (u << 0,
// where tanh u -> -1).  ex overflows to inf for t < RLPTRC - 2 088 K only; rr is then 0 and sech2 inf * 0 = NaN, far outside
// any temperature.  cloudsc2_nl needs the weight alone; cloudsc2_tl and the forward sweep of cloudsc2_ad keep ex and rr for
// sech2.  tests/primitives_probe.hip calls these two, so the accuracy test measures the code the level loops run.
template <typename T>
__device__ __forceinline__ T logistic_fwat(const ExpK<T>& xk, T fw2, T rlptrc, T t, T& ex, T& rr) {
    ex = fexp<T>(xk, -fw2 * (t - rlptrc));
    rr = frcp<T>(T(1.0) + ex);
    return T(1.09) * rr;
}
template <typename T>
__device__ __forceinline__ T logistic_fwat(const ExpK<T>& xk, T fw2, T rlptrc, T t) {
    T ex, rr;
    return logistic_fwat<T>(xk, fw2, rlptrc, t, ex, rr);
}
template <typename T>
__device__ __forceinline__ T logistic_sech2(T ex, T rr) {
    return T(4.0) * ex * rr * rr;
}

// Tangent-linear perturbation of the part of a precipitation flux f that evaporates, dpr f / prtot
// (tangent_linear/_stencils/cloudsc2.py, the evaporation block): (dpr_i f + dpr f_i) / prtot - dpr f prtot_i / prtot^2, with
// rpr = frcp(prtot).  When everything evaporates (dpr == prtot) the part is the flux itself and what is left of its
// perturbation, f_i - evaporated_i, is 0; the reference's spelling gives exactly 0 there for 82 % of all operands,
// this one with x * rpr for 46 %, and otherwise an ulp of perturbations that reach 1e12 at dt = 3600 s, which swamps
// the levels below (docs/TUNING_LOG.md 3.14: which of the two happened depended on the last bit of an exp).  For that
// case the same derivative is arranged as f_i + f / prtot (dpr_i - prtot_i): its second term is exactly 0 when the
// capped dpr_i equals prtot_i, so the perturbation left is exactly 0.  The trajectory keeps the reference's dpr f / prtot.
// The last term is formed from the ratios dpr / prtot and f / prtot: as dpr * f * prtot_i * rpr * rpr its first two products
// are of three small numbers (a residual flux of 5e-17 beside a prtot of 1e-10 and a prtot_i of 5e-12 gave 1e-38) and went
// subnormal in float32 before rpr^2 brought them back, which cost the term its last bits and the kernel its exact
// homogeneity in the perturbation (tests/test_metamorphic_linearity.py).
template <typename T>
__device__ __forceinline__ T evaporated_i(T dpr, T dpr_i, T f, T f_i, T prtot, T prtot_i, T rpr) {
    const T all = f_i + f * rpr * (dpr_i - prtot_i);
    const T part = (dpr_i * f + dpr * f_i) * rpr - (dpr * rpr) * (f * rpr) * prtot_i;
    return dpr == prtot ? all : part;
}

// ---- externals in the working precision -----------------------------------------------------
template <typename T>
struct Ext {
    T R2ES, R3IES, R3LES, R4IES, R4LES, R5IES, R5LES;
    T R5ALSCP, R5ALVCP, RALSDCP, RALVDCP;
    T RTICE, RTWAT, RTWAT_RTICE_R, RTICECU, RTWAT_RTICECU_R, RVTMP2;
    T RCPD, RD, RETV, RG, RLMLT, RLSTT, RLVTT, RTT;
    T RCLCRIT, RKCONV, RLMIN, RPECONS, RLPTRC;
    T ZEPS1, ZEPS2, ZQMAX, ZSCAL, QMAX;
    int32_t NLEV;
};

template <typename T>
inline Ext<T> make_ext(const Cloudsc2Params& p) {
    Ext<T> e;
#define CS2_CP(n) e.n = static_cast<T>(p.n)
    CS2_CP(R2ES); CS2_CP(R3IES); CS2_CP(R3LES); CS2_CP(R4IES); CS2_CP(R4LES); CS2_CP(R5IES); CS2_CP(R5LES);
    CS2_CP(R5ALSCP); CS2_CP(R5ALVCP); CS2_CP(RALSDCP); CS2_CP(RALVDCP);
    CS2_CP(RTICE); CS2_CP(RTWAT); CS2_CP(RTWAT_RTICE_R); CS2_CP(RTICECU); CS2_CP(RTWAT_RTICECU_R); CS2_CP(RVTMP2);
    CS2_CP(RCPD); CS2_CP(RD); CS2_CP(RETV); CS2_CP(RG); CS2_CP(RLMLT); CS2_CP(RLSTT); CS2_CP(RLVTT); CS2_CP(RTT);
    CS2_CP(RCLCRIT); CS2_CP(RKCONV); CS2_CP(RLMIN); CS2_CP(RPECONS); CS2_CP(RLPTRC);
    CS2_CP(ZEPS1); CS2_CP(ZEPS2); CS2_CP(ZQMAX); CS2_CP(ZSCAL); CS2_CP(QMAX);
#undef CS2_CP
    e.NLEV = p.NLEV;
    return e;
}

// ---- saturation (common/_stencils/saturation.py:23-42 + fcttre.py:22-57), one point -------------------------
// Shared by saturation_kernel / saturation_vec_kernel (cloudsc2_aux.hip) and the fused-saturation NL variant
// (cloudsc2_nl.hip).  Contraction is switched off inside: every caller then evaluates the literal sequence of
// multiplies and adds below (frcp / fexp spell their fma's out), so the three kernels agree bit for bit whatever
// their surrounding code looks like.  MODE 0: LPHYLIN; 1: not LPHYLIN, KFLAG == 1 (f_foeewmcu); 2: f_foeewm.
// KEEP IN STEP: saturation_point_d below repeats this sequence for its value, and ad_step_kernel calls both for the same
// point (the value at the head of a level, the derivative where its adjoints are stored).  Change the operations or the
// comparisons of one and the other must follow; tests/test_saturation_grad.py holds the two values bit-equal.
template <typename T>
__device__ __forceinline__ T foealfa(const Ext<T>& e, T t) {
#pragma clang fp contract(off)
    return rmin<T>(T(1.0), sq((rmax<T>(e.RTICE, rmin<T>(e.RTWAT, t)) - e.RTICE) * e.RTWAT_RTICE_R));
}
template <typename T>
__device__ __forceinline__ T foealfcu(const Ext<T>& e, T t) {
#pragma clang fp contract(off)
    return rmin<T>(T(1.0), sq((rmax<T>(e.RTICECU, rmin<T>(e.RTWAT, t)) - e.RTICECU) * e.RTWAT_RTICECU_R));
}
template <typename T, int MODE>
__device__ __forceinline__ T saturation_point(const Ext<T>& e, const ExpK<T>& xk, T tt, T app) {
#pragma clang fp contract(off)
    const T rap = frcp<T>(app);
    const T dl = tt - e.R4LES, di = tt - e.R4IES, dtt = tt - e.RTT;
    const T al = e.R3LES * dtt, ai = e.R3IES * dtt;
    const T foeewl = fexp<T>(xk, al * frcp<T>(dl));
    const T foeewi = fexp<T>(xk, ai * frcp<T>(di));
    T qs;
    if constexpr (MODE == 0) {
        const T alfa = foealfa(e, tt);
        const T wl = alfa * (e.R2ES * foeewl);
        const T wi = (T(1.0) - alfa) * (e.R2ES * foeewi);
        qs = rmin<T>((wl + wi) * rap, e.QMAX);
    } else {
        const T alfa = (MODE == 1) ? foealfcu(e, tt) : foealfa(e, tt);
        const T wl = alfa * foeewl;
        const T wi = (T(1.0) - alfa) * foeewi;
        qs = rmin<T>(e.R2ES * (wl + wi) * rap, e.QMAX);
    }
    const T den = T(1.0) - e.RETV * qs;
    return qs * frcp<T>(den);
}

// saturation_point with its derivative (BUILD EXTENSION: the reference has no TL / AD of `saturation`):
// qsat, g_t = d qsat / d t and g_ap = d qsat / d ap of one point.  The value is saturation_point's own sequence (same
// primitives, same comparisons, each exponential evaluated once), so the two agree bit for bit and the derivative is taken
// on the branch the value took; a clamped branch has derivative 0:
//     alfa' = 2 (t - TI) RI^2  for TI < t < RTWAT and alfa < 1, else 0   (RI is handed in, not formed from
//             RTWAT - TI: only where RI == 1 / (RTWAT - TI) do the inner and the outer clamp of alfa meet at t == RTWAT)
//     ew_t  = alfa' (el - ei) + alfa el R3LES (RTT - R4LES) / (t - R4LES)^2 + (1 - alfa) ei R3IES (RTT - R4IES) / (t - R4IES)^2
//     clipped at QMAX (the value's own `ew / ap < QMAX` is false): qs_t = qs_ap = 0;  else qs_t = ew_t / ap, qs_ap = -ew / ap^2
//     g_t = qs_t / (1 - RETV qs)^2,  g_ap = qs_ap / (1 - RETV qs)^2
// Callers: saturation_tl_kernel / saturation_ad_kernel (cloudsc2_aux.hip), tl_step_kernel, ad_step_kernel.
template <typename T>
struct SatD {
    T qsat, g_t, g_ap;
};
template <typename T, int MODE>
__device__ __forceinline__ SatD<T> saturation_point_d(const Ext<T>& e, const ExpK<T>& xk, T tt, T app) {
#pragma clang fp contract(off)
    const T rap = frcp<T>(app);
    const T dl = tt - e.R4LES, di = tt - e.R4IES, dtt = tt - e.RTT;
    const T al = e.R3LES * dtt, ai = e.R3IES * dtt;
    const T rdl = frcp<T>(dl), rdi = frcp<T>(di);
    const T foeewl = fexp<T>(xk, al * rdl);
    const T foeewi = fexp<T>(xk, ai * rdi);
    const T ti = (MODE == 1) ? e.RTICECU : e.RTICE, ri = (MODE == 1) ? e.RTWAT_RTICECU_R : e.RTWAT_RTICE_R;
    const T alfa = (MODE == 1) ? foealfcu(e, tt) : foealfa(e, tt);
    const T el = e.R2ES * foeewl, ei = e.R2ES * foeewi;
    T q0;
    if constexpr (MODE == 0) {
        q0 = (alfa * el + (T(1.0) - alfa) * ei) * rap;
    } else {
        q0 = e.R2ES * (alfa * foeewl + (T(1.0) - alfa) * foeewi) * rap;
    }
    const bool open = q0 < e.QMAX;            // rmin's own comparison
    const T qs = open ? q0 : e.QMAX;
    const T rden = frcp<T>(T(1.0) - e.RETV * qs);
    // the outer clamp min(1, .) of alfa binds below RTWAT whenever RI (RTWAT - TI) > 1 (RI is a parameter of its own):
    // alfa < 1 is that clamp's own comparison on the value already formed.  At the tie alfa == 1 with t < RTWAT the
    // derivative is taken as 0, like at the other clamps here (a subgradient; tests/saturation_oracle.py's torch.clamp
    // passes the gradient at x == max, so the two differ on that one point).  Written as a factor, which keeps
    // tl_ens_step_kernel<double> free of scratch (held by tests/test_ensemble_isa.py).
    const T dalfa = (ti < tt && tt < e.RTWAT) ? T(2.0) * (tt - ti) * ri * ri * (alfa < T(1.0) ? T(1.0) : T(0.0)) : T(0.0);
    const T ew_t = dalfa * (el - ei) + alfa * el * (e.R3LES * (e.RTT - e.R4LES)) * (rdl * rdl) +
                   (T(1.0) - alfa) * ei * (e.R3IES * (e.RTT - e.R4IES)) * (rdi * rdi);
    const T cor2 = rden * rden;
    SatD<T> r;
    r.qsat = qs * rden;
    r.g_t = open ? ew_t * rap * cor2 : T(0.0);
    r.g_ap = open ? -(q0 * rap) * cor2 : T(0.0);
    return r;
}

// Pin a wave-uniform value in a VGPR.  The fp64 kernels use ~45 named double constants; together with
// the 26 field pointers that is far more than the 102 SGPRs of a wave, and hipcc then spills SGPRs to
// VGPR lanes and pays two v_readlane per 64-bit constant per use.  A constant that lives in a VGPR
// pair is a plain VALU operand (no extra instruction); at one wave per SIMD there are VGPRs to spare.
template <typename T>
__device__ __forceinline__ void pin_vgpr(T& x) {
    asm volatile("" : "+v"(x));
}
// One pin per value, in argument order: register assignment follows that order, so each kernel keeps its own list.
template <typename... Ts>
__device__ __forceinline__ void pin_vgprs(Ts&... xs) {
    (pin_vgpr(xs), ...);
}
template <typename T>
__device__ __forceinline__ void pin_expk(ExpK<T>& xk) {
    pin_vgprs(xk.l2e, xk.ln2h, xk.ln2l, xk.c12, xk.c11, xk.c10, xk.c9, xk.c8, xk.c7, xk.c6, xk.c5, xk.c4, xk.c3);
}

// "This loaded word has landed": the value must be in its register here, so hipcc waits for its load HERE.  Used on
// words loaded before a level loop and first read inside it: a load still pending at the loop header makes hipcc's
// wait-count insertion settle for `s_waitcnt vmcnt(0)` at the first use INSIDE the loop - on every level, i.e. the
// prefetch of the next level is waited for in the middle of the current one (docs/TUNING_LOG.md 3.9).
template <typename T>
__device__ __forceinline__ void landed(T& x) {
    asm volatile("" : "+v"(x));
}

// "Every memory operation of this wave has completed": the level's stores are drained before the next level's loads are
// requested.  Costs the stores' completion latency once per level and buys HBM a cleaner read / write phase structure;
// the register-path NL and TL kernels measured faster with it, cloudsc2_ad without (docs/TUNING_LOG.md 3.9).
__device__ __forceinline__ void drain_vmem() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Field access by 32-bit BYTE offset from a uniform base pointer: hipcc then emits the
// `global_load_dwordx2 v, v_off, s[base:base+1]` form (no per-access 64-bit VALU address arithmetic).
// The launchers guarantee (nz+1) * lev_stride * sizeof(T) < 2^32.
// Loads and stores are non-temporal: every field element is touched exactly once per launch, and streaming reads/writes
// that do not linger in L2 measured faster on the mixed 16-read / 10-write stream pattern (profiles/microbench_stream.hip;
// A/B in profiles/ab_nl.py).
// The offset type `O` is uint32_t in every kernel but the BIG instantiations (fields of 4 GiB and more, see offset_t):
// there it is uint64_t and hipcc emits the `v[a:a+1], off` form after a 64-bit VALU add per access.
template <typename T, typename O>
__device__ __forceinline__ T ldg(const T* base, O boff) {
    return __builtin_nontemporal_load(reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + boff));
}
template <typename T, typename O>
__device__ __forceinline__ void stg(T* base, O boff, T v) {
    __builtin_nontemporal_store(v, reinterpret_cast<T*>(reinterpret_cast<char*>(base) + boff));
}
// Default-policy load for the ONE field with a producer just upstream: `in_qsat` is written by `saturation` right before
// cloudsc2_nl reads it (run_nonlinear.py:117-118) and, at 72 MB for 65 536 columns, is still in the 256 MB
// memory-side cache - unless the store or the load is marked non-temporal (measured: saturation + NL 391 -> 370 us).
template <typename T, typename O>
__device__ __forceinline__ T ldg_keep(const T* base, O boff) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + boff);
}
// streaming access for the pointwise helper kernels (64-bit indexing, same non-temporal policy)
template <typename T>
__device__ __forceinline__ T ntload(const T* a) {
    return __builtin_nontemporal_load(a);
}
template <typename T>
__device__ __forceinline__ void ntstore(T* a, T v) {
    __builtin_nontemporal_store(v, a);
}
// Producer-consumer residency of `qsat` (saturation -> cloudsc2_nl, run_nonlinear.py:117-118): default cache policy
// on that one store / load pays when the field fits the 256 MB memory-side cache beside the streams passing through
// (72 MB at 65 536 fp64 columns: saturation + NL 391 -> 370 us) and costs 3-4 % when it does not (289 MB at
// 524 288 fp32 columns: 1 598 -> 1 662 us), so both launchers decide with the same rule.
template <typename T>
inline bool qsat_fits_cache(int nz, int64_t ls) {
    return static_cast<uint64_t>(nz + 1) * static_cast<uint64_t>(ls) * sizeof(T) <= (uint64_t(128) << 20);
}
template <typename T>
inline bool fits_u32_offsets(int nz, int64_t ls) {
    return static_cast<uint64_t>(nz + 1) * static_cast<uint64_t>(ls) * sizeof(T) <= 0xFFFFFFFFull;
}
// Fields of 4 GiB and more ((nz+1) * lev_stride * sizeof(T) > 2^32 - 1: 3.89 M fp64 columns at 137 levels): the plain
// stencils (cloudsc2_nl / _tl / _ad) switch to the BIG instantiation of their register-path kernel, whose byte offsets are
// 64-bit; the fused build extensions and the LDS-ring kernels keep 32-bit offsets and refuse such a call
// (CLOUDSC2_E_UNSUPPORTED).  Columns are independent, so a caller can also split such a call into column windows of a
// narrower allocation - but NOT into windows of the same allocation: the level stride, not nx, is what overflows.
template <bool BIG>
using offset_t = typename std::conditional<BIG, uint64_t, uint32_t>::type;

// ---- field pointer bundles (kernel arguments, by value) --------------------------------------
template <typename T, int N>
struct CPtrs {
    const T* p[N];
    __device__ __forceinline__ const T* operator()(int i) const { return p[i]; }   // a field-pointer source (load_level)
};
template <typename T, int N>
struct MPtrs { T* p[N]; };

// ---- one level of the 16 NL input fields (the level sweeps of cloudsc2_nl / _tl / _ad) -------------------------------
template <typename T>
struct LevelIn {
    T ap, aph1, lu1, lude, mfd, mfu, q, qi, ql, qsat, supsat, t, tq, tqi, tql, tt;
};

// `ptr(i)`: base pointer of input field i (a CPtrs bundle, or a read from the kernarg segment); `o` = byte offset of
// (level k, this lane's column); `lsb` = level stride in bytes (`O`: uint32_t, or uint64_t in the BIG instantiations).
// aph and lu are read one half level below (aph[k+1], lu[k+1]).  skipq: in_qsat is not read (the fused-saturation NL
// variant computes it); keepq: in_qsat was just written by `saturation` and fits the memory-side cache (launch_nl), so its
// load uses the default cache policy and hits it.
template <typename T, typename O, typename P>
__device__ __forceinline__ LevelIn<T> load_level(const P& ptr, O lsb, O o, bool skipq = false, bool keepq = false) {
    LevelIn<T> x;
    x.ap = ldg(ptr(NL_IN_AP), o);
    x.aph1 = ldg(ptr(NL_IN_APH), o + lsb);
    x.lu1 = ldg(ptr(NL_IN_LU), o + lsb);
    x.lude = ldg(ptr(NL_IN_LUDE), o);
    x.mfd = ldg(ptr(NL_IN_MFD), o);
    x.mfu = ldg(ptr(NL_IN_MFU), o);
    x.q = ldg(ptr(NL_IN_Q), o);
    x.qi = ldg(ptr(NL_IN_QI), o);
    x.ql = ldg(ptr(NL_IN_QL), o);
    x.qsat = skipq ? T(0.0) : (keepq ? ldg_keep(ptr(NL_IN_QSAT), o) : ldg(ptr(NL_IN_QSAT), o));
    x.supsat = ldg(ptr(NL_IN_SUPSAT), o);
    x.t = ldg(ptr(NL_IN_T), o);
    x.tq = ldg(ptr(NL_IN_TND_CML_Q), o);
    x.tqi = ldg(ptr(NL_IN_TND_CML_QI), o);
    x.tql = ldg(ptr(NL_IN_TND_CML_QL), o);
    x.tt = ldg(ptr(NL_IN_TND_CML_T), o);
    return x;
}

// state_increment (common/_stencils/state_increment.py:61-80) applied on the fly: x_i = f * x, supsat_i = 0 with
// IGNORE_SUPSAT - the very products the stand-alone increment kernel stores (cloudsc2_aux.hip), so the fused variants feed
// the level function exactly the words the separate calls would load (rounded_product: never half of an fma).
template <typename T>
__device__ __forceinline__ LevelIn<T> increment(const LevelIn<T>& x, T f, bool zero_supsat) {
    LevelIn<T> y;
#define CS2_P(m) y.m = rounded_product<T>(f, x.m)
    CS2_P(ap); CS2_P(aph1); CS2_P(lu1); CS2_P(lude); CS2_P(mfd); CS2_P(mfu); CS2_P(q); CS2_P(qi); CS2_P(ql); CS2_P(qsat);
    CS2_P(t); CS2_P(tq); CS2_P(tqi); CS2_P(tql); CS2_P(tt);
#undef CS2_P
    y.supsat = zero_supsat ? T(0.0) : rounded_product<T>(f, x.supsat);
    return y;
}

// ---- LDS-DMA ring (nl_ring_kernel, tl_ring_kernel) --------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef const __attribute__((address_space(1))) void* glb_void_ptr;
constexpr int kDmaNT = 2;   // cache-policy operand of the ring's input DMAs: non-temporal (every byte is read once)

// Slot of a ring whose level holds NF input fields (+ XDMA more DMA images of 16 B x 64 lanes).  One DMA instruction moves
// 16 B per lane = NPL columns, so it carries NPL fields of the wave's 64 columns; field f of a slot starts at f * 64 * sizeof(T).
template <typename T, int NF, int XDMA = 0>
struct RingGeom {
    static constexpr int NPL = 16 / int(sizeof(T));       // columns per lane per DMA = fields per DMA
    static constexpr int NI = NF / NPL;                   // DMA instructions per level
    static constexpr int DATA = NF * 64 * int(sizeof(T));  // the NF input fields of one level
    static constexpr int SLOT = DATA + XDMA * 1024;
};
// LDS of a ring launch: [eta | scalm table][pad to 1 KB][wave 0: depth slots][wave 1: depth slots] ...
template <typename G, typename T>
inline size_t ring_lds_bytes(int nz, int depth) {
    return ((2 * size_t(nz + 1) * sizeof(T) + 1023) & ~size_t(1023)) + size_t(kColBlock / 64) * depth * G::SLOT;
}

// The ring reads: this lane's column of 16 consecutive fields of a slot at LDS byte address %[a] into operands %0 .. %15.
// Only the text is shared - every ring read stays ONE asm statement with its own `s_waitcnt vmcnt(N)` (nl_ring_kernel).
#define CS2_DS_READ16_B64            \
    "ds_read_b64 %0, %[a]\n\t"                \
    "ds_read_b64 %1, %[a] offset:512\n\t"     \
    "ds_read_b64 %2, %[a] offset:1024\n\t"    \
    "ds_read_b64 %3, %[a] offset:1536\n\t"    \
    "ds_read_b64 %4, %[a] offset:2048\n\t"    \
    "ds_read_b64 %5, %[a] offset:2560\n\t"    \
    "ds_read_b64 %6, %[a] offset:3072\n\t"    \
    "ds_read_b64 %7, %[a] offset:3584\n\t"    \
    "ds_read_b64 %8, %[a] offset:4096\n\t"    \
    "ds_read_b64 %9, %[a] offset:4608\n\t"    \
    "ds_read_b64 %10, %[a] offset:5120\n\t"   \
    "ds_read_b64 %11, %[a] offset:5632\n\t"   \
    "ds_read_b64 %12, %[a] offset:6144\n\t"   \
    "ds_read_b64 %13, %[a] offset:6656\n\t"   \
    "ds_read_b64 %14, %[a] offset:7168\n\t"   \
    "ds_read_b64 %15, %[a] offset:7680\n\t"
#define CS2_DS_READ16_B32            \
    "ds_read_b32 %0, %[a]\n\t"                \
    "ds_read_b32 %1, %[a] offset:256\n\t"     \
    "ds_read_b32 %2, %[a] offset:512\n\t"     \
    "ds_read_b32 %3, %[a] offset:768\n\t"     \
    "ds_read_b32 %4, %[a] offset:1024\n\t"    \
    "ds_read_b32 %5, %[a] offset:1280\n\t"    \
    "ds_read_b32 %6, %[a] offset:1536\n\t"    \
    "ds_read_b32 %7, %[a] offset:1792\n\t"    \
    "ds_read_b32 %8, %[a] offset:2048\n\t"    \
    "ds_read_b32 %9, %[a] offset:2304\n\t"    \
    "ds_read_b32 %10, %[a] offset:2560\n\t"   \
    "ds_read_b32 %11, %[a] offset:2816\n\t"   \
    "ds_read_b32 %12, %[a] offset:3072\n\t"   \
    "ds_read_b32 %13, %[a] offset:3328\n\t"   \
    "ds_read_b32 %14, %[a] offset:3584\n\t"   \
    "ds_read_b32 %15, %[a] offset:3840\n\t"
// ... and their output operands %0 .. %15
#define CS2_LEVEL_OUTS(x)                                                                                               \
    "=&v"(x.ap), "=&v"(x.aph1), "=&v"(x.lu1), "=&v"(x.lude), "=&v"(x.mfd), "=&v"(x.mfu), "=&v"(x.q), "=&v"(x.qi),         \
        "=&v"(x.ql), "=&v"(x.qsat), "=&v"(x.supsat), "=&v"(x.t), "=&v"(x.tq), "=&v"(x.tqi), "=&v"(x.tql), "=&v"(x.tt)

// Field pointers fetched from the KERNARG SEGMENT at their point of use (cloudsc2_ad).  The AD kernel takes 52 field
// pointers: 104 SGPRs, more than a wave has (102), before the first constant.  Passed as ordinary by-value arguments they
// are all preloaded at kernel entry, and hipcc spills the excess to VGPR lanes and restores each with two v_readlane_b32 -
// VALU issue slots - per memory instruction: 290 of the 1 800 VALU instructions of a cloudsc2_ad level in fp32, 396 of
// 2 386 in fp64 (r04, counted on the ISA).  With the arguments as ONE struct (kernarg offset 0) and this view, a pointer is
// read with a scalar load (s_load_dwordx16: SMEM, no VALU slot) right before the loads / stores that use it and its SGPRs
// are free again afterwards.  `fresh()` makes the compiler forget what it knows about the kernarg pointer, so the scalar
// loads behind `K->...` cannot be hoisted above that point (out of the level loop and back into long-lived SGPRs): call
// it once per level.  Worth -2 ... -4 % on cloudsc2_ad fp32 and 0 ... -1.6 % in fp64 (the kernels wait for HBM, not for
// issue slots: docs/TUNING_LOG.md 3.11); the same change on cloudsc2_tl measured +0.7 % and was not kept.
template <typename ARGS>
struct KernArgs {
    typedef const __attribute__((address_space(4))) ARGS KA;
    KA* ka;
    __device__ __forceinline__ KernArgs() : ka((KA*)__builtin_amdgcn_kernarg_segment_ptr()) {}
    template <bool ON = true>
    __device__ __forceinline__ void fresh() {
        if constexpr (ON) asm volatile("" : "+s"(ka));
    }
    __device__ __forceinline__ KA* operator->() const { return ka; }
};

// diagnostics: the launchers record the name of the kernel they enqueued (cloudsc2_last_kernel(), process-wide)
void note_kernel(const char* name);

// ---- per-device facts the launchers cache (host side) ---------------------------------------------------------
// The header asks for one host thread per device, but nothing here breaks if two threads launch on one device (a
// capture thread beside the main thread): the caches are relaxed atomics, so a reader sees either "not yet known" and
// repeats the (idempotent) query / hipFuncSetAttribute, or the final value - never a torn one.  Devices are indexed
// directly; an ordinal beyond kMaxDevices is refused instead of aliased.
constexpr int kMaxDevices = 64;
inline int current_device(int& dev) {
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    return (dev >= 0 && dev < kMaxDevices) ? 0 : -2;
}
inline int device_cus(int dev) {
    static std::atomic<int> cus[kMaxDevices] = {};
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}
// > 64 KB of dynamic LDS needs an opt-in per kernel function: done once per kernel K (one static array per
// instantiation), device and size; sizes only grow.
template <auto K>
inline bool lds_opt_in(int dev, size_t bytes) {
    static std::atomic<size_t> done[kMaxDevices] = {};
    if (done[dev].load(std::memory_order_relaxed) >= bytes) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)) !=
        hipSuccess)
        return false;
    size_t cur = done[dev].load(std::memory_order_relaxed);
    while (cur < bytes && !done[dev].compare_exchange_weak(cur, bytes, std::memory_order_relaxed)) {}
    return true;
}

// Host-side launch dispatch: runtime bools become compile-time flags.  with_flags(f, b0, b1, ...) calls
// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...), so the generic lambda `f` is instantiated for exactly the
// combinations of the flags passed here, and returns what f returns.  with_int<V...>(v, f) does the same for one int among
// the listed values (std::integral_constant<int, V>; -2 when v is none of them).
template <typename F>
inline int with_flags(F&& f) {
    return f();
}
template <typename F, typename... B>
inline int with_flags(F&& f, bool b, B... bs) {
    if (b) return with_flags([&](auto... c) { return f(std::true_type{}, c...); }, bs...);
    return with_flags([&](auto... c) { return f(std::false_type{}, c...); }, bs...);
}
template <int... Vs, typename F>
inline int with_int(int v, F&& f) {
    int rc = -2;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}

// ---- the tail of every launcher: LDS bound, opt-in, launch, recorded name, outcome ---------------------------------
constexpr size_t kLdsPerCU = size_t(160) * 1024;   // LDS of a CU: what one workgroup can ask for at most
constexpr size_t kLdsOptIn = size_t(64) * 1024;    // dynamic LDS beyond this needs lds_opt_in
// What a launch needs beside the kernel and its arguments.  device_always: look the device up below kLdsOptIn as well
// (see launch_ad_dirs).  dev >= 0: the ordinal current_device() gave the caller, who needed device_cus() to choose the
// kernel (the ring paths) - it is not looked up again.
struct Launch {
    dim3 grid;
    size_t smem;
    hipStream_t stream;
    const char* name;             // what cloudsc2_last_kernel() reports
    bool device_always = false;
    int dev = -1;
};
// Refuse more than kLdsPerCU of LDS (-2); above kLdsOptIn look the device up (current_device: -1 / -2) and opt kernel K in
// (-1 when that fails: no launch, no name recorded); launch kColBlock threads per workgroup; record the name; 0, or -1 when
// the launch was refused.
template <auto K, typename... A>
inline int launch_tail(const Launch& l, const A&... args) {
    if (l.smem > kLdsPerCU) return -2;
    int dev = l.dev;
    if (dev < 0 && (l.device_always || l.smem > kLdsOptIn))
        if (const int rc = current_device(dev)) return rc;
    if (l.smem > kLdsOptIn && !lds_opt_in<K>(dev, l.smem)) return -1;
    hipLaunchKernelGGL(K, l.grid, dim3(kColBlock), l.smem, l.stream, args...);
    note_kernel(l.name);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// A pointer bundle B (CPtrs / MPtrs) from the caller's pointer array; a null array gives null entries.
template <typename B, typename P>
inline B pack_ptrs(const P* a) {
    B b;
    for (size_t i = 0; i < sizeof(b.p) / sizeof(b.p[0]); ++i) b.p[i] = a ? a[i] : nullptr;
    return b;
}

// Per-level LDS table: eta[k] and scalm[k] = ZSCAL * max(eta[k]-0.2, ZEPS1)^0.2
// (nonlinear/_stencils/cloudsc2.py:127).  `pow` is evaluated once per level per workgroup instead
// of once per level per column.  Also returns the tropopause search window [klo, khi]: the levels
// k in [0, nz-2] with 0.1 < eta[k] < 0.4 (cloudsc2.py:109-110); klo > khi when the window is empty.
template <typename T>
__device__ __forceinline__ void build_level_table(const T* __restrict__ eta, int nz, const Ext<T>& e,
                                                  T* s_eta, T* s_scalm, int& klo, int& khi) {
    for (int k = threadIdx.x; k <= nz; k += blockDim.x) {
        T ek = eta[k];
        s_eta[k] = ek;
        s_scalm[k] = e.ZSCAL * rpow<T>(rmax<T>(ek - T(0.2), e.ZEPS1), T(0.2));
    }
    __syncthreads();
    klo = nz;
    khi = -1;
    for (int k = 0; k < nz - 1; ++k) {
        T ek = s_eta[k];
        if (ek > T(0.1) && ek < T(0.4)) {
            if (k < klo) klo = k;
            khi = k;
        }
    }
}

// (line references in this block: nonlinear/_stencils/cloudsc2.py)
// Level-independent derived constants (one set per launch, computed on the host in double).
template <typename T>
struct NLK {
    T rdt, ckcodtl, ckcodti, cons2, rgdt, cons3, meltp2, rlcrit, ricrit, rRD, rRCPD, rRLMLT, cormax, fw2;
};

// The two switch combinations the kernels are instantiated for: the precipitation-evaporation block (and make_nlk's
// thresholds), and the linearised-physics forms.
inline bool evap_on(const Cloudsc2Params& p) { return p.LEVAPLS2 || p.LDRAIN1D; }
inline bool lin_on(const Cloudsc2Params& p) { return p.LPHYLIN || p.LDRAIN1D; }

template <typename T>
inline NLK<T> make_nlk(const Cloudsc2Params& p, double dt, bool evap) {
    NLK<T> k;
    k.rdt = T(1.0 / dt);
    k.ckcodtl = T(2.0 * p.RKCONV * dt);              // :120
    k.ckcodti = T(5.0 * p.RKCONV * dt);              // :121
    k.cons2 = T(1.0 / (p.RG * dt));                  // :122
    k.rgdt = T(p.RG * dt);
    k.cons3 = T(p.RLVTT / p.RCPD);                   // :123
    k.meltp2 = T(p.RTT + 2.0);                       // :124
    k.rlcrit = T(1.0 / ((evap ? 1.9 : 2.0) * p.RCLCRIT));     // :250-253
    k.ricrit = T(1.0 / (evap ? 0.0001 : 2.0 * p.RCLCRIT));    // :263-266
    k.rRD = T(1.0 / p.RD);
    k.rRCPD = T(1.0 / p.RCPD);
    k.rRLMLT = T(1.0 / p.RLMLT);
    k.cormax = T(1.0 / (1.0 - p.RETV * p.ZQMAX));    // 1 / (1 - RETV * esdp) when esdp is clipped at ZQMAX
    k.fw2 = T(2.0 * 0.17);                           // tanh(u) + 1 = 2 / (1 + exp(-2u)), u = 0.17 (t - RLPTRC)
    return k;
}

// Tropopause pre-scan (nonlinear/_stencils/cloudsc2.py:107-111, same statement in the TL and AD stencils): eta of the
// LAST level k of the window [klo, khi] (the levels with 0.1 < eta < 0.4) whose first-guess temperature exceeds that
// of level k+1.  The column's first-guess t of up to 43 levels is needed before the sweep reaches level klo, and
// with one wave per SIMD a load-compare-load loop exposes the full HBM latency once per level (22 us of a 337 us
// kernel, measured).  The loads of CH levels are therefore issued back to back and compared afterwards: 3 round
// trips instead of 42.  (klo, khi) come from build_level_table; khi <= nz - 2, so level khi + 1 exists.
// PERT: the state is read as x + pf * x_i (the fused perturbed_state variants), exactly as nl_perturb forms it.
template <typename T, bool PERT = false, typename O = uint32_t>
__device__ __forceinline__ T trpaus_prescan(const T* __restrict__ pt, const T* __restrict__ ptt, O lsb,
                                            O colb, T dt, const T* s_eta, int klo, int khi,
                                            const T* __restrict__ pt_i = nullptr, const T* __restrict__ ptt_i = nullptr,
                                            T pf = T(0.0)) {
    T trpaus = T(0.1);
    if (klo > khi) return trpaus;
    constexpr int CH = PERT ? 8 : 16;
    const O o0 = O(klo) * lsb + colb;
    T t0 = ldg(pt, o0), tt0 = ldg(ptt, o0);
    if constexpr (PERT) {
        t0 = t0 + pf * ldg(pt_i, o0);
        tt0 = tt0 + pf * ldg(ptt_i, o0);
    }
    T tk = t0 + dt * tt0;
    for (int k0 = klo; k0 <= khi; k0 += CH) {
        T a[CH], b[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int kk = (k0 + j < khi ? k0 + j : khi) + 1;   // the tail re-reads level khi + 1 (cache hits)
            const O oj = O(kk) * lsb + colb;
            a[j] = ldg(pt, oj);
            b[j] = ldg(ptt, oj);
            if constexpr (PERT) {
                a[j] = a[j] + pf * ldg(pt_i, oj);
                b[j] = b[j] + pf * ldg(ptt_i, oj);
            }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int k = k0 + j;
            if (k <= khi) {
                const T tk1 = a[j] + dt * b[j];
                const T ek = s_eta[k];
                if (ek > T(0.1) && ek < T(0.4) && tk > tk1) trpaus = ek;
                tk = tk1;
            }
        }
    }
    return trpaus;
}

// Critical relative humidity profile (nonlinear/_stencils/cloudsc2.py:166-186); rh2/deta1 depend on
// the column's tropopause eta only and are hoisted out of the level loop by the callers.
template <typename T>
struct CrhCol { T trpaus, rh2, bound1, deta1, bound2; };

template <typename T>
__device__ __forceinline__ CrhCol<T> crh_setup(T trpaus) {
    CrhCol<T> c;
    c.trpaus = trpaus;
    c.rh2 = T(0.35) + T(0.14) * sq((trpaus - T(0.25)) / T(0.15)) +
            T(0.04) * rmin<T>(trpaus - T(0.25), T(0.0)) / T(0.15);
    c.bound1 = trpaus + T(0.3);
    c.deta1 = T(0.09) + T(0.16) * (T(0.4) - trpaus) / T(0.3);
    c.bound2 = T(1.0) - c.deta1;
    return c;
}

template <typename T>
__device__ __forceinline__ T crh2_at(const CrhCol<T>& c, T eta) {
    const T rh1 = T(1.0), rh3 = T(1.0);
    if (eta < c.trpaus) return rh3;
    if (eta < c.bound1) return rh3 + (c.rh2 - rh3) * (eta - c.trpaus) / T(0.3);
    if (eta < c.bound2) return c.rh2;
    return rh1 + (c.rh2 - rh1) * rsqrt_<T>((T(1.0) - eta) / c.deta1);
}

}  // namespace cs2
