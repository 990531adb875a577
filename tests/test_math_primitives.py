"""The arithmetic primitives of csrc/cloudsc2_common.hpp against correctly rounded references.

The parity tests hold whole stencils to `TOL` (helpers.py): 1e-9 relative in fp64, millions of ulp, because cancellations
amplify rounding.  Under that sit `frcp`, `fexp`, the saturation formulas, the logistic forms of the mixed-phase weight,
`rmin` / `rmax` and `rounded_product`, which every kernel calls dozens of times per grid point; the bit-equality tests
between kernel paths share them on both sides.  Here each is run alone (tests/primitives_probe.hip: one thread per
element, built into pytest's temporary directory, never part of libcloudsc2_hip.so) and measured in ulps of the
correctly rounded result:

  * frcp: exact rational arithmetic (`fractions.Fraction`) on the structured list and on the worst points of the bulk run,
    `np.longdouble` (64-bit significand, asserted) to rank the bulk.  Bound, derived: 1 ulp for normal x with normal 1/x -
    the last Newton step rounds r (2 - x r) = 1/x (1 - d^2) once, and d <= 2^-27 (2^-12 in fp32) before it puts that
    value within 2^-54 (2^-24) of 1/x.
  * fexp, saturation_point, logistic forms: mpmath at 50 digits on the structured lists and the worst 1 000 bulk points,
    longdouble to rank the bulk (longdouble alone, and said so in the output, where mpmath does not import).  Their bounds
    cannot be derived and are measured on the REFERENCE side, on the same inputs, never on the code under test:
      fexp<double>        worst error of ocml's exp (the function it replaced) + 0.5 ulp, the one more rounding of a
                          Horner form that ends in fma(p, r, 1.0) with p in [0.7, 1);  fexp<float> IS expf: bit-equal
      saturation_point    2 x worst error of the NumPy oracle's `saturation` in the same precision + 1 ulp: the same
                          formula, with divisions and exponentials of <= 1 ulp where NumPy's are <= 0.5 ulp
      logistic forms      worst error of the reference's own spelling, 0.545 (tanh u + 1) and 1 / cosh(u)^2 in NumPy in the
                          same precision, + 2 ulp for the one frcp and the one fexp
  * specials are exact: see test_fexp_specials and test_frcp_outside_the_normal_range.

Every test prints its figures before it asserts (`pytest -s`); the table in docs/TUNING_LOG.md 3.14 is a copy of them."""
import ctypes
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from helpers import externals, nl_case, oracle, run_oracle_nl

try:
    import mpmath

    mpmath.mp.dps = 50
except ImportError:                      # the bulk reference (longdouble) then serves everywhere; nothing is skipped
    mpmath = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
PROBE_SRC = os.path.join(ROOT, "tests", "primitives_probe.hip")
LAUNCHERS = tuple(f"probe_{n}_{s}" for n in ("frcp", "fexp", "foealf", "saturation", "minmax", "rounded_product", "logistic")
                  for s in ("f64", "f32"))
LD = np.longdouble
SEED = 20250117
NWORST = 1000
#: the argument where a host restatement of the Taylor-coefficient fexp<double> measured 2.31 ulp
X_TAYLOR_WORST = -371.1802813682641
DTYPES = [pytest.param(np.float64, id="fp64"), pytest.param(np.float32, id="fp32")]


def compile_probe(out_dir) -> str:
    out = os.path.join(str(out_dir), "libprimitives_probe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared",
                    "-I" + os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    PROBE_SRC, "-o", out], check=True, timeout=600)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_probe_cross_compiles_and_exports_every_launcher(tmp_path):
    """No GPU needed: a change to cloudsc2_common.hpp that breaks the probe shows up in the CPU suite."""
    lib = compile_probe(tmp_path)
    nm = next(p for p in ("/opt/rocm/llvm/bin/llvm-nm", shutil.which("llvm-nm"), shutil.which("nm")) if p and os.path.exists(p))
    out = subprocess.run([nm, "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert set(LAUNCHERS) <= exported, sorted(set(LAUNCHERS) - exported)


# ---- running the probe ---------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, path, device):
        self.lib = ctypes.CDLL(path)
        self.device = device
        for n in LAUNCHERS:
            getattr(self.lib, n).restype = ctypes.c_int

    def run(self, name, dtype, ins, nout, head=()):
        """launcher `probe_<name>_<f64|f32>(*head, *ins, *outs, n)` on equally long 1-d host arrays; returns the outputs"""
        import torch

        dtype = np.dtype(dtype)
        ins = [np.ascontiguousarray(a, dtype=dtype) for a in ins]
        n = ins[0].size
        assert all(a.shape == (n,) for a in ins)
        dev = [torch.from_numpy(a).to(self.device) for a in ins]
        outs = [torch.full((n,), 12345.0, dtype=dev[0].dtype, device=self.device) for _ in range(nout)]
        torch.cuda.synchronize()
        fn = getattr(self.lib, f"probe_{name}_{'f64' if dtype == np.float64 else 'f32'}")
        rc = fn(*head, *[ctypes.c_void_p(t.data_ptr()) for t in dev + outs], ctypes.c_int64(n))
        assert rc == 0, (name, rc)
        return [t.cpu().numpy() for t in outs]


@pytest.fixture(scope="module")
def probe(gpu, tmp_path_factory):
    assert os.path.exists(HIPCC), "the primitives probe is compiled by the test: hipcc is required"
    return Probe(compile_probe(tmp_path_factory.mktemp("primitives_probe")), gpu)


def params_ref(ext):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import make_params

    return ctypes.byref(make_params(ext))


# ---- ulps ------------------------------------------------------------------------------------------------------------
def test_longdouble_is_wide_enough():
    assert np.finfo(LD).nmant >= 63, "np.longdouble is not the x87 extended format: the bulk reference would be fp64 itself"


def tname(dtype):
    return "fp64" if np.dtype(dtype) == np.float64 else "fp32"


def bulk_ulps(got, ref, dtype):
    """|got - ref| in ulps of ref rounded to `dtype` (np.spacing: the subnormal spacing for subnormal results); `ref` is
    longdouble and must round to a finite value everywhere - the rest belongs to the specials"""
    cr = ref.astype(dtype)
    assert np.isfinite(cr).all(), "an input of the bulk run has no finite reference"
    assert not np.isnan(got).any(), "NaN from finite input"
    with np.errstate(over="ignore", invalid="ignore"):
        err = np.abs(got.astype(LD) - ref) / np.spacing(np.abs(cr)).astype(LD)
    return err, cr


def round_to(dtype, value):
    """`value` (Fraction or mpf) correctly rounded to dtype: the nearest of the float conversion and its two neighbours"""
    with np.errstate(over="ignore"):
        c = dtype(float(value))
    if not np.isfinite(c):
        return c
    cands = [c, np.nextafter(c, dtype(-np.inf)), np.nextafter(c, dtype(np.inf))]
    cands = [x for x in cands if np.isfinite(x)]
    return min(cands, key=lambda x: abs(exact(x, value) - value))


def exact(x, like):
    return Fraction(float(x)) if isinstance(like, Fraction) else mpmath.mpf(float(x))


def exact_ulps(got, value, dtype):
    """error of the finite `got` against the exact / 50-digit `value`, in ulps of the correctly rounded result; also
    whether `got` is that result"""
    cr = round_to(dtype, value)
    assert np.isfinite(cr)
    ulp = exact(np.spacing(np.abs(cr)), value)
    return abs(exact(got, value) - value) / ulp, got == cr


def refine(err, points, got, dtype, value_of, extra=None):
    """the worst NWORST of the bulk errors (plus the indices `extra`), recomputed against value_of(point); returns
    (worst error as float, index of the worst).  Without mpmath value_of is None and the bulk figures stand."""
    idx = np.argsort(err)[-NWORST:]
    if extra is not None:
        idx = np.union1d(idx, extra)
    if value_of is None:
        i = int(np.argmax(err))
        return float(err[i]), i
    memo = value_of.__dict__.setdefault("memo", {})          # the same points serve the device and the yardstick
    best, at = -1.0, -1
    for i in idx:
        if i not in memo:
            memo[i] = value_of(points[i])
        e, _ = exact_ulps(got[i], memo[i], dtype)
        if e > best:
            best, at = e, int(i)
    return best, at


def report(prim, dtype, n, worst, at, against, ncr):
    print(f"\n[primitives] {prim:<24s} {tname(dtype)}  n={n:>8d}  worst {float(worst):7.3f} ulp at {at}  | held against: {against}"
          f"  | not correctly rounded: {100.0 * ncr:.4f} %")


# ---- frcp ------------------------------------------------------------------------------------------------------------
def kernel_divisors(dtype):
    """the divisors the level loops really form, from nl_case(1024): dp, zz, t - R4LES, t - R4IES, ap, 1 - RETV esdp, clc,
    lu1, t (zeros dropped: 1/0 is on the specials list)"""
    e = externals()
    f, eta, dt = nl_case(1024)
    nz = f["in_t"].shape[0] - 1
    t, ap, q = f["in_t"][:nz], f["in_ap"][:nz], f["in_q"][:nz]
    dp = f["in_aph"][1:] - f["in_aph"][:-1]
    zz = e["RCPD"] + e["RCPD"] * e["RVTMP2"] * q
    foeew = e["R2ES"] * np.exp(np.where(t < e["RTT"], e["R3IES"], e["R3LES"]) * (t - e["RTT"])
                               / (t - np.where(t < e["RTT"], e["R4IES"], e["R4LES"])))
    esdp = np.minimum(foeew / ap, e["ZQMAX"])
    clc = run_oracle_nl(f, eta, dt, e)["clc"][:nz]
    parts = [dp, zz, t - e["R4LES"], t - e["R4IES"], ap, 1.0 - e["RETV"] * esdp, clc, f["in_lu"][1:], t]
    x = np.concatenate([p.ravel() for p in parts]).astype(dtype)
    return x[np.isfinite(x) & (x != 0)]


def frcp_bulk(dtype):
    rng = np.random.default_rng(SEED)
    fi = np.finfo(dtype)
    n = 3_000_000
    # normal x with normal 1/x: 2^minexp <= |x| < 2^(maxexp - 2)
    x = np.ldexp(1.0 + rng.random(n), rng.integers(fi.minexp, fi.maxexp - 2, n)).astype(dtype)
    x *= rng.choice(np.array([-1, 1], dtype=dtype), n)
    dense = (1.0 + rng.random(1_000_000)).astype(dtype)
    x = np.concatenate([x, dense, kernel_divisors(dtype)])
    tiny = dtype(fi.tiny)
    ok = (np.abs(x) >= tiny) & (np.abs(x) <= dtype(1) / tiny)
    return x[ok]


def frcp_structured(dtype):
    fi = np.finfo(dtype)
    one, two = dtype(1), dtype(2)
    xs = [np.ldexp(dtype(1), k) for k in range(fi.minexp, fi.maxexp - 1)]            # powers of two, 1/x normal
    up, dn, dn2 = one, one, two
    for _ in range(8):
        up, dn, dn2 = np.nextafter(up, two), np.nextafter(dn, dtype(0)), np.nextafter(dn2, dtype(0))
        xs += [up, dn, dn2]
    xs += [dtype(fi.tiny), np.ldexp(dtype(1), fi.maxexp - 2), dtype(3), dtype(1) / dtype(3), dtype(10), dtype(0.1)]
    x = np.array(xs, dtype=dtype)
    return np.concatenate([x, -x])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_frcp_is_faithful(probe, dtype):
    """frcp<T>(x) for normal x with normal 1/x: at most 1 ulp (derivation in the module docstring), checked EXACTLY.  The
    longdouble ranking of the bulk run is itself good to 2^-11 ulp of fp64 only, so every bulk point it puts above
    1 - 2^-9 ulp is recomputed in rational arithmetic, with the worst 1 000 and the whole structured list."""
    assert np.finfo(LD).nmant >= 63
    xb, xs = frcp_bulk(dtype), frcp_structured(dtype)
    assert xb.size >= 4_000_000
    x = np.concatenate([xb, xs])
    got, div = probe.run("frcp", dtype, [x], 2)
    ref = LD(1) / x.astype(LD)
    err, cr = bulk_ulps(got, ref, dtype)
    err_div, _ = bulk_ulps(div, ref, dtype)
    near = np.flatnonzero(err > 1.0 - 2.0 ** -9)
    check = np.union1d(np.union1d(np.argsort(err)[-NWORST:], near[:100_000]), np.arange(xb.size, x.size))
    worst, at, beyond = Fraction(0), 0, 0
    for i in check:
        e, _ = exact_ulps(got[i], 1 / Fraction(float(x[i])), dtype)
        beyond += e > 1
        if e > worst:
            worst, at = e, i
    ncr = float(np.mean(got != dtype(1) / x))             # NumPy's division IS the correctly rounded quotient
    report("frcp", dtype, x.size, worst, f"x={x[at]!r}", f"1 ulp (derived); IEEE 1/x measures {float(err_div.max()):.3f}", ncr)
    assert err_div.max() <= 0.5 + 2.0 ** -9, "the compiler's division is not the correctly rounded one: the yardstick is off"
    assert near.size <= 100_000 and beyond == 0 and worst <= 1, (float(worst), x[at], near.size, beyond)


#: what frcp returns outside the range it is used in (measured on gfx950, header comment of frcp): the Newton step forms
#: inf * 0.  class of x -> "nan" | "zero" (of x's sign) | "faithful" (<= 1 ulp of the IEEE quotient, subnormal spacing)
FRCP_OUTSIDE = {
    "zero": "nan",               # rcp = inf, fma(-0, inf, 1) = NaN
    "inf": "nan",                # rcp = 0,   fma(-inf, 0, 1) = NaN
    "nan": "nan",
    "subnormal, 1/x overflows": "nan",        # rcp = inf, fma(-x, inf, 1) = -inf, fma(-inf, inf, inf) = NaN
    # v_rcp_f64 handles subnormals; v_rcp_f32 takes a subnormal argument for 0 and flushes a subnormal result to 0
    "subnormal, 1/x finite": {np.float64: "faithful", np.float32: "nan"},
    "huge, 1/x subnormal": {np.float64: "faithful", np.float32: "zero"},
}


def frcp_outside_cases(dtype):
    fi = np.finfo(dtype)
    sub, big = dtype(fi.smallest_subnormal), dtype(fi.max)
    quarter = np.ldexp(dtype(1), fi.minexp - 2)           # the largest power of two whose reciprocal overflows
    c = {
        "zero": [dtype(0.0), dtype(-0.0)],
        "inf": [dtype(np.inf), dtype(-np.inf)],
        "nan": [dtype(np.nan)],
        "subnormal, 1/x overflows": [sub, -sub, sub * dtype(1000), quarter, -quarter, np.nextafter(quarter, dtype(0))],
        "subnormal, 1/x finite": [np.nextafter(dtype(fi.tiny), dtype(0)), -np.nextafter(dtype(fi.tiny), dtype(0)),
                                  np.ldexp(dtype(1.5), fi.minexp - 1), np.ldexp(dtype(1), fi.minexp - 1),
                                  np.ldexp(dtype(1.25), fi.minexp - 2)],
        "huge, 1/x subnormal": [big, -big, np.ldexp(dtype(1.5), fi.maxexp - 2), np.ldexp(dtype(1), fi.maxexp - 1),
                                np.ldexp(dtype(1.75), fi.maxexp - 1), np.nextafter(np.ldexp(dtype(1), fi.maxexp - 2), big)],
    }
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_frcp_outside_the_normal_range(probe, dtype):
    """+-0, +-inf, subnormal x and |x| > 2^(emax-1): IEEE division gives +-inf, +-0, a finite value or inf, and a subnormal.
    frcp does not where its Newton step meets inf * 0 (`FRCP_OUTSIDE`, the table in the header); pinned here so that
    a change of that behaviour is seen, and the compiler's 1/x beside it is held to IEEE."""
    cases = frcp_outside_cases(dtype)
    x = np.array([v for vs in cases.values() for v in vs], dtype=dtype)
    cls = [k for k, vs in cases.items() for _ in vs]
    got, div = probe.run("frcp", dtype, [x], 2)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        ieee = dtype(1) / x
    for xi, k, g, d, w in zip(x, cls, got, div, ieee):
        print(f"[primitives] frcp {tname(dtype)} outside: {k:<26s} x={xi!r:<28} frcp={g!r:<28} 1/x={d!r}")
    bad = []
    for xi, k, g, d, w in zip(x, cls, got, div, ieee):
        if not (d == w or (np.isnan(d) and np.isnan(w))) or (d == 0 and np.signbit(d) != np.signbit(w)):
            bad.append(("1/x", xi, d, w))
        pin = FRCP_OUTSIDE[k] if isinstance(FRCP_OUTSIDE[k], str) else FRCP_OUTSIDE[k][dtype]
        if pin == "nan":
            if not np.isnan(g):
                bad.append((k, xi, g, "NaN"))
        elif pin == "zero":
            if not (g == 0 and np.signbit(g) == np.signbit(xi)):
                bad.append((k, xi, g, "0 of x's sign"))
        else:
            e, _ = exact_ulps(g, 1 / Fraction(float(xi)), dtype) if np.isfinite(g) else (np.inf, False)
            if not e <= 1:
                bad.append((k, xi, g, f"{float(e)} ulp"))
    assert not bad, bad


# ---- fexp ------------------------------------------------------------------------------------------------------------
def fexp_bulk(dtype):
    rng = np.random.default_rng(SEED + 1)
    e = externals()
    n = 1_400_000
    lo, hi = (-708.0, 709.0) if dtype == np.float64 else (-87.0, 88.0)     # the range of normal results
    t = rng.uniform(150.0, 340.0, 500_000).astype(dtype)
    cld = 10.0 ** rng.uniform(-9.0, -1.0, 500_000)
    crit = np.where(rng.random(500_000) < 0.5, 2.0 * e["RCLCRIT"], 1.0e-4)
    parts = [rng.uniform(lo, hi, n), rng.uniform(-40.0, 40.0, n), rng.uniform(-1.0, 1.0, n),
             dtype(e["R3LES"]) * (t - dtype(e["RTT"])) / (t - dtype(e["R4LES"])),          # the Tetens arguments
             dtype(e["R3IES"]) * (t - dtype(e["RTT"])) / (t - dtype(e["R4IES"])),
             -((cld / crit) ** 2), np.full(16, -1.0e20)]                                  # autoconversion
    return np.concatenate([np.asarray(p, dtype=dtype) for p in parts])


def ulp_steps(x, ks):
    """x moved by k ulp for every k in ks (float64)"""
    out = []
    for k in ks:
        y = np.array(x, dtype=np.float64)
        for _ in range(abs(k)):
            y = np.nextafter(y, np.inf if k > 0 else -np.inf)
        out.append(y)
    return np.concatenate([np.atleast_1d(o) for o in out])


#: the largest double whose correctly rounded exp is finite (exp overflows above 709.782712893384)
X_OVERFLOW = float.fromhex("0x1.62e42fefa39efp+9")


def fexp_structured():
    """fp64: n ln2 +- k ulp for n in [-1075, 1024] (reduction ties, r at the interval ends), (n + 1/2) ln2 likewise, the
    clamp ends, the overflow threshold, the range of subnormal results, the finding that started this file"""
    ks = range(-8, 9)
    n = np.arange(-1075, 1025, dtype=np.float64)
    ln2 = float(np.log(LD(2)))
    xs = [ulp_steps(n * ln2, ks), ulp_steps((n + 0.5) * ln2, ks), ulp_steps(np.array([-746.0, 710.0, X_OVERFLOW, -708.0, -745.2,
          -745.1332191019412, -744.4400719213812, 0.0]), ks), np.linspace(-745.2, -708.0, 20_000),
          np.array([X_TAYLOR_WORST, -0.0, 1.0, -1.0, 0.5 * ln2, -0.5 * ln2, 1e-300, -1e-300, 5e-324, -800.0, -1e20, -1e300])]
    return np.concatenate(xs)


def exp_overflows(x):
    """correctly rounded exp(x) is inf (exact for the doubles next to the threshold, which exp cannot hit)"""
    return x > X_OVERFLOW


@pytest.mark.gpu
def test_fexp_f64_is_no_worse_than_the_exp_it_replaced(probe):
    """fexp<double> against mpmath (50 digits) on the structured list and the worst 1 000 of >= 4 M bulk arguments, bound:
    what ocml's exp measures on the same arguments against the same reference, + 0.5 ulp.

    Measured on gfx950: ocml 0.868 ulp, so the bound is 1.368 ulp; fexp 0.857 ulp.  With the Taylor coefficients
    1/3! .. 1/12! (before profiles/fit_exp_poly.py) fexp measured 2.324 ulp and this test failed; at
    x = -371.1802813682641, where a host restatement had predicted 2.31 ulp, the device gave 2.313 ulp (on the structured
    list by name)."""
    dtype = np.float64
    xb, xs = fexp_bulk(dtype), fexp_structured()
    assert xb.size >= 4_000_000
    x = np.concatenate([xb, xs])
    got, ocml = probe.run("fexp", dtype, [x], 2)
    over = exp_overflows(x)
    assert np.all(got[over] == np.inf), x[over][got[over] != np.inf]            # exactly where exp overflows ...
    assert np.all(np.isfinite(got[~over])), x[~over][~np.isfinite(got[~over])]  # ... and nowhere else
    x, got, ocml = x[~over], got[~over], ocml[~over]
    ref = np.exp(x.astype(LD))
    err, cr = bulk_ulps(got, ref, dtype)
    err_o, _ = bulk_ulps(ocml, ref, dtype)
    if mpmath is None:
        print("[primitives] mpmath does not import here: fexp is measured against np.longdouble alone")
    value_of = (lambda v: mpmath.exp(mpmath.mpf(float(v)))) if mpmath else None
    structured = np.arange(x.size - int((~over[xb.size:]).sum()), x.size)
    worst, at = refine(err, x, got, dtype, value_of, structured)
    worst_o, at_o = refine(err_o, x, ocml, dtype, value_of, structured)
    i371 = int(np.flatnonzero(x == X_TAYLOR_WORST)[0])
    report("fexp", dtype, x.size, worst, f"x={x[at]!r}", f"ocml exp {float(worst_o):.3f} ulp (at x={x[at_o]!r}) + 0.5",
           float(np.mean(got != cr)))
    print(f"[primitives] fexp fp64 at x={X_TAYLOR_WORST!r}: {float(err[i371]):.3f} ulp (ocml {float(err_o[i371]):.3f});"
          f" ocml not correctly rounded: {100.0 * float(np.mean(ocml != cr)):.4f} %")
    assert worst <= worst_o + 0.5, (float(worst), x[at], float(worst_o))


@pytest.mark.gpu
def test_fexp_f32_is_expf(probe):
    """fexp<float> is ocml's expf: bit-equal to rexp<float> on every argument, those with results of 0 and inf included;
    its error against the reference is printed for the table."""
    dtype = np.float32
    with np.errstate(over="ignore"):                       # -1e300 of the fp64 list is -inf here
        x = np.concatenate([fexp_bulk(dtype), fexp_structured().astype(dtype),
                            np.array([np.inf, -np.inf, np.nan, 88.72284, 88.7229, -103.97, -104.0], dtype=dtype)])
    assert x.size >= 4_000_000
    got, ocml = probe.run("fexp", dtype, [x], 2)
    fin = np.isfinite(x) & (x > -103.0) & (x < 88.7)
    err, cr = bulk_ulps(got[fin], np.exp(x[fin].astype(LD)), dtype)
    i = int(np.argmax(err))
    report("fexp (= expf)", dtype, int(fin.sum()), err[i], f"x={x[fin][i]!r}", "bit-equal to ocml expf", float(np.mean(got[fin] != cr)))
    assert np.array_equal(got.view(np.uint32), ocml.view(np.uint32))


@pytest.mark.gpu
def test_fexp_specials(probe):
    """Exact: fexp(NaN) is NaN whatever the payload or sign, fexp(-inf) = fexp(-1e20) = 0, fexp(+inf) = inf,
    fexp(+-0) = 1, and around the clamp ends [-746, 710] the result is 0 / inf as exp rounds there."""
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FF4000000000000, 0x7FFFFFFFFFFFFFFF,
                     0xFFF0000000000001, 0x7FF80000DEADBEEF], dtype=np.uint64).view(np.float64)
    x = np.concatenate([nans, [-np.inf, -1e20, -1e300, -800.0, -746.0, np.nextafter(-746.0, -np.inf), -745.14],
                        [np.inf, 1e300, 800.0, 710.0, np.nextafter(710.0, np.inf), np.nextafter(710.0, 0.0),
                         np.nextafter(X_OVERFLOW, np.inf)], [0.0, -0.0], [X_OVERFLOW]])
    got, ocml = probe.run("fexp", np.float64, [x], 2)
    for xi, g, o in zip(x, got, ocml):
        print(f"[primitives] fexp fp64 special x={xi!r:<24} fexp={g!r:<24} ocml={o!r}")
    assert np.isnan(got[:7]).all()
    assert np.array_equal(got[7:14], np.zeros(7)) and not np.signbit(got[7:14]).any()
    assert np.all(got[14:21] == np.inf)
    assert np.array_equal(got[21:23], np.ones(2))
    assert np.isfinite(got[23]) and got[23] > 1.79e308        # the largest argument whose exp is finite


# ---- foealfa / foealfcu / saturation_point ----------------------------------------------------------------------------------
def typed(ext, dtype):
    """the externals as make_ext<T> holds them: rounded to the working precision"""
    return {k: (dtype(v) if isinstance(v, float) else v) for k, v in ext.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_foealfa_and_foealfcu_equal_the_oracle(probe, dtype):
    """min, max, one subtraction, one product, one square with contraction off: single IEEE operations on both sides, so the
    device must EQUAL the oracle's f_foealfa / f_foealfcu in the same precision - at RTICE, RTICECU, RTWAT, RTT and their
    two neighbours each (RTICECU moved off RTICE so that the two ramps differ), and on 4 M temperatures."""
    ext = externals()
    ext["RTICECU"] = ext["RTT"] - 38.0
    ext["RTWAT_RTICECU_R"] = 1.0 / (ext["RTWAT"] - ext["RTICECU"])
    e = typed(ext, dtype)
    rng = np.random.default_rng(SEED + 2)
    edges = np.array([e[k] for k in ("RTICE", "RTICECU", "RTWAT", "RTT")], dtype=dtype)
    t = np.concatenate([edges, np.nextafter(edges, dtype(0)), np.nextafter(edges, dtype(1e4)),
                        rng.uniform(150.0, 340.0, 4_000_000).astype(dtype),
                        rng.uniform(float(e["RTICECU"]) - 1.0, float(e["RTWAT"]) + 1.0, 200_000).astype(dtype)])
    alfa, alfcu = probe.run("foealf", dtype, [t], 2, head=(params_ref(ext),))
    want_a, want_c = oracle.f_foealfa(t, e), oracle.f_foealfcu(t, e)
    assert want_a.dtype == dtype and want_c.dtype == dtype
    for k in range(12):
        print(f"[primitives] foealfa {tname(dtype)} t={t[k]!r:<22} alfa={alfa[k]!r:<24} alfcu={alfcu[k]!r}")
    report("foealfa / foealfcu", dtype, t.size, 0.0 if np.array_equal(alfa, want_a) and np.array_equal(alfcu, want_c) else np.inf,
           "-", "equal to the oracle", float(np.mean((alfa != want_a) | (alfcu != want_c))))
    assert np.array_equal(alfa, want_a), t[alfa != want_a][:5]
    assert np.array_equal(alfcu, want_c), t[alfcu != want_c][:5]
    assert alfa[0] == 0 and alfcu[1] == 0 and 0 < alfa.min() + 1 and alfa.max() <= 1 and (alfa != alfcu).any()


def saturation_ref(t, ap, e, mode, xp):
    """saturation.py:23-42 + fcttre.py on scalars (xp = mpmath) or longdouble arrays (xp = numpy); `e` typed externals
    converted exactly.  All three modes are the same function of foealfa / foealfcu mathematically."""
    mn = np.minimum if xp is np else min
    mx = np.maximum if xp is np else max
    ice, r = (e["RTICECU"], e["RTWAT_RTICECU_R"]) if mode == 1 else (e["RTICE"], e["RTWAT_RTICE_R"])
    alfa = mn(1, ((mx(ice, mn(e["RTWAT"], t)) - ice) * r) ** 2)
    foeewl = xp.exp(e["R3LES"] * (t - e["RTT"]) / (t - e["R4LES"]))
    foeewi = xp.exp(e["R3IES"] * (t - e["RTT"]) / (t - e["R4IES"]))
    qs = mn(e["R2ES"] * (alfa * foeewl + (1 - alfa) * foeewi) / ap, e["QMAX"])
    return qs / (1 - e["RETV"] * qs)


MODE_EXT = {0: dict(LPHYLIN=True), 1: dict(LPHYLIN=False, KFLAG=1), 2: dict(LPHYLIN=False, KFLAG=0)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_saturation_point(probe, dtype):
    """saturation_point<T, MODE> for the three modes on t in [150, 340] K x ap in [1, 1.1e5] Pa and on (ap, t) of
    nl_case(1024), against the formula at 50 digits.  Bound: 2 x what the NumPy oracle's `saturation` measures in the same
    precision on the same points, + 1 ulp (module docstring)."""
    rng = np.random.default_rng(SEED + 3)
    f, _, _ = nl_case(1024)
    nz = f["in_t"].shape[0] - 1
    n = 1_300_000
    t = np.concatenate([rng.uniform(150.0, 340.0, n), f["in_t"][:nz].ravel()]).astype(dtype)
    ap = np.concatenate([rng.uniform(1.0, 1.1e5, n // 2), np.exp(rng.uniform(0.0, np.log(1.1e5), n - n // 2)),
                         f["in_ap"][:nz].ravel()]).astype(dtype)
    assert 3 * t.size >= 4_000_000
    for mode in (0, 1, 2):
        ext = externals(**MODE_EXT[mode])
        ext["RTICECU"] = ext["RTT"] - 38.0            # apart from RTICE, so that mode 1 differs from mode 2
        ext["RTWAT_RTICECU_R"] = 1.0 / (ext["RTWAT"] - ext["RTICECU"])
        e = typed(ext, dtype)
        (got,) = probe.run("saturation", dtype, [t, ap], 1, head=(params_ref(ext), ctypes.c_int(mode)))
        ora = np.zeros((2, t.size), dtype=dtype)
        oracle.saturation(np.stack([ap, ap]), np.stack([t, t]), ora, e)
        ora = ora[0]
        assert ora.dtype == dtype
        eld = {k: (LD(v) if isinstance(v, np.floating) else v) for k, v in e.items()}
        ref = saturation_ref(t.astype(LD), ap.astype(LD), eld, mode, np)
        err, cr = bulk_ulps(got, ref, dtype)
        err_o, _ = bulk_ulps(ora, ref, dtype)
        value_of = None
        if mpmath:
            emp = {k: (mpmath.mpf(float(v)) if isinstance(v, np.floating) else v) for k, v in e.items()}
            value_of = lambda p: saturation_ref(mpmath.mpf(float(p[0])), mpmath.mpf(float(p[1])), emp, mode, mpmath)  # noqa: E731
        else:
            print("[primitives] mpmath does not import here: saturation_point is measured against np.longdouble alone")
        pts = np.stack([t, ap], axis=1)
        worst, at = refine(err, pts, got, dtype, value_of)
        worst_o, at_o = refine(err_o, pts, ora, dtype, value_of)
        report(f"saturation_point<{mode}>", dtype, t.size, worst, f"t={t[at]!r} ap={ap[at]!r}",
               f"2 x oracle {float(worst_o):.3f} ulp (t={t[at_o]!r} ap={ap[at_o]!r}) + 1", float(np.mean(got != cr)))
        assert worst <= 2 * worst_o + 1, (mode, float(worst), float(worst_o), t[at], ap[at])


# ---- the logistic forms -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_logistic_forms(probe, dtype):
    """logistic_fwat = 1.09 rr and logistic_sech2 = 4 ex rr^2 (ex = exp(-2u), rr = 1 / (1 + ex)) as cloudsc2_nl / _tl / _ad
    call them, against 0.545 (tanh u + 1) and 1 / cosh(u)^2 at 50 digits.  u = 0.17 (t - RLPTRC) is formed in the working
    precision from t in [150, 340] K and t of nl_case(1024); the device forms -0.34 (t - RLPTRC), which is -2u bit for bit
    (a scaling by two), so both sides work on the same u.  Bound: what the reference's own NumPy spelling measures in the same
    precision on the same u, + 2 ulp.

    That bound is wide where it matters: for cold t NumPy's tanh(u) + 1 cancels to nothing (fwat = 0 at u = -19 in fp64,
    2^52 ulp off), which is the very reason for the rewrite.  A second bound is therefore derived from the operations.  With
    eps the unit roundoff, k ulp are at most 2 k eps relative and eps relative is at most 1 ulp.  ex carries <= 2 E eps
    (fexp within E ulp; E <= 2 is what test_fexp_* hold it to), 1 + ex one rounding and ex's error scaled by
    ex / (1 + ex) < 1: (1 + 2 E) eps, frcp 2 eps more, the product with 1.09 one eps: fwat is within (4 + 2 E) eps = 8 ulp.
    sech2 = 4 ex rr rr: 2 E + 2 (3 + 2 E) for the factors, 3 roundings of the products: (9 + 6 E) eps = 21 ulp."""
    rng = np.random.default_rng(SEED + 4)
    ext = externals()
    e = typed(ext, dtype)
    f, _, _ = nl_case(1024)
    edges = np.array([e["RLPTRC"], e["RTT"], e["RTICE"]], dtype=dtype)
    t = np.concatenate([rng.uniform(150.0, 340.0, 4_000_000), f["in_t"][:-1].ravel(), edges, np.nextafter(edges, dtype(0)),
                        np.nextafter(edges, dtype(1e4)), [150.0, 340.0]]).astype(dtype)
    u = dtype(0.17) * (t - e["RLPTRC"])
    assert u.dtype == dtype and np.array_equal(-dtype(2.0 * 0.17) * (t - e["RLPTRC"]), dtype(-2) * u)
    fwat, fwat_nl, sech2 = probe.run("logistic", dtype, [t], 3, head=(params_ref(ext),))
    assert np.array_equal(fwat, fwat_nl)                    # the NL overload is the TL / AD one
    np_fwat = dtype(0.545) * (np.tanh(u) + dtype(1))
    np_sech2 = dtype(1) / np.cosh(u) ** 2
    assert np_fwat.dtype == dtype and np_sech2.dtype == dtype
    uld = u.astype(LD)
    ex = np.exp(-2 * uld)
    ref_fwat = 2 * LD(dtype(0.545)) / (1 + ex)              # = 0.545 (tanh u + 1) without the cancellation
    ref_sech2 = 4 * ex / (1 + ex) ** 2
    v_fwat = v_sech2 = None
    if mpmath:
        c = mpmath.mpf(float(dtype(0.545)))
        v_fwat = lambda v: c * (mpmath.tanh(mpmath.mpf(float(v))) + 1)          # noqa: E731
        v_sech2 = lambda v: 1 / mpmath.cosh(mpmath.mpf(float(v))) ** 2         # noqa: E731
    else:
        print("[primitives] mpmath does not import here: the logistic forms are measured against np.longdouble alone")
    for name, got, ora, ref, vf, derived in (("logistic_fwat", fwat, np_fwat, ref_fwat, v_fwat, 8),
                                             ("logistic_sech2", sech2, np_sech2, ref_sech2, v_sech2, 21)):
        err, cr = bulk_ulps(got, ref, dtype)
        err_o, _ = bulk_ulps(ora, ref, dtype)
        structured = np.arange(t.size - 11, t.size)
        worst, at = refine(err, u, got, dtype, vf, structured)
        worst_o, at_o = refine(err_o, u, ora, dtype, vf, structured)
        report(name, dtype, t.size, worst, f"t={t[at]!r} (u={u[at]!r})", f"NumPy spelling {float(worst_o):.3f} ulp (u={u[at_o]!r}) + 2",
               float(np.mean(got != cr)))
        assert worst <= worst_o + 2, (name, float(worst), float(worst_o), t[at])
        assert worst <= derived, (name, float(worst), derived, t[at])


# ---- rmin / rmax / rounded_product --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rmin_rmax_are_the_ternaries(probe, dtype):
    """rmin(a, b) = a < b ? a : b, rmax(a, b) = a > b ? a : b.  On finite operands and signed zeros they equal the oracle's
    np.minimum / np.maximum in value.  With a NaN in EITHER slot the comparison is false and the ternary returns b: the NaN
    when it sits in b, the other operand when it sits in a - where np.minimum / np.maximum (oracle/cloudsc2_numpy.py)
    propagate the NaN from both slots, and fmin / fmax would swallow it from both.  Pinned bit for bit."""
    rng = np.random.default_rng(SEED + 5)
    nan, inf = dtype(np.nan), dtype(np.inf)
    pairs = [(0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0), (1.5, 1.5), (-2.0, -2.0), (1.0, 2.0), (2.0, 1.0), (-1.0, 1.0),
             (inf, 1.0), (1.0, inf), (-inf, 1.0), (1.0, -inf), (inf, inf), (-inf, inf),
             (nan, 1.0), (1.0, nan), (nan, nan), (nan, -0.0), (-0.0, nan), (nan, inf), (-inf, nan)]
    a = np.concatenate([np.array([p[0] for p in pairs], dtype=dtype), rng.normal(size=100_000).astype(dtype)])
    b = np.concatenate([np.array([p[1] for p in pairs], dtype=dtype), rng.normal(size=100_000).astype(dtype)])
    b[-1000:] = a[-1000:]
    lo, hi = probe.run("minmax", dtype, [a, b], 2)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    with np.errstate(invalid="ignore"):
        want_lo, want_hi = np.where(a < b, a, b), np.where(a > b, a, b)
    for k in range(len(pairs)):
        print(f"[primitives] rmin/rmax {tname(dtype)} a={a[k]!r:<8} b={b[k]!r:<8} rmin={lo[k]!r:<8} rmax={hi[k]!r}")
    assert np.array_equal(lo.view(bits), want_lo.view(bits)) and np.array_equal(hi.view(bits), want_hi.view(bits))
    ok = ~(np.isnan(a) | np.isnan(b))
    assert np.all(lo[ok] == np.minimum(a, b)[ok]) and np.all(hi[ok] == np.maximum(a, b)[ok])
    an, bn = np.isnan(a) & ~np.isnan(b), np.isnan(b)
    assert an.sum() == 3 and bn.sum() == 4 and not np.isnan(lo[an]).any() and not np.isnan(hi[an]).any()     # NaN in a: dropped (NumPy: NaN)
    assert np.isnan(lo[bn]).all() and np.isnan(hi[bn]).all()                               # NaN in b: kept (fmin: dropped)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rounded_product_is_rounded_before_use(probe, dtype):
    """rounded_product(f, x) - y with y = fl(f x) is exactly 0 when the product is rounded as a product; were it contracted
    into the subtraction it would be the rounding residual fma(f, x, -y), which the probe spells out beside it and which is
    nonzero for most operands."""
    rng = np.random.default_rng(SEED + 6)
    f = np.concatenate([np.full(500_000, 0.01), rng.uniform(0.5, 2.0, 500_000)]).astype(dtype)
    x = (rng.normal(size=1_000_000) * 10.0 ** rng.uniform(-8, 5, 1_000_000)).astype(dtype)
    y = f * x
    assert y.dtype == dtype
    out, fused = probe.run("rounded_product", dtype, [f, x, y], 2)
    share = float(np.mean(fused != 0))
    report("rounded_product", dtype, x.size, 0.0 if not out.any() else np.inf, "-", f"exact; an fma would leave a residual on {100 * share:.1f} %", 0.0)
    assert share > 0.5
    assert not out.any(), (f[out != 0][:3], x[out != 0][:3])
