#!/usr/bin/env python3
"""Fitted coefficients c3 .. c12 for `cs2::fexp<double>` (csrc/cloudsc2_common.hpp, `make_expk`).

fexp evaluates exp(r) on |r| <= ln2/2 as 1 + r + r^2/2 + r^3 g(r) in Horner form, g of degree 9.  With the Taylor
coefficients 1/3! .. 1/12! the first dropped term r^13/13! is 2.4e-16 of exp(r) at the interval ends - a whole ulp of its
own, and fexp measures 2.32 ulp (ocml's exp: 0.87).  The same degree fitted to

    g(r) = (exp(r) - 1 - r - r^2/2) / r^3        on [-ln2/2, ln2/2]

in the Chebyshev sense spreads that error over the interval (1e-18 relative), which leaves the roundings of the Horner
steps as the only error: 0.86 ulp measured on the device with the literals printed here, which the header holds
(docs/TUNING_LOG.md 3.14).  The interval is widened by 2^-40: the Cody-Waite reduction lands a
few ulp beyond ln2/2 at its ties.

    python profiles/fit_exp_poly.py            prints the ten literals (17 significant digits, in the form `make_expk`
                                               takes them) and the worst relative error of the double-rounded polynomial
Needs mpmath; no GPU."""
import mpmath as mp

mp.mp.dps = 60
A = mp.log(2) / 2 * (1 + mp.mpf(2) ** -40)
DEG = 9          # g has the ten coefficients c3 .. c12


def g(r):
    if abs(r) < mp.mpf(10) ** -12:       # the series, where the closed form cancels
        return mp.mpf(1) / 6 + r / 24 + r * r / 120
    return (mp.exp(r) - 1 - r - r * r / 2) / r ** 3


def fit():
    """coefficients of g, lowest power first, rounded to double"""
    poly = mp.chebyfit(g, [-A, A], DEG + 1)            # highest power first
    return [float(c) for c in reversed(poly)]


def worst_relative_error(c, n=4001):
    """max over the interval of |1 + r + r^2/2 + r^3 sum c_k r^k - exp r| / exp r, coefficients as doubles, exact
    arithmetic: the approximation error alone"""
    worst = mp.mpf(0)
    for i in range(n):
        r = -A + 2 * A * i / (n - 1)
        p = mp.mpf(0)
        for ck in reversed(c):
            p = p * r + mp.mpf(ck)
        worst = max(worst, abs((1 + r + r * r / 2 + r ** 3 * p) / mp.exp(r) - 1))
    return worst


if __name__ == "__main__":
    c = fit()
    for k, ck in enumerate(c):
        print(f"k.c{k + 3} = T({ck:.17e});")
    print("// approximation error of the fit: %s relative;  Taylor 1/3! .. 1/12!: %s"
          % (mp.nstr(worst_relative_error(c), 3),
             mp.nstr(worst_relative_error([float(1 / mp.factorial(k)) for k in range(3, 13)]), 3)))
