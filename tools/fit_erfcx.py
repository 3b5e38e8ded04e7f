#!/usr/bin/env python
"""Fit the float32 erfcx(x), x >= 0, of ProbitLink (csrc/l2hmc_kernels.hpp) and measure the operation sequence it is used in.

    u = 1 / (x + K)     s = (x - K) u, refined by one Newton step (three fmaf)     E = P(s) u     P by Horner, one fmaf per coefficient

erfcx(x) (x + K) is smooth in s on the whole half line (s = -1 at x = 0, s = 1 at x = infinity, where it tends to 1 / sqrt(pi)),
so ONE polynomial serves every x >= 0: no branch, one reciprocal.  The coefficients are fitted here -- interpolation at the
Chebyshev nodes in float64 against scipy.special.erfcx, then a few steps of Remez-style reweighting on the relative error --
rounded to float32 and the float32 sequence is measured against scipy.special.erfcx in float64 over a dense grid of [0, 64]
(beyond it s is within 2^-4 of 1 and the error is that of P near 1; a logarithmic grid to 1e19 is measured too).

The Newton step -- e = fma(s + 1, -K, x); e = fma(s, -x, e), the residual (x - K) - s (x + K); s = fma(u, e, s) -- makes s
independent of the reciprocal's last bit: without it the worst error is 7.5 u, at x near 2, instead of 5.2 u, at large x.
The hardware reciprocal is within one ulp of the quotient, numpy's division within half of one: the measurement is repeated with
u moved one ulp down and one ulp up, and the worst of the three is the figure printed (ERFCX_ULPS of tests/probit_case.py, in
units of u = 2^-24).  numpy has no fused multiply-add: fma(a, b, c) is formed as float32(float64(a) float64(b) + float64(c)) --
the product of two float32 is exact in float64, so this is fmaf up to one double rounding in about 2^-29 of the cases.

    python tools/fit_erfcx.py [--degree 10] [--points 4000001]
prints the C array, the Python tuple and the measurements."""
import argparse

import numpy as np
from scipy.special import erfcx

K = 2.0
U24 = 2.0 ** -24
f32 = np.float32


def fma32(a, b, c):
    """float32 fma of arrays or scalars: the product is exact in float64."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def erfcx32(x, coef, nudge=0):
    """The device sequence in float32 numpy; coef from the highest power down; nudge moves the reciprocal by that many ulps."""
    x = np.asarray(x, dtype=f32)
    u = (f32(1.0) / (x + f32(K))).astype(f32)
    if nudge:
        u = np.nextafter(u, f32(np.inf if nudge > 0 else -np.inf)).astype(f32)
    s = ((x - f32(K)) * u).astype(f32)
    e = fma32(s + f32(1.0), f32(-K), x)                          # x - K (s + 1)
    e = fma32(s, -x, e)                                          # (x - K) - s (x + K), the residual of the quotient
    s = fma32(u, e, s)
    p = np.full(x.shape, f32(coef[0]), dtype=f32)
    for c in coef[1:]:
        p = fma32(p, s, f32(c))
    return (p * u).astype(f32)


def target(s):
    """erfcx(x) (x + K) at s = (x - K) / (x + K), float64; s = 1 is the limit 1 / sqrt(pi)."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(all="ignore"):
        x = K * (1.0 + s) / (1.0 - s)
        f = erfcx(x) * (x + K)
    return np.where(s >= 1.0, 1.0 / np.sqrt(np.pi), f)


def fit(degree, rounds=12):
    """Coefficients (highest power first) of the weighted least-squares fit on a dense Chebyshev-distributed set, reweighted
    towards the points of largest relative error (Lawson's iteration)."""
    from numpy.polynomial import chebyshev as C
    m = 4096
    s = np.cos(np.pi * (np.arange(m) + 0.5) / m)
    f = target(s)
    w = np.ones(m)
    V = C.chebvander(s, degree)
    best = None
    for _ in range(rounds):
        sw = np.sqrt(w) / f                                      # relative error
        c, *_ = np.linalg.lstsq(V * sw[:, None], f * sw, rcond=None)
        err = np.abs(V @ c - f) / f
        if best is None or err.max() < best[0]:
            best = (err.max(), c)
        w = w * (err / err.mean() + 1e-3)
        w /= w.sum()
    mono = C.cheb2poly(best[1])
    return [float(f32(v)) for v in mono[::-1]], best[0]


def measure(coef, points):
    """(worst relative error in units of 2^-24 over [0, 64], the x where, the worst over a log grid from 64 to 1e19)."""
    worst, where = 0.0, 0.0
    xs = np.linspace(0.0, 64.0, points).astype(f32)
    ref = erfcx(xs.astype(np.float64))
    for nudge in (0, -1, 1):
        e = np.abs(erfcx32(xs, coef, nudge).astype(np.float64) - ref) / ref
        i = int(np.argmax(e))
        if e[i] > worst:
            worst, where = float(e[i]), float(xs[i])
    far = np.logspace(np.log10(64.0), 19.0, 200001).astype(f32)
    reff = erfcx(far.astype(np.float64))
    wf = max(float((np.abs(erfcx32(far, coef, n).astype(np.float64) - reff) / reff).max()) for n in (0, -1, 1))
    return worst / U24, where, wf / U24


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--degree", type=int, default=None, help="fit this degree only (default: 8 .. 16, and print the table)")
    ap.add_argument("--points", type=int, default=4000001)
    a = ap.parse_args()
    for deg in ([a.degree] if a.degree else range(8, 17)):
        coef, fit_err = fit(deg)
        w, at, far = measure(coef, a.points)
        print("degree %2d: float64 fit %.3g relative; float32 sequence worst %.3f u at x = %.6g on [0, 64] (%d points, reciprocal "
              "+-1 ulp), %.3f u on 64 .. 1e19" % (deg, fit_err, w, at, a.points, far))
        if a.degree:
            print("C:      {" + ", ".join("%sf" % repr(c) for c in coef) + "}")
            print("Python: (" + ", ".join(repr(c) for c in coef) + ")")


if __name__ == "__main__":
    main()
