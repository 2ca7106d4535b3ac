#!/usr/bin/env python3
"""Writes csrc/kernel_tables.hpp: the 51-entry line-integral tables of the built-in SPH kernels.

A kernel is W(r, H) = H^-3 f(r / H) with support radius H (f = 0 for q >= 1) and
4 pi int_0^1 f(q) q^2 dq = 1.  Table entry i is the integral of f along the whole chord at impact
parameter b = i / 50:

    F_i = 2 int_0^sqrt(1 - b^2) f(sqrt(b^2 + z^2)) dz,        F_50 = 0.

The chord is split where q = sqrt(b^2 + z^2) crosses a breakpoint of f (the kinks of the
splines), and each piece is integrated by Gauss-Legendre in t, z = b sinh t (q = b cosh t), which
takes the integrand's branch points at z = +-i b off the interval: the integrand is entire in t,
so the quadrature converges to rounding even for small b.  At b = 0 the pieces are polynomials in
z and are integrated directly.  The tables are the true integrals (to <= 1e-13), NOT renormalised:
the lerp of 51 points integrates to slightly more than 1 (the bias is listed in INTEGRATION.md).

`cubic` is not computed: it is the reference's table, kept bit for bit (it differs from the exact
M4 integrals by up to 2.1e-5).

    python3 tools/gen_kernel_tables.py            # rewrites csrc/kernel_tables.hpp
    python3 tools/gen_kernel_tables.py --check    # exit 1 if the committed header differs
"""
import math
import os
import sys

import numpy as np

N_TABLE = 51
PI = math.pi

# The reference's cubic-spline (M4) table (include/grace/cuda/trace_sph.cuh), as written there.
CUBIC = [
    "1.90986019771937", "1.90563449910964", "1.89304415940934", "1.87230928086763",
    "1.84374947679902", "1.80776276033034", "1.76481079856299", "1.71540816859939",
    "1.66011373131439", "1.59952322363667", "1.53426266082279", "1.46498233888091",
    "1.39235130929287", "1.31705223652377", "1.23977618317103", "1.16121278415369",
    "1.08201943664419", "1.00288866679720", "0.924475767210246", "0.847415371038733",
    "0.772316688105931", "0.699736940377312", "0.630211918937167", "0.564194562399538",
    "0.502076205853037", "0.444144023534733", "0.390518196140658", "0.341148855945766",
    "0.295941946237307", "0.254782896476983", "0.217538645099225", "0.184059547649710",
    "0.154181189781890", "0.127726122453554", "0.104505535066266",
    "8.432088120445191E-002", "6.696547102921641E-002", "5.222604427168923E-002",
    "3.988433820097490E-002", "2.971866601747601E-002", "2.150552303075515E-002",
    "1.502124104014533E-002", "1.004371608622562E-002", "6.354242122978656E-003",
    "3.739494884706115E-003", "1.993729589156428E-003", "9.212900163813992E-004",
    "3.395908945333921E-004", "8.287326418242995E-005", "7.387919939044624E-006",
    "0.000000000000000E+000",
]


def _pos(x):
    return np.maximum(x, 0.0)


def quartic(q):
    s = 2.5 * q
    return 25.0 / (32.0 * PI) * (_pos(2.5 - s) ** 4 - 5.0 * _pos(1.5 - s) ** 4 + 10.0 * _pos(0.5 - s) ** 4)


def quintic(q):
    s = 3.0 * q
    return 9.0 / (40.0 * PI) * (_pos(3.0 - s) ** 5 - 6.0 * _pos(2.0 - s) ** 5 + 15.0 * _pos(1.0 - s) ** 5)


def wendland_c2(q):
    u = _pos(1.0 - q)
    return 21.0 / (2.0 * PI) * u ** 4 * (1.0 + 4.0 * q)


def wendland_c4(q):
    u = _pos(1.0 - q)
    return 495.0 / (32.0 * PI) * u ** 6 * (1.0 + 6.0 * q + 35.0 / 3.0 * q * q)


def wendland_c6(q):
    u = _pos(1.0 - q)
    return 1365.0 / (64.0 * PI) * u ** 8 * (1.0 + 8.0 * q + 25.0 * q * q + 32.0 * q ** 3)


# name, f, interior breakpoints of f in q, closed-form F(0); in the order of GRACE_SPH_KERNEL_*.
KERNELS = [
    ("cubic", None, (0.5,), 6.0 / PI),
    ("quartic", quartic, (0.2, 0.6), 15.0 / (2.0 * PI)),
    ("quintic", quintic, (1.0 / 3.0, 2.0 / 3.0), 9.0 / PI),
    ("wendland_c2", wendland_c2, (), 7.0 / PI),
    ("wendland_c4", wendland_c4, (), 55.0 / (6.0 * PI)),
    ("wendland_c6", wendland_c6, (), 91.0 / (8.0 * PI)),
]

_X, _W = np.polynomial.legendre.leggauss(64)


def _gl(fn, lo, hi):
    if hi <= lo:
        return 0.0
    x = 0.5 * (hi - lo) * _X + 0.5 * (hi + lo)
    return 0.5 * (hi - lo) * float(np.dot(_W, fn(x)))


def chord_integral(f, breaks, b):
    """2 int_0^sqrt(1 - b^2) f(sqrt(b^2 + z^2)) dz, split at the breakpoints q_k > b."""
    if b >= 1.0:
        return 0.0
    qs = [b] + [q for q in breaks if q > b] + [1.0]
    total = 0.0
    for q0, q1 in zip(qs[:-1], qs[1:]):
        if b == 0.0:
            total += _gl(f, q0, q1)
        else:
            total += _gl(lambda t: f(b * np.cosh(t)) * b * np.cosh(t), math.acosh(q0 / b), math.acosh(q1 / b))
    return 2.0 * total


def volume_norm(f, breaks):
    qs = [0.0] + list(breaks) + [1.0]
    return sum(_gl(lambda q: 4.0 * PI * f(q) * q * q, a, c) for a, c in zip(qs[:-1], qs[1:]))


def tables():
    out = []
    for name, f, breaks, f0 in KERNELS:
        if f is None:
            out.append([float(v) for v in CUBIC])
            continue
        norm = volume_norm(f, breaks)
        assert abs(norm - 1.0) < 1e-14, (name, norm)
        t = [chord_integral(f, breaks, i / (N_TABLE - 1)) for i in range(N_TABLE)]
        assert abs(t[0] - f0) < 1e-13, (name, t[0], f0)
        out.append(t)
    return out


def header():
    lines = [
        "// Generated by tools/gen_kernel_tables.py -- do not edit; rerun the script instead.",
        "// Line integrals F_i = int f(sqrt((i/50)^2 + z^2)) dz over the whole chord of the built-in SPH",
        "// kernels (support radius 1), in the order of GRACE_SPH_KERNEL_* (include/grace_hip.h).  Row 0",
        "// is the reference's cubic-spline table bit for bit; the others are the exact integrals, not",
        "// renormalised.  Used once for the device array and once for the host copy (trace.hip).",
        "#pragma once",
        "",
        "#define GRACE_SPH_KERNEL_TABLE_ROWS %d" % len(KERNELS),
        "",
        "#define GRACE_SPH_KERNEL_TABLES_INIT { \\",
    ]
    for k, ((name, *_), t) in enumerate(zip(KERNELS, tables())):
        lines.append("    /* %s */ { \\" % name)
        vals = CUBIC if k == 0 else ["%.17g" % v for v in t]
        for i in range(0, N_TABLE, 4):
            lines.append("        " + ", ".join(vals[i:i + 4]) + ("," if i + 4 < N_TABLE else "") + " \\")
        lines.append("    }%s \\" % ("," if k + 1 < len(KERNELS) else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernel_tables.hpp")
    text = header()
    if "--check" in sys.argv[1:]:
        with open(path) as fh:
            same = fh.read() == text
        print("%s is %s" % (path, "up to date" if same else "STALE"))
        return 0 if same else 1
    with open(path, "w") as fh:
        fh.write(text)
    print("wrote", path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
