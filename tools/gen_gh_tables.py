#!/usr/bin/env python3
"""Generate the adaptive Gauss-Hermite tables BayesW integrates with.

hydra hard-codes, for n in {3,5,7,9,11,13,15,17,25}, the positive roots x of
the Hermite polynomial H_n and the "adjusted" weights w = w_GH(x) * exp(x^2)
as 14-significant-digit decimal literals (src/BayesW.cpp:186-707), and sums
    w1 f(s x1) + w2 f(s x2) + ... + w_{n-1} f(s x_{n-1}) + w_n        (f(0) = 1)
with x_{2m} = -x_{2m-1}, w_{2m} = w_{2m-1}.  We recompute roots and weights
with mpmath, round to 14 significant digits, and apply the reference's own
deviations so that the doubles are the very same:

  * 28 literals carry fewer decimals than 14 significant digits (DECIMALS);
  * five literals differ from correct rounding in the last digit (LAST_DIGIT);
  * for every n >= 11 the sixth abscissa is -x3 instead of -x5 (a slip in the
    reference, src/BayesW.cpp n == "11" block and every later one); a drop-in
    must integrate with the same nodes, so the slip is reproduced (X6_IS_MINUS_X3).

When /root/reference is present the output is checked literal by literal
against the reference's text.  Writes oracle/gh_tables.h (ORC_GH_*) and
hydra_amd/csrc/hg_gh_tables.h (HG_GH_*).
"""
import os
import re
import sys

import mpmath as mp

ORDERS = [3, 5, 7, 9, 11, 13, 15, 17, 25]
SIG = 14
# (n, kind, 1-based index in the reference's numbering) -> literal as the reference has it
LAST_DIGIT = {
    (7, "x", 5): "0.81628788285897",
    (13, "x", 9): "1.2200550365908",
    (17, "x", 15): "0.53163300134266",
    (25, "x", 17): "1.7780011243372",
    (25, "w", 25): "0.43986872216949",
}
# (n, kind, index) -> decimal places the reference's literal was rounded to (default: 14 significant digits)
DECIMALS = {
    (7, "w", 3): 13, (7, "w", 5): 13, (9, "w", 5): 13, (11, "w", 3): 13, (11, "w", 5): 12, (11, "w", 7): 13,
    (13, "w", 1): 12, (13, "w", 3): 13, (13, "w", 5): 13, (13, "w", 7): 13, (13, "w", 9): 13, (15, "x", 13): 13,
    (15, "w", 3): 13, (15, "w", 5): 13, (15, "w", 7): 13, (15, "w", 9): 13, (17, "w", 1): 12, (17, "w", 3): 12,
    (17, "w", 5): 13, (17, "w", 7): 13, (17, "w", 9): 13, (25, "x", 9): 12, (25, "w", 1): 13, (25, "w", 3): 12,
    (25, "w", 5): 13, (25, "w", 9): 12, (25, "w", 11): 13, (25, "w", 13): 13,
}
X6_IS_MINUS_X3 = lambda n: n >= 11

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/BayesW.cpp"


def lit(v, key):
    if key in LAST_DIGIT:
        return LAST_DIGIT[key]
    d = DECIMALS.get(key, SIG - 1 if v >= 1 else SIG)
    q = mp.mpf(10) ** d
    r = mp.floor(v * q + mp.mpf("0.5")) / q
    s = mp.nstr(r, 20, strip_zeros=True)
    assert mp.mpf(s) == r
    return s


def tables():
    mp.mp.dps = 60
    out = {}
    for n in ORDERS:
        coeffs = [mp.mpf(c) for c in mp.taylor(lambda t: mp.hermite(n, t), 0, n)][::-1]
        roots = mp.polyroots(coeffs, maxsteps=500, extraprec=400)
        pos = sorted([mp.re(r) for r in roots if mp.re(r) > mp.mpf("1e-20")], reverse=True)
        assert len(pos) == (n - 1) // 2

        def w(x):
            return (2 ** (n - 1) * mp.factorial(n) * mp.sqrt(mp.pi)) / (n ** 2 * mp.hermite(n - 1, x) ** 2) * mp.exp(x * x)

        xs, ws = [], []
        for m, r in enumerate(pos):
            k = 2 * m + 1  # reference index of the positive node of this pair
            xl = lit(r, (n, "x", k))
            wl = lit(w(r), (n, "w", k))
            xs += [xl, "-" + xl]
            ws += [wl, wl]
        if X6_IS_MINUS_X3(n):
            xs[5] = "-" + xs[2]
        ws.append(lit(w(mp.mpf(0)), (n, "w", n)))
        out[n] = (xs, ws)
    return out


def reference_literals(path=REF):
    """{n: (x_1..x_{n-1}, w_1..w_n)}: the doubles the reference's literals denote, in its own numbering."""
    src = open(path).read()
    body = src[src.index("double BayesW::gauss_hermite_adaptive_integral"):src.index("void BayesW::marginal_likelihood_vec_calc")]
    blocks = re.split(r'if\s*\(\s*n\s*==\s*"(\d+)"\s*\)', body)
    out = {}
    for i in range(1, len(blocks), 2):
        n = int(blocks[i])
        blk = re.sub(r"//.*", "", blocks[i + 1])
        x = {int(a): float(b) for a, b in re.findall(r"\bx(\d+)\s*=\s*([0-9.]+)\s*;", blk)}
        for a, b in re.findall(r"\bx(\d+)\s*=\s*-\s*x(\d+)\s*;", blk):
            x[int(a)] = -x[int(b)]
        w = {int(a): float(b) for a, b in re.findall(r"\bw(\d+)\s*=\s*([0-9.]+)\s*;", blk)}
        for a, b in re.findall(r"\bw(\d+)\s*=\s*w(\d+)\s*;", blk):
            w[int(a)] = w[int(b)]
        assert len(x) == n - 1 and len(w) == n, (n, len(x), len(w))
        out[n] = ([x[k] for k in range(1, n)], [w[k] for k in range(1, n + 1)])
    return out


def check_against_reference(tabs, literals=None):
    """Literal-by-literal comparison with the reference (its text, or reference_literals() recorded earlier)."""
    literals = literals if literals is not None else reference_literals()
    checked = 0
    for n, (x, w) in literals.items():
        xs, ws = tabs[n]
        assert len(x) == n - 1 and len(w) == n, (n, len(x), len(w))
        for k in range(1, n):
            assert float(xs[k - 1]) == x[k - 1], (n, "x", k, xs[k - 1], x[k - 1])
        for k in range(1, n + 1):
            assert float(ws[k - 1]) == w[k - 1], (n, "w", k, ws[k - 1], w[k - 1])
        checked += 2 * n - 1
    return checked


def emit(path, prefix, tabs, note):
    with open(path, "w") as f:
        f.write("/* GENERATED by tools/gen_gh_tables.py -- do not edit.\n")
        f.write(" * Adaptive Gauss-Hermite nodes and exp(x^2)-adjusted weights as hydra's BayesW uses them\n")
        f.write(" * (src/BayesW.cpp:186-707): 14 significant digits, node 6 = -node 3 for n >= 11.\n")
        f.write(" * %s */\n#pragma once\n\n" % note)
        f.write("static const int %s_ORDERS[%d] = {%s};\n\n" % (prefix, len(ORDERS), ", ".join(map(str, ORDERS))))
        for n in ORDERS:
            xs, ws = tabs[n]
            f.write("static const double %s_X%d[%d] = {%s};\n" % (prefix, n, n - 1, ", ".join(xs)))
            f.write("static const double %s_W%d[%d] = {%s};\n\n" % (prefix, n, n, ", ".join(ws)))
        f.write("/* nodes (n-1 of them) and weights (n; the last one multiplies f(0) = 1); returns 0 for an unsupported order */\n")
        f.write("static inline int %s_lookup(int n, const double** x, const double** w)\n{\n    switch (n) {\n" % prefix.lower())
        for n in ORDERS:
            f.write("    case %d: *x = %s_X%d; *w = %s_W%d; return 1;\n" % (n, prefix, n, prefix, n))
        f.write("    default: *x = 0; *w = 0; return 0;\n    }\n}\n")


def main():
    tabs = tables()
    if os.path.exists(REF):
        n = check_against_reference(tabs)
        print("checked %d literals against %s: all equal" % (n, REF))
    else:
        print("reference absent: tables written unchecked", file=sys.stderr)
    emit(os.path.join(ROOT, "oracle", "gh_tables.h"), "ORC_GH", tabs, "Test infrastructure copy (oracle).")
    emit(os.path.join(ROOT, "hydra_amd", "csrc", "hg_gh_tables.h"), "HG_GH", tabs, "Product copy.")


if __name__ == "__main__":
    main()
