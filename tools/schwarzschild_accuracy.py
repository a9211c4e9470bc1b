#!/usr/bin/env python3
"""Accuracy of the Schwarzschild kind's metric functions and of rays integrated through it, on the CPU (the library's host
accessors: the strict step compiled for x86).  Writes profiles/schwarzschild_accuracy.txt:

  - the maximum ulp errors of R and R' against mpmath at 40 digits over the sweep of tests/test_schwarzschild_host.py (A2), which
    asserts twice these figures;
  - the critical angle of the shadow for three observers (A3) and the deflection integral for three impact parameters (A4),
    stepped with delta, delta/2 and delta/4: values, differences, ratios.

    python tools/schwarzschild_accuracy.py [output file]
"""
import math
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_schwarzschild_host as H  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "schwarzschild_accuracy.txt")
    lines = ["Schwarzschild kind: accuracy of the metric functions and of integrated rays (tools/schwarzschild_accuracy.py)",
             "host: %s, %s; the library's host accessors (x86, the strict step); mpmath at 40 digits" % (platform.machine(), platform.python_version()), ""]
    w = H.measure_metric_errors()
    lines += ["A2. R and R' over l/M in {0, +-tiny, 2001 points in [0, 6], 1000 log-spaced up to 2^80, the photon sphere}, M in %s" % (H.MASSES,),
              "  max error of R : %.3f ulp  (M = %r, l = %r)" % w["R"],
              "  max error of R': %.3f ulp  (M = %r, l = %r)" % w["Rd"],
              "  min of R over the sweep against 3 sqrt(3) M: %.3f ulp" % w["min_R_ulp"],
              "  (R' = (2u - 1) / (2 sqrt(u (1 + u))) passes through zero at the photon sphere: next to it the error of u, about an ulp of",
              "   1/2, is many ulp of the small R'.  The tests assert twice the two maxima.)", ""]
    lines.append("A3. critical angle of the shadow (alpha from the outward radial direction), Heun, delta = %s M, fan spacing %g" % (H.SHADOW_DELTAS, H.FAN_SPACING))
    for r, (alpha_c, flips) in H.shadow_figures().items():
        d1, d2 = flips[0] - flips[1], flips[1] - flips[2]
        lines.append("  r = %4g M: closed form %.12f; flips %s; differences %.3e %.3e (ratio %.3f); finest - closed form %.3e" % (
            r, alpha_c, " ".join("%.12f" % f for f in flips), d1, d2, d1 / d2 if d2 else math.nan, flips[2] - alpha_c))
    lines.append("")
    lines.append("A4. swept phi minus the integral over the same two legs, delta = %s M; (b/M, start r/M) = %s" % (H.DEFLECTION_DELTAS, H.DEFLECTION_CASES))
    for integ, name in ((1, "Heun"), (0, "Euler")):
        for b, de in H.deflection_defects(integ).items():
            d1, d2 = de[0] - de[1], de[1] - de[2]
            lines.append("  %-5s b = %4g M: defects %s; differences %.3e %.3e (ratio %.3f)" % (name, b, " ".join("%.3e" % v for v in de), d1, d2, d1 / d2 if d2 else math.nan))
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
