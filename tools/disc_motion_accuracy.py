#!/usr/bin/env python3
"""Accuracy of the disc's emission shift on the CPU (the library's host accessor curvis_disc_shift: cv_device.h disc_shift compiled
for x86).  Writes profiles/disc_motion_accuracy.txt:

  - the maximum error in ulp of F / G against the closed form g^4 at 40 digits with mpmath, fed the exact r_e = r(l_hit), r_c =
    r(l_camera) and the double p_phi, over the sweep of tests/test_disc_motion_host.py (r_e/M from 3.5 to 2^20, r_c/M from 4 to 2^20,
    |p_phi| up to R(r_e), both motions, four masses), which asserts twice this figure;
  - separately, how the error grows towards u = 1/2 (r_e -> 3M), where n = 2u - 1 magnifies the one-ulp error of u.

    python tools/disc_motion_accuracy.py [output file]
"""
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_disc_motion_host as H  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "disc_motion_accuracy.txt")
    lines = ["Disc emission shift: accuracy of F / G against the closed form (tools/disc_motion_accuracy.py)",
             "host: %s, %s; the library's host accessor curvis_disc_shift (x86); mpmath at 40 digits" % (platform.machine(), platform.python_version()), "",
             "F / G = ((1 - 3M/r_e) / ((1 - 2M/r_c) (1 + sigma sqrt(M/r_e^3) p_phi)^2))^2 with the exact r_e = r(l_hit), r_c = r(l_camera) of the doubles",
             "l_hit = l_of_radius(r_e), l_camera = l_of_radius(r_c), and p_phi = fraction * R(r_e) as a double", "",
             "1. r_e/M in 24 log-spaced points from 3.5 to 2^20, r_c/M in %s, fraction in %s, sigma = +-1, M in %s" % (H.RC_OVER_M, H.P_FRACTIONS, H.MASSES)]
    w = H.measure_shift_errors()
    lines += ["  max error of F / G: %.3f ulp  (M = %r, r_e/M = %r, r_c/M = %r, fraction = %r, sigma = %r)" % w["max"],
              "  worst per r_e/M: " + ", ".join("%.4g: %.1f" % (re, e) for re, e in sorted(w["by_re"].items())),
              "  (tests/test_disc_motion_host.py asserts twice the maximum.)", "",
              "2. towards the photon sphere, the same sweep at r_e/M in 3 + {2^-40, 2^-30, 2^-20, 2^-10}, 3.01, 3.1, 3.25, 3.49 (combinations with",
              "   1 + Omega p_phi below 2^-20, the closed form's own pole at |p_phi| = R next to r = 3M, left out)"]
    n = H.measure_shift_errors(H.NEAR_RE_OVER_M)
    lines += ["  worst per r_e/M: " + ", ".join("3 + %.3g: %.4g" % (re - 3.0, e) for re, e in sorted(n["by_re"].items())),
              "  n = 2 u_e - 1 is exact given u_e, but u_e carries an error of about an ulp of 1/2 whatever n is: relative to n that is",
              "  2^-53 / n, and F, which holds n squared, sees twice that -- the error in ulp grows as 1 / (r_e/M - 3), as the README describes for R'.", ""]
    text = "\n".join(lines)
    with open(out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
