#!/usr/bin/env python3
"""What the disc's emission shift costs the brute renderer, on the GPU.  Writes profiles/disc_motion_cost.txt:

  - the kernel time of a brute 1080p launch of the README's Schwarzschild disc frame (camera at l = 8, disc from l_of_radius(6 M) to
    l = 20, delta = 0.05) with the static disc (the DISC = 1 kernel) and with the prograde disc (the DISC = 2 kernel).  Both legs
    trace the same rays through the same steps -- the motion changes colours, never codes or counts -- so the difference is the
    kernel's: the shift sits behind the crossing branch, in the few iterations in which a lane gets its texel.

The legs are interleaved in one session and each runs twice (A, B, A', B'), so that the spread of identical legs shows beside the
difference.

    python tools/gpu_disc_motion_cost.py [output file]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import curvis_amd  # noqa: E402
from curvis_amd import skies  # noqa: E402

DELTA, ROUNDS, RES = 0.05, 7, (1920, 1080)


def leg(ctx, metric, cam, cap, radius, disc):
    ctx.set_disc(disc)
    ms = []
    for _ in range(ROUNDS):
        _, st = ctx.render_brute(metric, cam, cap, radius, DELTA, download=False)
        ms.append(st.kernel_ms)
    return float(np.median(ms)), min(ms), max(ms), st, ctx.frame_disc_hits(0)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "disc_motion_cost.txt")
    ctx = curvis_amd.Context(0)
    ctx.set_option("variant", 1)
    for k in (0, 1):
        ctx.set_sky(k, curvis_amd.SphericalImage(skies.checker(512, 256, seed=k + 1)))
    tex = skies.ring_texture(1024, 128)
    hole = curvis_amd.SchwarzschildMetric(1.0)
    l_in = hole.l_of_radius(6.0)
    cam = curvis_amd.Camera((0.0, 8.0, 1.35, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, *RES)
    cap, radius = 40000, 25.0
    static, prograde = curvis_amd.Disc(tex, l_in, 20.0), curvis_amd.Disc(tex, l_in, 20.0, motion="prograde")
    info = ctx.device_info()
    lines = ["Disc emission shift: a brute 1080p launch with the prograde disc beside the same launch with the static disc (tools/gpu_disc_motion_cost.py)",
             "device: %s, %d CUs; static kernel (variant = 1), fast step, delta %g; disc texture ring_texture(1024, 128)" % (info["name"], info["compute_units"], DELTA),
             "Schwarzschild M = 1, camera at l = 8, theta = 1.35, looking at the hole; disc from l_of_radius(6 M) = %.4f to l = 20; max_radius 25, cap 40000" % l_in,
             "legs interleaved in one session, %d launches each (median [min, max] of the kernel time); A = static disc (DISC = 1 kernel), B = prograde disc (DISC = 2 kernel)" % ROUNDS, ""]
    leg(ctx, hole, cam, cap, radius, static), leg(ctx, hole, cam, cap, radius, prograde)   # warm-up: code objects, clocks
    med_of, counts = {}, {}
    for name, d in (("A ", static), ("B ", prograde), ("A'", static), ("B'", prograde)):
        med, lo, hi, st, n_disc = leg(ctx, hole, cam, cap, radius, d)
        assert st.rays == st.n_pos + st.n_neg + st.n_none + n_disc
        med_of.setdefault(name[0], []).append(med)
        counts.setdefault(name[0], set()).add((st.steps, st.n_pos, st.n_neg, st.n_none, n_disc))
        lines.append("  %s %8.3f ms [%8.3f, %8.3f]  %12d steps  %7.3f ps/step  (+l %d, -l %d, capped %d, disc %d = %.1f %% of the rays)" % (
            name, med, lo, hi, st.steps, med * 1e9 / st.steps, st.n_pos, st.n_neg, st.n_none, n_disc, 100.0 * n_disc / st.rays))
    assert counts["A"] == counts["B"] and len(counts["A"]) == 1, "the motion changes no code and no count"
    a, b = np.mean(med_of["A"]), np.mean(med_of["B"])
    spread = ", ".join("%.2f %%" % (100.0 * abs(med_of[k][0] / med_of[k][1] - 1.0)) for k in "AB")
    lines.append("  prograde against static (B against A): %+.2f %%; identical legs differ by %s (A, B)" % (100.0 * (b / a - 1.0), spread))
    ctx.set_disc(None)
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
