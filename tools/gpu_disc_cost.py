#!/usr/bin/env python3
"""What a disc costs the brute renderer, on the GPU.  Writes profiles/disc_cost.txt:

  - the kernel time of a brute 1080p launch of the static kernel (variant = 1) and the time per executed step, with a disc set (the
    DISC kernels) and with none (the kernels every call launched before there was a disc), on two scenes: a Schwarzschild hole seen
    from l = 8 with a disc from l_of_radius(6 M) to l = 20, and the Ellis pose of the benchmark (l = 5 on the equator) with a disc at
    l in [1.5, 6];
  - the share of the frame's rays that end on the disc, and the executed steps per frame with and without it.  A disc ends rays early
    (in front of a hole: rays that would have fallen to -max_radius), and a wave whose lanes have partly ended costs what a full one
    costs, so the time per frame and even the time per executed step mix several effects;
  - therefore a third leg: the same disc moved beyond the escape radius, where no ray reaches it.  Every ray then takes exactly the
    steps it takes without a disc, through the DISC kernel with its plane test and its crossing branch: that leg against the plain one
    is the cost of the loop itself.

The legs are interleaved in one session and each runs twice (A, B, C, A', B', C'), so that the spread of identical legs shows beside
the difference.

    python tools/gpu_disc_cost.py [output file]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import curvis_amd  # noqa: E402
from curvis_amd import skies  # noqa: E402

DELTA, ROUNDS, RES = 0.05, 5, (1920, 1080)


def leg(ctx, metric, cam, cap, radius, disc):
    ctx.set_disc(disc)
    ms = []
    for _ in range(ROUNDS):
        _, st = ctx.render_brute(metric, cam, cap, radius, DELTA, download=False)
        ms.append(st.kernel_ms)
    return float(np.median(ms)), min(ms), max(ms), st, ctx.frame_disc_hits(0)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "disc_cost.txt")
    ctx = curvis_amd.Context(0)
    ctx.set_option("variant", 1)
    for k in (0, 1):
        ctx.set_sky(k, curvis_amd.SphericalImage(skies.checker(512, 256, seed=k + 1)))
    tex = skies.ring_texture(1024, 128)
    hole = curvis_amd.SchwarzschildMetric(1.0)
    scenes = [
        ("Schwarzschild M = 1, camera at l = 8, theta = 1.35, looking at the hole; disc from l_of_radius(6 M) = %.4f to l = 20; max_radius 25, cap 40000" % hole.l_of_radius(6.0),
         hole, curvis_amd.Camera((0.0, 8.0, 1.35, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, *RES), 40000, 25.0,
         curvis_amd.Disc(tex, hole.l_of_radius(6.0), 20.0)),
        ("Ellis rho = 1, the benchmark's pose (l = 5, theta = pi/2, looking at the throat); disc at l in [1.5, 6]; max_radius 100, cap 4096",
         curvis_amd.EllisMetric(1.0), curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, *RES), 4096, 100.0,
         curvis_amd.Disc(tex, 1.5, 6.0)),
    ]
    info = ctx.device_info()
    lines = ["Accretion disc: cost of a brute 1080p launch with a disc set beside the same launch with none (tools/gpu_disc_cost.py)",
             "device: %s, %d CUs; static kernel (variant = 1), fast step, delta %g; disc texture ring_texture(1024, 128)" % (info["name"], info["compute_units"], DELTA),
             "legs interleaved in one session, %d launches each (median [min, max] of the kernel time); A = disc set (DISC kernel), B = no disc (the plain kernel), "
             "C = the disc moved beyond max_radius, where no ray reaches it (DISC kernel, the steps of B)" % ROUNDS]
    for title, metric, cam, cap, radius, disc in scenes:
        lines += ["", title]
        leg(ctx, metric, cam, cap, radius, disc), leg(ctx, metric, cam, cap, radius, None)   # warm-up: code objects, clocks
        per_step = {}
        far = curvis_amd.Disc(tex, 2.0 * radius, 3.0 * radius)
        for name, d in (("A ", disc), ("B ", None), ("C ", far), ("A'", disc), ("B'", None), ("C'", far)):
            med, lo, hi, st, n_disc = leg(ctx, metric, cam, cap, radius, d)
            assert st.rays == st.n_pos + st.n_neg + st.n_none + n_disc
            per_step.setdefault(name[0], []).append(med * 1e9 / st.steps)
            lines.append("  %s %8.3f ms [%8.3f, %8.3f]  %12d steps  %7.3f ps/step  (+l %d, -l %d, capped %d, disc %d = %.1f %% of the rays)" % (
                name, med, lo, hi, st.steps, med * 1e9 / st.steps, st.n_pos, st.n_neg, st.n_none, n_disc, 100.0 * n_disc / st.rays))
        a, b, c = np.mean(per_step["A"]), np.mean(per_step["B"]), np.mean(per_step["C"])
        spread = ", ".join("%.1f %%" % (100.0 * abs(per_step[k][0] / per_step[k][1] - 1.0)) for k in "ABC")
        lines.append("  per executed step: disc %.3f ps, none %.3f ps, unreachable disc %.3f ps; the loop itself (C against B): %+.1f %%; with rays ending on the disc (A against B): %+.1f %%" % (
            a, b, c, 100.0 * (c / b - 1.0), 100.0 * (a / b - 1.0)))
        lines.append("  identical legs differ by %s (A, B, C)" % spread)
    ctx.set_disc(None)
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
