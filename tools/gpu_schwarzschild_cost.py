#!/usr/bin/env python3
"""What the Schwarzschild kind costs beside Interstellar, on the GPU.  Writes profiles/schwarzschild_cost.txt:

  - the kernel time of a brute 1080p launch (the static kernel for both kinds: variant = 1) and the time per executed step, for the
    Schwarzschild kind and for Interstellar at the same camera radius, escape radius and delta; the legs are interleaved in one
    session and one of them runs twice (A, B, A', B') so that the spread of identical legs shows beside the difference;
  - the share of the frame's steps spent by captured rays between the photon sphere and -max_radius (from a debug dump of a 240 x 135
    frame of the same camera, its rays walked again on the host up to the photon sphere).

    python tools/gpu_schwarzschild_cost.py [output file]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import curvis_amd  # noqa: E402

L_CAM, R, DELTA, CAP, ROUNDS = 8.0, 25.0, 0.05, 40000, 5


def camera(res):
    return curvis_amd.Camera((0.0, L_CAM, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, res[0], res[1])


def leg(ctx, metric, cam):
    ms, steps = [], 0
    for _ in range(ROUNDS):
        _, st = ctx.render_brute(metric, cam, CAP, R, DELTA, download=False)
        ms.append(st.kernel_ms)
        steps = int(st.steps)
    return float(np.median(ms)), min(ms), max(ms), steps, st


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "schwarzschild_cost.txt")
    ctx = curvis_amd.Context(0)
    ctx.set_option("variant", 1)
    from curvis_amd import skies
    for k in (0, 1):
        ctx.set_sky(k, curvis_amd.SphericalImage(skies.checker(512, 256, seed=k + 1)))
    hole, worm = curvis_amd.SchwarzschildMetric(1.0), curvis_amd.InterstellarMetric(0.1, 1e-4, 1.0)
    cam = camera((1920, 1080))
    info = ctx.device_info()
    lines = ["Schwarzschild kind: cost of a brute 1080p launch beside Interstellar (tools/gpu_schwarzschild_cost.py)",
             "device: %s, %d CUs; static kernel (variant = 1), fast step, camera at l = %g looking at the centre, max_radius %g, delta %g" % (
                 info["name"], info["compute_units"], L_CAM, R, DELTA),
             "legs interleaved in one session, %d launches each (median [min, max] of the kernel time); A = Schwarzschild M = 1, B = Interstellar (0.1, 1e-4, 1)" % ROUNDS, ""]
    leg(ctx, hole, cam), leg(ctx, worm, cam)   # warm-up: code objects, clocks
    for name, metric in (("A ", hole), ("B ", worm), ("A'", hole), ("B'", worm)):
        med, lo, hi, steps, st = leg(ctx, metric, cam)
        lines.append("  %s %8.3f ms [%8.3f, %8.3f]  %12d steps  %7.3f ps/step  (+l %d, -l %d, capped %d)" % (
            name, med, lo, hi, steps, med * 1e9 / steps, st.n_pos, st.n_neg, st.n_none))
    # captured rays: steps spent after the ray has crossed the photon sphere inward
    small = camera((120, 68))
    _, st, dbg = ctx.render_brute(hole, small, CAP, R, DELTA, debug=True)
    import ctypes as C
    import schwarzschild_ref as SR
    from curvis_amd import _abi
    l_ps = hole.l_of_radius(3.0)
    after = 0
    m = hole._c()
    for j, i in np.argwhere(dbg["code"] == -1):
        d = small.outward_vector_on_world_space_from_x_y(int(i), int(j))
        x, p = SR.new_photon(hole, small.position, d)
        k = 0
        while x[1] > l_ps and k < CAP:
            _abi.lib().curvis_update_relativistic_object(C.byref(m), SR._dp(x), SR._dp(p), DELTA)
            k += 1
        after += int(dbg["steps"][j, i]) - k
    lines += ["", "120 x 68 frame of the same camera: %d rays, %d captured; %d of %d steps (%.1f %%) are spent by captured rays between the photon sphere and -max_radius" % (
        st.rays, st.n_neg, after, st.steps, 100.0 * after / st.steps)]
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
