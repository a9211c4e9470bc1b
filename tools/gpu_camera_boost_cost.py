#!/usr/bin/env python3
"""What the moving camera (curvis_ctx_set_camera_velocities) costs, on the GPU.  Writes profiles/camera_boost_cost.txt, two parts:

  1. the dead branch: the PROJ = 1 kernels now test a launch-uniform bit in their prologue.  An equirectangular launch WITHOUT a
     velocity in this build against the same launch in the parent commit's build, through tools/gpu_ab.py (child processes, the two
     libraries interleaved): brute 1080p, the direct renderer, the efficient renderer's per-pixel kernel.  It needs both libraries:
         build/ab/this.so     a copy of curvis_amd/lib/libcurvis_hip.so
         build/ab/parent.so   the same file built from the parent commit (a worktree of it, `make -C curvis_amd/csrc`)
     and is left out, with a line saying so, where build/ab/parent.so does not exist.
  2. the boost itself: perspective frames with beta = (0.3, -0.4, 0.5) against the same frames with the camera at rest, in this
     build, legs interleaved A B A' B'.  Other rays take other step counts, so the brute and the direct renderer are compared per
     executed step; the per-pixel kernel has no steps and is compared per frame of a 32-frame call.  Both brute legs run the static
     kernel (variant = 1), which is the one a moving camera takes.

Every difference stands beside the spread of the identical legs: a difference inside that spread is not resolved, not zero.

    python tools/gpu_camera_boost_cost.py [output file]
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BETA, R, DELTA, CAP, ROUNDS, RES = (0.3, -0.4, 0.5), 100.0, 0.05, 4096, 9, (1920, 1080)


def dead_branch():
    ab = os.path.join(ROOT, "build", "ab")
    if not (os.path.exists(os.path.join(ab, "parent.so")) and os.path.exists(os.path.join(ab, "this.so"))):
        return ["1. PROJ = 1 without a velocity, this build against the parent's: NOT MEASURED (build/ab/parent.so or build/ab/this.so is missing)"]
    env = dict(os.environ, LIBS="parent,this", ROUNDS="4", AB_OPTIONS="projection=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_ab.py")], capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        sys.exit("tools/gpu_ab.py failed (%d); nothing more is started on the GPU\n%s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    return ["1. PROJ = 1 without a velocity (equirectangular, max_radius %g), the parent's build and this one interleaved, 4 rounds (tools/gpu_ab.py, AB_OPTIONS=projection=1):" % R] + \
           ["   " + line for line in r.stdout.strip().splitlines()]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "camera_boost_cost.txt")
    lines = dead_branch()          # child processes first: this process has not opened the GPU yet
    import curvis_amd
    from curvis_amd import skies
    ctx = curvis_amd.Context(0)
    ctx.set_option("variant", 1)
    for k in (0, 1):
        ctx.set_sky(k, curvis_amd.SphericalImage(skies.smooth(512, 256, k)))
    metric = curvis_amd.EllisMetric(1.0)
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, *RES)
    cams = [curvis_amd.Camera((0.0, 3.0 + 0.05 * k, np.pi / 2, 0.1 * k), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, *RES) for k in range(32)]

    def brute():
        _, st = ctx.render_brute(metric, cam, CAP, R, DELTA, download=False)
        return st.kernel_ms * 1e9 / st.steps, st.steps

    def direct():
        _, st = ctx.render_direct(metric, cam, CAP, R, DELTA, download=False)
        return st.kernel_ms * 1e9 / st.steps, st.steps

    def pixel():
        _, st = ctx.render_efficient(metric, cams, CAP, R, DELTA, 100, 100, 1e-5, 1e-5, download=False)
        return st.shade_ms / 32.0 * 1e3, 0

    info = ctx.device_info()
    lines += ["", "2. perspective with beta = %s against perspective at rest, this build; Ellis rho = 1, %d x %d, max_radius %g, delta %g, cap %d;" % ((BETA,) + RES + (R, DELTA, CAP)),
              "   device: %s, %d CUs; A = at rest (PROJ = 0 kernels), B = moving (PROJ = 1 kernels); legs interleaved, %d launches each, median [min, max]" % (
                  info["name"], info["compute_units"], ROUNDS)]
    for name, unit, run in (("brute, static kernel", "ps per executed step", brute), ("direct renderer", "ps per executed step", direct),
                            ("efficient per-pixel kernel", "us per frame of a 32-frame call", pixel)):
        med = {"A": [], "B": []}
        for leg in ("A", "B", "A", "B", "A", "B"):          # the first pair warms up: code objects, clocks
            ctx.set_camera_velocities([BETA] if leg == "B" else None)
            vals = [run() for _ in range(ROUNDS)]
            med[leg].append((float(np.median([v[0] for v in vals])), min(v[0] for v in vals), max(v[0] for v in vals), vals[-1][1]))
        lines.append("   %s (%s):" % (name, unit))
        for leg in "AB":
            for k, tag in ((1, leg + " "), (2, leg + "'")):
                m = med[leg][k]
                lines.append("     %s %10.3f [%10.3f, %10.3f]%s" % (tag, m[0], m[1], m[2], "  %d steps" % m[3] if m[3] else ""))
        a, b = (np.mean([m[0] for m in med[leg][1:]]) for leg in "AB")
        spread = max(abs(med[leg][1][0] / med[leg][2][0] - 1.0) for leg in "AB")
        diff = b / a - 1.0
        lines.append("     B against A: %+.2f %%; identical legs differ by up to %.2f %%: %s" % (
            100.0 * diff, 100.0 * spread, "outside the spread" if abs(diff) > spread else "not resolved"))
    ctx.set_camera_velocities(None)
    text = "Moving camera: what the boost costs (tools/gpu_camera_boost_cost.py)\n" + "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
