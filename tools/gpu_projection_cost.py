#!/usr/bin/env python3
"""What the camera projections (option "projection" = 1 equirectangular, 2 fisheye) cost on the GPU beside the perspective camera,
measured in ONE process with the three settings interleaved, and written to profiles/projection_cost.txt (or --out).  Skies: the
benchmark's procedural 8192 x 4096 pair.

  * brute renderer, configs[1] of BASELINE.json (Ellis rho = 1, 1080p, camera at l = 5, cap 4096, R = 100, delta = 0.05): ms per
    launch by HIP events (kernel_ms), automatic kernel choice.  Another projection traces other rays, so the launch does another
    number of Euler steps: the second line gives the launches in ns per 1000 executed steps, where the prologue is what is left.
  * efficient renderer's per-pixel kernel: ms per 1080p frame of a 128-frame call on the poses of the reference's orbit path
    (shade_ms / 128, HIP events around the one launch), device-resident sampler.

Each round measures projection = 0, then 1, then 2; the figure is the median over the rounds, and the two perspective columns of the
first and second half of the rounds show the session's own spread.  There is no pass threshold.

    python tools/gpu_projection_cost.py [--out FILE] [--rounds 9] [--frames 128]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import curvis_amd  # noqa: E402
from curvis_amd import rendering, skies  # noqa: E402

W, H, CAP, R, DELTA = 1920, 1080, 4096, 100.0, 0.05


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_cost.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=128)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = curvis_amd.Context(0)
    info, before = ctx.device_info(), ctx.device_status()
    say("projection cost on %s (PCI %s); medians of %d interleaved rounds after two warm-up rounds" % (
        info["name"], before["pci_bus_id"], a.rounds))
    say("1080p, Ellis rho = 1, focal 15, diagonal 43, cap %d, R = %g, delta = %g; skies 8192 x 4096 (skies.smooth, the benchmark's)" % (
        CAP, R, DELTA))
    ctx.set_sky(0, curvis_amd.SphericalImage(skies.smooth(8192, 4096, 128)))
    ctx.set_sky(1, curvis_amd.SphericalImage(skies.smooth(8192, 4096, 32)))
    metric = curvis_amd.EllisMetric(1.0)
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, W, H)
    from refpaths import reference_path_file
    it = rendering.Interpolator.from_file(reference_path_file("path_orbit.csv"))
    times = np.linspace(it.min_time(), it.max_time(), a.frames, endpoint=False)
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 15.0, 43.0, W, H) for t in times]
    ctx.set_option("device_sampler", 1)

    def brute(proj):
        ctx.set_option("projection", proj)
        _, st = ctx.render_brute(metric, cam, CAP, R, DELTA, download=False)
        return st.kernel_ms, st.kernel_ms * 1e9 / max(int(st.steps), 1)       # ms; ns per 1000 steps

    def pixel(proj):
        ctx.set_option("projection", proj)
        _, st = ctx.render_efficient(metric, cams, CAP, R, DELTA, 100, 100, 1e-5, 1e-5, download=False)
        return st.shade_ms / len(cams), 0.0

    say()
    say("%-60s %11s %15s %9s %11s %9s %24s" % ("", "perspective", "equirectangular", "ratio", "fisheye", "ratio", "perspective, halves of run"))
    clocks = []
    for names, call in ((("brute configs[1], ms per launch", "brute configs[1], ns per 1000 executed Euler steps"), brute),
                        (("efficient pixel kernel, ms per frame of a %d-frame call" % a.frames,), pixel)):
        for _ in range(2):
            call(0), call(1), call(2)
        got = np.array([[call(0), call(1), call(2)] for _ in range(a.rounds)])      # [round, projection, figure]
        clocks.append(ctx.device_status()["sclk_mhz"])
        half = a.rounds // 2
        for k, name in enumerate(names):
            p0, p1, p2 = (np.median(got[:, j, k]) for j in range(3))
            say("%-60s %11.4f %15.4f %8.4fx %11.4f %8.4fx %12.4f %11.4f" % (name, p0, p1, p1 / p0, p2, p2 / p0,
                                                                           np.median(got[:half, 0, k]) if half else p0, np.median(got[half:, 0, k])))
    ctx.set_option("projection", 0)
    after = ctx.device_status()
    say()
    say("shader clock (sysfs level, MHz): %s before, %s after the brute rounds, %s after the pixel-kernel rounds; board power %s -> %s W" % (
        before["sclk_mhz"], clocks[0], clocks[1], before["power_w"], after["power_w"]))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
