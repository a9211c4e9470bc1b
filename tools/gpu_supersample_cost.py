#!/usr/bin/env python3
"""What supersampling costs on the GPU, measured in ONE process and written to profiles/supersample_cost.txt (or --out).

For 1080p output, Ellis metric (rho = 1, camera at l = 5, cap 4096, R = 100, delta = 0.05), N = 2 and 4:
  * brute renderer, one frame, static kernel (variant 1) and relay kernel (variant 2): kernel_ms with supersample = N, beside the
    supersample = 1 render at N x the resolution -- the same rays through the kernels as they were before the option existed, the
    yardstick.  The fine leg is measured twice (A, A'): their difference is the session's repeat-to-repeat spread, and a
    supersampled figure above the fine render by more than that needs an explanation.
  * efficient renderer, 64 frames per call: the per-pixel kernel's time per frame (shade_ms / 64), the same way.
  * end to end: `curvis video --mode efficient` frames/s on the reference's orbit path with --supersample 4 beside --supersample 1
    (no pass threshold: the number users ask for).

    python tools/gpu_supersample_cost.py [--out FILE] [--reps 7] [--video-frames 240] [--no-video]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import curvis_amd  # noqa: E402
from curvis_amd import pngio, skies  # noqa: E402

W, H, CAP, R, DELTA = 1920, 1080, 4096, 100.0, 0.05


def camera(w, h, k=0):
    return curvis_amd.Camera((0.0, 5.0 - 0.03 * k, np.pi / 2, 0.02 * k), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, w, h)


def median_ms(call, reps):
    call()   # warm-up: buffers, the relay kernel's checked first launch of a shape
    call()
    return float(np.median([call() for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "supersample_cost.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--video-frames", type=int, default=240)
    ap.add_argument("--no-video", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = curvis_amd.Context(0)
    say("supersampling cost on %s; medians of %d calls after two warm-up calls, ms" % (ctx.device_info()["name"], a.reps))
    say("1080p output, Ellis rho = 1, camera at l = 5, cap %d, R = %g, delta = %g; sky 512 x 256" % (CAP, R, DELTA))
    ctx.set_sky(0, curvis_amd.SphericalImage(skies.smooth(512, 256, 0)))
    ctx.set_sky(1, curvis_amd.SphericalImage(skies.smooth(512, 256, 1)))
    metric = curvis_amd.EllisMetric(1.0)

    def brute(cam, ss):
        def call():
            ctx.set_option("supersample", ss)
            _, st = ctx.render_brute(metric, cam, CAP, R, DELTA, download=False)
            return st.kernel_ms
        return call

    def efficient(cams, ss):
        def call():
            ctx.set_option("supersample", ss)
            _, st = ctx.render_efficient(metric, cams, CAP, R, DELTA, 100, 100, 1e-5, 1e-5, download=False)
            return st.shade_ms / len(cams)
        return call

    say()
    say("%-44s %12s %12s %12s %10s %10s" % ("kernel_ms", "supersample N", "fine A", "fine A'", "N / fine", "|A - A'|"))

    def row(name, ss_call, fine_call):
        fine_a = median_ms(fine_call, a.reps)
        got = median_ms(ss_call, a.reps)
        fine_b = median_ms(fine_call, a.reps)
        fine = 0.5 * (fine_a + fine_b)
        say("%-44s %12.4f %12.4f %12.4f %9.3fx %9.2f%%" % (name, got, fine_a, fine_b, got / fine, 100.0 * abs(fine_a - fine_b) / fine))

    base = median_ms(brute(camera(W, H), 1), a.reps)
    say("%-44s %12.4f" % ("brute, 1080p, supersample = 1 (automatic kernel)", base))
    for variant, kernel in ((1, "static"), (2, "relay")):
        ctx.set_option("variant", variant)
        for n in (2, 4):
            row("brute %s, N = %d (fine: %d x %d)" % (kernel, n, W * n, H * n), brute(camera(W, H), n), brute(camera(W * n, H * n), 1))
            if variant == 2:
                assert ctx.get_option("last_relay_launches") >= 1, "the relay kernel did not run"
    ctx.set_option("variant", -1)
    ctx.set_option("device_sampler", 1)
    for n in (2, 4):
        row("efficient pixel kernel per frame of 64, N = %d" % n, efficient([camera(W, H, k) for k in range(64)], n),
            efficient([camera(W * n, H * n, k) for k in range(64)], 1))
    ctx.set_option("supersample", 1)
    ctx.close()

    if not a.no_video:
        from refpaths import reference_path_file
        orbit = reference_path_file("path_orbit.csv")
        with tempfile.TemporaryDirectory() as d:
            pngio.write_png(os.path.join(d, "pos.png"), skies.smooth(2048, 1024, 0))
            pngio.write_png(os.path.join(d, "neg.png"), skies.smooth(2048, 1024, 1))
            with open(os.path.join(d, "vid.toml"), "w") as f:   # the path spans 60 s
                f.write('video_name = "v"\nframe_rate = %r\nfilepath_to_camera_path = "%s"\n' % (a.video_frames / 60.0, orbit))
            with open(os.path.join(d, "cam.toml"), "w") as f:
                f.write("resolution_x = %d\nresolution_y = %d\ndiagonal = 43.0\nfocal_length = 15.0\n" % (W, H))
            say()
            say("end to end: curvis video --mode efficient, 1080p, ~%d frames of the orbit path, default settings otherwise" % a.video_frames)
            for n in (1, 4, 1, 4):
                out = os.path.join(d, "out%d_%d" % (n, len(lines)))
                os.mkdir(out)
                t0 = time.perf_counter()
                r = subprocess.run([os.path.join(ROOT, "curvis_amd", "bin", "curvis"), "video", os.path.join(d, "pos.png"),
                                    os.path.join(d, "neg.png"), out, "-v", os.path.join(d, "vid.toml"), "-c", os.path.join(d, "cam.toml"),
                                    "--mode", "efficient", "--supersample", str(n)], capture_output=True, text=True, timeout=600)
                dt = time.perf_counter() - t0
                if r.returncode != 0:
                    say("  --supersample %d: FAILED (%d) %s" % (n, r.returncode, r.stderr[-300:]))
                    break
                frames = len(os.listdir(os.path.join(out, "tmp")))
                say("  --supersample %d: %4d frames in %6.2f s of the process = %7.1f frames/s" % (n, frames, dt, frames / dt))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
