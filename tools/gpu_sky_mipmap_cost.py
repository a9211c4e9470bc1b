#!/usr/bin/env python3
"""What the mip-mapped sky lookup (option "sky_mipmap" = 1 on top of "sky_filter" = 1) costs on the GPU beside the bilinear one,
measured in ONE process with the two settings interleaved, and written to profiles/sky_mipmap_cost.txt (or --out).  Skies: the
benchmark's procedural 8192 x 4096 pair.

  * brute renderer, configs[1] of BASELINE.json (Ellis rho = 1, 1080p, camera at l = 5, cap 4096, R = 100, delta = 0.05): ms per
    launch by HIP events (kernel_ms).  With the option on the static kernel renders (there is no relay form), so the bilinear leg is
    measured twice: with the automatic kernel choice and with variant = 1, the static kernel, which is the like-for-like pair.
  * direct renderer, the same frame: ms per launch.
  * efficient renderer's per-pixel kernel: ms per 1080p frame of a 128-frame call on the poses of the reference's orbit path
    (shade_ms / 128), device-resident sampler.  With the option on this is the tile-enumerating kernel, with it off the linear
    efficient_pixel_kernel<1>.  Three legs keep the two costs apart: the enumeration alone (bilinear both times: the linear kernel
    beside the tile-enumerating one, which library option "pixel_tiled" = 1 forces), the lookup alone (tile-enumerating both times:
    bilinear beside mip-mapped), and both together (what a caller who switches the option on sees).
  * the pyramid build of one 8192 x 4096 sky: HIP-event time of its 13 launches on the context's stream (read-only option
    "last_sky_mip_build_us"), the bytes it reads and writes, and beside it a device-to-device copy of the sky on the same stream
    (curvis_ctx_set_sky_device with copy = 1; HIP events around the copy alone, "last_sky_copy_us").

Each round measures off, then on; the figure is the median over the rounds, and the two "off" columns of the first and second half of
the rounds show the session's own spread.  There is no pass threshold.

    python tools/gpu_sky_mipmap_cost.py [--out FILE] [--rounds 9] [--frames 128]"""
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
SKY_W, SKY_H = 8192, 4096


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_mipmap_cost.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=128)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = curvis_amd.Context(0)
    info, before = ctx.device_info(), ctx.device_status()
    say("sky mipmap cost on %s (PCI %s); medians of %d interleaved rounds after two warm-up rounds, ms" % (
        info["name"], before["pci_bus_id"], a.rounds))
    say("1080p, Ellis rho = 1, cap %d, R = %g, delta = %g; skies %d x %d (skies.smooth, the benchmark's); sky_filter = 1 throughout" % (
        CAP, R, DELTA, SKY_W, SKY_H))
    ctx.set_sky(0, curvis_amd.SphericalImage(skies.smooth(SKY_W, SKY_H, 128)))
    ctx.set_sky(1, curvis_amd.SphericalImage(skies.smooth(SKY_W, SKY_H, 32)))
    metric = curvis_amd.EllisMetric(1.0)
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, W, H)
    from refpaths import reference_path_file
    it = rendering.Interpolator.from_file(reference_path_file("path_orbit.csv"))
    times = np.linspace(it.min_time(), it.max_time(), a.frames, endpoint=False)
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 15.0, 43.0, W, H) for t in times]
    ctx.set_option("device_sampler", 1)
    ctx.set_option("sky_filter", 1)

    def brute(mip):
        ctx.set_option("sky_mipmap", mip)
        _, st = ctx.render_brute(metric, cam, CAP, R, DELTA, download=False)
        return st.kernel_ms

    def brute_static(mip):
        ctx.set_option("variant", 1)
        try:
            return brute(mip)
        finally:
            ctx.set_option("variant", -1)

    def direct(mip):
        ctx.set_option("sky_mipmap", mip)
        _, st = ctx.render_direct(metric, cam, CAP, R, DELTA, download=False)
        return st.kernel_ms

    def pixel_as(mip, tiled):
        ctx.set_option("sky_mipmap", mip)
        ctx.set_option("pixel_tiled", tiled)
        try:
            _, st = ctx.render_efficient(metric, cams, CAP, R, DELTA, 100, 100, 1e-5, 1e-5, download=False)
            assert ctx.get_option("last_pixel_tiled") == (1 if mip or tiled else 0)
        finally:
            ctx.set_option("pixel_tiled", 0)
        return st.shade_ms / len(cams)

    def pixel(mip):                   # what a caller sees: linear bilinear | tiled mip-mapped
        return pixel_as(mip, 0)

    def pixel_enumeration(tiled):     # bilinear both times: linear | tiled
        return pixel_as(0, tiled)

    def pixel_lookup(mip):            # tiled both times: bilinear | mip-mapped
        return pixel_as(mip, 1)

    say()
    say("%-66s %10s %10s %9s %22s" % ("", "first", "second", "ratio", "first, halves of run"))
    say("(first | second = bilinear | bilinear + mipmap unless the line says otherwise)")
    legs = (("brute configs[1], automatic kernel choice when off, ms per launch", brute),
            ("brute configs[1], static kernel both times, ms per launch", brute_static),
            ("direct renderer, the same frame, ms per launch", direct),
            ("efficient pixel kernel, linear bilinear | tiled mipmap, ms per frame of %d" % a.frames, pixel),
            ("  enumeration alone: linear bilinear | tiled bilinear", pixel_enumeration),
            ("  lookup alone: tiled bilinear | tiled mipmap", pixel_lookup))
    for name, call in legs:
        for _ in range(2):
            call(0), call(1)
        got = np.array([[call(0), call(1)] for _ in range(a.rounds)])
        off, on = np.median(got[:, 0]), np.median(got[:, 1])
        half = a.rounds // 2
        say("%-66s %10.4f %10.4f %8.4fx %10.4f %10.4f" % (name, off, on, on / off, np.median(got[:half, 0]) if half else off,
                                                          np.median(got[half:, 0])))
    ctx.set_option("sky_mipmap", 0)

    # the pyramid build beside a device-to-device copy of the same sky, both by HIP events on the context's stream
    build, copy = [], []
    levels, moved = 0, 0
    wk, hk = SKY_W, SKY_H
    while wk > 1 or hk > 1:
        wd, hd = (wk + 1) >> 1, (hk + 1) >> 1
        moved += 4 * (4 * wd * hd + wd * hd)       # four source texels read (a repeated one counts once more) and one written per texel
        wk, hk, levels = wd, hd, levels + 1
    sky = curvis_amd.SphericalImage(skies.smooth(SKY_W, SKY_H, 128))
    for _ in range(a.rounds + 1):
        ctx.set_sky(0, sky)                        # drops the chain
        ctx.sky_mip_level(0, levels)               # builds it
        build.append(ctx.get_option("last_sky_mip_build_us") / 1e3)
        ctx.set_sky_device(1, ctx_sky_pointer(ctx), SKY_W, SKY_H, copy=True)
        copy.append(ctx.get_option("last_sky_copy_us") / 1e3)
    b, c = np.median(build[1:]), np.median(copy[1:])
    sky_bytes = 4 * SKY_W * SKY_H
    say()
    say("pyramid of one %d x %d sky: %d levels above level 0, %.1f MiB read and written in %.3f ms = %.0f GB/s (first build %.3f ms)" % (
        SKY_W, SKY_H, levels, moved / 2 ** 20, b, moved / b / 1e6, build[0]))
    say("device-to-device copy of the sky (the copy alone): %.1f MiB read and written in %.3f ms = %.0f GB/s" % (
        2 * sky_bytes / 2 ** 20, c, 2 * sky_bytes / c / 1e6))
    after = ctx.device_status()
    say()
    say("shader clock (sysfs level, MHz): %s before, %s after; board power %s -> %s W" % (
        before["sclk_mhz"], after["sclk_mhz"], before["power_w"], after["power_w"]))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


def ctx_sky_pointer(ctx):
    """a device buffer that holds a sky-sized image: the context's frame buffer after an upload of that many bytes"""
    p, n = ctx.framebuffer()
    if n < 4 * SKY_W * SKY_H:
        ctx.upload_frames(np.zeros(4 * SKY_W * SKY_H, np.uint8))
        p, n = ctx.framebuffer()
    return p


if __name__ == "__main__":
    sys.exit(main())
