#!/usr/bin/env python3
"""What the mip-mapped sky lookup (option "sky_mipmap") does to a frame, measured against supersampling and written to
profiles/sky_mipmap_quality.txt (or --out).  There is no pass threshold: the figures are what was measured.

Scenes, 1920 x 1080, Ellis rho = 1, cap 4096, R = 100, delta = 0.05: configs[1] of BASELINE.json (camera at l = 5 facing the
wormhole) through the brute renderer, and a frame of the reference's orbit path (--orbit-frame of --orbit-frames) through the
efficient renderer, which is what `curvis video` runs -- and the one in which the orbit changes the frame at all: the brute
renderer looks the sky up in the local spherical basis, as the reference's render_image does, so an orbit in phi at a fixed local
forward gives it the same frame every time.  Skies: two 8192 x 4096 checker
boards of 8-texel cells (skies.checker: hard edges, so that a lookup which picks one point of a squeezed sky shows).

Each scene is rendered at supersample = 1 with the nearest lookup, the bilinear one, and bilinear + mipmap, and compared with the
supersample = 8 bilinear frame of the same camera: RMS and 99th percentile of the absolute 8-bit difference over all channels, over
the whole frame and over the annulus around the ring -- pixels between 0.75 and 1.5 times the radius of the -l sky's image (the disc
of equal area around its centroid, found by a render over two flat skies).  Then the same for the DIFFERENCE between two consecutive
orbit frames (frame k + 1 minus frame k, as signed numbers), against the supersample = 8 pair's difference: what a viewer sees as
crawl and flicker is the part of that difference which the reference pair does not have.

    python tools/gpu_sky_mipmap_quality.py [--out FILE] [--orbit-frames 240] [--orbit-frame 60]"""
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
SKY_W, SKY_H, CELL = 8192, 4096, 8
MODES = (("nearest", dict(sky_filter=0, sky_mipmap=0)), ("bilinear", dict(sky_filter=1, sky_mipmap=0)),
         ("bilinear + mipmap", dict(sky_filter=1, sky_mipmap=1)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_mipmap_quality.txt"))
    ap.add_argument("--orbit-frames", type=int, default=240)
    ap.add_argument("--orbit-frame", type=int, default=60)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = curvis_amd.Context(0)
    metric = curvis_amd.EllisMetric(1.0)
    say("sky mipmap quality on %s: difference to the supersample = 8 bilinear frame, 8-bit units, all channels" % ctx.device_info()["name"])
    say("%d x %d, Ellis rho = 1, cap %d, R = %g, delta = %g; skies %d x %d checker boards of %d-texel cells" % (
        W, H, CAP, R, DELTA, SKY_W, SKY_H, CELL))
    real = [curvis_amd.SphericalImage(skies.checker(SKY_W, SKY_H, seed=s, cell=CELL)) for s in (0xC0FFEE, 0xBADC0DE)]
    flat = []
    for colour in ((255, 0, 0, 255), (0, 0, 255, 255)):
        flat.append(curvis_amd.SphericalImage(np.broadcast_to(np.array(colour, np.uint8), (2, 4, 4)).copy()))

    def bind(images):
        for k, img in enumerate(images):
            ctx.set_sky(k, img)

    def render(cam, supersample=1, sky_filter=0, sky_mipmap=0, efficient=False):
        ctx.set_option("supersample", supersample)
        ctx.set_option("sky_filter", sky_filter)
        ctx.set_option("sky_mipmap", sky_mipmap)
        try:
            if efficient:
                return ctx.render_efficient(metric, cam, CAP, R, DELTA, 100, 100, 1e-5, 1e-5)[0].astype(np.int16)
            return ctx.render_brute(metric, cam, CAP, R, DELTA)[0].astype(np.int16)
        finally:
            for key, value in (("supersample", 1), ("sky_filter", 0), ("sky_mipmap", 0)):
                ctx.set_option(key, value)

    def annulus(cam, efficient):
        bind(flat)
        far = render(cam, efficient=efficient)[..., 2] > 127                     # the -l sky's image
        bind(real)
        if not far.any():
            return None, 0.0
        ys, xs = np.nonzero(far)
        cy, cx, r = ys.mean(), xs.mean(), np.sqrt(far.sum() / np.pi)
        yy, xx = np.mgrid[0:H, 0:W]
        d = np.hypot(yy - cy, xx - cx)
        return (d >= 0.75 * r) & (d <= 1.5 * r), r

    def figures(diff, mask):
        out = []
        for m in (None, mask):
            v = np.abs(diff if m is None else diff[m]).astype(np.float64).reshape(-1)
            out += [np.sqrt(np.mean(v * v)), np.percentile(v, 99)]
        return tuple(out)

    it = rendering.Interpolator.from_file(__import__("refpaths").reference_path_file("path_orbit.csv"))
    times = np.linspace(it.min_time(), it.max_time(), a.orbit_frames, endpoint=False)

    def orbit_camera(k):
        t = times[k]
        return curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 15.0, 43.0, W, H)

    scenes = (("configs[1], brute renderer", curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, W, H), False),
              ("orbit frame %d of %d, efficient renderer" % (a.orbit_frame, a.orbit_frames), orbit_camera(a.orbit_frame), True))
    bind(real)
    head = "%-22s %12s %12s %14s %14s" % ("", "RMS, frame", "p99, frame", "RMS, annulus", "p99, annulus")
    kept = {}
    for name, cam, eff in scenes:
        mask, r = annulus(cam, eff)
        ref = render(cam, 8, 1, 0, eff)
        say()
        say("%s; annulus: %d pixels around a -l image of radius %.0f pixels" % (name, 0 if mask is None else int(mask.sum()), r))
        say(head)
        for mode, opts in MODES:
            frame = render(cam, 1, efficient=eff, **opts)
            kept[(name, mode)] = frame
            say("%-22s %12.3f %12.1f %14.3f %14.1f" % ((mode,) + figures(frame - ref, mask)))
        kept[(name, "ref")], kept[(name, "mask")] = ref, mask
    # two consecutive orbit frames: the change from one to the next, beside the reference pair's change
    name = scenes[1][0]
    nxt = orbit_camera(a.orbit_frame + 1)
    ref_change = render(nxt, 8, 1, 0, True) - kept[(name, "ref")]
    mask = kept[(name, "mask")]
    say()
    say("frame-to-frame change, orbit frames %d -> %d, minus the supersample = 8 pair's change (its own RMS: %.3f frame, %.3f annulus)" % (
        a.orbit_frame, a.orbit_frame + 1, figures(ref_change, mask)[0], figures(ref_change, mask)[2]))
    say(head)
    for mode, opts in MODES:
        change = render(nxt, 1, efficient=True, **opts) - kept[(name, mode)]
        say("%-22s %12.3f %12.1f %14.3f %14.1f" % ((mode,) + figures(change - ref_change, mask)))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
