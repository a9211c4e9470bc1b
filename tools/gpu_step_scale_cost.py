#!/usr/bin/env python3
"""What distance-scaled Euler steps (option "step_scale" = S, L0 = S / 256) do to the GPU time of the three renderers, measured in ONE
process with the settings interleaved, and written to profiles/step_scale_cost.txt (or --out).  Skies: the benchmark's procedural
8192 x 4096 pair.  step_scale = 0 launches the kernels that exist without the option.

  * brute renderer, 1080p, camera at l = 5 facing the throat, cap 4096, R = 100, delta = 0.05: configs[1] of BASELINE.json (Ellis rho = 1)
    and the same frame under the Interstellar metric (m = 0.1, a = 1e-4, rho = 1).  Legs per round: S = 0 with the static kernel
    (variant = 1), S = 0 with the relay kernel (the automatic choice), S = 1024 (always the static kernel), S = 0 static again.  Per leg:
    ms per launch by HIP events and ns per 1000 EXECUTED steps.  The expectation to check is per executed step: the scaled step is two
    more FP64 VALU instructions, 2/83 of an Ellis step and 2/113 of an Interstellar one; the two S = 0 static legs of the same rounds
    show the spread that figure has to be read against.
  * direct renderer, the same two frames: S = 0 and S = 1024, the same two figures.
  * cost per ray and per step: brute (static kernel) and direct, S = 0 at R = 100 and R = 20, S = 1024 at R = 100 and R = 10000 (cap
    2^20) -- two step counts per ray for each kernel --, solved for time = A x rays + B x executed steps.  B(S = 1024) over B(S = 0) is
    the price of the scaled step itself; A is what a ray costs whatever its steps (prologue, epilogue, the launch's ramp and tail),
    which a fifth of the steps carries five times as heavily.
  * efficient renderer's sampler: ms of the sampler kernel per job (distinct camera radius) of a call over the poses of the reference's
    fly-through path, device-resident sampler, S = 0 and S = 1024.

The frame-time ratio is reported as measured, next to the step-count ratio.  There is no pass threshold.

    python tools/gpu_step_scale_cost.py [--out FILE] [--rounds 7] [--frames 64] [--scale 1024]"""
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
VALU = {"Ellis": 83, "Interstellar": 113}     # FP64 VALU instructions of one fast step


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_scale_cost.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--scale", type=int, default=1024)
    a = ap.parse_args()
    S = a.scale
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = curvis_amd.Context(0)
    info, before = ctx.device_info(), ctx.device_status()
    say("step_scale cost on %s (PCI %s); medians of %d interleaved rounds after one warm-up round" % (info["name"], before["pci_bus_id"], a.rounds))
    say("1080p, camera at l = 5, focal 15, diagonal 43, cap %d, R = %g, delta = %g; step_scale = %d (L0 = %g); skies 8192 x 4096 (skies.smooth, the benchmark's)" % (
        CAP, R, DELTA, S, S / 256.0))
    ctx.set_sky(0, curvis_amd.SphericalImage(skies.smooth(8192, 4096, 128)))
    ctx.set_sky(1, curvis_amd.SphericalImage(skies.smooth(8192, 4096, 32)))
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, W, H)
    metrics = (("Ellis", curvis_amd.EllisMetric(1.0)), ("Interstellar", curvis_amd.InterstellarMetric(0.1, 1e-4, 1.0)))

    def leg(render, scale, variant=None):
        ctx.set_option("step_scale", scale)
        if variant is not None:
            ctx.set_option("variant", variant)
        st = render()
        ctx.set_option("variant", -1)
        ctx.set_option("step_scale", 0)
        return st.kernel_ms, st.kernel_ms * 1e9 / max(int(st.steps), 1), float(st.steps)     # ms; ns per 1000 steps; steps

    say()
    say("brute renderer: ms per launch | ns per 1000 executed steps | executed steps")
    for name, metric in metrics:
        def render():
            return ctx.render_brute(metric, cam, CAP, R, DELTA, download=False)[1]
        legs = (("S = 0, static kernel", 0, 1), ("S = 0, relay kernel", 0, -1), ("S = %d (static kernel)" % S, S, -1), ("S = 0, static kernel again", 0, 1))
        for _, scale, variant in legs:
            leg(render, scale, variant)
        got = np.array([[leg(render, scale, variant) for _, scale, variant in legs] for _ in range(a.rounds)])   # [round, leg, figure]
        med = np.median(got, axis=0)
        for k, (what, _, _) in enumerate(legs):
            say("  %-13s %-28s %9.4f ms %10.3f ns %14.0f steps" % (name, what, med[k, 0], med[k, 1], med[k, 2]))
        spread = abs(med[3, 1] / med[0, 1] - 1.0)
        say("  %-13s per executed step, S = %d over S = 0 static: %+.2f %% (two more VALU instructions: %+.2f %%; the two S = 0 static legs differ by %.2f %%)" % (
            name, S, 100.0 * (med[2, 1] / med[0, 1] - 1.0), 200.0 / VALU[name], 100.0 * spread))
        say("  %-13s frame time, S = %d over S = 0: %.4fx of the static kernel, %.4fx of the relay kernel; executed steps %.4fx" % (
            name, S, med[2, 0] / med[0, 0], med[2, 0] / med[1, 0], med[2, 2] / med[0, 2]))
    clock_brute = ctx.device_status()["sclk_mhz"]

    say()
    say("direct renderer: ms per launch | ns per 1000 executed steps | executed steps")
    for name, metric in metrics:
        def render():
            return ctx.render_direct(metric, cam, CAP, R, DELTA, download=False)[1]
        legs = (("S = 0", 0), ("S = %d" % S, S), ("S = 0 again", 0))
        for _, scale in legs:
            leg(render, scale)
        got = np.array([[leg(render, scale) for _, scale in legs] for _ in range(a.rounds)])
        med = np.median(got, axis=0)
        for k, (what, _) in enumerate(legs):
            say("  %-13s %-28s %9.4f ms %10.3f ns %14.0f steps" % (name, what, med[k, 0], med[k, 1], med[k, 2]))
        say("  %-13s per executed step %+.2f %% (the two S = 0 legs differ by %.2f %%); frame time %.4fx; executed steps %.4fx" % (
            name, 100.0 * (med[1, 1] / med[0, 1] - 1.0), 100.0 * abs(med[2, 1] / med[0, 1] - 1.0), med[1, 0] / med[0, 0], med[1, 2] / med[0, 2]))
    clock_direct = ctx.device_status()["sclk_mhz"]

    # fixed cost per ray against cost per step: every kernel at TWO step counts per ray (another escape radius; the kernels, the
    # camera and the rays are the same), so that time = A x rays + B x executed steps can be solved for each kernel on its own
    say()
    say("cost per ray (A) and per step (B) of each kernel from two escape radii, time = A x rays + B x executed steps:")
    say("  %-13s %-8s %-22s %9s %9s %12s %12s   %s" % ("", "", "kernel", "R", "ms", "steps / ray", "ns / 1000", "A ps per ray | B ns per 1000 steps"))
    radii = {0: (100.0, 20.0), S: (100.0, 10000.0)}
    for renderer in ("brute", "direct"):
        for name, metric in metrics:
            fit = {}
            for scale in (0, S):
                pts = []
                for radius in radii[scale]:
                    def render():
                        if renderer == "brute":
                            return ctx.render_brute(metric, cam, 1 << 20, radius, DELTA, download=False)[1]
                        return ctx.render_direct(metric, cam, 1 << 20, radius, DELTA, download=False)[1]
                    leg(render, scale, 1)
                    got = np.array([leg(render, scale, 1) for _ in range(a.rounds)])
                    ms, _, steps = np.median(got, axis=0)
                    pts.append((ms, steps))
                (m1, s1), (m2, s2) = pts
                B = (m1 - m2) / (s1 - s2)                     # ms per step
                A = (m1 - B * s1) / (W * H)                   # ms per ray
                fit[scale] = (A * 1e9, B * 1e9)
                for radius, (ms, steps) in zip(radii[scale], pts):
                    say("  %-13s %-8s %-22s %9g %9.4f %12.1f %12.3f   %s" % (
                        name, renderer, "S = %d%s" % (scale, "" if scale else " (static)"), radius, ms, steps / (W * H), ms * 1e9 / steps,
                        "A = %.0f | B = %.3f" % fit[scale] if radius == radii[scale][1] else ""))
            say("  %-13s %-8s per step, B(S = %d) over B(S = 0): %+.2f %% (two more VALU instructions: %+.2f %%); per ray, A: %.0f -> %.0f ps = %.1f -> %.1f steps' worth" % (
                name, renderer, S, 100.0 * (fit[S][1] / fit[0][1] - 1.0), 200.0 / VALU[name], fit[0][0], fit[S][0],
                fit[0][0] / fit[0][1], fit[S][0] / fit[S][1]))
    clock_fit = ctx.device_status()["sclk_mhz"]

    say()
    from refpaths import reference_path_file
    it = rendering.Interpolator.from_file(reference_path_file("path_through.csv"))
    times = np.linspace(it.min_time(), it.max_time(), a.frames, endpoint=False)
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 15.0, 43.0, 480, 270) for t in times]
    jobs = len({float(c.position[1]) for c in cams})      # one sampler job per distinct camera radius
    say("efficient renderer, device-resident sampler, %d poses of the fly-through path (%d jobs): ms of the sampler kernel per job | sampler steps" % (a.frames, jobs))
    ctx.set_option("device_sampler", 1)
    for name, metric in metrics:
        def render():
            return ctx.render_efficient(metric, cams, CAP, R, DELTA, 100, 100, 1e-5, 1e-5, download=False)[1]

        def sampler(scale):
            ctx.set_option("step_scale", scale)
            st = render()
            ctx.set_option("step_scale", 0)
            return st.integrate_ms / jobs, float(st.steps)
        for scale in (0, S, 0):
            sampler(scale)
        got = np.array([[sampler(0), sampler(S), sampler(0)] for _ in range(max(3, a.rounds // 2))])
        med = np.median(got, axis=0)
        say("  %-13s S = 0 %9.4f ms %14.0f steps | S = %d %9.4f ms %14.0f steps | S = 0 again %9.4f ms | time %.4fx, steps %.4fx" % (
            name, med[0, 0], med[0, 1], S, med[1, 0], med[1, 1], med[2, 0], med[1, 0] / med[0, 0], med[1, 1] / med[0, 1]))
    ctx.set_option("device_sampler", -1)
    after = ctx.device_status()
    say()
    say("shader clock (sysfs level, MHz): %s before, %s after the brute rounds, %s after the direct rounds, %s after the two-radius rounds, %s at the end; board power %s -> %s W" % (
        before["sclk_mhz"], clock_brute, clock_direct, clock_fit, after["sclk_mhz"], before["power_w"], after["power_w"]))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
