#!/usr/bin/env python3
"""What Heun's method (option "integrator" = 1) costs on the GPU beside the Euler kernels, measured in ONE process with the settings
interleaved, and written to profiles/integrator_cost.txt (or --out).  Skies: the benchmark's procedural 8192 x 4096 pair.  The baseline
of every figure is a kernel that exists without the option, run in the same rounds: integrator = 0 with step_scale = 0 (the static
kernel, variant = 1) and integrator = 0 with step_scale = S (the ADAPT = 1 kernels).

  * brute renderer, 1080p, camera at l = 5 facing the throat, cap 4096, R = 100: configs[1] of BASELINE.json (Ellis rho = 1) and the same
    frame under the Interstellar metric (m = 0.1, a = 1e-4, rho = 1).  Legs per round: Euler delta = 0.05 S = 0; Euler delta = 0.05 S;
    Heun delta = 0.1 S; Heun delta = 0.05 S = 0; Euler delta = 0.05 S = 0 again.  Per leg: ms per launch by HIP events, executed
    EVALUATIONS of the right-hand side (steps, twice the steps under Heun) and ns per 1000 of them.
  * direct renderer, the same two frames, the same legs.
  * efficient renderer's sampler: ms of the sampler kernel per job (distinct camera radius) of a call over the poses of the reference's
    fly-through path, device-resident sampler, the same legs.
  * where a Heun evaluation costs more than the expectation (two steps plus 8 to 10 VALU instructions per 166 to 226: about +5 %):
    brute and direct at two escape radii each, solved for time = A x rays + B x evaluations.

Every figure is reported as measured, next to the spread between the two identical legs.  There is no pass threshold.

    python tools/gpu_integrator_cost.py [--out FILE] [--rounds 7] [--frames 64] [--scale 1024]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import curvis_amd  # noqa: E402
from curvis_amd import rendering, skies  # noqa: E402

W, H, CAP, R = 1920, 1080, 4096, 100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrator_cost.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--scale", type=int, default=1024)
    a = ap.parse_args()
    S = a.scale
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # (label, integrator, delta, step_scale)
    LEGS = (("Euler delta = 0.05, S = 0", 0, 0.05, 0), ("Euler delta = 0.05, S = %d" % S, 0, 0.05, S), ("Heun  delta = 0.1,  S = %d" % S, 1, 0.1, S),
            ("Heun  delta = 0.05, S = 0", 1, 0.05, 0), ("Euler delta = 0.05, S = 0 again", 0, 0.05, 0))

    ctx = curvis_amd.Context(0)
    info, before = ctx.device_info(), ctx.device_status()
    say("integrator cost on %s (PCI %s); medians of %d interleaved rounds after one warm-up round" % (info["name"], before["pci_bus_id"], a.rounds))
    say("1080p, camera at l = 5, focal 15, diagonal 43, cap %d, R = %g; S = %d is L0 = %g; skies 8192 x 4096 (skies.smooth, the benchmark's)" % (
        CAP, R, S, S / 256.0))
    say("evaluations = executed steps under Euler, twice the executed steps under Heun; brute S = 0 Euler runs the static kernel (variant = 1)")
    ctx.set_sky(0, curvis_amd.SphericalImage(skies.smooth(8192, 4096, 128)))
    ctx.set_sky(1, curvis_amd.SphericalImage(skies.smooth(8192, 4096, 32)))
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, W, H)
    metrics = (("Ellis", curvis_amd.EllisMetric(1.0)), ("Interstellar", curvis_amd.InterstellarMetric(0.1, 1e-4, 1.0)))

    def leg(render, integrator, delta, scale, ms_of=lambda st: st.kernel_ms):
        ctx.set_option("integrator", integrator)
        ctx.set_option("step_scale", scale)
        ctx.set_option("variant", 1)
        st = render(delta)
        ctx.set_option("variant", -1)
        ctx.set_option("step_scale", 0)
        ctx.set_option("integrator", 0)
        evals = float(st.steps) * (2 if integrator else 1)
        ms = ms_of(st)
        return ms, ms * 1e9 / max(evals, 1.0), evals          # ms; ns per 1000 evaluations; evaluations

    def rounds(render, n, ms_of=lambda st: st.kernel_ms):
        for _, integrator, delta, scale in LEGS:
            leg(render, integrator, delta, scale, ms_of)
        got = np.array([[leg(render, integrator, delta, scale, ms_of) for _, integrator, delta, scale in LEGS] for _ in range(n)])
        return np.median(got, axis=0)

    def report(name, med, unit="ms per launch"):
        for k, (what, _, _, _) in enumerate(LEGS):
            say("  %-13s %-32s %9.4f ms %10.3f ns %14.0f evaluations" % (name, what, med[k, 0], med[k, 1], med[k, 2]))
        spread = 100.0 * abs(med[4, 0] / med[0, 0] - 1.0)
        say("  %-13s per evaluation: Heun S = %d over Euler S = %d %+.2f %%; Heun S = 0 over Euler S = 0 %+.2f %% (the two Euler S = 0 legs differ by %.2f %%)" % (
            name, S, S, 100.0 * (med[2, 1] / med[1, 1] - 1.0), 100.0 * (med[3, 1] / med[0, 1] - 1.0), spread))
        say("  %-13s %s: Heun 0.1 / S = %d is %.4fx of Euler 0.05 / S = %d and %.4fx of Euler 0.05 / S = 0; Heun 0.05 / S = 0 is %.4fx of Euler 0.05 / S = 0" % (
            name, unit, S, med[2, 0] / med[1, 0], S, med[2, 0] / med[0, 0], med[3, 0] / med[0, 0]))
        return 100.0 * (med[2, 1] / med[1, 1] - 1.0), 100.0 * (med[3, 1] / med[0, 1] - 1.0)

    over = {}
    say()
    say("brute renderer: ms per launch | ns per 1000 evaluations | evaluations")
    for name, metric in metrics:
        over["brute", name] = report(name, rounds(lambda delta: ctx.render_brute(metric, cam, CAP, R, delta, download=False)[1], a.rounds))
    clock_brute = ctx.device_status()["sclk_mhz"]

    say()
    say("direct renderer: ms per launch | ns per 1000 evaluations | evaluations")
    for name, metric in metrics:
        over["direct", name] = report(name, rounds(lambda delta: ctx.render_direct(metric, cam, CAP, R, delta, download=False)[1], a.rounds))
    clock_direct = ctx.device_status()["sclk_mhz"]

    say()
    from refpaths import reference_path_file
    it = rendering.Interpolator.from_file(reference_path_file("path_through.csv"))
    times = np.linspace(it.min_time(), it.max_time(), a.frames, endpoint=False)
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 15.0, 43.0, 480, 270) for t in times]
    jobs = len({float(c.position[1]) for c in cams})      # one sampler job per distinct camera radius
    say("efficient renderer, device-resident sampler, %d poses of the fly-through path (%d jobs): ms of the sampler kernel per job | ns per 1000 evaluations | evaluations" % (
        a.frames, jobs))
    ctx.set_option("device_sampler", 1)
    for name, metric in metrics:
        report(name, rounds(lambda delta: ctx.render_efficient(metric, cams, CAP, R, delta, 100, 100, 1e-5, 1e-5, download=False)[1],
                            max(3, a.rounds // 2), lambda st: st.integrate_ms / jobs), "ms per job")
    ctx.set_option("device_sampler", -1)
    clock_sampler = ctx.device_status()["sclk_mhz"]

    # a Heun evaluation above the expectation: what is per ray and what is per evaluation, from two escape radii per kernel
    say()
    say("cost per ray (A) and per evaluation (B) from two escape radii, time = A x rays + B x evaluations, fixed steps (S = 0), delta = 0.05:")
    say("  %-13s %-8s %-8s %9s %9s %14s %12s   %s" % ("", "", "kernel", "R", "ms", "evals / ray", "ns / 1000", "A ps per ray | B ns per 1000 evaluations"))
    for renderer in ("brute", "direct"):
        for name, metric in metrics:
            fit = {}
            for integrator in (0, 1):
                pts = []
                for radius in (100.0, 20.0):
                    def render(delta):
                        if renderer == "brute":
                            return ctx.render_brute(metric, cam, 1 << 20, radius, delta, download=False)[1]
                        return ctx.render_direct(metric, cam, 1 << 20, radius, delta, download=False)[1]
                    leg(render, integrator, 0.05, 0)
                    got = np.array([leg(render, integrator, 0.05, 0) for _ in range(a.rounds)])
                    ms, _, evals = np.median(got, axis=0)
                    pts.append((ms, evals))
                (m1, e1), (m2, e2) = pts
                B = (m1 - m2) / (e1 - e2)
                A = (m1 - B * e1) / (W * H)
                fit[integrator] = (A * 1e9, B * 1e9)
                for radius, (ms, evals) in zip((100.0, 20.0), pts):
                    say("  %-13s %-8s %-8s %9g %9.4f %14.1f %12.3f   %s" % (
                        name, renderer, "Heun" if integrator else "Euler", radius, ms, evals / (W * H), ms * 1e9 / evals,
                        "A = %.0f | B = %.3f" % fit[integrator] if radius == 20.0 else ""))
            say("  %-13s %-8s per evaluation, B(Heun) over B(Euler): %+.2f %%; per ray, A: %.0f -> %.0f ps (whole-launch figure above: %+.2f %%)" % (
                name, renderer, 100.0 * (fit[1][1] / fit[0][1] - 1.0), fit[0][0], fit[1][0], over[renderer, name][1]))
    after = ctx.device_status()
    say()
    say("shader clock (sysfs level, MHz): %s before, %s after the brute rounds, %s after the direct rounds, %s after the sampler rounds, %s at the end; board power %s -> %s W" % (
        before["sclk_mhz"], clock_brute, clock_direct, clock_sampler, after["sclk_mhz"], before["power_w"], after["power_w"]))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
