#!/usr/bin/env python3
"""What Heun's method (option "integrator" = 1) does to the image beside the Euler step, with and without distance-scaled steps (option
"step_scale", L0 = S / 256), measured on the CPU with the oracle's own Euler step under CVO_CV (no GPU), and written to
profiles/integrator_accuracy.txt (or --out).

Poses, size, metrics and error measure are those of tools/step_scale_accuracy.py: for every pose, 48 x 27 rays of the default camera
(focal 15, diagonal 43) are walked to |l| > 100; error of a ray: the angle between its final sky direction (cvo_vector_to_direction)
and the yardstick's, in texels of an 8192-wide sky (2 pi / 8192 rad); rays that end on the other sky than the yardstick's, or do not
escape, are counted separately ("other") and left out of the percentiles.  Two things differ: the yardstick is a fixed-step HEUN run at
delta = 0.05 / 32 (second order: its own error is about a thousandth of the Euler yardstick's), and the rows are the Euler rows of that
tool plus Heun at delta in {0.05, 0.1, 0.2} x L0 in {off, 4, 2}.  Work is counted in EVALUATIONS of the right-hand side per ray: one
per Euler step, two per Heun step.  The walks are the compositions the GPU tests compare with (tests/step_scale_ref.py,
tests/integrator_ref.py).

    python tools/integrator_accuracy.py [--out FILE] [--res 48x27] [--yardstick 32] [--jobs 8]"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import integrator_ref as IR  # noqa: E402
import oracle_lib as O  # noqa: E402
import step_scale_ref as SR  # noqa: E402
from curvis_amd import rendering  # noqa: E402

R, DELTA = 100.0, 0.05
TEXEL = 2.0 * np.pi / 8192.0
# (label, integrator, delta, L0 or None)
ROWS = [("Euler delta = 0.05 (the reference)", 0, 0.05, None), ("Euler delta = 0.05, L0 = 4", 0, 0.05, 4.0), ("Euler delta = 0.05, L0 = 2", 0, 0.05, 2.0),
        ("Euler delta = 0.025, L0 = 2", 0, 0.025, 2.0)]
ROWS += [("Heun delta = %g, %s" % (d, "fixed" if l0 is None else "L0 = %g" % l0), 1, d, l0) for d in (0.05, 0.1, 0.2) for l0 in (None, 4.0, 2.0)]


def poses():
    from refpaths import reference_path_file
    out = [("configs[1]: l = 5, equator, facing the throat", (0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0))]
    for name, fracs in (("path_orbit.csv", (0.25,)), ("path_through.csv", (0.1, 0.25, 0.7))):
        it = rendering.Interpolator.from_file(reference_path_file(name))
        for frac in fracs:
            t = it.min_time() + frac * (it.max_time() - it.min_time())
            p = it.camera_position(t)
            out.append(("%s at %.0f %% (l = %.3f, theta = %.3f)" % (name, 100 * frac, p[1], p[2]), tuple(float(v) for v in p),
                        tuple(float(v) for v in it.camera_forward(t)), tuple(float(v) for v in it.camera_up(t))))
    return out


def errors(codes, dirs, ref_codes, ref_dirs):
    ok = (codes == ref_codes) & (ref_codes != O.NOT_ESCAPED)
    return IR.angles_between(dirs[ok], ref_dirs[ok]) / TEXEL, int((~ok).sum())


def one_scene(job):
    """every row of one metric x pose: [(label, evaluations per ray, median, p90, max, other)]"""
    kind, (what, pos, fwd, up), res, yardstick = job
    om = O.ellis(1.0) if kind == "ellis" else O.interstellar(0.1, 1e-4, 1.0)
    oc = O.camera(pos, fwd, up, 15.0, 43.0, res)
    dirs = SR.world_dirs(oc)
    ref_codes, ref_dirs, _ = IR.final_directions(om, oc, dirs, DELTA / yardstick, 0, 1 << 24, R, 1)
    rows = []
    for label, integrator, delta, l0 in ROWS:
        codes, out, steps = IR.final_directions(om, oc, dirs, delta, int(l0 * 256) if l0 else 0, 1 << 20, R, integrator)
        err, other = errors(codes, out, ref_codes, ref_dirs)
        rows.append((label, float(steps.mean()) * (2 if integrator else 1), float(np.median(err)), float(np.percentile(err, 90)), float(err.max()), other))
    return kind, what, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrator_accuracy.txt"))
    ap.add_argument("--res", default="48x27")
    ap.add_argument("--yardstick", type=int, default=32)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    res = tuple(int(v) for v in a.res.split("x"))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ps = poses()
    say("integrator accuracy: %d x %d rays per pose, R = %g, oracle CVO_CV; error in texels of an 8192-wide sky against fixed-step Heun at delta = %g / %d" % (
        res[0], res[1], R, DELTA, a.yardstick))
    say("scaled: delta_k = max(delta, |l_k| delta / L0), step_scale = 256 L0; evaluations: of the right-hand side per ray, 1 per Euler step, 2 per Heun step;")
    say("'other': rays on another sky than the yardstick's, or not escaped (not in the percentiles)")
    jobs = [(kind, pose, res, a.yardstick) for kind in ("ellis", "interstellar") for pose in ps]
    with multiprocessing.Pool(max(1, min(a.jobs, len(jobs)))) as pool:
        done = pool.map(one_scene, jobs, chunksize=1)
    table = {}
    for kind, what, rows in done:
        say()
        say("%s, %s" % (kind, what))
        say("  %-36s %12s %10s %10s %10s %6s" % ("integration", "evaluations", "median", "p90", "max", "other"))
        for row in rows:
            table.setdefault(row[0], []).append(row[1:])
            say("  %-36s %12.1f %10.3f %10.3f %10.1f %6d" % row)
    say()
    say("ranges over the %d poses x 2 metrics" % len(ps))
    say("  %-36s %17s %17s %17s %19s %8s" % ("integration", "evaluations", "median", "p90", "max", "other"))
    for label, rows in table.items():
        r = np.array(rows)
        say("  %-36s %8.0f-%-8.0f %8.3f-%-8.3f %8.3f-%-8.3f %9.1f-%-9.1f %3d-%-3d" % (
            label, r[:, 0].min(), r[:, 0].max(), r[:, 1].min(), r[:, 1].max(), r[:, 2].min(), r[:, 2].max(), r[:, 3].min(), r[:, 3].max(),
            int(r[:, 4].min()), int(r[:, 4].max())))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
