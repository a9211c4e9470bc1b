#!/usr/bin/env python3
"""What distance-scaled Euler steps (option "step_scale", L0 = S / 256) do to the image, measured on the CPU with the oracle's own Euler
step under CVO_CV (no GPU), and written to profiles/step_scale_accuracy.txt (or --out).

For every pose, 48 x 27 rays of the default camera (focal 15, diagonal 43) are walked to |l| > 100 four or more ways: with the
reference's fixed step delta = 0.05 (cvo_escape_photon), and with delta_k = max(delta, |l_k| delta / L0) for each (delta, L0) pair
(cvo_update in the loop of tests/step_scale_ref.py, the composition the GPU tests compare with).  The yardstick is a fixed-step run
at delta = 0.05 / 32.  Error of a ray: the angle between its final sky direction (cvo_vector_to_direction) and the yardstick's, in
texels of an 8192-wide sky (2 pi / 8192 rad).  Rays that end on the other sky than the yardstick's, or do not escape, are counted
separately ("other") and left out of the percentiles.

Poses: BASELINE configs[1] (l = 5 on the equator, facing the throat), one frame of the reference's orbit path (its frames are one scene
up to a rotation about the polar axis) and three of its fly-through path; metrics: Ellis rho = 1 and Interstellar m = 0.1, a = 1e-4, rho = 1.

    python tools/step_scale_accuracy.py [--out FILE] [--res 48x27] [--yardstick 32]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O  # noqa: E402
import ref_compose as RC  # noqa: E402
import step_scale_ref as SR  # noqa: E402
from curvis_amd import rendering  # noqa: E402

R, DELTA = 100.0, 0.05
PAIRS = ((0.05, 4.0), (0.05, 2.0), (0.025, 2.0), (0.0125, 1.0))      # (delta, L0)
TEXEL = 2.0 * np.pi / 8192.0


def final_directions(metric, cam, dirs, delta, S, cap):
    """(escape codes [n], unit sky directions [n, 3], steps [n]) of the rays: fixed steps by the oracle's escape_photon, scaled ones by
    the composition's loop"""
    L = O.lib()
    flat = dirs.reshape(-1, 3)
    codes, out, steps = np.zeros(len(flat), np.int64), np.zeros((len(flat), 3)), np.zeros(len(flat), np.int64)
    pos = np.array(cam.pos[:])
    w = RC.Walk(RC.OracleStepper(metric))
    d = np.zeros(3)
    n = C.c_uint32(0)
    for i, v in enumerate(flat):
        L.cvo_new_photon(O.CV, w.mp, O._dp(pos), O._dp(np.ascontiguousarray(v)), w.xp, w.pp)
        if S == 0:
            codes[i] = L.cvo_escape_photon(O.CV, w.mp, w.xp, w.pp, delta, cap, R, C.byref(n))
            steps[i] = n.value
        else:
            codes[i], steps[i] = w.run(delta, S, 0, cap, R)[:2]
        if codes[i] in (O.POSITIVE, O.NEGATIVE):
            L.cvo_vector_to_direction(O.CV, w.mp, w.pp, w.xp, O._dp(d))
            out[i] = d / np.sqrt(d @ d)
    return codes, out, steps


def errors(codes, dirs, ref_codes, ref_dirs):
    ok = (codes == ref_codes) & (ref_codes != O.NOT_ESCAPED)
    cross = np.linalg.norm(np.cross(dirs[ok], ref_dirs[ok]), axis=1)
    dot = np.einsum("ij,ij->i", dirs[ok], ref_dirs[ok])
    return np.arctan2(cross, dot) / TEXEL, int((~ok).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_scale_accuracy.txt"))
    ap.add_argument("--res", default="48x27")
    ap.add_argument("--yardstick", type=int, default=32)
    a = ap.parse_args()
    res = tuple(int(v) for v in a.res.split("x"))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from refpaths import reference_path_file
    poses = [("configs[1]: l = 5, equator, facing the throat", (0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0))]
    # (every frame of the orbit is the same scene up to a rotation about the polar axis -- l = 3 on the equator, facing the throat --:
    # one frame of it, and three of the fly-through)
    for name, fracs in (("path_orbit.csv", (0.25,)), ("path_through.csv", (0.1, 0.25, 0.7))):
        it = rendering.Interpolator.from_file(reference_path_file(name))
        for frac in fracs:
            t = it.min_time() + frac * (it.max_time() - it.min_time())
            p = it.camera_position(t)
            poses.append(("%s at %.0f %% (l = %.3f, theta = %.3f)" % (name, 100 * frac, p[1], p[2]), tuple(p), tuple(it.camera_forward(t)),
                          tuple(it.camera_up(t))))
    say("step_scale accuracy: %d x %d rays per pose, R = %g, oracle CVO_CV; error in texels of an 8192-wide sky against fixed delta = %g / %d" % (
        res[0], res[1], R, DELTA, a.yardstick))
    say("scaled: delta_k = max(delta, |l_k| delta / L0), step_scale = 256 L0; 'other': rays on another sky than the yardstick's, or not escaped (not in the percentiles)")
    table = {}
    for kind in ("ellis", "interstellar"):
        om = O.ellis(1.0) if kind == "ellis" else O.interstellar(0.1, 1e-4, 1.0)
        for what, pos, fwd, up in poses:
            oc = O.camera(pos, fwd, up, 15.0, 43.0, res)
            dirs = SR.world_dirs(oc)
            ref_codes, ref_dirs, _ = final_directions(om, oc, dirs, DELTA / a.yardstick, 0, 1 << 24)
            say()
            say("%s, %s" % (kind, what))
            say("  %-34s %12s %10s %10s %10s %6s" % ("integration", "mean steps", "median", "p90", "max", "other"))
            runs = [("fixed delta = 0.05 (the reference)", DELTA, 0)] + [("delta = %g, L0 = %g" % (d, l0), d, int(l0 * 256)) for d, l0 in PAIRS]
            for label, delta, S in runs:
                codes, out, steps = final_directions(om, oc, dirs, delta, S, 1 << 20)
                err, other = errors(codes, out, ref_codes, ref_dirs)
                row = (steps.mean(), np.median(err), np.percentile(err, 90), err.max(), other)
                table.setdefault(label, []).append(row)
                say("  %-34s %12.1f %10.2f %10.2f %10.1f %6d" % ((label,) + row))
    say()
    say("ranges over the %d poses x 2 metrics" % len(poses))
    say("  %-34s %17s %15s %17s %19s %8s" % ("integration", "mean steps", "median", "p90", "max", "other"))
    for label, rows in table.items():
        r = np.array(rows)
        say("  %-34s %8.0f-%-8.0f %7.1f-%-7.1f %8.1f-%-8.1f %9.0f-%-9.0f %3d-%-3d" % (
            label, r[:, 0].min(), r[:, 0].max(), r[:, 1].min(), r[:, 1].max(), r[:, 2].min(), r[:, 2].max(), r[:, 3].min(), r[:, 3].max(),
            int(r[:, 4].min()), int(r[:, 4].max())))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
