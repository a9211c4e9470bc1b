"""Library option "step_scale" (an integer S; L0 = S / 256): the definition in Python doubles, written from the option's paragraph in
include/curvis_hip.h, and each renderer's frame composed per ray by tests/ref_compose.py from primitives of the CPU oracle that exist
already.  Nothing here calls the product, and nothing is added to the oracle.

  kappa   = RN(delta / L0)                       one IEEE division per call
  a       = RN(|l_k| kappa)                      l_k: the radial coordinate BEFORE step k
  delta_k = a if a > delta else delta            (a NaN l_k fails the compare)
and step k is the oracle's own Euler step cvo_update(..., delta_k) under CVO_CV, followed by the reference's escape test.  S = 0 means
delta_k = delta: then every composition below is the oracle's own entry point bit for bit (tests/test_step_scale_host.py pins that
before anything here is trusted)."""
import ctypes as C
import math

import numpy as np

import oracle_lib as O
import projection_ref as P
import ref_compose as RC

COUNTERS = P.COUNTERS
S_MAX = 1 << 20


def kappa(delta, S):
    return delta / (float(S) / 256.0)


def step_delta(delta, S, l, k=None):
    """delta_k of the definition (Python floats are IEEE doubles; one multiply, one compare)"""
    if S == 0:
        return delta
    a = abs(l) * (kappa(delta, S) if k is None else k)
    return a if a > delta else delta


def strict_radius(metric):
    """Interstellar: the fast step's guard sends |l| < a + pi m to the strict step"""
    return metric.a + math.pi * metric.m if metric.kind == O.INTERSTELLAR else None


def evaluator(metric, l, delta, S, max_iter, max_radius, integrator=0):
    """ref_compose's escape-angle evaluator over the oracle's stepper, counting the strict zone's steps"""
    return RC.EscapeAngle(RC.OracleStepper(metric), l, delta, S, integrator, max_iter, max_radius, strict_radius(metric))


def _texel_of(sky_pos, sky_neg):
    tx, ty = C.c_uint32(0), C.c_uint32(0)

    def texel(code, d):
        O.lib().cvo_sky_indices(O.CV, C.byref(sky_pos if code == O.POSITIVE else sky_neg), O._dp(d), C.byref(tx), C.byref(ty))
        return tx.value, ty.value
    return texel


def brute(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta, S, integrator=0):
    """the brute renderer's frame with scaled steps: (frame, counters, debug records [H, W] of O.RAY_DEBUG, classes -- per ray (plain
    steps, scaled steps, strict-zone steps) --, per ray the Heun second stages begun beyond the radius)"""
    rays = RC.compose_brute(RC.OracleStepper(metric), cam.pos, dirs, max_iter, max_radius, delta, S, integrator, inner=strict_radius(metric))
    rgb, cnt = RC.frame_nearest(rays, None, (sky_pos, sky_neg))
    classes = np.stack([rays["plain"], rays["steps"] - rays["plain"], rays["inside"]], axis=-1)
    return rgb, cnt[:6], RC.debug_records(rays, O.RAY_DEBUG, _texel_of(sky_pos, sky_neg)), classes, rays["beyond"]


def direct(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta, S, integrator=0):
    """"direct" mode with scaled steps: (frame, counters, evaluator, per call the Heun second stages begun beyond the radius)"""
    f = evaluator(metric, cam.pos[1], delta, S, max_iter, max_radius, integrator)
    rgb, cnt = RC.frame_nearest(RC.compose_direct(f, cam, dirs), None, (sky_pos, sky_neg))
    return rgb, cnt[:6], f, np.array(f.beyond, np.int64)


def efficient(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta, S, alpha_nums, max_it_sampling, thr1, thr2, integrator=0):
    """render_image_efficient with scaled steps in its sampler: (frame, counters -- steps are the sampler's --, table, evaluator, per call
    the Heun second stages begun beyond the radius)"""
    f = evaluator(metric, cam.pos[1], delta, S, max_iter, max_radius, integrator)
    table = RC.sample_table(f, alpha_nums, max_it_sampling, thr1, thr2)
    rgb, cnt = RC.frame_nearest(RC.compose_efficient(table, cam, dirs), None, (sky_pos, sky_neg), f.steps)
    return rgb, cnt[:6], table, f, np.array(f.beyond, np.int64)


box_average = RC.box_average


# ---- the scenes of the GPU tests ---------------------------------------------------------------------------------------------------
R, DELTA = 30.0, 0.05
SKY_SHAPES = ((1000, 500), (333, 777))      # +l, -l (w, h)
SKY_SALTS = (0x5C3A71, 0x1BE4D2)
RES, RES_RAGGED = (40, 24), (37, 19)
EFF = dict(n0=100, maxit=100, t1=1e-5, t2=1e-5)
HALF_PI = np.pi / 2
# name -> (metric, position, forward, up, focal)
POSES = {
    "facing": ((0.0, 5.0, HALF_PI, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0),
    "tilted": ((0.0, 3.0, 0.9, 0.4), (-1.0, 0.1, 0.6), (0.0, 0.0, 1.0), 9.0),          # rays cross the poles
    "negative": ((0.0, -4.0, HALF_PI, 0.3), (1.0, 0.05, 0.1), (0.0, 0.0, 1.0), 12.0),
    "inside": ((0.0, 0.3, 1.2, 0.0), (-0.2, 1.0, 0.1), (0.0, 0.0, 1.0), 10.0),          # starts inside L0, looks across the throat
}
INTERSTELLAR = (0.5, 2.0, 1.0)              # m, a, rho: a throat long enough that strict steps (|l| < a + pi m) occur
_cache = {}


def metrics(kind):
    """(oracle metric, product metric)"""
    import curvis_amd
    if kind == "ellis":
        return O.ellis(1.0), curvis_amd.EllisMetric(1.0)
    if kind == "interstellar":
        return O.interstellar(*INTERSTELLAR), curvis_amd.InterstellarMetric(*INTERSTELLAR)
    return O.flat(), curvis_amd.FlatSphericalMetric()


def cameras(pose, res):
    """(oracle camera, product camera)"""
    import curvis_amd
    pos, fwd, up, focal = POSES[pose]
    return O.camera(pos, fwd, up, focal, 43.0, res), curvis_amd.Camera(pos, fwd, up, focal, 43.0, res[0], res[1])


def index_skies():
    return RC.index_skies(SKY_SHAPES, SKY_SALTS)


def oracle_skies():
    if "oskies" not in _cache:
        _cache["oskies"] = tuple(O.sky(np.array(t)) for t in index_skies())
    return _cache["oskies"]


def world_dirs(oc, projection=P.PERSPECTIVE):
    return P.outward_vectors(oc, projection)[1]


def fine_oracle_skies():
    """option "sky_filter": the index skies of 256 w x 256 h texels that tests/sky_filter_ref.py decodes the filter's taps from"""
    import sky_filter_ref as F
    if "ofine" not in _cache:
        _cache["ofine"] = tuple(O.sky(img) for img in F.fine_skies())
    return _cache["ofine"]


def expected(renderer, kind, pose, S, res=RES, cap=4096, projection=P.PERSPECTIVE, skies="index", max_radius=R):
    """the composition for a scene (skies: "index", or "fine" for the filter's virtual skies); computed once, shared, read-only"""
    key = (renderer, kind, pose, S, res, cap, projection, skies, max_radius)
    if key not in _cache:
        om = metrics(kind)[0]
        oc = cameras(pose, res)[0]
        sp, sn = oracle_skies() if skies == "index" else fine_oracle_skies()
        dirs = world_dirs(oc, projection)
        if renderer == "brute":
            out = brute(om, oc, dirs, sp, sn, cap, max_radius, DELTA, S)[:4]
        elif renderer == "direct":
            out = direct(om, oc, dirs, sp, sn, cap, max_radius, DELTA, S)[:3]
        else:
            out = efficient(om, oc, dirs, sp, sn, cap, max_radius, DELTA, S, EFF["n0"], EFF["maxit"], EFF["t1"], EFF["t2"])[:4]
        out[0].setflags(write=False)
        _cache[key] = out
    return _cache[key]


def assert_brute_classes(kind, pose, S, res=RES, cap=4096, projection=P.PERSPECTIVE, skies="index", capped=False, neg=True, least=8):
    """what a brute case relies on, from the composition alone: at least 8 rays escaped to +l, to -l (where the scene has a far side),
    capped ones where the case is about them, rays with plain steps and rays with scaled steps, and -- Interstellar -- rays with
    steps inside the strict zone"""
    _, st, dbg, classes = expected("brute", kind, pose, S, res, cap, projection, skies)
    who = (kind, pose, S, res, cap, st)
    assert st[2] >= least, who
    if neg:
        assert st[3] >= least, who
    if capped:
        assert st[4] >= least, who
    assert (classes[..., 0] > 0).sum() >= least and (classes[..., 1] > 0).sum() >= least, who
    if kind == "interstellar":
        assert (classes[..., 2] > 0).sum() >= least, who


def assert_angle_classes(f, kind, least=8, neg=True):
    """the same for the evaluator of a direct or efficient composition"""
    c = np.array(f.classes)
    assert (c[:, 0] == O.POSITIVE).sum() >= least, kind
    if neg:
        assert (c[:, 0] == O.NEGATIVE).sum() >= least, kind
    assert (c[:, 1] > 0).sum() >= least and (c[:, 2] > 0).sum() >= least, kind
    if kind == "interstellar":
        assert (c[:, 3] > 0).sum() >= least, kind
