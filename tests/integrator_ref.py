"""Library option "integrator" = 1 (Heun's method): the definition in Python doubles, written from the option's paragraph in
include/curvis_hip.h, over the oracle's own Euler step.  With E(y, d) = cvo_update under CVO_CV,

  delta_k = step_scale_ref's step from l_k (delta itself at S = 0)
  y''     = E(E(y_k, delta_k), delta_k)                  both stages with the same delta_k
  y_k+1   = (y_k + y'') * 0.5                            t, l, theta, phi, p_l, p_theta: one add, one multiply each; p_t and p_phi are kept

followed by the reference's escape test on y_k+1 only.  The walk is a subclass of step_scale_ref.Walk, and each renderer's frame is
step_scale_ref's composition with that walk in place of its own.  Nothing here calls the product, and nothing is added to the oracle.
integrator = 0 runs step_scale_ref's walk itself."""
import contextlib
import ctypes as C

import numpy as np

import oracle_lib as O
import projection_ref as P
import step_scale_ref as SR

COUNTERS = SR.COUNTERS
R = SR.R
DELTA = 0.1                    # the Heun cases' step; one case keeps step_scale_ref's 0.05


class HeunWalk(SR.Walk):
    """step_scale_ref.Walk with Heun steps.  `log` collects, per finished run, the number of steps whose second stage started beyond
    the escape radius (the compositions make their walks themselves, so the count leaves through the class)"""
    log = []

    def __init__(self, metric):
        super().__init__(metric)
        # the same eight doubles as scalars: a frame makes a few hundred thousand steps
        self.cx, self.cp = (C.c_double * 4).from_buffer(self.x), (C.c_double * 4).from_buffer(self.p)

    def step(self, dk):
        """one Heun step of (self.x, self.p) in place; returns |l'| of the stage state"""
        cx, cp, update, mp, xp, pp = self.cx, self.cp, self.update, self.mp, self.xp, self.pp
        x0, x1, x2, x3 = cx[0], cx[1], cx[2], cx[3]
        p0, p1, p2, p3 = cp[0], cp[1], cp[2], cp[3]
        update(O.CV, mp, xp, pp, dk)
        stage_l = abs(cx[1])
        update(O.CV, mp, xp, pp, dk)
        cx[0] = (x0 + cx[0]) * 0.5
        cx[1] = (x1 + cx[1]) * 0.5
        cx[2] = (x2 + cx[2]) * 0.5
        cx[3] = (x3 + cx[3]) * 0.5
        cp[0] = p0
        cp[1] = (p1 + cp[1]) * 0.5
        cp[2] = (p2 + cp[2]) * 0.5
        cp[3] = p3
        return stage_l

    def run(self, delta, S, max_iter, max_radius, inner=None):
        """step_scale_ref.Walk.run with Heun steps: (code, Heun steps, steps taken with delta_k == delta, steps taken from |l| < inner)"""
        cx = self.cx
        if abs(cx[1]) > max_radius:
            return O.PANIC, 0, 0, 0
        k = SR.kappa(delta, S) if S else 0.0
        code, steps, plain, inside, beyond = O.NOT_ESCAPED, 0, 0, 0, 0
        while steps < max_iter:
            l = cx[1]
            dk = delta
            if S:
                a = abs(l) * k
                if a > delta:
                    dk = a
            plain += dk == delta
            if inner is not None and abs(l) < inner:
                inside += 1
            beyond += self.step(dk) > max_radius
            steps += 1
            if cx[1] > max_radius:
                code = O.POSITIVE
                break
            if cx[1] < -max_radius:
                code = O.NEGATIVE
                break
        HeunWalk.log.append(beyond)
        return code, steps, plain, inside


@contextlib.contextmanager
def walking(integrator):
    """step_scale_ref's compositions make their walk by the name Walk: for the duration, that name is the integrator's walk"""
    assert integrator in (0, 1)
    saved = SR.Walk
    SR.Walk = HeunWalk if integrator else saved
    HeunWalk.log = []
    try:
        yield HeunWalk.log
    finally:
        SR.Walk = saved


def compose_brute(integrator, *args):
    """step_scale_ref.compose_brute(*args) under the integrator, plus the per-ray count of second stages begun beyond the radius"""
    with walking(integrator) as log:
        out = SR.compose_brute(*args)
        beyond = np.array(log, np.int64).reshape(out[0].shape[:2]) if integrator else np.zeros(out[0].shape[:2], np.int64)
    return out + (beyond,)


def compose_direct(integrator, *args):
    with walking(integrator) as log:
        out = SR.compose_direct(*args)
        return out + (np.array(log, np.int64),)


def compose_efficient(integrator, *args):
    with walking(integrator) as log:
        out = SR.compose_efficient(*args)
        return out + (np.array(log, np.int64),)


_cache = {}


def expected(renderer, kind, pose, S, delta=DELTA, integrator=1, res=SR.RES, cap=4096, projection=P.PERSPECTIVE, skies="index",
             max_radius=R):
    """the composition for a scene, computed once, shared, read-only.  brute: (frame, counters, debug records, classes, beyond);
    direct: (frame, counters, evaluator, beyond); efficient: (frame, counters, table, evaluator, beyond)"""
    key = (renderer, kind, pose, S, delta, integrator, res, cap, projection, skies, max_radius)
    if key not in _cache:
        om = SR.metrics(kind)[0]
        oc = SR.cameras(pose, res)[0]
        sp, sn = SR.oracle_skies() if skies == "index" else SR.fine_oracle_skies()
        dirs = SR.world_dirs(oc, projection)
        if renderer == "brute":
            out = compose_brute(integrator, om, oc, dirs, sp, sn, cap, max_radius, delta, S)
        elif renderer == "direct":
            out = compose_direct(integrator, om, oc, dirs, sp, sn, cap, max_radius, delta, S)
        else:
            out = compose_efficient(integrator, om, oc, dirs, sp, sn, cap, max_radius, delta, S, SR.EFF["n0"], SR.EFF["maxit"],
                                    SR.EFF["t1"], SR.EFF["t2"])
        out[0].setflags(write=False)
        _cache[key] = out
    return _cache[key]


def expected_case(case, renderer="brute"):
    return expected(renderer, case["kind"], case["pose"], case["S"], case.get("delta", DELTA), 1, case.get("res", SR.RES),
                    case.get("cap", 4096), case.get("projection", 0), case.get("skies", "index"))


def assert_brute_classes(case, least=8):
    """what a brute case relies on, from the composition alone: step_scale_ref.assert_brute_classes' classes -- rays escaped to +l, to
    -l where the scene has a far side, capped ones where the case is about them, rays with plain steps, rays with scaled steps where
    the steps are scaled, Interstellar rays with steps inside the strict zone -- and rays whose second stage started beyond R"""
    _, st, _, classes, beyond = expected_case(case)
    who = (case["id"], st)
    assert st[2] >= least, who
    if case["kind"] != "flat":
        assert st[3] >= least, who
    if case.get("capped", False):
        assert st[4] >= least, who
    assert (classes[..., 0] > 0).sum() >= least, who
    if case["S"]:
        assert (classes[..., 1] > 0).sum() >= least, who
    else:
        assert (classes[..., 1] == 0).all(), who
    if case["kind"] == "interstellar":
        assert (classes[..., 2] > 0).sum() >= least, who
    assert (beyond > 0).sum() >= least, who + ("second stages begun beyond R", int((beyond > 0).sum()))


def assert_angle_classes(case, least=8):
    """the same for the evaluator of a direct or efficient composition"""
    out = expected_case(case, case["renderer"])
    f, beyond = out[-2], out[-1]
    c = np.array(f.classes)
    assert (c[:, 0] == O.POSITIVE).sum() >= least and (c[:, 0] == O.NEGATIVE).sum() >= least, case["id"]
    assert (c[:, 1] > 0).sum() >= least, case["id"]
    if case["S"]:
        assert (c[:, 2] > 0).sum() >= least, case["id"]
    if case["kind"] == "interstellar":
        assert (c[:, 3] > 0).sum() >= least, case["id"]
    assert (beyond > 0).sum() >= least, case["id"]
    assert out[1][2] >= least and out[1][3] >= least, (case["id"], out[1])     # pixels of both skies


def final_directions(metric, cam, dirs, delta, S, cap, max_radius, integrator):
    """the rays of dirs [..., 3] walked from the camera: (codes [n], unit sky directions of the final states [n, 3], steps [n]); the
    direction is formed for every ray, escaped or not (cvo_vector_to_direction of the state the walk ended in)"""
    L = O.lib()
    flat = dirs.reshape(-1, 3)
    codes, out, steps = np.zeros(len(flat), np.int64), np.zeros((len(flat), 3)), np.zeros(len(flat), np.int64)
    pos = np.array(cam.pos[:])
    w = (HeunWalk if integrator else SR.Walk)(metric)
    d = np.zeros(3)
    for i, v in enumerate(flat):
        L.cvo_new_photon(O.CV, w.mp, O._dp(pos), O._dp(np.ascontiguousarray(v)), w.xp, w.pp)
        codes[i], steps[i] = w.run(delta, S, cap, max_radius)[:2]
        L.cvo_vector_to_direction(O.CV, w.mp, w.pp, w.xp, O._dp(d))
        out[i] = d / np.sqrt(d @ d)
    return codes, out, steps


def angles_between(a, b):
    """angle between unit vectors, row by row, in radians"""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.einsum("ij,ij->i", a, b))
