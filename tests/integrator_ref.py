"""Library option "integrator" = 1 (Heun's method): the definition, written from the option's paragraph in include/curvis_hip.h, over
the oracle's own Euler step.  With E(y, d) = cvo_update under CVO_CV,

  delta_k = step_scale_ref's step from l_k (delta itself at S = 0)
  y''     = E(E(y_k, delta_k), delta_k)                  both stages with the same delta_k
  y_k+1   = (y_k + y'') * 0.5                            t, l, theta, phi, p_l, p_theta: one add, one multiply each; p_t and p_phi are kept

followed by the reference's escape test on y_k+1 only.  The update is ref_compose.Walk.heun, in Python doubles, and each renderer's frame
is step_scale_ref's composition with integrator = 1, which also hands out, per ray, the number of second stages begun beyond the escape
radius.  Nothing here calls the product, and nothing is added to the oracle."""
import numpy as np

import oracle_lib as O
import projection_ref as P
import ref_compose as RC
import step_scale_ref as SR

COUNTERS = SR.COUNTERS
R = SR.R
DELTA = 0.1                    # the Heun cases' step; one case keeps step_scale_ref's 0.05
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
            out = SR.brute(om, oc, dirs, sp, sn, cap, max_radius, delta, S, integrator)
        elif renderer == "direct":
            out = SR.direct(om, oc, dirs, sp, sn, cap, max_radius, delta, S, integrator)
        else:
            out = SR.efficient(om, oc, dirs, sp, sn, cap, max_radius, delta, S, SR.EFF["n0"], SR.EFF["maxit"], SR.EFF["t1"], SR.EFF["t2"],
                               integrator)
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
    flat = dirs.reshape(-1, 3)
    codes, out, steps = np.zeros(len(flat), np.int64), np.zeros((len(flat), 3)), np.zeros(len(flat), np.int64)
    pos = np.array(cam.pos[:])
    st = RC.OracleStepper(metric)
    w = RC.Walk(st)
    d = np.zeros(3)
    for i, v in enumerate(flat):
        st.new_photon(pos, v)
        codes[i], steps[i] = w.run(delta, S, integrator, cap, max_radius)[:2]
        st.direction(d)
        out[i] = d / np.sqrt(d @ d)
    return codes, out, steps


def angles_between(a, b):
    """angle between unit vectors, row by row, in radians"""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.einsum("ij,ij->i", a, b))
