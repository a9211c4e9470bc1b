"""The moving camera (curvis_ctx_set_camera_velocities), the parts that need no GPU: curvis_camera_boost_prepare and
curvis_camera_outward_vector_boosted against the definition in numpy (tests/camera_boost_ref.py), bit for bit; zero velocity against
curvis_camera_outward_vector_projected; the refusals; the aberration formula in closed form at 50 digits; a boost along the optical
axis; curvis_camera_path_velocity against its restatement on rows of both committed camera paths; the Python keywords."""
import ctypes as C
import inspect

import mpmath
import numpy as np
import pytest

import camera_boost_ref as B
import common
import oracle_lib as O
import projection_ref as P
import refpaths
import curvis_amd
from curvis_amd import _abi, rendering, systems

VELOCITIES = (B.VELOCITY, B.VELOCITY_PHI, (-0.6, 0.2, 0.0))
DP = C.POINTER(C.c_double)


def _dp(a):
    return a.ctypes.data_as(DP)


def prepare(pc, beta):
    out = np.full(5, 7.0)
    rc = _abi.lib().curvis_camera_boost_prepare(C.byref(pc._c), _dp(np.array(beta, dtype=np.float64)), _dp(out))
    return rc, out


def boosted(pc, projection, beta, px, py):
    """the ABI function over pixel lists: (camera space [n, 3], world space [n, 3])"""
    f = _abi.lib().curvis_camera_outward_vector_boosted
    b = np.array(beta, dtype=np.float64)
    cs, ws = np.zeros((len(px), 3)), np.zeros((len(px), 3))
    for k in range(len(px)):
        assert f(C.byref(pc._c), projection, _dp(b), int(px[k]), int(py[k]), C.cast(cs.ctypes.data + 24 * k, DP), C.cast(ws.ctypes.data + 24 * k, DP)) == 0
    return cs, ws


# ---- 1. the two accessors are the definition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("projection", (P.PERSPECTIVE, P.EQUIRECTANGULAR, P.FISHEYE), ids=P.NAMES)
def test_accessors_are_the_definition(projection):
    size = B.RES[projection]
    _, oc, _, pc = P.scene("ellis", size)                # a tilted camera
    px, py = (a.reshape(-1) for a in P.pixel_grid(oc))
    if projection == P.FISHEYE:
        assert P.pixel_vectors(oc, projection, np.array([10]), np.array([7]))[0].tolist() == [1.0, 0.0, 0.0]      # the axis pixel is in
    for beta in VELOCITIES:
        want_K = B.boost_prepare(oc.rot[:], beta)
        rc, K = prepare(pc, beta)
        assert rc == 0 and common.bits(K).tobytes() == common.bits(want_K).tobytes(), (beta, K.tolist(), want_K.tolist())
        assert K[4] > 0.0
        want_cs, want_ws = B.outward_vectors(oc, projection, beta, px, py)
        cs, ws = boosted(pc, projection, beta, px, py)
        for got, want, name in ((cs, want_cs, "camera space"), (ws, want_ws, "world space")):
            bad = np.nonzero((common.bits(got) != common.bits(want)).any(axis=1))[0]
            assert len(bad) == 0, (P.NAMES[projection], name, beta, len(bad), [(int(px[i]), int(py[i]), got[i].tolist(), want[i].tolist()) for i in bad[:3]])
        still = P.outward_vectors(oc, projection, px, py)[0]
        assert (common.bits(cs) != common.bits(still)).any(axis=1).sum() > len(px) // 2       # the velocity does something


def test_zero_velocity_is_the_projected_vector():
    f = _abi.lib().curvis_camera_outward_vector_projected
    for projection in (P.PERSPECTIVE, P.EQUIRECTANGULAR, P.FISHEYE):
        _, oc, _, pc = P.scene("interstellar", B.RES[projection])
        px, py = (a.reshape(-1) for a in P.pixel_grid(oc))
        for beta in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)):
            rc, K = prepare(pc, beta)
            assert rc == 0 and common.bits(K).tobytes() == bytes(40)
            cs, ws = boosted(pc, projection, beta, px, py)
            a, b = np.zeros(3), np.zeros(3)
            for k in range(len(px)):
                assert f(C.byref(pc._c), projection, int(px[k]), int(py[k]), _dp(a), _dp(b)) == 0
                assert common.bits(a).tobytes() == common.bits(cs[k]).tobytes() and common.bits(b).tobytes() == common.bits(ws[k]).tobytes()


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = _abi.lib()
    pc = P.scene("ellis", (8, 8))[3]                                  # tilted: a speed of exactly 1 may round to either side of it
    straight = common.scene("ellis", res=(8, 8))[3]                   # rot of zeros and ones: the camera-space speed is the caller's
    assert sorted(set(abs(v) for v in straight._c.rot[:])) == [0.0, 1.0]
    out3 = np.zeros(3)
    for bad in ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.6, 0.8, 0.1), (2.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.1, np.nan, 0.0), (0.0, 0.0, np.inf)):
        assert B.boost_prepare(straight._c.rot[:], bad) is None, bad
        for cam in (straight, pc):
            refused = B.boost_prepare(cam._c.rot[:], bad) is None
            assert (prepare(cam, bad)[0] == _abi.E_INVALID) == refused and prepare(cam, bad)[0] in (0, _abi.E_INVALID), bad
            rc = L.curvis_camera_outward_vector_boosted(C.byref(cam._c), 0, _dp(np.array(bad)), 0, 0, _dp(out3), None)
            assert (rc == _abi.E_INVALID) == refused and rc in (0, _abi.E_INVALID), bad
        with pytest.raises(ValueError, match="velocity"):
            systems.check_velocity(bad)
    for bad in ((2.0, 0.0, 0.0), (0.7, 0.7, 0.7), (np.nan, 0.0, 0.0), (0.0, 0.0, np.inf)):      # far enough from 1 for any camera
        assert B.boost_prepare(pc._c.rot[:], bad) is None and prepare(pc, bad)[0] == _abi.E_INVALID
    ok = np.array(B.VELOCITY)
    assert L.curvis_camera_boost_prepare(None, _dp(ok), _dp(np.zeros(5))) == _abi.E_INVALID
    assert L.curvis_camera_boost_prepare(C.byref(pc._c), None, _dp(np.zeros(5))) == _abi.E_INVALID
    assert L.curvis_camera_boost_prepare(C.byref(pc._c), _dp(ok), None) == _abi.E_INVALID
    for projection in (3, -1):
        assert L.curvis_camera_outward_vector_boosted(C.byref(pc._c), projection, _dp(ok), 0, 0, _dp(out3), None) == _abi.E_INVALID
    assert L.curvis_camera_outward_vector_boosted(C.byref(pc._c), 0, None, 0, 0, _dp(out3), None) == _abi.E_INVALID
    assert L.curvis_ctx_set_camera_velocities(None, _dp(ok), 1) == _abi.E_INVALID      # no context: refused, nothing dereferenced
    for bad in ((1, 2), "fast", (0.1, 0.2, 0.3, 0.4), 0.5):
        with pytest.raises(ValueError, match="velocity"):
            systems.check_velocity(bad)
    assert systems.check_velocity(None) is None and systems.check_velocity([0.3, -0.4, 0.5]) == B.VELOCITY
    # the largest speed below 1 along the optical axis is taken
    top = float(np.sqrt(np.float64(1.0) - np.float64(2.0) ** -53))
    assert B.boost_prepare(np.eye(3), (top, 0.0, 0.0)) is not None


# ---- 3. the closed form -------------------------------------------------------------------------------------------------------------
def test_aberration_against_the_closed_form():
    """(gamma (d_par - beta), d_perp), normalised, at 50 digits from the FP64 inputs -- the camera's rot, beta and the pixel's FP64 vec --
    against the unit camera-space vector of the accessor: the angle between them is at most 16 gamma^2 2^-53 rad (five times the
    largest of 21 000 random cases, 3.2 gamma^2 2^-53)."""
    mpmath.mp.dps = 50
    rng = np.random.default_rng(20261020)
    worst = 0.0
    for case in range(400):
        fwd, up = rng.normal(size=3), rng.normal(size=3)
        res = (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        projection = case % 3
        pos = (0.0, float(rng.uniform(-3, 3)), float(rng.uniform(0.3, 2.8)), float(rng.uniform(0, 6)))
        pc = curvis_amd.Camera(pos, tuple(fwd), tuple(up), float(rng.uniform(5, 30)), 43.0, res[0], res[1])
        oc = O.camera(pos, tuple(fwd), tuple(up), float(pc._c.focal), 43.0, res)
        assert common.bits(np.array(oc.rot[:])).tobytes() == common.bits(np.array(pc._c.rot[:])).tobytes()
        speed = 0.999 if case < 8 else 1e-8 if case < 16 else float(10.0 ** rng.uniform(-8, np.log10(0.999)))
        direction = rng.normal(size=3)
        beta = tuple(speed * direction / np.sqrt((direction ** 2).sum()) * (1.0 - 1e-12))
        px, py = int(rng.integers(0, res[0])), int(rng.integers(0, res[1]))
        cs, _ = boosted(pc, projection, beta, [px], [py])
        vec = P.pixel_vectors(oc, projection, np.array([px]), np.array([py]))[0]
        rot = [[mpmath.mpf(float(oc.rot[3 * r + i])) for i in range(3)] for r in range(3)]
        c = [sum(rot[r][i] * mpmath.mpf(beta[r]) for r in range(3)) for i in range(3)]
        b2 = sum(x * x for x in c)
        b, g = mpmath.sqrt(b2), 1 / mpmath.sqrt(1 - b2)
        u = [x / b for x in c]
        v = [mpmath.mpf(float(x)) for x in vec]
        n = mpmath.sqrt(sum(x * x for x in v))
        d = [x / n for x in v]
        dpar = sum(d[i] * u[i] for i in range(3))
        exact = [g * (dpar - b) * u[i] + (d[i] - dpar * u[i]) for i in range(3)]
        got = [mpmath.mpf(float(x)) for x in cs[0]]
        cross = [exact[1] * got[2] - exact[2] * got[1], exact[2] * got[0] - exact[0] * got[2], exact[0] * got[1] - exact[1] * got[0]]
        angle = mpmath.atan2(mpmath.sqrt(sum(x * x for x in cross)), sum(exact[i] * got[i] for i in range(3)))
        # the aberration formula itself, on the exact vector: cos theta_static = (cos theta' - beta) / (1 - beta cos theta')
        en = mpmath.sqrt(sum(x * x for x in exact))
        assert abs(sum(exact[i] * u[i] for i in range(3)) / en - (dpar - b) / (1 - b * dpar)) < mpmath.mpf(10) ** -40
        bound = 16 * g * g * mpmath.mpf(2) ** -53
        worst = max(worst, float(angle / (g * g * mpmath.mpf(2) ** -53)))
        assert angle <= bound, (case, beta, (px, py), res, P.NAMES[projection], float(angle), float(bound))
    print("largest angle error: %.3f gamma^2 2^-53" % worst)


def test_boost_along_the_axis_keeps_the_axis_pixel():
    """21 x 15 fisheye, whose centre pixel looks along (1, 0, 0): a velocity along the camera's forward leaves its direction alone,
    bit for bit, and moves every other pixel"""
    _, oc, _, pc = P.scene("ellis", P.RES_ODD)
    fwd = np.array(oc.rot[:]).reshape(3, 3)[:, 0]            # the camera's x axis in the tangent frame: rot (1, 0, 0)
    px, py = (a.reshape(-1) for a in P.pixel_grid(oc))
    still = P.outward_vectors(oc, P.FISHEYE, px, py)[0]
    centre = 7 * 21 + 10
    assert still[centre].tolist() == [1.0, 0.0, 0.0]
    for speed in (0.5, -0.5, 0.9):
        cs, ws = boosted(pc, P.FISHEYE, tuple(speed * fwd), px, py)
        # rot is orthonormal to rounding only, so u is (1, 0, 0) to rounding only: the bound of the closed-form test
        bound = 16.0 / (1.0 - speed * speed) * 2.0 ** -53
        assert abs(cs[centre][0] - 1.0) <= 2.0 ** -52 and abs(cs[centre][1]) <= bound and abs(cs[centre][2]) <= bound, cs[centre].tolist()
        # a camera whose rot holds zeros and ones alone: u is exactly (+-1, 0, 0) and the axis pixel keeps its bits
        straight = common.scene("ellis", res=P.RES_ODD)[3]
        axis = tuple(speed * v for v in np.array(straight._c.rot[:]).reshape(3, 3)[:, 0])
        assert boosted(straight, P.FISHEYE, axis, [10], [7])[0][0].tolist() == [1.0, 0.0, 0.0]
        moved = (common.bits(cs) != common.bits(still)).any(axis=1)
        assert moved.sum() >= len(px) - 1
        # towards the direction of travel the view is compressed: every other pixel looks further away from +x (speed > 0) than before
        others = np.arange(len(px)) != centre
        assert ((cs[others, 0] < still[others, 0]) if speed > 0 else (cs[others, 0] > still[others, 0])).all()


# ---- 4. the velocity of a camera on a path -------------------------------------------------------------------------------------------
def path_rows(name):
    rows = np.array([[float(v) for v in line.split(",")[:4]] for line in refpaths.reference_path_bytes(name).decode().split("\r\n")[1:] if line])
    assert rows.shape == (1000, 4)
    return rows


@pytest.mark.parametrize("name", ("path_through.csv", "path_orbit.csv"))
def test_path_velocity_is_its_restatement(name):
    rows = path_rows(name)
    L = _abi.lib()
    sin = lambda a: float(O.math_array(O.CV, 0, np.array([a]))[0])
    for kind in ("ellis", "interstellar"):
        pm = P.scene(kind, (8, 8))[2]
        m = pm._c()
        for light_speed in (1.0, 0.75):
            for k in list(range(0, 1000, 37)) + [1, 998, 999]:
                prev, pos, nxt = rows[max(k - 1, 0)], rows[k], rows[min(k + 1, 999)]
                out = np.full(3, 7.0)
                assert L.curvis_camera_path_velocity(C.byref(m), _dp(prev), _dp(pos), _dp(nxt), light_speed, _dp(out)) == 0
                want = B.path_velocity(pm.r, sin, prev, pos, nxt, light_speed)
                assert common.bits(out).tobytes() == common.bits(np.array(want)).tobytes(), (name, kind, k, out.tolist(), want)
                assert systems.camera_path_velocity(pm, prev, pos, nxt, light_speed) == want
                if name == "path_orbit.csv":
                    assert out[0] == 0.0 and out[1] == 0.0 and out[2] != 0.0
                else:
                    assert out[0] > 0.0
        out = np.full(3, 7.0)
        assert L.curvis_camera_path_velocity(C.byref(m), _dp(rows[5]), _dp(rows[5]), _dp(rows[5]), 1.0, _dp(out)) == 0 and out.tolist() == [0.0, 0.0, 0.0]
        assert L.curvis_camera_path_velocity(None, _dp(rows[5]), _dp(rows[5]), _dp(rows[5]), 1.0, _dp(out)) == _abi.E_INVALID
        assert L.curvis_camera_path_velocity(C.byref(m), _dp(rows[5]), _dp(rows[5]), _dp(rows[5]), 1.0, None) == _abi.E_INVALID
    # the speeds the issue speaks of: a third to a half of c at light_speed = 1
    pm = P.scene("ellis", (8, 8))[2]
    through = systems.camera_path_velocity(pm, rows[499], rows[500], rows[501], 1.0) if name == "path_through.csv" else None
    if through is not None:
        assert 0.3 < through[0] < 0.6


# ---- 5. the Python keywords ---------------------------------------------------------------------------------------------------------
def test_python_keywords():
    for f in (systems.RelativisticSystem.render_image, systems.RelativisticSystem.render_image_efficient, systems.RelativisticSystem.render_image_direct):
        assert inspect.signature(f).parameters["velocity"].default is None, f
    for f in (rendering.ImageRenderingSystem.__init__, rendering.ImageRenderingSystem.new):
        assert inspect.signature(f).parameters["velocity"].default is None, f
    for f in (rendering.VideoRenderingSystem.__init__, rendering.VideoRenderingSystem.new):
        assert inspect.signature(f).parameters["camera_motion"].default == "static", f
        assert inspect.signature(f).parameters["light_speed"].default == 1.0, f
    assert callable(curvis_amd.Context.set_camera_velocities)
