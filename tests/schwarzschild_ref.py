"""References for the Schwarzschild kind (CURVIS_METRIC_SCHWARZSCHILD), which the CPU oracle does not know.  They are composed from two
sources: the library's HOST accessors, which run the strict (IEEE) step compiled for x86 -- curvis_new_photon, curvis_walk_ray (the
kernels' loop over curvis_update_relativistic_object / curvis_heun_step / curvis_step_delta), curvis_vector_to_direction,
curvis_sky_texel_index --, and the oracle's metric-independent primitives (rotations, interpolation, the sky lookup), put together
the way tests/projection_ref.py composes the renderers.  A comparison of a GPU result with these is x86 strict step against gfx950
fast step: it checks the guard, the device math and the plumbing; the formulas themselves are pinned by the mpmath tests of
tests/test_schwarzschild_host.py."""
import ctypes as C

import numpy as np

import curvis_amd
import oracle_lib as O
import projection_ref as PR
from curvis_amd import _abi

COUNTERS = PR.COUNTERS
HALF_PI = float.fromhex("0x1.921fb54442d18p+0")


def metric(mass=1.0):
    return curvis_amd.SchwarzschildMetric(mass)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def new_photon(pm, pos, direction):
    m = pm._c()
    x, p = np.zeros(4), np.zeros(4)
    rc = _abi.lib().curvis_new_photon(C.byref(m), _dp(np.ascontiguousarray(pos, dtype=np.float64)),
                                      _dp(np.ascontiguousarray(direction, dtype=np.float64)), _dp(x), _dp(p))
    assert rc == 0, rc
    return x, p


def walk(pm, x, p, delta, cap, max_radius, step_scale=0, integrator=0):
    """the ray (x, p) walked in place to escape, capture or the cap with the strict step: (steps, code)"""
    m = pm._c()
    steps, code = C.c_uint32(0), C.c_int32(0)
    rc = _abi.lib().curvis_walk_ray(C.byref(m), _dp(x), _dp(p), float(delta), int(step_scale), int(integrator), int(cap), float(max_radius),
                                    C.byref(steps), C.byref(code))
    assert rc == 0, rc
    return steps.value, code.value


def direction(pm, x, p):
    m = pm._c()
    d = np.zeros(3)
    assert _abi.lib().curvis_vector_to_direction(C.byref(m), _dp(x), _dp(p), _dp(d)) == 0
    return d


def texel(sky_shape, d):
    """raw (tx, ty) of the nearest lookup on a sky of (w, h) texels with the identity orientation, and whether it is out of bounds"""
    tx, ty = C.c_uint32(0), C.c_uint32(0)
    rc = _abi.lib().curvis_sky_texel_index(sky_shape[0], sky_shape[1], None, _dp(d), C.byref(tx), C.byref(ty))
    return tx.value, ty.value, rc != 0


def debug_dump(pm, cam, dirs, sky_shapes, delta, cap, max_radius, step_scale=0, integrator=0):
    """what curvis_render_brute_debug records for the rays along the world-space directions dirs [H, W, 3] from the oracle camera cam"""
    H, W = dirs.shape[:2]
    out = np.zeros((H, W), _abi.RAY_DEBUG)
    pos = np.array(cam.pos[:])
    for j in range(H):
        for i in range(W):
            x, p = new_photon(pm, pos, dirs[j, i])
            steps, code = walk(pm, x, p, delta, cap, max_radius, step_scale, integrator)
            r = out[j, i]
            r["x"], r["p"], r["steps"], r["code"] = x, p, steps, code
            if code != 0:
                tx, ty, _ = texel(sky_shapes[0 if code == 1 else 1], direction(pm, x, p))
                r["tx"], r["ty"] = tx, ty
    return out


def compose_brute(pm, cam, dirs, sky_pos, sky_neg, cap, max_radius, delta, step_scale=0, integrator=0):
    """RelativisticSystem::render_image over dirs, as projection_ref.compose_brute, the ray walked by the library's host accessors:
    (frame, counters, codes)"""
    H, W = dirs.shape[:2]
    rgb = np.zeros((H, W, 3), np.uint8)
    codes = np.zeros((H, W), np.int64)
    cnt = dict.fromkeys(COUNTERS, 0)
    pos = np.array(cam.pos[:])
    for j in range(H):
        for i in range(W):
            x, p = new_photon(pm, pos, dirs[j, i])
            steps, code = walk(pm, x, p, delta, cap, max_radius, step_scale, integrator)
            codes[j, i] = code
            cnt["rays"] += 1
            cnt["steps"] += steps
            if code != 0:
                cnt["n_oob"] += PR._shade(sky_pos if code == 1 else sky_neg, direction(pm, x, p), rgb[j, i])
                cnt["n_pos" if code == 1 else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in COUNTERS), codes


def compute_escape_angle(pm, l, alpha, delta, cap, max_radius, step_scale=0, integrator=0):
    """compute_escape_angle (src/systems.rs:203-261) in the convention of the kernels' escape_angle_lane: a photon at (0, l, pi/2, 0)
    along (cos a, 0, sin a), walked, its world direction's angle.  (code, angle, steps); code -2 where the reference panics"""
    L = O.lib()
    a = np.array([alpha], dtype=np.float64)
    ca, sa = float(O.math_array(O.CV, 1, a)[0]), float(O.math_array(O.CV, 0, a)[0])
    x, p = new_photon(pm, (0.0, l, HALF_PI, 0.0), (ca, 0.0, sa))
    steps, code = walk(pm, x, p, delta, cap, max_radius, step_scale, integrator)
    if code == 0:
        return 0, float("nan"), steps
    t = direction(pm, x, p)
    wpos, rot, ex, wd = np.zeros(3), np.zeros(9), np.array([1.0, 0.0, 0.0]), np.zeros(3)
    L.cvo_vector3_from_theta_phi(O.CV, x[2], x[3], _dp(wpos))
    if L.cvo_rotation_from_two_vectors(O.CV, _dp(ex), _dp(wpos), _dp(rot)) != 0:
        return O.PANIC, float("nan"), steps
    L.cvo_mat3_vec(_dp(rot), _dp(t), _dp(wd))
    n = np.sqrt(wd[0] * wd[0] + wd[1] * wd[1] + wd[2] * wd[2])
    wd = np.array([wd[0] / n, wd[1] / n, wd[2] / n])
    vx = wd[0] * 1.0 + wd[1] * 0.0 + wd[2] * 0.0
    vy = wd[0] * 0.0 + wd[1] * 1.0 + wd[2] * 0.0
    ac = float(O.math_array(O.CV, 3, np.array([vx]))[0])
    return code, (ac if vy >= 0.0 else 2.0 * np.pi - ac), steps


def compose_direct(pm, cam, dirs, sky_pos, sky_neg, cap, max_radius, delta, step_scale=0, integrator=0):
    """"direct" mode, as projection_ref.compose_direct with compute_escape_angle above: (frame, counters, codes)"""
    H, W = dirs.shape[:2]
    alphas, axes, cam_bg = PR.pixel_geometry(cam, dirs)
    rgb = np.zeros((H, W, 3), np.uint8)
    codes = np.zeros((H, W), np.int64)
    cnt = dict.fromkeys(COUNTERS, 0)
    for j in range(H):
        for i in range(W):
            code, ang, steps = compute_escape_angle(pm, cam.pos[1], float(alphas[j, i]), delta, cap, max_radius, step_scale, integrator)
            assert code != O.PANIC
            codes[j, i] = code
            cnt["rays"] += 1
            cnt["steps"] += steps
            if code != 0:
                fin = PR._final_direction(axes[j, i], ang, cam_bg)
                cnt["n_oob"] += PR._shade(sky_pos if code == 1 else sky_neg, fin, rgb[j, i])
                cnt["n_pos" if code == 1 else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in COUNTERS), codes


def compose_efficient_from_table(cam, dirs, sky_pos, sky_neg, table):
    """steps 2, 4 and 5 of render_image_efficient over dirs from a given sample table (alpha, escape angle, escape space: the
    refinement logic that builds it does not depend on the metric and has its own tests): (frame, (rays, n_pos, n_neg, n_none, n_oob))"""
    L = O.lib()
    H, W = dirs.shape[:2]
    alphas, axes, cam_bg = PR.pixel_geometry(cam, dirs)
    a, e, s = (np.ascontiguousarray(table[k], dtype=np.float64) for k in ("a", "e", "s"))
    flat = np.ascontiguousarray(alphas.reshape(-1))
    esc, spc = np.zeros(flat.size), np.zeros(flat.size)
    L.cvo_interp_slice(_dp(a), _dp(e), a.size, _dp(flat), flat.size, _dp(esc))
    L.cvo_interp_slice(_dp(a), _dp(s), a.size, _dp(flat), flat.size, _dp(spc))
    esc, spc = esc.reshape(H, W), spc.reshape(H, W)
    rgb = np.zeros((H, W, 3), np.uint8)
    cnt = dict.fromkeys(COUNTERS, 0)
    for j in range(H):
        for i in range(W):
            cnt["rays"] += 1
            v = spc[j, i]
            if v == 1.0 or v == -1.0:
                fin = PR._final_direction(axes[j, i], esc[j, i], cam_bg)
                cnt["n_oob"] += PR._shade(sky_pos if v == 1.0 else sky_neg, fin, rgb[j, i])
                cnt["n_pos" if v == 1.0 else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in ("rays", "n_pos", "n_neg", "n_none", "n_oob"))


# ---- the scene of the GPU tests ----------------------------------------------------------------------------------------------------
MASS, L_CAM, R, DELTA, CAP = 1.0, 8.0, 25.0, 0.05, 4096
FOCAL, DIAG = 15.0, 43.0
SKY_SHAPES = ((333, 177), (129, 301))       # +l, -l (w, h)
SKY_SALTS = (0x7A3C1B, 0xDEA5C4)
FRAMES = ((24, 16), (32, 24))
_cache = {}


def scene(res):
    """camera at l = 8 M on the equator looking 20 degrees off the hole: (product metric, oracle camera, product camera)"""
    a = np.deg2rad(20.0)
    pos, fwd, up = (0.0, L_CAM, HALF_PI, 0.0), (-float(np.cos(a)), float(np.sin(a)), 0.05), (0.0, 0.0, 1.0)
    return metric(MASS), O.camera(pos, fwd, up, FOCAL, DIAG, res), curvis_amd.Camera(pos, fwd, up, FOCAL, DIAG, res[0], res[1])


def index_skies():
    import common
    if "skies" not in _cache:
        _cache["skies"] = tuple(common.index_sky(w, h, s) for (w, h), s in zip(SKY_SHAPES, SKY_SALTS))
        for t in _cache["skies"]:
            t.setflags(write=False)
    return _cache["skies"]


def memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]
