"""Library option "projection" (0 perspective, 1 equirectangular, 2 fisheye): the definition in numpy FP64, written from the option's
paragraph in include/curvis_hip.h, and each renderer's frame composed per pixel from primitives of the CPU oracle that exist already.
Nothing here calls the product.

The option replaces only the un-normalised camera-space vector vec = (x, y, z) of a pixel (x forward, y left, z up):
  u = (double)(2 px + 1) / (double)(2 res_x),  v = (double)(2 py + 1) / (double)(2 res_y)          (projection != 0)
  1: psi = (0.5 - u) * (2 pi), th = v * pi, vec = (sin(th) cos(psi), sin(th) sin(psi), cos(th))
  2: ys = -sensor_w * (u - 0.5), zs = sensor_h * (0.5 - v), rho = sqrt(ys ys + zs zs), b = rho / focal,
     vec = (cos(b), sin(b) (ys / rho), sin(b) (zs / rho)), and (1, 0, 0) when rho == 0
Behind it the reference's sequence: vec / sqrt((x x + y y) + z z), the camera rotation, then the renderer.  Every numpy operation
below is one individually rounded FP64 operation (separate ufunc calls: nothing is fused); sin, cos and acos are cv_math.h's through
the oracle's CVO_CV flavour."""
import ctypes as C

import numpy as np

import common
import oracle_lib as O

PERSPECTIVE, EQUIRECTANGULAR, FISHEYE = 0, 1, 2
NAMES = ("perspective", "equirectangular", "fisheye")
COUNTERS = ("rays", "steps", "n_pos", "n_neg", "n_none", "n_oob")


def _sin(a):
    return O.math_array(O.CV, 0, a)


def _cos(a):
    return O.math_array(O.CV, 1, a)


def pixel_vectors(cam, projection, px, py):
    """vec of the definition for the pixels (px, py) (integer arrays of one shape) of the oracle camera `cam`: float64 [..., 3]"""
    px, py = np.asarray(px, dtype=np.int64), np.asarray(py, dtype=np.int64)
    rx, ry = np.float64(cam.res_x), np.float64(cam.res_y)
    sw, sh, focal = np.float64(cam.sensor_w), np.float64(cam.sensor_h), np.float64(cam.focal)
    out = np.empty(px.shape + (3,), np.float64)
    if projection == PERSPECTIVE:       # src/cameras.rs:150-164
        h = 0.5 - (py.astype(np.float64) / ry)
        w = (px.astype(np.float64) / rx) - 0.5
        out[..., 0] = np.full(px.shape, focal * 1.0)
        out[..., 1] = -sw * w
        out[..., 2] = sh * h
        return out
    u = (2 * px + 1).astype(np.float64) / np.float64(2 * int(cam.res_x))
    v = (2 * py + 1).astype(np.float64) / np.float64(2 * int(cam.res_y))
    if projection == EQUIRECTANGULAR:
        psi = (0.5 - u) * (2.0 * np.pi)
        th = v * np.pi
        st, ct, sp, cp = _sin(th), _cos(th), _sin(psi), _cos(psi)
        out[..., 0] = st * cp
        out[..., 1] = st * sp
        out[..., 2] = ct
        return out
    assert projection == FISHEYE
    ys = -sw * (u - 0.5)
    zs = sh * (0.5 - v)
    rho = np.sqrt(ys * ys + zs * zs)
    b = rho / focal
    sb, cb = _sin(b), _cos(b)
    zero = rho == 0.0
    safe = np.where(zero, 1.0, rho)
    out[..., 0] = np.where(zero, 1.0, cb)
    out[..., 1] = np.where(zero, 0.0, sb * (ys / safe))
    out[..., 2] = np.where(zero, 0.0, sb * (zs / safe))
    return out


def normalize(vec):
    """Vector3::normalize: norm sqrt((x x + y y) + z z), three divisions"""
    x, y, z = vec[..., 0], vec[..., 1], vec[..., 2]
    n = np.sqrt((x * x + y * y) + z * z)
    return np.stack([x / n, y / n, z / n], axis=-1)


def mat3_vec(m, v):
    """nalgebra gemv, y_i = ((m_i0 x0) + m_i1 x1) + m_i2 x2, for vectors [..., 3]"""
    m = np.asarray(m, dtype=np.float64).reshape(9)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([(m[3 * i] * x + m[3 * i + 1] * y) + m[3 * i + 2] * z for i in range(3)], axis=-1)


def pixel_grid(cam):
    py, px = np.meshgrid(np.arange(cam.res_y), np.arange(cam.res_x), indexing="ij")
    return px, py


def outward_vectors(cam, projection, px=None, py=None):
    """(unit camera-space vectors, world-space vectors) of the pixels -- the whole frame [H, W, 3] by default"""
    if px is None:
        px, py = pixel_grid(cam)
    unit = normalize(pixel_vectors(cam, projection, px, py))
    return unit, mat3_vec(np.array(cam.rot[:]), unit)


def oracle_perspective_world(cam):
    """cvo_camera_outward_world for every pixel: [H, W, 3]"""
    out = np.zeros((cam.res_y, cam.res_x, 3))
    v = np.zeros(3)
    for j in range(cam.res_y):
        for i in range(cam.res_x):
            O.lib().cvo_camera_outward_world(C.byref(cam), i, j, O._dp(v))
            out[j, i] = v
    return out


def fisheye_in_range(cam):
    return bool(0.5 * np.sqrt(np.float64(cam.sensor_w) ** 2 + np.float64(cam.sensor_h) ** 2) / np.float64(cam.focal) <= np.pi)


# ---- the renderers, composed per pixel -------------------------------------------------------------------------------------------
def _shade(sky, d, out):
    px = (C.c_uint8 * 4)()
    oob = O.lib().cvo_sky_pixel(O.CV, C.byref(sky), O._dp(d), px)
    out[:] = (px[0], px[1], px[2])
    return int(oob)


def compose_brute(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta):
    """RelativisticSystem::render_image (src/systems.rs:307-330) over the world-space directions dirs [H, W, 3]:
    (frame, (rays, steps, n_pos, n_neg, n_none, n_oob), escape codes [H, W])"""
    L = O.lib()
    H, W = dirs.shape[:2]
    rgb = np.zeros((H, W, 3), np.uint8)
    codes = np.zeros((H, W), np.int64)
    cnt = dict.fromkeys(COUNTERS, 0)
    pos = np.array(cam.pos[:])
    x, p, d = np.zeros(4), np.zeros(4), np.zeros(3)
    for j in range(H):
        for i in range(W):
            L.cvo_new_photon(O.CV, C.byref(metric), O._dp(pos), O._dp(np.ascontiguousarray(dirs[j, i])), O._dp(x), O._dp(p))
            steps = C.c_uint32(0)
            code = L.cvo_escape_photon(O.CV, C.byref(metric), O._dp(x), O._dp(p), delta, max_iter, max_radius, C.byref(steps))
            assert code != O.PANIC
            codes[j, i] = code
            cnt["rays"] += 1
            cnt["steps"] += steps.value
            if code in (O.POSITIVE, O.NEGATIVE):
                L.cvo_vector_to_direction(O.CV, C.byref(metric), O._dp(p), O._dp(x), O._dp(d))
                cnt["n_oob"] += _shade(sky_pos if code == O.POSITIVE else sky_neg, d, rgb[j, i])
                cnt["n_pos" if code == O.POSITIVE else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in COUNTERS), codes


def frame_pose(cam):
    """the two once-per-frame values of render_image_efficient (src/systems.rs:393-397, :411) in the flavour the oracle's CVO_CV render
    takes them: the platform libm, one sincos() per pair"""
    L = O.lib()
    cam_bg, rot_bg, ex = np.zeros(3), np.zeros(9), np.array([1.0, 0.0, 0.0])
    L.cvo_vector3_from_theta_phi(O.LIBM_SINCOS, cam.pos[2], cam.pos[3], O._dp(cam_bg))
    assert L.cvo_rotation_from_two_vectors(O.LIBM_SINCOS, O._dp(ex), O._dp(cam_bg), O._dp(rot_bg)) == 0
    return cam_bg, rot_bg


def pixel_geometry(cam, dirs):
    """step 2 (src/systems.rs:405-433): (alpha [H, W], axes [H, W, 3], cam_bg)"""
    cam_bg, rot_bg = frame_pose(cam)
    out_bg = mat3_vec(rot_bg, dirs)
    a, b = cam_bg, out_bg
    axes = np.stack([a[1] * b[..., 2] - a[2] * b[..., 1], a[2] * b[..., 0] - a[0] * b[..., 2], a[0] * b[..., 1] - a[1] * b[..., 0]], axis=-1)
    dot = (dirs[..., 0] * 1.0 + dirs[..., 1] * 0.0) + dirs[..., 2] * 0.0
    return O.math_array(O.CV, 3, dot), axes, cam_bg


def _final_direction(axis, angle, cam_bg):
    """step 5 (src/systems.rs:498-506): from_axis_angle(normalize(axis), angle) * cam_bg"""
    L = O.lib()
    n = np.sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2])
    u = np.array([axis[0] / n, axis[1] / n, axis[2] / n])
    rot, fin = np.zeros(9), np.zeros(3)
    L.cvo_from_axis_angle(O.CV, O._dp(u), float(angle), O._dp(rot))
    L.cvo_mat3_vec(O._dp(rot), O._dp(np.ascontiguousarray(cam_bg)), O._dp(fin))
    return fin


def compose_efficient(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta, alpha_nums, max_it_sampling, thr1, thr2):
    """render_image_efficient (src/systems.rs:333-527) over dirs: (frame, counters -- steps are the sampler's --, escape space [H, W])"""
    L = O.lib()
    H, W = dirs.shape[:2]
    alphas, axes, cam_bg = pixel_geometry(cam, dirs)
    smp = O.Samples()
    rc = L.cvo_doubly_sample(O.CV, C.byref(metric), cam.pos[1], delta, max_iter, max_radius, -0.1 * np.pi, 1.1 * np.pi, alpha_nums,
                             max_it_sampling, thr1, thr2, C.byref(smp))
    assert rc == 0, rc
    flat = np.ascontiguousarray(alphas.reshape(-1))
    esc, spc = np.zeros(flat.size), np.zeros(flat.size)
    L.cvo_interp_slice(smp.a, smp.e, smp.n, O._dp(flat), flat.size, O._dp(esc))
    L.cvo_interp_slice(smp.a, smp.s, smp.n, O._dp(flat), flat.size, O._dp(spc))
    sampler_steps = int(smp.steps)
    L.cvo_samples_free(C.byref(smp))
    esc, spc = esc.reshape(H, W), spc.reshape(H, W)
    rgb = np.zeros((H, W, 3), np.uint8)
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["steps"] = sampler_steps
    for j in range(H):
        for i in range(W):
            cnt["rays"] += 1
            s = spc[j, i]
            if s == 1.0 or s == -1.0:
                fin = _final_direction(axes[j, i], esc[j, i], cam_bg)
                cnt["n_oob"] += _shade(sky_pos if s == 1.0 else sky_neg, fin, rgb[j, i])
                cnt["n_pos" if s == 1.0 else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in COUNTERS), spc


def compose_direct(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta):
    """"direct" mode: cvo_compute_escape_angle per pixel in place of the table: (frame, counters, escape codes [H, W])"""
    H, W = dirs.shape[:2]
    alphas, axes, cam_bg = pixel_geometry(cam, dirs)
    rgb = np.zeros((H, W, 3), np.uint8)
    codes = np.zeros((H, W), np.int64)
    cnt = dict.fromkeys(COUNTERS, 0)
    for j in range(H):
        for i in range(W):
            code, ang, steps = O.compute_escape_angle(O.CV, metric, cam.pos[1], float(alphas[j, i]), delta, max_iter, max_radius)
            codes[j, i] = code
            cnt["rays"] += 1
            cnt["steps"] += steps
            if code in (O.POSITIVE, O.NEGATIVE):
                fin = _final_direction(axes[j, i], ang, cam_bg)
                cnt["n_oob"] += _shade(sky_pos if code == O.POSITIVE else sky_neg, fin, rgb[j, i])
                cnt["n_pos" if code == O.POSITIVE else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in COUNTERS), codes


# ---- the scene of the GPU tests --------------------------------------------------------------------------------------------------
POS = (0.0, 1.0, np.pi / 2, 0.0)
FWD, UP = (-1.0, 0.3, 0.2), (0.0, 0.0, 1.0)
FOCAL, DIAG = 7.0, 43.0
R, DELTA, CAP = 10.0, 0.05, 240
SKY_SHAPES = ((333, 777), (1000, 500))      # +l, -l (w, h)
SKY_SALTS = (0x7A3C1B, 0xDEA5C4)
RES = {EQUIRECTANGULAR: (32, 16), FISHEYE: (20, 14)}
RES_ODD = (21, 15)                          # fisheye: its centre pixel has rho == 0
EFF = dict(n0=100, maxit=100, t1=1e-5, t2=1e-5)
KINDS = ("ellis", "interstellar")
_cache = {}


def scene(kind, res, focal=FOCAL, l=POS[1]):
    """(oracle metric, oracle camera, product metric, product camera)"""
    return common.scene(kind, res=res, pos=(POS[0], l, POS[2], POS[3]), fwd=FWD, up=UP, focal=focal, diag=DIAG)


def index_skies():
    import ref_compose      # (it imports this module)
    return ref_compose.index_skies(SKY_SHAPES, SKY_SALTS)


def efficient_args(cap=CAP):
    return (cap, R, DELTA, EFF["n0"], EFF["maxit"], EFF["t1"], EFF["t2"])


def expected(renderer, kind, projection, res=None, skies=None, n=1, l=POS[1]):
    """the composition's (frame, counters, codes or escape space) for the scene -- camera at radius l -- at n times the resolution
    `res`; read-only, shared"""
    res = res or RES[projection]
    key = (renderer, kind, projection, res, n, l, id(skies) if skies is not None else None)
    if key not in _cache:
        om, oc = scene(kind, (res[0] * n, res[1] * n), l=l)[:2]
        sp, sn = skies if skies is not None else tuple(O.sky(np.array(t)) for t in index_skies())
        dirs = outward_vectors(oc, projection)[1]
        if renderer == "brute":
            out = compose_brute(om, oc, dirs, sp, sn, CAP, R, DELTA)
        elif renderer == "direct":
            out = compose_direct(om, oc, dirs, sp, sn, CAP, R, DELTA)
        else:
            out = compose_efficient(om, oc, dirs, sp, sn, *efficient_args())
        for a in (out[0], out[2]):
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def assert_classes(renderer, kind, projection, res=None, skies=None, n=1, least=8):
    """what every comparison relies on: brute -- at least 8 rays to each sky and 8 capped ones; efficient, direct -- 8 pixels per sky"""
    _, st, _ = expected(renderer, kind, projection, res, skies, n)
    classes = st[2:5] if renderer == "brute" else st[2:4]
    assert all(c >= least for c in classes), (renderer, kind, NAMES[projection], res, st)
