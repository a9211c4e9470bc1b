"""The moving camera (curvis_ctx_set_camera_velocities): the definition in numpy FP64, written from its paragraph in
include/curvis_hip.h, the boosted world-space directions of a frame, and each renderer's frame composed from them over the oracle's
primitives (projection_ref.compose_*).  Nothing here calls the product.

Once per frame, from the camera's rot (row-major 3 x 3) and beta = (b_l, b_theta, b_phi):
  c_i = ((rot[0][i] b_l) + rot[1][i] b_theta) + rot[2][i] b_phi,  b2 = (c_0 c_0 + c_1 c_1) + c_2 c_2
  b2 == 0: not boosted;  !(b2 < 1): refused
  b = sqrt(b2), g = 1 / sqrt(1 - b2), u_i = c_i / b, A = g - 1, B = g b
Per ray, vec = (x, y, z) un-normalised:
  n = sqrt((x x + y y) + z z), p = (x u_0 + y u_1) + z u_2, s = A p - B n, vec' = (x + u_0 s, y + u_1 s, z + u_2 s)
then the reference's normalize and rotation.  Every numpy operation below is one individually rounded FP64 operation (separate ufunc
calls: nothing is fused)."""
import numpy as np

import oracle_lib as O
import projection_ref as P

VELOCITY = (0.3, -0.4, 0.5)
VELOCITY_PHI = (0.0, 0.0, 0.9)
RES_PERSPECTIVE = (24, 16)
RES = {P.PERSPECTIVE: RES_PERSPECTIVE, P.EQUIRECTANGULAR: (32, 16), P.FISHEYE: (21, 15)}
_cache = {}


def boost_prepare(rot, beta):
    """(u_0, u_1, u_2, A, B) as float64[5]; zeros for a frame that is not boosted; None for a refused speed"""
    rot = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    bl, bt, bp = (np.float64(v) for v in beta)
    with np.errstate(all="ignore"):
        c = [((rot[0][i] * bl) + rot[1][i] * bt) + rot[2][i] * bp for i in range(3)]
        b2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        if b2 == 0.0:
            return np.zeros(5)
        if not (b2 < 1.0):
            return None
        b = np.sqrt(b2)
        g = np.float64(1.0) / np.sqrt(np.float64(1.0) - b2)
        return np.array([c[0] / b, c[1] / b, c[2] / b, g - np.float64(1.0), g * b])


def boost(vec, K):
    """vec' for vectors [..., 3]; K of a frame that is not boosted (B == 0) leaves them alone"""
    if K[4] == 0.0:
        return np.array(vec, dtype=np.float64)
    x, y, z = vec[..., 0], vec[..., 1], vec[..., 2]
    u0, u1, u2, A, B = (np.float64(k) for k in K)
    n = np.sqrt((x * x + y * y) + z * z)
    p = (x * u0 + y * u1) + z * u2
    s = A * p - B * n
    return np.stack([x + u0 * s, y + u1 * s, z + u2 * s], axis=-1)


def outward_vectors(cam, projection, beta, px=None, py=None):
    """(unit camera-space vectors, world-space vectors) of the pixels of a camera with velocity beta -- the whole frame by default"""
    if px is None:
        px, py = P.pixel_grid(cam)
    K = boost_prepare(cam.rot[:], beta)
    assert K is not None
    unit = P.normalize(boost(P.pixel_vectors(cam, projection, px, py), K))
    return unit, P.mat3_vec(np.array(cam.rot[:]), unit)


def path_velocity(r_of_l, sin, prev, pos, nxt, light_speed):
    """curvis_camera_path_velocity restated: poses (t, l, theta, phi); r_of_l and sin are the product's own r(l) and sine"""
    prev, pos, nxt = (np.asarray(v, dtype=np.float64) for v in (prev, pos, nxt))
    dt = nxt[0] - prev[0]
    if dt == 0.0:
        return (0.0, 0.0, 0.0)
    inv = np.float64(1.0) / (dt * np.float64(light_speed))
    r = np.float64(r_of_l(pos[1]))
    return (float((nxt[1] - prev[1]) * inv), float(r * (nxt[2] - prev[2]) * inv), float((r * np.float64(sin(pos[2]))) * (nxt[3] - prev[3]) * inv))


def expected(renderer, kind, projection, beta, res=None, skies=None, n=1, l=P.POS[1]):
    """the composition's (frame, counters, codes or escape space) for projection_ref's scene -- camera at radius l, moving with beta --
    at n times the resolution res; read-only, shared"""
    res = res or RES[projection]
    key = (renderer, kind, projection, tuple(beta), res, n, l, id(skies) if skies is not None else None)
    if key not in _cache:
        om, oc = P.scene(kind, (res[0] * n, res[1] * n), l=l)[:2]
        sp, sn = skies if skies is not None else tuple(O.sky(np.array(t)) for t in P.index_skies())
        dirs = outward_vectors(oc, projection, beta)[1]
        if renderer == "brute":
            out = P.compose_brute(om, oc, dirs, sp, sn, P.CAP, P.R, P.DELTA)
        elif renderer == "direct":
            out = P.compose_direct(om, oc, dirs, sp, sn, P.CAP, P.R, P.DELTA)
        else:
            out = P.compose_efficient(om, oc, dirs, sp, sn, *P.efficient_args())
        for a in (out[0], out[2]):
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def assert_classes(renderer, kind, projection, beta, res=None, skies=None, n=1, least=8, l=P.POS[1]):
    """brute: at least 8 rays to each sky and 8 capped ones; efficient, direct: 8 pixels per sky"""
    _, st, _ = expected(renderer, kind, projection, beta, res, skies, n, l)
    classes = st[2:5] if renderer == "brute" else st[2:4]
    assert all(c >= least for c in classes), (renderer, kind, P.NAMES[projection], beta, res, st)
