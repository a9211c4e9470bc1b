"""The accretion disc (include/curvis_hip.h, the disc's paragraph): the definition in Python doubles, written from that text, and the
brute renderer's frame composed per ray from primitives that existed before the disc did.  Nothing here calls anything of the feature.

A ray is walked the way step_scale_ref.Walk walks it -- the oracle's own Euler step cvo_update under CVO_CV with delta_k as
step_scale_ref forms it, or the Heun average as integrator_ref forms it; for the Schwarzschild kind, which the oracle does not know, the
library's host accessors curvis_update_relativistic_object / curvis_heun_step as schwarzschild_ref uses them -- with the plane test at the
top of every iteration but the first:

  (s_k, c_k) = the oracle's CVO_CV sin and cos of theta_k
  crossed    = (c_{k-1} < 0) != (c_k < 0)
  t          = c_{k-1} / (c_{k-1} - c_k)
  l_hit      = l_{k-1} + t (l_k - l_{k-1});   phi_hit = phi_{k-1} + t (phi_k - phi_{k-1})
  on disc    = l_in <= l_hit <= l_out
  s_k < 0:     phi_hit += pi
  tx         = min(as_u32(rem_euclid(phi_hit, 2 pi) / (2 pi) * w), w - 1);   ty = min(as_u32((l_hit - l_in) / (l_out - l_in) * h), h - 1)
  alpha(D[ty][tx]) >= 128: the ray ends, code DISC, k steps, colour D[ty][tx]

Python floats are IEEE doubles and every operation above is one Python operation.  With no disc the composition is
step_scale_ref.compose_brute bit for bit (tests/test_disc_host.py pins that first)."""
import ctypes as C
import math

import numpy as np

import common
import oracle_lib as O
import projection_ref as P
import sky_filter_ref as F
import sky_mipmap_ref as M
import step_scale_ref as SR

DISC = 2
COUNTERS = P.COUNTERS + ("n_disc",)
TWO_PI = 2.0 * math.pi


def as_u32(v):
    """Rust's `v as u32`: truncation, NaN and negatives to 0, saturating"""
    if v != v or v <= 0.0:
        return 0
    if v >= 4294967295.0:
        return 4294967295
    return int(v)


def rem_euclid_pos(a, b):
    """f64::rem_euclid(a, b) for b > 0"""
    if abs(a) < b or a != a:
        r = a
    elif math.isinf(a):
        r = math.nan
    else:
        r = math.fmod(a, b)
    return r + b if r < 0.0 else r


def _div(n, d):
    """the IEEE quotient (Python raises on a zero divisor)"""
    return float(np.float64(n) / np.float64(d))


def crossing(c_prev, c_cur, s_cur, l_prev, l_cur, ph_prev, ph_cur, l_in, l_out, w, h):
    """steps 1-7 of the definition: the texel (tx, ty), or None when the ray did not cross the plane inside [l_in, l_out]"""
    if (c_prev < 0.0) == (c_cur < 0.0):
        return None
    with np.errstate(all="ignore"):
        t = _div(c_prev, c_prev - c_cur)
        l_hit = l_prev + t * (l_cur - l_prev)
        ph_hit = ph_prev + t * (ph_cur - ph_prev)
        if not (l_in <= l_hit and l_hit <= l_out):
            return None
        if s_cur < 0.0:
            ph_hit = ph_hit + math.pi
        tx = min(as_u32(_div(rem_euclid_pos(ph_hit, TWO_PI), TWO_PI) * float(w)), w - 1)
        ty = min(as_u32(_div(l_hit - l_in, l_out - l_in) * float(h)), h - 1)
    return tx, ty


class Disc:
    def __init__(self, rgba, l_in, l_out):
        self.rgba = np.ascontiguousarray(rgba)
        self.h, self.w = self.rgba.shape[:2]
        self.l_in, self.l_out = float(l_in), float(l_out)
        self.alpha = self.rgba[..., 3].tolist()      # plain ints: the walk looks one up per crossing


class OracleStepper:
    """the oracle's photon, Euler step and direction under CVO_CV (Ellis, Interstellar, flat)"""

    def __init__(self, metric):
        self.mp = C.byref(metric)
        self._metric = metric
        self.x, self.p = np.zeros(4), np.zeros(4)
        self.xp, self.pp = O._dp(self.x), O._dp(self.p)
        self._update = O.lib().cvo_update

    def new_photon(self, pos, d):
        O.lib().cvo_new_photon(O.CV, self.mp, O._dp(pos), O._dp(np.ascontiguousarray(d)), self.xp, self.pp)

    def euler(self, dk):
        self._update(O.CV, self.mp, self.xp, self.pp, dk)

    def direction(self, out):
        O.lib().cvo_vector_to_direction(O.CV, self.mp, self.pp, self.xp, O._dp(out))


class HostStepper:
    """the library's pre-existing host accessors (the Schwarzschild kind): curvis_new_photon, curvis_update_relativistic_object,
    curvis_vector_to_direction -- the strict step compiled for x86"""

    def __init__(self, product_metric):
        from curvis_amd import _abi
        self._L = _abi.lib()
        self._m = product_metric._c()
        self.mp = C.byref(self._m)
        self.x, self.p = np.zeros(4), np.zeros(4)
        self.xp, self.pp = O._dp(self.x), O._dp(self.p)

    def new_photon(self, pos, d):
        assert self._L.curvis_new_photon(self.mp, O._dp(np.ascontiguousarray(pos, dtype=np.float64)),
                                         O._dp(np.ascontiguousarray(d, dtype=np.float64)), self.xp, self.pp) == 0

    def euler(self, dk):
        assert self._L.curvis_update_relativistic_object(self.mp, self.xp, self.pp, dk) == 0

    def direction(self, out):
        assert self._L.curvis_vector_to_direction(self.mp, self.xp, self.pp, O._dp(out)) == 0


class Walk:
    """one ray's loop over a stepper, the plane test at the top of each iteration (the step_scale_ref.Walk pattern)"""

    def __init__(self, stepper):
        self.st = stepper
        self.cx = (C.c_double * 4).from_buffer(stepper.x)
        self.cp = (C.c_double * 4).from_buffer(stepper.p)
        self._in, self._out = np.zeros(1), np.zeros(1)
        self._ip, self._op = O._dp(self._in), O._dp(self._out)
        self._math = O.lib().cvo_math_array
        self._cin = (C.c_double * 1).from_buffer(self._in)
        self._cout = (C.c_double * 1).from_buffer(self._out)

    def sincos(self, theta):
        self._cin[0] = theta
        self._math(O.CV, 0, self._ip, None, self._op, 1)
        s = self._cout[0]
        self._math(O.CV, 1, self._ip, None, self._op, 1)
        return s, self._cout[0]

    def heun(self, dk):
        """integrator_ref.HeunWalk.step: two Euler steps with one delta_k, every integrated component (y_k + y'') * 0.5"""
        cx, cp, euler = self.cx, self.cp, self.st.euler
        x0, x1, x2, x3 = cx[0], cx[1], cx[2], cx[3]
        p0, p1, p2, p3 = cp[0], cp[1], cp[2], cp[3]
        euler(dk)
        euler(dk)
        cx[0] = (x0 + cx[0]) * 0.5
        cx[1] = (x1 + cx[1]) * 0.5
        cx[2] = (x2 + cx[2]) * 0.5
        cx[3] = (x3 + cx[3]) * 0.5
        cp[0] = p0
        cp[1] = (p1 + cp[1]) * 0.5
        cp[2] = (p2 + cp[2]) * 0.5
        cp[3] = p3

    def run(self, disc, delta, S, integrator, max_iter, max_radius):
        """(code, steps, (tx, ty) or None, crossings that passed a gap, in-range crossings with s_k < 0, plane crossings with s_k < 0 in
        or out of range)"""
        cx = self.cx
        assert abs(cx[1]) <= max_radius
        kap = SR.kappa(delta, S) if S else 0.0
        code, steps, gaps, sneg, sneg_plane = O.NOT_ESCAPED, 0, 0, 0, 0
        c_prev = l_prev = ph_prev = 0.0
        while steps < max_iter:
            l, ph = cx[1], cx[3]
            if disc is not None:
                s, c = self.sincos(cx[2])
                if steps >= 1:
                    sneg_plane += ((c_prev < 0.0) != (c < 0.0)) and s < 0.0
                    hit = crossing(c_prev, c, s, l_prev, l, ph_prev, ph, disc.l_in, disc.l_out, disc.w, disc.h)
                    if hit is not None:
                        sneg += s < 0.0
                        if disc.alpha[hit[1]][hit[0]] >= 128:
                            return DISC, steps, hit, gaps, sneg, sneg_plane
                        gaps += 1
                c_prev, l_prev, ph_prev = c, l, ph
            dk = delta
            if S:
                a = abs(l) * kap
                if a > delta:
                    dk = a
            if integrator:
                self.heun(dk)
            else:
                self.st.euler(dk)
            steps += 1
            if cx[1] > max_radius:
                code = O.POSITIVE
                break
            if cx[1] < -max_radius:
                code = O.NEGATIVE
                break
        return code, steps, None, gaps, sneg, sneg_plane


def walk_rays(stepper, cam_pos, dirs, disc, max_iter, max_radius, delta, S=0, integrator=0):
    """every ray of dirs [H, W, 3] walked from the camera position: a dict of per-ray arrays -- code, steps, the final state (x, p), the
    sky direction of an escaped ray, the disc texel of a disc ray, gap passes, in-range s_k < 0 crossings, all s_k < 0 plane crossings"""
    H, W = dirs.shape[:2]
    r = dict(code=np.zeros((H, W), np.int64), steps=np.zeros((H, W), np.int64), x=np.zeros((H, W, 4)), p=np.zeros((H, W, 4)),
             d=np.zeros((H, W, 3)), texel=np.zeros((H, W, 2), np.int64), gaps=np.zeros((H, W), np.int64), sneg=np.zeros((H, W), np.int64),
             sneg_plane=np.zeros((H, W), np.int64))
    pos = np.array(cam_pos[:], dtype=np.float64)
    w = Walk(stepper)
    d = np.zeros(3)
    for j in range(H):
        for i in range(W):
            stepper.new_photon(pos, dirs[j, i])
            code, steps, hit, gaps, sneg, sneg_plane = w.run(disc, delta, S, integrator, max_iter, max_radius)
            r["code"][j, i], r["steps"][j, i], r["gaps"][j, i], r["sneg"][j, i], r["sneg_plane"][j, i] = code, steps, gaps, sneg, sneg_plane
            r["x"][j, i], r["p"][j, i] = stepper.x, stepper.p
            if code == DISC:
                r["texel"][j, i] = hit
            elif code != O.NOT_ESCAPED:
                stepper.direction(d)
                r["d"][j, i] = d
    for v in r.values():
        v.setflags(write=False)
    return r


def counters(rays, n_oob):
    c = rays["code"]
    return (c.size, int(rays["steps"].sum()), int((c == O.POSITIVE).sum()), int((c == O.NEGATIVE).sum()), int((c == O.NOT_ESCAPED).sum()),
            int(n_oob), int((c == DISC).sum()))


def _paint_disc(rays, disc, rgb):
    m = rays["code"] == DISC
    if m.any():
        rgb[m] = disc.rgba[rays["texel"][m][:, 1], rays["texel"][m][:, 0], :3]


def frame_nearest(rays, disc, oracle_skies):
    """the nearest lookup: (frame, counters)"""
    H, W = rays["code"].shape
    rgb = np.zeros((H, W, 3), np.uint8)
    oob = 0
    for j in range(H):
        for i in range(W):
            c = rays["code"][j, i]
            if c in (O.POSITIVE, O.NEGATIVE):
                oob += P._shade(oracle_skies[0 if c == O.POSITIVE else 1], np.ascontiguousarray(rays["d"][j, i]), rgb[j, i])
    _paint_disc(rays, disc, rgb)
    return rgb, counters(rays, oob)


def decode_sky_rays(rays, skies):
    """sky_filter_ref.decode's result without a fine render: (which: -1 capped or on the disc, 0 +l, 1 -l; Xc; Yc; rays out of bounds),
    from the oracle's lookup on the virtual sky of 256 w x 256 h texels (step 1 and 2 of "sky_filter")"""
    code = rays["code"]
    which = np.full(code.shape, -1, np.int64)
    Xc, Yc = np.zeros(code.shape, np.int64), np.zeros(code.shape, np.int64)
    oob = 0
    for k, c in enumerate((O.POSITIVE, O.NEGATIVE)):
        m = code == c
        if not m.any():
            continue
        h, w = skies[k].shape[:2]
        X, Y = F.oracle_virtual_indices(w, h, None, rays["d"][m])
        X, Y = X.astype(np.int64), Y.astype(np.int64)
        oob += int((((X >> 8) >= w) | ((Y >> 8) >= h)).sum())
        which[m], Xc[m], Yc[m] = k, np.minimum(X, 256 * w - 1), np.minimum(Y, 256 * h - 1)
    return which, Xc, Yc, oob


def frame_bilinear(rays, disc, skies):
    """option "sky_filter" = 1: sky rays blended as sky_filter_ref does, disc rays their own texel, unfiltered"""
    which, Xc, Yc, oob = decode_sky_rays(rays, skies)
    rgb = np.zeros(which.shape + (3,), np.uint8)
    for k, T in enumerate(skies):
        m = which == k
        if m.any():
            h, w = T.shape[:2]
            x0, x1, y0, y1, fx, fy, _, _, _ = F.taps(Xc[m], Yc[m], w, h)
            rgb[m] = F.blend(T, x0, x1, y0, y1, fx, fy)
    _paint_disc(rays, disc, rgb)
    return rgb, counters(rays, oob)


def frame_mipmap(rays, disc, skies):
    """option "sky_mipmap" = 1 on top: sky_mipmap_ref.mip_frame over the decoded rays -- a disc ray is which = -1 there, a quad partner
    that saw no sky -- then the disc rays take their texel"""
    which, Xc, Yc, oob = decode_sky_rays(rays, skies)
    rgb = np.array(M.mip_frame(which, Xc, Yc, skies)[0])
    _paint_disc(rays, disc, rgb)
    return rgb, counters(rays, oob)


# ---- the scenes of the tests --------------------------------------------------------------------------------------------------------
R, DELTA, CAP, DIAG = SR.R, SR.DELTA, 4096, 43.0
DISC_SHAPE = (97, 53)                       # w, h
DISC_SALT = 0x3D96E7                        # distinct from both of step_scale_ref.SKY_SALTS
# name -> (kind, position, forward, up, focal, resolution, (l_in, l_out))
SCENES = {
    "A": ("ellis", (0.0, 6.0, 1.25, 0.0), (-1.0, 0.0, -0.25), (0.0, 0.0, 1.0), 15.0, (24, 16), (1.5, 5.0)),
    "B": ("interstellar", (0.0, 7.0, 1.3, 0.2), (-1.0, 0.0, -0.2), (0.0, 0.0, 1.0), 12.0, (24, 16), (2.5, 6.0)),
    "C": ("ellis", (0.0, 1.0, 0.9, 0.4), (-1.0, 0.1, -0.5), (0.0, 0.0, 1.0), 7.0, (24, 16), (-6.0, -0.8)),      # the far side
    "D": ("ellis", (0.0, 2.5, 1.15, 0.0), (-1.0, 0.0, -0.3), (0.0, 0.0, 1.0), 9.0, (21, 13), (-3.0, 4.0)),      # ragged tiles
    "F": ("ellis", (0.0, 4.0, 0.15, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 9.0, (24, 16), (-5.0, 5.0)),       # camera over the pole
}
# the ray classes of each scene: (disc rays, +l rays, -l rays, rays that passed a gap and went on, plane crossings with s_k < 0 in or out
# of [l_in, l_out]), and of the last class those inside the range, where step 5 of the definition shifts the azimuth by pi
SCENE_COUNTS = {"A": (141, 233, 10, 39, 0), "B": (101, 274, 9, 23, 0), "C": (19, 285, 80, 5, 11), "D": (133, 135, 5, 26, 3),
                "F": (157, 224, 3, 34, 7)}
SCENE_SNEG_IN_RANGE = {"A": 0, "B": 0, "C": 1, "D": 3, "F": 6}
# what a case about theta outside [0, pi] asserts of its in-range s_k < 0 crossings before it compares: at least 3.  Scene C alone has
# fewer: of its 11 plane crossings with s_k < 0 one lies inside [-6, -0.8]; it asserts that one, and at least 3 plane crossings.
SNEG_IN_RANGE_MIN = {"C": 1, "D": 3, "F": 3}
_cache = {}


def disc_texture():
    """common.index_sky with a third salt -- a pixel comparison is a texel comparison and a which-surface comparison -- alpha 0 where
    (x + 2 y) % 5 == 0"""
    if "tex" not in _cache:
        w, h = DISC_SHAPE
        t = np.array(common.index_sky(w, h, DISC_SALT))
        x, y = np.arange(w)[None, :], np.arange(h)[:, None]
        t[..., 3] = np.where((x + 2 * y) % 5 == 0, 0, 255)
        t.setflags(write=False)
        _cache["tex"] = t
    return _cache["tex"]


def scene_from(kind, pos, fwd, up, focal, res, l_range, product_res=None):
    """a scene from explicit parameters: (kind, oracle metric, product metric, oracle camera, product camera, Disc).  The Schwarzschild
    kind has no oracle metric (None): its rays are walked by HostStepper.  product_res: the product camera's resolution where it is not
    the oracle camera's (a supersampled call: the oracle camera is the fine grid's)"""
    import curvis_amd
    if kind == "schwarzschild":
        om, pm = None, curvis_amd.SchwarzschildMetric(SCHW_MASS)
    else:
        om, pm = SR.metrics(kind)
    pres = product_res or res
    return (kind, om, pm, O.camera(pos, fwd, up, focal, DIAG, res), curvis_amd.Camera(pos, fwd, up, focal, DIAG, pres[0], pres[1]),
            Disc(disc_texture(), l_range[0], l_range[1]))


def stepper_of(om, pm):
    """the stepper that walks a scene_from scene's rays"""
    return HostStepper(pm) if om is None else OracleStepper(om)


def scene(name, res=None, phi=None):
    """(kind, oracle metric, product metric, oracle camera, product camera, Disc)"""
    kind, pos, fwd, up, focal, res0, l_range = SCENES[name]
    if phi is not None:
        pos = pos[:3] + (phi,)
    return scene_from(kind, pos, fwd, up, focal, res or res0, l_range)


def scene_rays(name, S=0, integrator=0, projection=P.PERSPECTIVE, res=None, disc=True, phi=None, delta=DELTA):
    """the walked rays of a scene, computed once, shared, read-only"""
    key = ("rays", name, S, integrator, projection, res, disc, phi, delta)
    if key not in _cache:
        _, om, _, oc, _, dsc = scene(name, res, phi)
        _cache[key] = walk_rays(OracleStepper(om), oc.pos, SR.world_dirs(oc, projection), dsc if disc else None, CAP, R, delta, S, integrator)
    return _cache[key]


def scene_frame(name, lookup="nearest", **kw):
    """(frame, counters, rays) of a scene under a sky lookup: "nearest", "bilinear" or "mipmap"; over step_scale_ref's index skies"""
    key = ("frame", name, lookup) + tuple(sorted(kw.items()))
    if key not in _cache:
        rays = scene_rays(name, **kw)
        dsc = scene(name)[5]
        if lookup == "nearest":
            out = frame_nearest(rays, dsc, SR.oracle_skies())
        elif lookup == "bilinear":
            out = frame_bilinear(rays, dsc, SR.index_skies())
        else:
            out = frame_mipmap(rays, dsc, SR.index_skies())
        out[0].setflags(write=False)
        _cache[key] = out + (rays,)
    return _cache[key]


def classes(rays):
    """(disc rays, +l rays, -l rays, rays that passed a gap and went on, plane crossings with s_k < 0): SCENE_COUNTS' five columns"""
    c = rays["code"]
    return (int((c == DISC).sum()), int((c == O.POSITIVE).sum()), int((c == O.NEGATIVE).sum()), int((rays["gaps"] > 0).sum()),
            int(rays["sneg_plane"].sum()))


def assert_classes(rays, who, sneg_in_range=0):
    """what a GPU case relies on, from the reference alone: at least 8 disc rays, 8 +l rays and 4 rays that passed a gap and went on;
    sneg_in_range (the cases about theta outside [0, pi]: SNEG_IN_RANGE_MIN of scenes C, D, F): at least that many crossings inside
    [l_in, l_out] with s_k < 0, and at least 3 plane crossings with s_k < 0"""
    d, pos, _, gaps, sn = classes(rays)
    assert d >= 8 and pos >= 8 and gaps >= 4, (who, classes(rays))
    if sneg_in_range:
        assert sn >= 3 and int(rays["sneg"].sum()) >= sneg_in_range, (who, classes(rays), int(rays["sneg"].sum()), sneg_in_range)


# ---- the Schwarzschild scene --------------------------------------------------------------------------------------------------------
SCHW_MASS, SCHW_L_CAM, SCHW_THETA, SCHW_L_OUT, SCHW_RES, SCHW_FOCAL = 1.0, 8.0, 1.25, 14.0, (24, 16), 15.0
SCHW_POS, SCHW_FWD, SCHW_UP = (0.0, SCHW_L_CAM, SCHW_THETA, 0.0), (-1.0, 0.0, -0.05), (0.0, 0.0, 1.0)


def schwarzschild_scene():
    """camera at l = 8 M, theta = 1.25, looking at the hole; a disc from l_of_radius(6 M) to l = 14:
    (product metric, oracle camera, product camera, Disc)"""
    import curvis_amd
    pm = curvis_amd.SchwarzschildMetric(SCHW_MASS)
    pos, fwd, up = SCHW_POS, SCHW_FWD, SCHW_UP
    return (pm, O.camera(pos, fwd, up, SCHW_FOCAL, DIAG, SCHW_RES),
            curvis_amd.Camera(pos, fwd, up, SCHW_FOCAL, DIAG, SCHW_RES[0], SCHW_RES[1]), Disc(disc_texture(), pm.l_of_radius(6.0 * SCHW_MASS), SCHW_L_OUT))


def schwarzschild_frame():
    """(frame, counters, rays) of the Schwarzschild scene, the horizon painted with the -l index sky"""
    if "schw" not in _cache:
        pm, oc, _, dsc = schwarzschild_scene()
        rays = walk_rays(HostStepper(pm), oc.pos, SR.world_dirs(oc), dsc, CAP, R, DELTA)
        out = frame_nearest(rays, dsc, SR.oracle_skies())
        out[0].setflags(write=False)
        _cache["schw"] = out + (rays,)
    return _cache["schw"]
