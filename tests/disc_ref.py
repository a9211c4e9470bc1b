"""The accretion disc (include/curvis_hip.h, the disc's paragraph): the definition in Python doubles, written from that text, and the
brute renderer's frame composed per ray from primitives that existed before the disc did.  Nothing here calls anything of the feature.

A ray is walked by ref_compose.Walk -- the oracle's own Euler step cvo_update under CVO_CV with delta_k as step_scale_ref forms it, or the
Heun average as integrator_ref forms it; for the Schwarzschild kind, which the oracle does not know, the library's host accessor
curvis_update_relativistic_object -- with the plane test below as its probe, at the top of every iteration but the first:

  (s_k, c_k) = the oracle's CVO_CV sin and cos of theta_k
  crossed    = (c_{k-1} < 0) != (c_k < 0)
  t          = c_{k-1} / (c_{k-1} - c_k)
  l_hit      = l_{k-1} + t (l_k - l_{k-1});   phi_hit = phi_{k-1} + t (phi_k - phi_{k-1})
  on disc    = l_in <= l_hit <= l_out
  s_k < 0:     phi_hit += pi
  tx         = min(as_u32(rem_euclid(phi_hit, 2 pi) / (2 pi) * w), w - 1);   ty = min(as_u32((l_hit - l_in) / (l_out - l_in) * h), h - 1)
  alpha(D[ty][tx]) >= 128: the ray ends, code DISC, k steps, colour D[ty][tx]

Python floats are IEEE doubles and every operation above is one Python operation.  With no disc the composition is
step_scale_ref's brute frame bit for bit (tests/test_disc_host.py pins that first)."""
import math

import numpy as np

import common
import oracle_lib as O
import projection_ref as P
import ref_compose as RC
import step_scale_ref as SR
from ref_compose import (DISC, COUNTERS, OracleStepper, HostStepper, stepper_of, counters, frame_nearest, frame_bilinear, frame_mipmap,  # noqa: F401
                         decode_sky_rays)

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


_div = RC._div


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


def probe_of(disc, motion=False):
    """the plane test as ref_compose.Walk's probe: (tx, ty, opaque, l_hit) of a crossing inside [l_in, l_out], else None; motion: l_hit
    (steps 2-3) is handed out for an opaque texel, for disc_motion_ref's shift -- otherwise 0.  disc None: no probe"""
    if disc is None:
        return None

    def probe(c_prev, c, s, l_prev, l, ph_prev, ph):
        hit = crossing(c_prev, c, s, l_prev, l, ph_prev, ph, disc.l_in, disc.l_out, disc.w, disc.h)
        if hit is None:
            return None
        opaque = disc.alpha[hit[1]][hit[0]] >= 128
        return hit + (opaque, l_prev + _div(c_prev, c_prev - c) * (l - l_prev) if motion and opaque else 0.0)
    return probe


def walk_rays(stepper, cam_pos, dirs, disc, max_iter, max_radius, delta, S=0, integrator=0, motion=False):
    """every ray of dirs [H, W, 3] walked from the camera position: ref_compose.compose_brute's per-ray arrays with the disc's probe"""
    return RC.compose_brute(stepper, cam_pos, dirs, max_iter, max_radius, delta, S, integrator, probe_of(disc, motion))


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
        _cache[key] = RC.frame(rays, dsc, lookup, SR.index_skies(), SR.oracle_skies()) + (rays,)
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
