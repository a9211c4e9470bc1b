"""The disc's emission shift (include/curvis_hip.h, the paragraph after the disc's): the definition in Python doubles, written from that
text, and the brute renderer's frame with a moving disc composed per ray over disc_ref, whose probe hands out l_hit and p_phi.  Step 1
is the library's pre-existing host accessor curvis_schwarzschild_u; everything else is one Python operation per operation of the header:

  w = 1 + u_e;  n = 2 u_e - 1;            !(n > 0): F = 0
  a = n / (2 w)
  om = RN(1/2M) / (w sqrt(2 w))
  den = 1 + (sigma om) p_phi;             !(den > 0): F = 0
  A_c = u_c / (1 + u_c)
  g2 = a / (A_c (den den))
  F = G (g2 g2)
  channel: v = c F + 0.5;  c' = 255 if v >= 255 else as_u32(v);  alpha kept

Nothing here calls curvis_disc_shift, curvis_disc_shade or curvis_ctx_set_disc_motion."""
import ctypes as C
import math

import numpy as np

import disc_ref as D
import oracle_lib as O
import projection_ref as P
import ref_compose as RC
import step_scale_ref as SR

STATIC, PROGRADE, RETROGRADE = 0, 1, -1
_div = RC._div


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan


def u_of_l(metric_c, l):
    """step 1: the kind's own function, funnel included"""
    from curvis_amd import _abi
    u = C.c_double(0.0)
    assert _abi.lib().curvis_schwarzschild_u(C.byref(metric_c), float(l), C.byref(u)) == 0
    return u.value


def inv_2m(mass):
    """RN(1 / 2M): 2M is exact"""
    return _div(1.0, 2.0 * mass)


def shift_u(inv, u_e, u_c, sigma, gain, p_phi):
    """steps 2-8 from u_e and u_c"""
    with np.errstate(all="ignore"):
        w = 1.0 + u_e
        n = 2.0 * u_e - 1.0
        if not n > 0.0:
            return 0.0
        a = _div(n, 2.0 * w)
        om = _div(inv, w * _sqrt(2.0 * w))
        den = 1.0 + (float(sigma) * om) * p_phi
        if not den > 0.0:
            return 0.0
        A_c = _div(u_c, 1.0 + u_c)
        g2 = _div(a, float(np.float64(A_c) * (np.float64(den) * np.float64(den))))
        return float(np.float64(gain) * (np.float64(g2) * np.float64(g2)))


def shift(metric_c, mass, l_hit, l_camera, sigma, gain, p_phi):
    """F of the header for motion sigma = +-1"""
    return shift_u(inv_2m(mass), u_of_l(metric_c, l_hit), u_of_l(metric_c, l_camera), sigma, gain, p_phi)


def g_squared(metric_c, mass, l_hit, l_camera, sigma, p_phi):
    """g2 of step 7 (0 where steps 2 or 5 give F = 0): sqrt(F) at G = 1"""
    return _sqrt(shift(metric_c, mass, l_hit, l_camera, sigma, 1.0, p_phi))


def shade_channel(c, F):
    with np.errstate(all="ignore"):
        v = float(np.float64(c) * np.float64(F) + np.float64(0.5))
    return 255 if v >= 255.0 else D.as_u32(v)


def shade(texel, F):
    """a packed RGBA8 texel (red in the low byte) -> the shaded one"""
    out = texel & 0xFF000000
    for k in range(3):
        out |= shade_channel((texel >> (8 * k)) & 0xFF, F) << (8 * k)
    return out


def shade_rgb(rgb, F):
    return [shade_channel(int(c), F) for c in rgb]


# ---- the scenes: disc_ref's Schwarzschild scene (SCHW_*, CAP, R, DELTA), walked once per shape and shaded per motion and gain --------
R, DELTA, CAP = D.R, D.DELTA, D.CAP
_cache = {}


def scene(l_cam=D.SCHW_L_CAM, l_inner=None, res=D.SCHW_RES, product_res=None):
    """(product metric, oracle camera, product camera, disc_ref.Disc): disc_ref.schwarzschild_scene with the camera's l, the disc's
    inner edge (None: l_of_radius(6 M), disc_ref's) and the resolution to choose"""
    import curvis_amd
    pm = curvis_amd.SchwarzschildMetric(D.SCHW_MASS)
    pos = (0.0, float(l_cam), D.SCHW_THETA, 0.0)
    pres = product_res or res
    l_in = pm.l_of_radius(6.0 * D.SCHW_MASS) if l_inner is None else float(l_inner)
    return (pm, O.camera(pos, D.SCHW_FWD, D.SCHW_UP, D.SCHW_FOCAL, D.DIAG, res),
            curvis_amd.Camera(pos, D.SCHW_FWD, D.SCHW_UP, D.SCHW_FOCAL, D.DIAG, pres[0], pres[1]), D.Disc(D.disc_texture(), l_in, D.SCHW_L_OUT))


def scene_rays(l_cam=D.SCHW_L_CAM, l_inner=None, res=D.SCHW_RES, S=0, integrator=0, projection=P.PERSPECTIVE):
    """the walked rays of a scene, computed once, shared, read-only"""
    key = ("rays", l_cam, l_inner, res, S, integrator, projection)
    if key not in _cache:
        pm, oc, _, dsc = scene(l_cam, l_inner, res)
        _cache[key] = D.walk_rays(D.HostStepper(pm), oc.pos, SR.world_dirs(oc, projection), dsc, CAP, R, DELTA, S, integrator, motion=True)
    return _cache[key]


def factors(rays, l_cam, sigma, gain):
    """F of every ray of the scene (0 where the ray did not end on the disc)"""
    pm = scene()[0]
    mc = pm._c()
    F = np.zeros(rays["code"].shape)
    for j, i in np.argwhere(rays["code"] == D.DISC):
        F[j, i] = shift(mc, D.SCHW_MASS, rays["l_hit"][j, i], l_cam, sigma, gain, rays["p_phi"][j, i])
    return F


def scene_frame(sigma, gain=1.0, lookup="nearest", l_cam=D.SCHW_L_CAM, l_inner=None, **kw):
    """(frame, counters, rays, F per ray) of a scene with the disc in motion sigma (0: static) under a sky lookup: the static disc's
    frame as disc_ref composes it, with every disc ray's colour replaced by its shaded texel -- disc_ref paints the disc rays last under
    every lookup, so the replacement is the definition's "the shifted colour replaces the texel's colour" """
    key = ("frame", sigma, gain, lookup, l_cam, l_inner) + tuple(sorted(kw.items()))
    if key not in _cache:
        rays = scene_rays(l_cam, l_inner, **kw)
        dsc = scene(l_cam, l_inner)[3]
        rgb, cnt = RC.frame(rays, dsc, lookup, SR.index_skies(), SR.oracle_skies())
        rgb = np.array(rgb)
        F = factors(rays, l_cam, sigma, gain) if sigma else np.zeros(rays["code"].shape)
        if sigma:
            for j, i in np.argwhere(rays["code"] == D.DISC):
                tx, ty = rays["texel"][j, i]
                rgb[j, i] = shade_rgb(dsc.rgba[ty, tx, :3], F[j, i])
        rgb.setflags(write=False)
        F.setflags(write=False)
        _cache[key] = (rgb, cnt, rays, F)
    return _cache[key]


def conditions(rays, F, gain, dsc):
    """what the scenes must contain, from the reference alone: (disc rays with F = 0, disc rays with a saturated channel whose texel's
    channel was below 255, disc rays with g > 1, disc rays with g < 1)"""
    on = rays["code"] == D.DISC
    zero = int((on & (F == 0.0)).sum())
    sat = 0
    for j, i in np.argwhere(on):
        tx, ty = rays["texel"][j, i]
        t = dsc.rgba[ty, tx, :3]
        sat += any(int(c) < 255 and shade_channel(int(c), F[j, i]) == 255 for c in t)
    g4 = F / gain if gain else F * 0.0
    return zero, int(sat), int((on & (g4 > 1.0)).sum()), int((on & (g4 < 1.0) & (F > 0.0)).sum())
