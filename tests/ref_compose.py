"""What every reference of the GPU suite shares: the one per-step ray walk, the one escape-angle evaluator, one composition per renderer
from (stepper, camera, world directions, walk options) to per-ray arrays, and the functions that turn per-ray arrays into counters, debug
records and frames.  The feature modules (step_scale_ref, integrator_ref, disc_ref, disc_motion_ref, schwarzschild_ref, kernel_matrix_ref,
efficient_matrix_ref) keep the definitions written from include/curvis_hip.h, their scenes and their caches.  Nothing here calls the
product's renderers, and nothing is added to the oracle.

A ray is walked by a stepper's own Euler step -- the oracle's cvo_update under CVO_CV, or, for the Schwarzschild kind, which the oracle
does not know, the library's host accessor curvis_update_relativistic_object -- with

  kappa   = RN(delta / (S / 256));  a = RN(|l_k| kappa);  delta_k = a if a > delta else delta      (step_scale_ref; S = 0: delta_k = delta)
  Euler:    y_k+1 = E(y_k, delta_k)
  Heun:     y'' = E(E(y_k, delta_k), delta_k);  y_k+1 = (y_k + y'') * 0.5 on t, l, theta, phi, p_l, p_theta; p_t and p_phi kept (integrator_ref)

an optional plane probe at the top of every iteration but the first (disc_ref), and the reference's escape test on y_k+1.  At S = 0, Euler
and no probe the walk is the oracle's own cvo_escape_photon bit for bit, and for the Schwarzschild kind the library's curvis_walk_ray:
`whole=True` walks a ray by that whole-ray entry point instead, and the host tests pin the one to the other."""
import collections
import ctypes as C
import functools
import math

import numpy as np

import oracle_lib as O
import projection_ref as P
import ref_python
import sky_filter_ref as F
import sky_mipmap_ref as M
from sky_filter_ref import box_average  # noqa: F401  (option "supersample": the one definition; it has to live below this module)

DISC = 2                                       # a ray's code beside O.POSITIVE, O.NEGATIVE, O.NOT_ESCAPED and O.PANIC
COUNTERS = P.COUNTERS + ("n_disc",)
A_MIN, A_MAX = -0.1 * np.pi, 1.1 * np.pi       # src/systems.rs:437-438
_cache = {}


# ---- small helpers --------------------------------------------------------------------------------------------------------------------
def memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frozen(r):
    for v in r.values():
        v.setflags(write=False)
    return r


def _div(n, d):
    """the IEEE quotient (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(n) / np.float64(d))


def index_skies(shapes, salts):
    """common.index_sky of the +l and the -l sky, (w, h) each: computed once per (shapes, salts), shared, read-only"""
    import common

    def make():
        skies = tuple(common.index_sky(w, h, s) for (w, h), s in zip(shapes, salts))
        for t in skies:
            t.setflags(write=False)
        return skies
    return memo(("index skies", tuple(shapes), tuple(salts)), make)


# ---- steppers -------------------------------------------------------------------------------------------------------------------------
def host_new_photon(metric_c, pos, d, x, p):
    from curvis_amd import _abi
    rc = _abi.lib().curvis_new_photon(C.byref(metric_c), O._dp(np.ascontiguousarray(pos, dtype=np.float64)),
                                      O._dp(np.ascontiguousarray(d, dtype=np.float64)), O._dp(x), O._dp(p))
    assert rc == 0, rc


def host_walk_ray(metric_c, x, p, delta, S, integrator, max_iter, max_radius):
    """the library's curvis_walk_ray -- the kernels' loop over the strict step, compiled for x86 -- on (x, p) in place: (code, steps)"""
    from curvis_amd import _abi
    steps, code = C.c_uint32(0), C.c_int32(0)
    rc = _abi.lib().curvis_walk_ray(C.byref(metric_c), O._dp(x), O._dp(p), float(delta), int(S), int(integrator), int(max_iter), float(max_radius),
                                    C.byref(steps), C.byref(code))
    assert rc == 0, rc
    return code.value, steps.value


class OracleStepper:
    """the oracle's photon, Euler step and direction under CVO_CV (Ellis, Interstellar, flat)"""

    def __init__(self, metric):
        self.mp = C.byref(metric)
        self._metric = metric
        self.x, self.p = np.zeros(4), np.zeros(4)
        self.xp, self.pp = O._dp(self.x), O._dp(self.p)
        self.euler = functools.partial(O.lib().cvo_update, O.CV, self.mp, self.xp, self.pp)      # euler(delta_k): one step in place

    def new_photon(self, pos, d):
        O.lib().cvo_new_photon(O.CV, self.mp, O._dp(pos), O._dp(np.ascontiguousarray(d)), self.xp, self.pp)

    def direction(self, out):
        O.lib().cvo_vector_to_direction(O.CV, self.mp, self.pp, self.xp, O._dp(out))

    def walk_ray(self, delta, S, integrator, max_iter, max_radius):
        """the oracle's whole-ray entry point cvo_escape_photon (it knows fixed Euler steps alone): (code, steps)"""
        assert S == 0 and integrator == 0
        steps = C.c_uint32(0)
        code = O.lib().cvo_escape_photon(O.CV, self.mp, self.xp, self.pp, delta, max_iter, max_radius, C.byref(steps))
        return code, steps.value


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
        host_new_photon(self._m, pos, d, self.x, self.p)

    def euler(self, dk):
        assert self._L.curvis_update_relativistic_object(self.mp, self.xp, self.pp, dk) == 0

    def direction(self, out):
        assert self._L.curvis_vector_to_direction(self.mp, self.xp, self.pp, O._dp(out)) == 0

    def walk_ray(self, delta, S, integrator, max_iter, max_radius):
        return host_walk_ray(self._m, self.x, self.p, delta, S, integrator, max_iter, max_radius)


def stepper_of(om, pm):
    """the stepper that walks a scene's rays: the oracle's, or the library's where the oracle has no such metric (om None)"""
    return HostStepper(pm) if om is None else OracleStepper(om)


# ---- the walk -------------------------------------------------------------------------------------------------------------------------
# One ray's record.  plain: steps taken with delta_k == delta; inside: steps taken from |l| < inner (the strict zone); beyond: Heun steps
# whose second stage began beyond the radius; texel, l_hit: the probe's, for a ray that ended on the disc; gaps: crossings that passed a
# transparent texel; sneg, sneg_plane: crossings with s_k < 0 inside the disc's range and anywhere; p_phi: of the final state
Ray = collections.namedtuple("Ray", "code steps plain inside beyond texel l_hit gaps sneg sneg_plane p_phi")


class Walk:
    """one ray's loop over a stepper: buffers and pointers made once, since a frame makes a few hundred thousand oracle calls"""

    def __init__(self, stepper):
        self.st = stepper
        self.x, self.p, self.xp, self.pp, self.mp = stepper.x, stepper.p, stepper.xp, stepper.pp, stepper.mp
        self.cx = (C.c_double * 4).from_buffer(stepper.x)      # the same eight doubles as scalars
        self.cp = (C.c_double * 4).from_buffer(stepper.p)
        self._in, self._out = np.zeros(1), np.zeros(1)
        self._ip, self._op = O._dp(self._in), O._dp(self._out)
        self._math = O.lib().cvo_math_array
        self._cin = (C.c_double * 1).from_buffer(self._in)
        self._cout = (C.c_double * 1).from_buffer(self._out)

    def sincos(self, theta):
        """the oracle's CVO_CV sin and cos"""
        self._cin[0] = theta
        self._math(O.CV, 0, self._ip, None, self._op, 1)
        s = self._cout[0]
        self._math(O.CV, 1, self._ip, None, self._op, 1)
        return s, self._cout[0]

    def heun(self, dk):
        """one Heun step of the state in place: two Euler steps with one delta_k, every integrated component (y_k + y'') * 0.5;
        returns |l'| of the stage state"""
        cx, cp, euler = self.cx, self.cp, self.st.euler
        x0, x1, x2, x3 = cx[0], cx[1], cx[2], cx[3]
        p0, p1, p2, p3 = cp[0], cp[1], cp[2], cp[3]
        euler(dk)
        stage_l = abs(cx[1])
        euler(dk)
        cx[0] = (x0 + cx[0]) * 0.5
        cx[1] = (x1 + cx[1]) * 0.5
        cx[2] = (x2 + cx[2]) * 0.5
        cx[3] = (x3 + cx[3]) * 0.5
        cp[0] = p0
        cp[1] = (p1 + cp[1]) * 0.5
        cp[2] = (p2 + cp[2]) * 0.5
        cp[3] = p3
        return stage_l

    def run(self, delta, S, integrator, max_iter, max_radius, probe=None, inner=None, whole=False):
        """escape_photon (src/systems.rs:115-139) on the stepper's state in place, with delta_k per step: a Ray.

        probe(c_prev, c, s, l_prev, l, phi_prev, phi) -> None or (tx, ty, opaque, l_hit): the plane test between the states before and
        after a step (disc_ref.probe_of); the sine and cosine of theta are evaluated only where there is a probe.
        whole: the stepper's whole-ray entry point walks the ray; of the diagnostics it gives none"""
        cx, cp = self.cx, self.cp
        if whole:
            assert probe is None
            code, steps = self.st.walk_ray(delta, S, integrator, max_iter, max_radius)
            return Ray(code, steps, 0, 0, 0, None, 0.0, 0, 0, 0, cp[3])
        if abs(cx[1]) > max_radius:                                # src/systems.rs:122-124
            return Ray(O.PANIC, 0, 0, 0, 0, None, 0.0, 0, 0, 0, cp[3])
        kap = delta / (float(S) / 256.0) if S else 0.0             # step_scale_ref.kappa
        euler = self.st.euler
        code, steps, plain, inside, beyond, gaps, sneg, sneg_plane = O.NOT_ESCAPED, 0, 0, 0, 0, 0, 0, 0
        c_prev = l_prev = ph_prev = 0.0
        while steps < max_iter:
            l = cx[1]
            if probe is not None:
                ph = cx[3]
                s, c = self.sincos(cx[2])
                if steps >= 1:
                    sneg_plane += ((c_prev < 0.0) != (c < 0.0)) and s < 0.0
                    hit = probe(c_prev, c, s, l_prev, l, ph_prev, ph)
                    if hit is not None:
                        sneg += s < 0.0
                        if hit[2]:
                            return Ray(DISC, steps, plain, inside, beyond, hit[:2], hit[3], gaps, sneg, sneg_plane, cp[3])
                        gaps += 1
                c_prev, l_prev, ph_prev = c, l, ph
            dk = delta
            if S:
                a = abs(l) * kap
                if a > delta:
                    dk = a
            plain += dk == delta
            if inner is not None and abs(l) < inner:
                inside += 1
            if integrator:
                beyond += self.heun(dk) > max_radius
            else:
                euler(dk)
            steps += 1
            if cx[1] > max_radius:
                code = O.POSITIVE
                break
            if cx[1] < -max_radius:
                code = O.NEGATIVE
                break
        return Ray(code, steps, plain, inside, beyond, None, 0.0, gaps, sneg, sneg_plane, cp[3])


# ---- the brute renderer: every ray walked from the camera -----------------------------------------------------------------------------
def compose_brute(stepper, cam_pos, dirs, max_iter, max_radius, delta, S=0, integrator=0, probe=None, inner=None, whole=False):
    """RelativisticSystem::render_image (src/systems.rs:307-330) over the world-space directions dirs [H, W, 3], up to the sky lookup: a
    dict of per-ray arrays -- code, steps, the final state (x, p), the sky direction d of an escaped ray, the disc texel and l_hit of a
    disc ray, and the walk's diagnostics (Ray's fields)"""
    H, W = dirs.shape[:2]
    r = dict(code=np.zeros((H, W), np.int64), steps=np.zeros((H, W), np.int64), x=np.zeros((H, W, 4)), p=np.zeros((H, W, 4)),
             d=np.zeros((H, W, 3)), texel=np.zeros((H, W, 2), np.int64), l_hit=np.zeros((H, W)), p_phi=np.zeros((H, W)))
    diagnostics = ("plain", "inside", "beyond", "gaps", "sneg", "sneg_plane")
    r.update((k, np.zeros((H, W), np.int64)) for k in diagnostics)
    pos = np.array(cam_pos[:], dtype=np.float64)
    w = Walk(stepper)
    d = np.zeros(3)
    for j in range(H):
        for i in range(W):
            stepper.new_photon(pos, dirs[j, i])
            ray = w.run(delta, S, integrator, max_iter, max_radius, probe, inner, whole)
            assert ray.code != O.PANIC
            r["code"][j, i], r["steps"][j, i], r["l_hit"][j, i], r["p_phi"][j, i] = ray.code, ray.steps, ray.l_hit, ray.p_phi
            r["x"][j, i], r["p"][j, i] = stepper.x, stepper.p
            for k in diagnostics:
                r[k][j, i] = getattr(ray, k)
            if ray.code == DISC:
                r["texel"][j, i] = ray.texel
            elif ray.code != O.NOT_ESCAPED:
                stepper.direction(d)
                r["d"][j, i] = d
    return frozen(r)


# ---- the escape angle and the sample table --------------------------------------------------------------------------------------------
class EscapeAngle:
    """compute_escape_angle (src/systems.rs:203-261, tail :144-187, :246-252) in the convention of the kernels' escape_angle_lane: a photon
    at (0, l, pi/2, 0) along (cos a, 0, sin a), walked under S and the integrator, its world direction's angle.  A call returns
    (code, angle, steps): the angle NaN where the photon did not escape, code O.PANIC where the reference panics (the start lies beyond
    the radius, or the tangent rotation is undefined).  calls and steps count every call, as the reference's closure would; classes and
    beyond hold, per call, (code, plain steps, scaled steps, strict-zone steps) and the Heun second stages begun beyond the radius.
    memo: an alpha is walked once"""

    def __init__(self, stepper, l, delta, S, integrator, max_iter, max_radius, inner=None, memo=False, whole=False):
        self.st, self.walk = stepper, Walk(stepper)
        self.l, self.delta, self.S, self.integrator, self.max_iter, self.max_radius = float(l), delta, S, integrator, max_iter, max_radius
        self.inner, self.whole = inner, whole
        self.calls = self.steps = 0
        self.classes, self.beyond = [], []
        self.seen = {} if memo else None

    def _eval(self, alpha):
        L, st = O.lib(), self.st
        a1 = np.array([alpha], dtype=np.float64)
        sa, ca = float(O.math_array(O.CV, 0, a1)[0]), float(O.math_array(O.CV, 1, a1)[0])
        st.new_photon(np.array([0.0, self.l, np.pi / 2.0, 0.0]), np.array([ca, 0.0, sa]))
        ray = self.walk.run(self.delta, self.S, self.integrator, self.max_iter, self.max_radius, None, self.inner, self.whole)
        if ray.code in (O.PANIC, O.NOT_ESCAPED):
            return ray, ray.code, float("nan")
        tdir, wpos, rot, wd = np.zeros(3), np.zeros(3), np.zeros(9), np.zeros(3)
        st.direction(tdir)
        L.cvo_vector3_from_theta_phi(O.CV, float(st.x[2]), float(st.x[3]), O._dp(wpos))
        if L.cvo_rotation_from_two_vectors(O.CV, O._dp(np.array([1.0, 0.0, 0.0])), O._dp(wpos), O._dp(rot)) != 0:
            return ray, O.PANIC, float("nan")
        L.cvo_mat3_vec(O._dp(rot), O._dp(tdir), O._dp(wd))
        x, y, z = float(wd[0]), float(wd[1]), float(wd[2])
        n = math.sqrt(x * x + y * y + z * z)
        x, y, z = x / n, y / n, z / n
        vx = x * 1.0 + y * 0.0 + z * 0.0
        vy = x * 0.0 + y * 1.0 + z * 0.0
        acos = float(O.math_array(O.CV, 3, np.array([vx]))[0])
        return ray, ray.code, (acos if vy >= 0.0 else 2.0 * np.pi - acos)

    def __call__(self, alpha):
        alpha = float(alpha)
        if self.seen is None:
            ray, code, ang = self._eval(alpha)
        else:
            key = alpha.hex()
            if key not in self.seen:
                self.seen[key] = self._eval(alpha)
            ray, code, ang = self.seen[key]
        self.calls += 1
        self.steps += ray.steps
        self.classes.append((ray.code, ray.plain, ray.steps - ray.plain, ray.inside))
        self.beyond.append(ray.beyond)
        return code, ang, ray.steps

    def sample(self, alpha):
        """the closure of src/systems.rs:473-485: (escape angle, escape space), NaN when not escaped"""
        code, ang, _ = self(alpha)
        if code == O.POSITIVE:
            return ang, 1.0
        if code == O.NEGATIVE:
            return ang, -1.0
        assert code != O.PANIC, (self.l, alpha)
        return float("nan"), float("nan")


def sample_table(f, alpha_nums, max_it_sampling, thr1, thr2):
    """doubly_sample_function over the evaluator's closure: (alpha, escape angle, escape space) as float64 arrays"""
    a, e, s = ref_python.doubly_sample_function(A_MIN, A_MAX, alpha_nums, max_it_sampling, thr1, thr2, f.sample)
    return np.array(a, dtype=np.float64), np.array(e, dtype=np.float64), np.array(s, dtype=np.float64)


# ---- the direct and the efficient renderer ----------------------------------------------------------------------------------------------
def _angle_rays(cam, dirs, geometry, pixel):
    """{code, steps, d} over dirs [H, W, 3]: pixel(alpha) -> (code, escape angle, steps); d is the final sky direction (step 5)"""
    alphas, axes, cam_bg = (geometry or P.pixel_geometry(cam, dirs))[:3]
    H, W = alphas.shape
    r = dict(code=np.zeros((H, W), np.int64), steps=np.zeros((H, W), np.int64), d=np.zeros((H, W, 3)))
    with np.errstate(all="ignore"):      # (an optical-axis pixel's rotation axis may be an exact zero and normalise to NaN)
        for j in range(H):
            for i in range(W):
                code, ang, steps = pixel(j, i, alphas[j, i])
                r["steps"][j, i] = steps
                if code in (O.POSITIVE, O.NEGATIVE):      # (a panic of the reference is a black pixel)
                    r["code"][j, i] = code
                    r["d"][j, i] = P._final_direction(axes[j, i], ang, cam_bg)
                else:
                    r["code"][j, i] = O.NOT_ESCAPED
    return frozen(r)


def compose_direct(f, cam, dirs, geometry=None):
    """"direct" mode over dirs: the evaluator f per pixel in place of the table; geometry: projection_ref.pixel_geometry(cam, dirs) where
    the caller has it already"""
    return _angle_rays(cam, dirs, geometry, lambda j, i, alpha: f(float(alpha)))


def compose_efficient(table, cam, dirs, geometry=None):
    """steps 2, 4 and 5 of render_image_efficient (src/systems.rs:333-527) over dirs from a sample table (alpha, escape angle, escape
    space): the oracle's interp_slice at every pixel's alpha; steps are zeros (the sampler's are the evaluator's)"""
    geometry = geometry or P.pixel_geometry(cam, dirs)
    alphas = geometry[0]
    a, e, s = (np.ascontiguousarray(t, dtype=np.float64) for t in table)
    flat = np.ascontiguousarray(alphas.reshape(-1))
    esc, spc = np.zeros(flat.size), np.zeros(flat.size)
    O.lib().cvo_interp_slice(O._dp(a), O._dp(e), a.size, O._dp(flat), flat.size, O._dp(esc))
    O.lib().cvo_interp_slice(O._dp(a), O._dp(s), a.size, O._dp(flat), flat.size, O._dp(spc))
    esc, spc = esc.reshape(alphas.shape), spc.reshape(alphas.shape)

    def pixel(j, i, alpha):
        v = spc[j, i]
        return (O.POSITIVE if v == 1.0 else O.NEGATIVE if v == -1.0 else O.NOT_ESCAPED), esc[j, i], 0
    return _angle_rays(cam, dirs, geometry, pixel)


# ---- per-ray arrays -> counters, debug records, frames ----------------------------------------------------------------------------------
def counters(rays, n_oob, steps=None):
    """(rays, steps, n_pos, n_neg, n_none, n_oob, n_disc): COUNTERS; steps: the sampler's, in place of the rays' sum"""
    c = rays["code"]
    return (c.size, int(rays["steps"].sum() if steps is None else steps), int((c == O.POSITIVE).sum()), int((c == O.NEGATIVE).sum()),
            int((c == O.NOT_ESCAPED).sum()), int(n_oob), int((c == DISC).sum()))


def debug_records(rays, dtype, texel_of):
    """what the brute renderer's debug dump records for walked rays: x, p, steps, code, and for an escaped ray texel_of(code, d) -> (tx, ty)"""
    H, W = rays["code"].shape
    out = np.zeros((H, W), dtype)
    out["x"], out["p"], out["steps"], out["code"] = rays["x"], rays["p"], rays["steps"], rays["code"]
    for j, i in np.argwhere((rays["code"] == O.POSITIVE) | (rays["code"] == O.NEGATIVE)):
        out["tx"][j, i], out["ty"][j, i] = texel_of(rays["code"][j, i], np.ascontiguousarray(rays["d"][j, i]))
    return out


def _paint_disc(rays, disc, rgb):
    m = rays["code"] == DISC
    if m.any():
        rgb[m] = disc.rgba[rays["texel"][m][:, 1], rays["texel"][m][:, 0], :3]


def frame_nearest(rays, disc, oracle_skies, steps=None):
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
    return rgb, counters(rays, oob, steps)


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


def frame_bilinear(rays, disc, skies, steps=None):
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
    return rgb, counters(rays, oob, steps)


def frame_mipmap(rays, disc, skies, steps=None):
    """option "sky_mipmap" = 1 on top: sky_mipmap_ref.mip_frame over the decoded rays -- a disc ray is which = -1 there, a quad partner
    that saw no sky -- then the disc rays take their texel"""
    which, Xc, Yc, oob = decode_sky_rays(rays, skies)
    rgb = np.array(M.mip_frame(which, Xc, Yc, skies)[0])
    _paint_disc(rays, disc, rgb)
    return rgb, counters(rays, oob, steps)


def frame(rays, disc, lookup, images, oracle_skies, steps=None):
    """(read-only frame, counters) of per-ray arrays under a lookup -- "nearest" (over the oracle's skies), "bilinear" or "mipmap" (over
    the sky images); disc None: no ray ended on one"""
    if lookup == "nearest":
        out = frame_nearest(rays, disc, oracle_skies, steps)
    else:
        out = (frame_bilinear if lookup == "bilinear" else frame_mipmap)(rays, disc, images, steps)
    out[0].setflags(write=False)
    return out
