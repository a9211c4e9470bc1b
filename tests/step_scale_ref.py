"""Library option "step_scale" (an integer S; L0 = S / 256): the definition in Python doubles, written from the option's paragraph in
include/curvis_hip.h, and each renderer's frame composed per ray from primitives of the CPU oracle that exist already.  Nothing here
calls the product, and nothing is added to the oracle.

  kappa   = RN(delta / L0)                       one IEEE division per call
  a       = RN(|l_k| kappa)                      l_k: the radial coordinate BEFORE step k
  delta_k = a if a > delta else delta            (a NaN l_k fails the compare)
and step k is the oracle's own Euler step cvo_update(..., delta_k) under CVO_CV, followed by the reference's escape test.  S = 0 means
delta_k = delta: then every composition below is the oracle's own entry point bit for bit (tests/test_step_scale_host.py pins that
before anything here is trusted)."""
import ctypes as C
import math

import numpy as np

import common
import oracle_lib as O
import projection_ref as P
import ref_python

COUNTERS = P.COUNTERS
S_MAX = 1 << 20


def kappa(delta, S):
    return delta / (float(S) / 256.0)


def step_delta(delta, S, l, k=None):
    """delta_k of the definition (Python floats are IEEE doubles; one multiply, one compare)"""
    if S == 0:
        return delta
    a = abs(l) * (kappa(delta, S) if k is None else k)
    return a if a > delta else delta


class Walk:
    """one ray's loop: buffers and pointers made once, since a frame makes a few hundred thousand oracle calls"""

    def __init__(self, metric):
        self.metric = metric
        self.mp = C.byref(metric)
        self.x, self.p = np.zeros(4), np.zeros(4)
        self.xp, self.pp = O._dp(self.x), O._dp(self.p)
        self.update = O.lib().cvo_update

    def run(self, delta, S, max_iter, max_radius, inner=None):
        """escape_photon (src/systems.rs:115-139) on (self.x, self.p) in place with delta_k per step:
        (code, steps, steps taken with delta_k == delta, steps taken from |l| < inner)"""
        x, xp, pp, mp, update = self.x, self.xp, self.pp, self.mp, self.update
        if abs(x[1]) > max_radius:
            return O.PANIC, 0, 0, 0
        k = kappa(delta, S) if S else 0.0
        code, steps, plain, inside = O.NOT_ESCAPED, 0, 0, 0
        while steps < max_iter:
            l = float(x[1])
            dk = delta
            if S:
                a = abs(l) * k
                if a > delta:
                    dk = a
            plain += dk == delta
            if inner is not None and abs(l) < inner:
                inside += 1
            update(O.CV, mp, xp, pp, dk)
            steps += 1
            if x[1] > max_radius:
                code = O.POSITIVE
                break
            if x[1] < -max_radius:
                code = O.NEGATIVE
                break
        return code, steps, plain, inside


def strict_radius(metric):
    """Interstellar: the fast step's guard sends |l| < a + pi m to the strict step"""
    return metric.a + math.pi * metric.m if metric.kind == O.INTERSTELLAR else None


def compose_brute(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta, S):
    """RelativisticSystem::render_image over the world-space directions dirs [H, W, 3] with scaled steps:
    (frame, counters, debug records [H, W] of O.RAY_DEBUG, classes) -- classes: per ray (plain steps, scaled steps, strict-zone steps)"""
    L = O.lib()
    H, W = dirs.shape[:2]
    rgb = np.zeros((H, W, 3), np.uint8)
    dbg = np.zeros((H, W), O.RAY_DEBUG)
    classes = np.zeros((H, W, 3), np.int64)
    cnt = dict.fromkeys(COUNTERS, 0)
    pos = np.array(cam.pos[:])
    d = np.zeros(3)
    w = Walk(metric)
    inner = strict_radius(metric)
    tx, ty = C.c_uint32(0), C.c_uint32(0)
    for j in range(H):
        for i in range(W):
            L.cvo_new_photon(O.CV, w.mp, O._dp(pos), O._dp(np.ascontiguousarray(dirs[j, i])), w.xp, w.pp)
            code, steps, plain, inside = w.run(delta, S, max_iter, max_radius, inner)
            assert code != O.PANIC
            r = dbg[j, i]
            r["x"], r["p"], r["steps"], r["code"] = w.x, w.p, steps, code
            classes[j, i] = (plain, steps - plain, inside)
            cnt["rays"] += 1
            cnt["steps"] += steps
            if code in (O.POSITIVE, O.NEGATIVE):
                sky = sky_pos if code == O.POSITIVE else sky_neg
                L.cvo_vector_to_direction(O.CV, w.mp, w.pp, w.xp, O._dp(d))
                L.cvo_sky_indices(O.CV, C.byref(sky), O._dp(d), C.byref(tx), C.byref(ty))
                r["tx"], r["ty"] = tx.value, ty.value
                cnt["n_oob"] += P._shade(sky, d, rgb[j, i])
                cnt["n_pos" if code == O.POSITIVE else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in COUNTERS), dbg, classes


class EscapeAngle:
    """compute_escape_angle (src/systems.rs:203-261, tail :144-187, :246-252) with scaled steps, from the oracle's primitives"""

    def __init__(self, metric, l, delta, S, max_iter, max_radius):
        self.w = Walk(metric)
        self.l, self.delta, self.S, self.max_iter, self.max_radius = l, delta, S, max_iter, max_radius
        self.inner = strict_radius(metric)
        self.calls = self.steps = 0
        self.classes = []       # per call: (code, plain steps, scaled steps, strict-zone steps)

    def __call__(self, alpha):
        """(code, angle, steps)"""
        L, w = O.lib(), self.w
        a1 = np.array([alpha])
        sa, ca = float(O.math_array(O.CV, 0, a1)[0]), float(O.math_array(O.CV, 1, a1)[0])
        pos = np.array([0.0, self.l, np.pi / 2.0, 0.0])
        L.cvo_new_photon(O.CV, w.mp, O._dp(pos), O._dp(np.array([ca, 0.0, sa])), w.xp, w.pp)
        code, steps, plain, inside = w.run(self.delta, self.S, self.max_iter, self.max_radius, self.inner)
        self.calls += 1
        self.steps += steps
        self.classes.append((code, plain, steps - plain, inside))
        if code in (O.PANIC, O.NOT_ESCAPED):
            return code, 0.0, steps
        tdir, wpos, rot, wd = np.zeros(3), np.zeros(3), np.zeros(9), np.zeros(3)
        L.cvo_vector_to_direction(O.CV, w.mp, w.pp, w.xp, O._dp(tdir))
        L.cvo_vector3_from_theta_phi(O.CV, float(w.x[2]), float(w.x[3]), O._dp(wpos))
        if L.cvo_rotation_from_two_vectors(O.CV, O._dp(np.array([1.0, 0.0, 0.0])), O._dp(wpos), O._dp(rot)) != 0:
            return O.PANIC, 0.0, steps
        L.cvo_mat3_vec(O._dp(rot), O._dp(tdir), O._dp(wd))
        x, y, z = float(wd[0]), float(wd[1]), float(wd[2])
        n = math.sqrt(x * x + y * y + z * z)
        x, y, z = x / n, y / n, z / n
        vx = x * 1.0 + y * 0.0 + z * 0.0
        vy = x * 0.0 + y * 1.0 + z * 0.0
        acos = float(O.math_array(O.CV, 3, np.array([vx]))[0])
        return code, (acos if vy >= 0.0 else 2.0 * np.pi - acos), steps

    def sample(self, alpha):
        """the closure of src/systems.rs:473-485: (escape angle, escape space), NaN when not escaped"""
        code, ang, _ = self(alpha)
        if code == O.POSITIVE:
            return ang, 1.0
        if code == O.NEGATIVE:
            return ang, -1.0
        assert code != O.PANIC
        return float("nan"), float("nan")


def sample_table(metric, l, delta, S, max_iter, max_radius, alpha_nums, max_it_sampling, thr1, thr2):
    """doubly_sample_function over the composed closure: (alpha, escape angle, escape space) arrays, the evaluator (calls, steps, classes)"""
    f = EscapeAngle(metric, l, delta, S, max_iter, max_radius)
    a, e, s = ref_python.doubly_sample_function(-0.1 * np.pi, 1.1 * np.pi, alpha_nums, max_it_sampling, thr1, thr2, f.sample)
    return np.array(a), np.array(e), np.array(s), f


def compose_efficient(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta, S, alpha_nums, max_it_sampling, thr1, thr2):
    """render_image_efficient over dirs with scaled steps in its sampler: (frame, counters -- steps are the sampler's --, table, evaluator)"""
    L = O.lib()
    H, W = dirs.shape[:2]
    alphas, axes, cam_bg = P.pixel_geometry(cam, dirs)
    ta, te, ts, f = sample_table(metric, cam.pos[1], delta, S, max_iter, max_radius, alpha_nums, max_it_sampling, thr1, thr2)
    flat = np.ascontiguousarray(alphas.reshape(-1))
    esc, spc = np.zeros(flat.size), np.zeros(flat.size)
    L.cvo_interp_slice(O._dp(ta), O._dp(te), ta.size, O._dp(flat), flat.size, O._dp(esc))
    L.cvo_interp_slice(O._dp(ta), O._dp(ts), ta.size, O._dp(flat), flat.size, O._dp(spc))
    esc, spc = esc.reshape(H, W), spc.reshape(H, W)
    rgb = np.zeros((H, W, 3), np.uint8)
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["steps"] = f.steps
    for j in range(H):
        for i in range(W):
            cnt["rays"] += 1
            s = spc[j, i]
            if s == 1.0 or s == -1.0:
                fin = P._final_direction(axes[j, i], esc[j, i], cam_bg)
                cnt["n_oob"] += P._shade(sky_pos if s == 1.0 else sky_neg, fin, rgb[j, i])
                cnt["n_pos" if s == 1.0 else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in COUNTERS), (ta, te, ts), f


def compose_direct(metric, cam, dirs, sky_pos, sky_neg, max_iter, max_radius, delta, S):
    """"direct" mode with scaled steps: (frame, counters, evaluator)"""
    H, W = dirs.shape[:2]
    alphas, axes, cam_bg = P.pixel_geometry(cam, dirs)
    f = EscapeAngle(metric, cam.pos[1], delta, S, max_iter, max_radius)
    rgb = np.zeros((H, W, 3), np.uint8)
    cnt = dict.fromkeys(COUNTERS, 0)
    for j in range(H):
        for i in range(W):
            code, ang, steps = f(float(alphas[j, i]))
            cnt["rays"] += 1
            cnt["steps"] += steps
            if code in (O.POSITIVE, O.NEGATIVE):
                fin = P._final_direction(axes[j, i], ang, cam_bg)
                cnt["n_oob"] += P._shade(sky_pos if code == O.POSITIVE else sky_neg, fin, rgb[j, i])
                cnt["n_pos" if code == O.POSITIVE else "n_neg"] += 1
            else:
                cnt["n_none"] += 1
    return rgb, tuple(cnt[k] for k in COUNTERS), f


def box_average(fine, n):
    """option "supersample" (include/curvis_hip.h): out = (sum of the n x n block + n^2 / 2) >> (2 log2 n)"""
    H, W = fine.shape[0] // n, fine.shape[1] // n
    s = fine.astype(np.uint32).reshape(H, n, W, n, 3).sum(axis=(1, 3))
    return ((s + n * n // 2) >> (2 * int(math.log2(n)))).astype(np.uint8)


# ---- the scenes of the GPU tests ---------------------------------------------------------------------------------------------------
R, DELTA = 30.0, 0.05
SKY_SHAPES = ((1000, 500), (333, 777))      # +l, -l (w, h)
SKY_SALTS = (0x5C3A71, 0x1BE4D2)
RES, RES_RAGGED = (40, 24), (37, 19)
EFF = dict(n0=100, maxit=100, t1=1e-5, t2=1e-5)
HALF_PI = np.pi / 2
# name -> (metric, position, forward, up, focal)
POSES = {
    "facing": ((0.0, 5.0, HALF_PI, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0),
    "tilted": ((0.0, 3.0, 0.9, 0.4), (-1.0, 0.1, 0.6), (0.0, 0.0, 1.0), 9.0),          # rays cross the poles
    "negative": ((0.0, -4.0, HALF_PI, 0.3), (1.0, 0.05, 0.1), (0.0, 0.0, 1.0), 12.0),
    "inside": ((0.0, 0.3, 1.2, 0.0), (-0.2, 1.0, 0.1), (0.0, 0.0, 1.0), 10.0),          # starts inside L0, looks across the throat
}
INTERSTELLAR = (0.5, 2.0, 1.0)              # m, a, rho: a throat long enough that strict steps (|l| < a + pi m) occur
_cache = {}


def metrics(kind):
    """(oracle metric, product metric)"""
    import curvis_amd
    if kind == "ellis":
        return O.ellis(1.0), curvis_amd.EllisMetric(1.0)
    if kind == "interstellar":
        return O.interstellar(*INTERSTELLAR), curvis_amd.InterstellarMetric(*INTERSTELLAR)
    return O.flat(), curvis_amd.FlatSphericalMetric()


def cameras(pose, res):
    """(oracle camera, product camera)"""
    import curvis_amd
    pos, fwd, up, focal = POSES[pose]
    return O.camera(pos, fwd, up, focal, 43.0, res), curvis_amd.Camera(pos, fwd, up, focal, 43.0, res[0], res[1])


def index_skies():
    if "skies" not in _cache:
        _cache["skies"] = tuple(common.index_sky(w, h, s) for (w, h), s in zip(SKY_SHAPES, SKY_SALTS))
        for t in _cache["skies"]:
            t.setflags(write=False)
    return _cache["skies"]


def oracle_skies():
    if "oskies" not in _cache:
        _cache["oskies"] = tuple(O.sky(np.array(t)) for t in index_skies())
    return _cache["oskies"]


def world_dirs(oc, projection=P.PERSPECTIVE):
    return P.outward_vectors(oc, projection)[1]


def fine_oracle_skies():
    """option "sky_filter": the index skies of 256 w x 256 h texels that tests/sky_filter_ref.py decodes the filter's taps from"""
    import sky_filter_ref as F
    if "ofine" not in _cache:
        _cache["ofine"] = tuple(O.sky(img) for img in F.fine_skies())
    return _cache["ofine"]


def expected(renderer, kind, pose, S, res=RES, cap=4096, projection=P.PERSPECTIVE, skies="index", max_radius=R):
    """the composition for a scene (skies: "index", or "fine" for the filter's virtual skies); computed once, shared, read-only"""
    key = (renderer, kind, pose, S, res, cap, projection, skies, max_radius)
    if key not in _cache:
        om = metrics(kind)[0]
        oc = cameras(pose, res)[0]
        sp, sn = oracle_skies() if skies == "index" else fine_oracle_skies()
        dirs = world_dirs(oc, projection)
        if renderer == "brute":
            out = compose_brute(om, oc, dirs, sp, sn, cap, max_radius, DELTA, S)
        elif renderer == "direct":
            out = compose_direct(om, oc, dirs, sp, sn, cap, max_radius, DELTA, S)
        else:
            out = compose_efficient(om, oc, dirs, sp, sn, cap, max_radius, DELTA, S, EFF["n0"], EFF["maxit"], EFF["t1"], EFF["t2"])
        out[0].setflags(write=False)
        _cache[key] = out
    return _cache[key]


def assert_brute_classes(kind, pose, S, res=RES, cap=4096, projection=P.PERSPECTIVE, skies="index", capped=False, neg=True, least=8):
    """what a brute case relies on, from the composition alone: at least 8 rays escaped to +l, to -l (where the scene has a far side),
    capped ones where the case is about them, rays with plain steps and rays with scaled steps, and -- Interstellar -- rays with
    steps inside the strict zone"""
    _, st, dbg, classes = expected("brute", kind, pose, S, res, cap, projection, skies)
    who = (kind, pose, S, res, cap, st)
    assert st[2] >= least, who
    if neg:
        assert st[3] >= least, who
    if capped:
        assert st[4] >= least, who
    assert (classes[..., 0] > 0).sum() >= least and (classes[..., 1] > 0).sum() >= least, who
    if kind == "interstellar":
        assert (classes[..., 2] > 0).sum() >= least, who


def assert_angle_classes(f, kind, least=8, neg=True):
    """the same for the evaluator of a direct or efficient composition"""
    c = np.array(f.classes)
    assert (c[:, 0] == O.POSITIVE).sum() >= least, kind
    if neg:
        assert (c[:, 0] == O.NEGATIVE).sum() >= least, kind
    assert (c[:, 1] > 0).sum() >= least and (c[:, 2] > 0).sum() >= least, kind
    if kind == "interstellar":
        assert (c[:, 3] > 0).sum() >= least, kind
