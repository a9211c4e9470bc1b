"""The kernel lattices of the direct and the efficient renderer, with the reference frame, table and counters of every cell:

  direct_kernel<KIND, FAST, SS, FILTER, PROJ, ADAPT>      metric kind x step form x supersample x lookup x projection, 384 forms
  escape_angle_kernel / sampler_kernel<KIND, FAST, ADAPT>  metric kind x step form, 16 forms each (host-paced and device sampler)
  efficient_pixel_kernel<FILTER, PROJ>                     4 forms, and
  efficient_pixel_ss_kernel<SS, FILTER, PROJ>              24 forms: 28 pixel forms (pixel_forms())

The vocabulary and the grids are tests/kernel_matrix_ref.py's, unchanged; so are the scenes of the flat and the Schwarzschild kind and the
camera positions of the other two, whose cameras are turned towards the throat (MOVED says why).  The enumeration is written from with_launch_shape
(curvis_amd/csrc/render_host.h) and from the launches in curvis_amd/csrc/efficient_host.h; nothing of it is read from the product.

The reference composes what tests/ref_compose.py holds: its equatorial escape-angle evaluator over the kind's stepper under the step
option and the integrator, an alpha walked once; its direct and efficient compositions over projection_ref's pixel geometry; its sample
table; its three lookups over a {code, steps, d} array; and box_average.  Every walk, table and fine frame is computed once, shared and
read-only.  No GPU."""
import math

import numpy as np

import disc_ref as D
import oracle_lib as O
import projection_ref as P
import ref_compose as RC
import step_scale_ref as SR
import kernel_matrix_ref as K
from kernel_matrix_ref import (KINDS, STEPS, SUPERSAMPLES, LOOKUPS, PROJECTIONS, STEP_OPTIONS, STEP_WALKS, LOOKUP_OPTIONS, cell_options,  # noqa: F401
                               GRIDS, product_res, scene_parameters, R, DELTA, CAP)

EFF = SR.EFF                                   # n0 = 100, maxit = 100, thresholds 1e-5
A_MIN, A_MAX = RC.A_MIN, RC.A_MAX
# scaled Heun steps: the walk of "everything at once" -- not one of the four step forms, both options of the ADAPT = 2 kernels at once
EVERYTHING = "everything"
WALKS = dict(STEP_WALKS, everything=(K.STEP_SCALE, 1))
WALK_OPTIONS = dict(STEP_OPTIONS, everything=dict(step_scale=K.STEP_SCALE, integrator=1))
memo = RC.memo


# ---- the enumerations ------------------------------------------------------------------------------------------------------------------
def direct_cells():
    """the 384 forms of direct_kernel: kernel_matrix_ref's lattice"""
    return K.cells()


def table_forms():
    """the 16 forms of either table kernel: (kind, step)"""
    return [(kind, step) for kind in KINDS for step in STEPS]


def pixel_forms():
    """the 28 forms of the efficient renderer's pixel kernels: (supersample, lookup, projection, pixel_tiled, kernel) -- the option
    "pixel_tiled" that reaches the form, and kernel = ("linear", FILTER, PROJ) or ("ss", SS, FILTER, PROJ).  The 24 cells of
    kernel_matrix_ref.inner_cells() with pixel_tiled = 0 -- supersample 1 with the nearest or the bilinear lookup takes the linear
    kernel -- and the four forms efficient_pixel_ss_kernel<1, 0 | 1, PROJ> that pixel_tiled = 1 alone reaches"""
    out = []
    for n, lookup, projection in K.inner_cells():
        filt, proj = LOOKUPS.index(lookup), PROJECTIONS.index(projection)
        linear = n == 1 and lookup != "mipmap"
        out.append((n, lookup, projection, 0, ("linear", filt, proj) if linear else ("ss", n, filt, proj)))
        if linear:
            out.append((n, lookup, projection, 1, ("ss", 1, filt, proj)))
    return out


# what the host-paced sampler's leg renders: the four forms inner_cells() does not separate -- linear and tiled, nearest and bilinear
HOST_PACED_FORMS = ((1, "nearest", "perspective", 0), (1, "nearest", "fisheye", 1), (1, "bilinear", "fisheye", 0), (1, "bilinear", "perspective", 1))


# ---- the equatorial escape-angle evaluator -----------------------------------------------------------------------------------------------
def metrics_of(kind):
    """(oracle metric or None, product metric): disc_ref.scene_from's"""
    sc = K.scene(kind, GRIDS[1])
    return sc[1], sc[2]


# Ellis and Interstellar: kernel_matrix_ref's cameras TURNED AND ZOOMED -- their frames look past the throat (a disc cell wants the disc),
# and at these grids hold 7 (20 x 12) and 2 to 5 (16 x 8) pixels on -l where a cell here wants 8 --: the same positions, so the same
# tables, looking almost straight at the throat through a longer lens.  name -> (forward, focal)
MOVED = {"ellis": ((-1.0, 0.02, -0.03), 26.0), "interstellar": ((-1.0, 0.02, -0.03), 26.0)}


def camera_parameters(kind):
    """(position, forward, up, focal) of a kind's camera: kernel_matrix_ref's scene, moved where MOVED says so"""
    pos, fwd, up, focal, _ = scene_parameters(kind)
    if kind in MOVED:
        fwd, focal = MOVED[kind]
    return pos, fwd, up, focal


def camera_radius(kind):
    return float(scene_parameters(kind)[0][1])


def evaluator(kind, step, l=None, cap=CAP):
    """the one evaluator of (kind, step walk, camera radius, cap)"""
    S, integrator = WALKS[step]
    l = camera_radius(kind) if l is None else float(l)
    return memo(("evaluator", kind, S, integrator, l, cap),
                lambda: RC.EscapeAngle(RC.stepper_of(*metrics_of(kind)), l, DELTA, S, integrator, cap, R, memo=True))


# ---- cameras and geometry ---------------------------------------------------------------------------------------------------------------
def cameras(kind, grid, supersample=1, pose=None):
    """(oracle camera over the fine grid, product camera over grid / supersample); pose: (position, forward) in place of the scene's"""
    import curvis_amd
    pos, fwd, up, focal = camera_parameters(kind)
    if pose is not None:
        pos, fwd = pose
    w, h = grid[0] // supersample, grid[1] // supersample
    return O.camera(pos, fwd, up, focal, D.DIAG, grid), curvis_amd.Camera(pos, fwd, up, focal, D.DIAG, w, h)


def geometry(kind, projection, grid, pose=None):
    """(alpha [H, W], rotation axes [H, W, 3], cam_bg, unit camera-space vectors [H, W, 3]) of the fine grid's pixels"""
    def make():
        oc = cameras(kind, grid, 1, pose)[0]
        unit, dirs = P.outward_vectors(oc, K.PROJECTION_OPTION[projection])
        assert projection != "fisheye" or P.fisheye_in_range(oc)      # (the fisheye definition has no image circle to fall outside of)
        with np.errstate(all="ignore"):
            return P.pixel_geometry(oc, dirs) + (unit,)
    return memo(("geometry", kind, projection, grid, pose), make)


def optical_axis_pixels(kind, projection, grid, pose=None):
    """(pixels whose camera-space vector is the optical axis exactly, those of them whose rotation axis does not normalise: NaN)"""
    _, axes, _, unit = geometry(kind, projection, grid, pose)
    on_axis = (unit[..., 0] == 1.0) & (unit[..., 1] == 0.0) & (unit[..., 2] == 0.0)
    with np.errstate(all="ignore"):
        n = np.sqrt((axes[..., 0] * axes[..., 0] + axes[..., 1] * axes[..., 1]) + axes[..., 2] * axes[..., 2])
        nan_axis = ~np.isfinite(axes[..., 0] / n)
    return int(on_axis.sum()), int((on_axis & nan_axis).sum())


# ---- the direct renderer -----------------------------------------------------------------------------------------------------------------
def _direct_rays(kind, step, projection, grid, cap=CAP, pose=None):
    S, integrator = WALKS[step]
    l = camera_radius(kind) if pose is None else float(pose[0][1])

    def make():
        return RC.compose_direct(evaluator(kind, step, l, cap), None, None, geometry(kind, projection, grid, pose))
    return memo(("direct rays", kind, S, integrator, projection, grid, cap, pose), make)


def direct_rays(kind, step, projection, grid):
    """{code, steps, d} of the direct renderer's rays over a fine grid, d the final sky direction; one walk set per (kind, step walk,
    projection, grid): the strict and the fast step share it"""
    return _direct_rays(kind, step, projection, grid)


def compose(rays, lookup, steps=None):
    """(frame, (rays, steps, n_pos, n_neg, n_none, n_oob)) of a {code, steps, d} array under a lookup; steps: the sampler's, in place of
    the rays' sum"""
    rgb, cnt = RC.frame(rays, None, lookup, SR.index_skies(), SR.oracle_skies(), steps)
    return rgb, cnt[:6]


def _resolve(fine, supersample):
    out = fine[0] if supersample == 1 else SR.box_average(fine[0], supersample)
    out.setflags(write=False)
    return out, fine[1]


def direct_fine(kind, step, projection, grid, lookup):
    S, integrator = WALKS[step]
    return memo(("direct fine", kind, S, integrator, projection, grid, lookup), lambda: compose(direct_rays(kind, step, projection, grid), lookup))


def direct_cell(kind, step, supersample, lookup, projection):
    """what render_direct returns for a cell: (frame, six counters); the counters are the fine grid's"""
    return _resolve(direct_fine(kind, step, projection, GRIDS[supersample], lookup), supersample)


# ---- the efficient renderer ----------------------------------------------------------------------------------------------------------------
TIGHT = (EFF["t1"], EFF["t2"])       # the thresholds of every cell ...
LOOSE = (1e-3, 1e-3)                 # ... but, on the device sampler, of the forms whose table outgrows it at TIGHT (device_thresholds)
SAMPLER_CAP = 1536                   # cv_sampler_dev.h kSamplerCap: samples a device table may hold
AIMED = "aimed"


def table(kind, step, l=None, cap=CAP, thr=TIGHT):
    """the sample table of (kind, step walk, camera radius, thresholds): dict a, e, s (float64 arrays) and n, calls, steps, rounds,
    warned, peak (its largest size after any round) -- ref_python.doubly_sample_function over the evaluator.  The function returns the
    table alone.  The evaluator's own counters give calls and steps.  rounds and warned follow from running it again with
    max_iterations = 0, 1, 2 ...: every executed round changes the pair (table, calls) -- it either evaluates new points or, refining
    nothing, drops the last two (its loop ends at n - 2) --, so the number of rounds the full run executed is the smallest
    max_iterations that gives the full run's pair, and the run ended at max_iterations without a break -- the warning -- where one more
    iteration would change the pair again.  (A returned table is finite: the function cleans it.)  tests/test_efficient_matrix_host.py
    pins all five numbers to the oracle's own sampler for the kinds and the step it knows"""
    S, integrator = WALKS[step]
    l = camera_radius(kind) if l is None else float(l)

    def run(f, maxit):
        calls, steps = f.calls, f.steps

        a, e, s = RC.sample_table(f, EFF["n0"], maxit, thr[0], thr[1])
        return (a.tolist(), e.tolist(), s.tolist()), f.calls - calls, f.steps - steps

    def make():
        f = evaluator(kind, step, l, cap)
        full = run(f, EFF["maxit"])
        rounds = next(k for k in range(EFF["maxit"] + 1) if run(f, k)[:2] == full[:2])
        peak = max(len(run(f, k)[0][0]) for k in range(rounds + 1))
        warned = int(rounds == EFF["maxit"] and run(f, EFF["maxit"] + 1)[:2] != full[:2])
        (a, e, s), calls, steps = full
        t = dict(a=np.array(a, dtype=np.float64), e=np.array(e, dtype=np.float64), s=np.array(s, dtype=np.float64))
        RC.frozen(t)
        t.update(n=len(a), calls=calls, steps=steps, rounds=rounds, warned=warned, peak=peak)
        return t
    return memo(("table", kind, S, integrator, l, cap, thr), make)


def bookkeeping(t):
    return t["n"], t["calls"], t["steps"], t["rounds"], t["warned"]


def efficient_args(cap=CAP, thr=TIGHT):
    return (cap, R, DELTA, EFF["n0"], EFF["maxit"], thr[0], thr[1])


def sampler_path(tables, device_sampler):
    """what "last_sampler_path" reports for a call over these tables: 0 the host-paced sampler; 1 the device sampler; 2 the device
    sampler ran out of room -- a table grew past SAMPLER_CAP between two rounds -- and the host-paced one took the call"""
    if not device_sampler:
        return 0
    return 2 if any(t["peak"] > SAMPLER_CAP for t in tables) else 1


def device_thresholds(kind, step, radii=None):
    """the thresholds of a form's cells behind the DEVICE sampler: TIGHT where every table of the call fits it, else LOOSE.  At TIGHT the
    flat kind's tables (the escape angle jumps by 2 pi at alpha = 0 and is refined there until the abscissae meet), the scaled
    Interstellar and Schwarzschild tables and their scaled Heun ones outgrow it, the call falls back to the host-paced sampler, and the
    device table would never be compared; at LOOSE they hold a few hundred samples"""
    radii = radii or (camera_radius(kind),)
    if sampler_path([table(kind, step, l) for l in radii], 1) == 1:
        return TIGHT
    assert sampler_path([table(kind, step, l, thr=LOOSE) for l in radii], 1) == 1, (kind, step, radii)
    return LOOSE


def edge_interval(t):
    """(a_i, a_i+1) of the first pair of neighbouring samples on different skies -- in between the interpolated escape space is neither
    +1 nor -1 --, or None"""
    i = np.nonzero(t["s"][:-1] != t["s"][1:])[0]
    return (float(t["a"][i[0]]), float(t["a"][i[0] + 1])) if len(i) else None


def aimed_pose(kind, step, projection, grid, thr=TIGHT):
    """the pose of an efficient cell: the scene's position, the camera turned in the equatorial plane -- forward (cos psi, sin psi, 0) --
    until the alpha of pixel (W / 2, H / 2) lies in the middle of the table's edge interval, some 1e-6 rad wide: that pixel is black.
    Under the perspective projection the pixel is on the optical axis and alpha = psi; under the fisheye one it is half a pixel off.  psi
    is found by bisection on the reference's own alpha.  None for the flat kind: the scene's pose"""
    S, integrator = WALKS[step]

    def make():
        iv = edge_interval(table(kind, step, thr=thr))
        if iv is None or kind == "flat":      # (flat: only the ray through the origin changes sides, at alpha = pi, out of a fisheye pixel's reach)
            return None
        pos, _, up, focal = camera_parameters(kind)
        px, py = np.array([grid[0] // 2]), np.array([grid[1] // 2])
        quarter = 0.25 * (iv[1] - iv[0])

        def alpha(psi):
            oc = O.camera(pos, (math.cos(psi), math.sin(psi), 0.0), up, focal, D.DIAG, grid)
            return float(P.pixel_geometry(oc, P.outward_vectors(oc, K.PROJECTION_OPTION[projection], px, py)[1])[0][0])
        lo, hi = iv[0] - 0.4, min(iv[1] + 0.4, math.pi)
        assert alpha(lo) < iv[0] and alpha(hi) > iv[1], (kind, step, projection, grid, alpha(lo), alpha(hi), iv)
        for _ in range(80):
            psi = 0.5 * (lo + hi)
            a = alpha(psi)
            if iv[0] + quarter <= a <= iv[1] - quarter:
                return tuple(pos), (math.cos(psi), math.sin(psi), 0.0)
            lo, hi = (psi, hi) if a < iv[0] + quarter else (lo, psi)
        raise AssertionError(("no pose found", kind, step, projection, grid, iv))
    return memo(("aimed pose", kind, S, integrator, projection, grid, thr), make)


def _pose(kind, step, projection, grid, pose, thr):
    return aimed_pose(kind, step, projection, grid, thr) if pose == AIMED else pose


def efficient_camera(kind, step, supersample, projection, thr=TIGHT):
    """the product camera of an efficient cell"""
    grid = GRIDS[supersample]
    return cameras(kind, grid, supersample, aimed_pose(kind, step, projection, grid, thr))[1]


def _efficient_rays(kind, step, projection, grid, pose=None, thr=TIGHT):
    S, integrator = WALKS[step]
    l = camera_radius(kind) if pose is None else float(pose[0][1])

    def make():
        t = table(kind, step, l, thr=thr)
        return RC.compose_efficient((t["a"], t["e"], t["s"]), None, None, geometry(kind, projection, grid, pose))
    return memo(("efficient rays", kind, S, integrator, projection, grid, pose, thr), make)


def efficient_rays(kind, step, projection, grid, pose=AIMED, thr=TIGHT):
    """{code, steps (zeros), d} of the efficient renderer's pixels over a fine grid: the table interpolated at every pixel's alpha;
    pose: AIMED (a cell's), None (the scene's) or an explicit one"""
    return _efficient_rays(kind, step, projection, grid, _pose(kind, step, projection, grid, pose, thr), thr)


def efficient_fine(kind, step, projection, grid, lookup, pose=AIMED, thr=TIGHT):
    S, integrator = WALKS[step]
    pose = _pose(kind, step, projection, grid, pose, thr)
    l = camera_radius(kind) if pose is None else float(pose[0][1])
    return memo(("efficient fine", kind, S, integrator, projection, grid, lookup, pose, thr),
                lambda: compose(_efficient_rays(kind, step, projection, grid, pose, thr), lookup, table(kind, step, l, thr=thr)["steps"]))


def efficient_cell(kind, step, supersample, lookup, projection, thr=TIGHT):
    """what render_efficient returns for a cell: (frame, six counters); rays are the fine grid's pixels, steps the sampler's"""
    return _resolve(efficient_fine(kind, step, projection, GRIDS[supersample], lookup, thr=thr), supersample)


# ---- the ray classes a cell relies on, from the reference alone ------------------------------------------------------------------------------
def classes(rays):
    c = rays["code"]
    return int((c == O.POSITIVE).sum()), int((c == O.NEGATIVE).sum()), int((c == O.NOT_ESCAPED).sum())


def assert_classes(rays, kind, renderer, who):
    """at least 8 pixels on +l; 8 on -l for Ellis and Interstellar; at least 4 pixels of the Schwarzschild shadow: the rays the hole
    captured, which leave through -l and take the -l sky's colour (nothing of this kind's frames is black below the step cap); and in
    the efficient cells of the three kinds with two skies at least 1 black pixel: an interpolated escape space that is neither +1 nor
    -1 (aimed_pose).  Black pixels of the direct renderer are what its capped cells hold"""
    pos, neg, none = classes(rays)
    who = (who, renderer, (pos, neg, none))
    assert pos >= 8, who
    if kind in ("ellis", "interstellar"):
        assert neg >= 8, who
    if kind == "schwarzschild":
        assert neg >= 4, who
    if renderer == "efficient" and kind != "flat":
        assert none >= 1, who


def assert_cell_classes(renderer, kind, step, supersample, projection, thr=TIGHT):
    grid = GRIDS[supersample]
    rays = direct_rays(kind, step, projection, grid) if renderer == "direct" else efficient_rays(kind, step, projection, grid, thr=thr)
    assert_classes(rays, kind, renderer, (kind, step, supersample, projection, thr))


# ---- the three-frame batch ------------------------------------------------------------------------------------------------------------------
# the equirectangular cells: the whole sphere in one frame -- for Ellis and Interstellar fine enough that the throat covers 8 pixels
EQUI_GRIDS = {"ellis": (80, 40), "interstellar": (80, 40), "flat": GRIDS[1], "schwarzschild": GRIDS[1]}


def equirectangular_rays(renderer, kind, thr=TIGHT):
    if renderer == "direct":
        return direct_rays(kind, "fast", "equirectangular", EQUI_GRIDS[kind])
    return efficient_rays(kind, "fast", "equirectangular", EQUI_GRIDS[kind], None, thr)


def assert_equirectangular_classes(renderer, kind, thr=TIGHT):
    """the scene's pose, not an aimed one: the classes of a direct cell"""
    assert_classes(equirectangular_rays(renderer, kind, thr), kind, "direct", (kind, "equirectangular", renderer))


def equirectangular_cell(renderer, kind, thr=TIGHT):
    """(frame, six counters) of a kind's equirectangular cell: the fast step, the nearest lookup, supersample 1, the scene's pose"""
    if renderer == "direct":
        return _resolve(direct_fine(kind, "fast", "equirectangular", EQUI_GRIDS[kind], "nearest"), 1)
    return _resolve(efficient_fine(kind, "fast", "equirectangular", EQUI_GRIDS[kind], "nearest", None, thr), 1)


BATCH_RES = (37, 19)          # W H 3 = 2109 bytes: frames 1 and 2 start off a 4-byte boundary, and the last wave of a frame is partial


def batch_radii(kind):
    """three frames over two tables: the scene's radius, one on the -l side for the kinds that have one, and the first again"""
    l = camera_radius(kind)
    return (l, -0.5 * l if kind in ("ellis", "interstellar") else 0.75 * l, l)


NAN_AXIS_POSE = (1.0, 0.0)     # (theta, phi) of batch frame 0


def batch_poses(kind):
    """frame k at its radius.  Frame 0 stands at theta = 1, phi = 0 and looks straight at the centre: on an even grid its optical-axis
    pixel has alpha = pi and a rotation axis cam_bg x out_bg that is an exact zero and normalises to NaN (most poses that look at the
    centre give a few 1e-17 there instead; tests/test_efficient_matrix_host.py asserts the zero).  Frames 1 and 2 stand near the equator
    and are turned a little more with every k"""
    ls = batch_radii(kind)
    first = ((0.0, ls[0], NAN_AXIS_POSE[0], NAN_AXIS_POSE[1]), (-1.0, 0.0, 0.0))
    return (first,) + tuple(((0.0, l, SR.HALF_PI + 0.05 * k, 0.3 * k), (-1.0 if l > 0 else 1.0, 0.1 * k, 0.02 * k)) for k, l in enumerate(ls) if k)


def batch_grid(supersample):
    return BATCH_RES if supersample == 1 else GRIDS[supersample]


def batch_cameras(kind, supersample):
    """the product cameras of the batch for a cell: 37 x 19 at supersample 1, the cell's product resolution otherwise"""
    return [cameras(kind, batch_grid(supersample), supersample, pose)[1] for pose in batch_poses(kind)]


def batch_cell(kind, step, supersample, lookup, projection, thr=TIGHT):
    """[(frame, six counters)] of the three frames"""
    grid = batch_grid(supersample)
    return [_resolve(efficient_fine(kind, step, projection, grid, lookup, pose, thr), supersample) for pose in batch_poses(kind)]


BATCH_KINDS = dict(zip(STEPS, KINDS))          # one kind per step form, all four kinds


# ---- the direct loop's cap ------------------------------------------------------------------------------------------------------------------
EDGE_KIND, EDGE_GRID = "ellis", GRIDS[1]
LOW_CAPS = (0, 1)


def median_caps(step):
    """the median step count of the step form's escaping rays at the full cap, and that + 1"""
    full = direct_rays(EDGE_KIND, step, "perspective", EDGE_GRID)
    n = np.sort(full["steps"][full["code"] != O.NOT_ESCAPED])
    m = int(n[len(n) // 2])
    return m, m + 1


def capped_cell(step, cap, supersample=1, lookup="nearest", projection="perspective"):
    """(frame, six counters, rays) of the Ellis scene under a step form at a cap"""
    S, integrator = WALKS[step]
    rays = _direct_rays(EDGE_KIND, step, projection, EDGE_GRID, cap)
    return memo(("capped", S, integrator, cap, supersample, lookup, projection), lambda: _resolve(compose(rays, lookup), supersample)) + (rays,)


# black lanes in the other two store epilogues: at the median cap, a mip-mapped and a resolved cell (both over EDGE_GRID)
CAPPED_EXTRA = ((2, "mipmap", "fisheye"), (4, "bilinear", "perspective"))


def mixed_tiles(step, cap):
    """the 8 x 8 tiles -- waves -- of the capped frame that hold a ray that escapes in the last iteration (steps == cap) and one that does
    not escape at all"""
    rays = capped_cell(step, cap)[2]
    code, steps = rays["code"], rays["steps"]
    H, W = code.shape
    out = []
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            c, s = code[ty:ty + 8, tx:tx + 8], steps[ty:ty + 8, tx:tx + 8]
            if ((c != O.NOT_ESCAPED) & (s == cap)).any() and (c == O.NOT_ESCAPED).any():
                out.append((tx // 8, ty // 8))
    return out
