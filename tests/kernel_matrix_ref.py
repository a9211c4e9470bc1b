"""The brute renderer's kernel lattice: every form of the fused static kernel -- metric kind x step form x supersample x lookup x
projection, 384 cells, each once plain and once as a DISC form -- and the 96 forms of the relay kernel, with the reference frame and
counters of every cell.  The enumeration is written from the static asserts of geodesic_static and from the launch shapes each kernel
family exists for (curvis_amd/csrc/brute_plan.h family_exists, render_host.h launch_integrate); nothing of it is read from the product.

The reference is tests/disc_ref.py's over tests/ref_compose.py, which is compositional: a ray is walked by the oracle's own step (the
library's host accessors for the Schwarzschild kind) under the step option, and the lookup and the supersampling are pure functions of a
walked fine grid.  So the twelve cells of one (kind, step walk, projection) share two walks, one per fine grid:

  20 x 12  supersample 1, 2 and 4: ragged 8 x 8 tiles in both directions; frames of 20 x 12, 10 x 6 and 5 x 3
  16 x  8  supersample 8: a frame of 2 x 1 (a fine grid of 8 N can never be ragged)

The strict and the fast step share the Euler walk.  Every walk and every fine frame is computed once, shared and read-only.  No GPU."""
import itertools

import numpy as np

import disc_ref as D
import oracle_lib as O
import projection_ref as P
import ref_compose as RC
import step_scale_ref as SR

KINDS = ("ellis", "interstellar", "flat", "schwarzschild")
STEPS = ("strict", "fast", "scaled", "heun")
SUPERSAMPLES = (1, 2, 4, 8)
LOOKUPS = ("nearest", "bilinear", "mipmap")
PROJECTIONS = ("perspective", "fisheye")

STEP_SCALE = 4 * 256
# the library options of a step form, and its walk: (S, integrator)
STEP_OPTIONS = {"strict": dict(fast_math=0), "fast": dict(fast_math=1), "scaled": dict(step_scale=STEP_SCALE), "heun": dict(integrator=1)}
STEP_WALKS = {"strict": (0, 0), "fast": (0, 0), "scaled": (STEP_SCALE, 0), "heun": (0, 1)}
LOOKUP_OPTIONS = {"nearest": dict(sky_filter=0, sky_mipmap=0), "bilinear": dict(sky_filter=1, sky_mipmap=0), "mipmap": dict(sky_filter=1, sky_mipmap=1)}
PROJECTION_OPTION = {"perspective": P.PERSPECTIVE, "equirectangular": P.EQUIRECTANGULAR, "fisheye": P.FISHEYE}
EQUIRECTANGULAR_KINDS = KINDS           # the kinds whose equirectangular walk holds the ray classes of a disc cell
GRIDS = {1: (20, 12), 2: (20, 12), 4: (20, 12), 8: (16, 8)}      # the fine ray grid of a supersampling factor (w, h)

R, DELTA, CAP = D.R, D.DELTA, D.CAP
_cache = {}


def cells():
    """the 384 forms of the fused static kernel: (kind, step, supersample, lookup, projection)"""
    return list(itertools.product(KINDS, STEPS, SUPERSAMPLES, LOOKUPS, PROJECTIONS))


def inner_cells():
    """the 24 cells of one (kind, step): (supersample, lookup, projection)"""
    return list(itertools.product(SUPERSAMPLES, LOOKUPS, PROJECTIONS))


def relay_cells():
    """the 96 forms of the relay kernel: no Schwarzschild kind, no scaled or Heun step, no mip-mapped lookup"""
    return [c for c in cells() if c[0] != "schwarzschild" and c[1] in ("strict", "fast") and c[3] != "mipmap"]


def cell_options(step, supersample, lookup, projection):
    """the library options that select a cell's kernel"""
    opts = dict(supersample=supersample, projection=PROJECTION_OPTION[projection])
    opts.update(STEP_OPTIONS[step])
    opts.update(LOOKUP_OPTIONS[lookup])
    return opts


def product_res(supersample):
    """the resolution of the product's camera for a cell: the fine grid over the factor"""
    w, h = GRIDS[supersample]
    return w // supersample, h // supersample


# ---- the scenes, one per kind: (position, forward, up, focal, (l_in, l_out)) -----------------------------------------------------------
# Ellis and Interstellar: disc_ref's scenes A and B.  Schwarzschild: disc_ref.schwarzschild_scene() MOVED -- at the small grids here its
# walks hold 2 rays that passed a gap and went on where a disc cell wants 4 (the hole fills two thirds of that frame) --: the camera
# further out (l = 10 M, theta = 1.3), looking a little past the hole, a shorter lens and the disc out to l = 16.  Every walk of the
# lattice then holds at least 43 disc rays, 56 +l rays and 7 gap rays, and the hole's shadow stays in the frame.
SCHW_POS, SCHW_FWD, SCHW_FOCAL, SCHW_L_OUT = (0.0, 10.0, 1.3, 0.0), (-1.0, 0.1, -0.05), 10.0, 16.0


def scene_parameters(kind):
    if kind == "ellis":
        return D.SCENES["A"][1:5] + (D.SCENES["A"][6],)
    if kind == "interstellar":
        return D.SCENES["B"][1:5] + (D.SCENES["B"][6],)
    if kind == "flat":
        return (0.0, 5.0, 1.2, 0.5), (-1.0, 0.2, -0.2), (0.0, 0.0, 1.0), 12.0, (1.0, 8.0)
    import curvis_amd
    l_in = curvis_amd.SchwarzschildMetric(D.SCHW_MASS).l_of_radius(6.0 * D.SCHW_MASS)
    return SCHW_POS, SCHW_FWD, D.SCHW_UP, SCHW_FOCAL, (l_in, SCHW_L_OUT)


def scene(kind, grid, supersample=1):
    """disc_ref.scene_from's tuple for a kind: the oracle camera over the fine grid, the product camera over grid / supersample"""
    pos, fwd, up, focal, l_range = scene_parameters(kind)
    return D.scene_from(kind, pos, fwd, up, focal, grid, l_range, (grid[0] // supersample, grid[1] // supersample))


def cell_scene(kind, supersample):
    return scene(kind, GRIDS[supersample], supersample)


# ---- walks and frames ----------------------------------------------------------------------------------------------------------------
def _walk(key, sc, S, integrator, projection, disc, cap, max_radius):
    if key not in _cache:
        _, om, pm, oc, _, dsc = sc
        dirs = SR.world_dirs(oc, PROJECTION_OPTION[projection])
        _cache[key] = D.walk_rays(D.stepper_of(om, pm), oc.pos, dirs, dsc if disc else None, cap, max_radius, DELTA, S, integrator)
    return _cache[key]


def walk(kind, step, projection, grid, disc):
    """the walked rays of a kind's scene over a fine grid; one walk per (kind, step walk, projection, grid, disc or none)"""
    S, integrator = STEP_WALKS[step]
    return _walk(("walk", kind, S, integrator, projection, grid, bool(disc)), scene(kind, grid), S, integrator, projection, disc, CAP, R)


def compose(rays, dsc, lookup):
    """(frame, counters) of walked rays under a lookup; dsc None: the plain kernel's frame"""
    return RC.frame(rays, dsc, lookup, SR.index_skies(), SR.oracle_skies())


def fine_frame(kind, step, projection, grid, lookup, disc):
    """(frame over the fine grid, the seven counters)"""
    S, integrator = STEP_WALKS[step]
    key = ("fine", kind, S, integrator, projection, grid, lookup, bool(disc))
    if key not in _cache:
        _cache[key] = compose(walk(kind, step, projection, grid, disc), scene(kind, grid)[5] if disc else None, lookup)
    return _cache[key]


def cell_frame(kind, step, supersample, lookup, projection, disc):
    """what the product returns for a cell: (frame, (rays, steps, n_pos, n_neg, n_none, n_oob, n_disc)); the counters are the fine
    walk's"""
    fine, cnt = fine_frame(kind, step, projection, GRIDS[supersample], lookup, disc)
    return (fine if supersample == 1 else SR.box_average(fine, supersample)), cnt


def assert_walk_classes(rays, who, disc):
    """the ray classes a cell relies on, from the reference alone: with a disc disc_ref.assert_classes (8 disc rays, 8 +l rays, 4 rays
    that passed a gap and went on), without one 8 +l rays"""
    if disc:
        D.assert_classes(rays, who)
    else:
        assert int((rays["code"] == O.POSITIVE).sum()) >= 8, (who, D.classes(rays))


def assert_cell_classes(kind, step, supersample, projection, disc):
    assert_walk_classes(walk(kind, step, projection, GRIDS[supersample], disc), (kind, step, supersample, projection, disc), disc)


# ---- the edges of the disc loop ------------------------------------------------------------------------------------------------------
EDGE_RES = D.SCENES["A"][5]
LOW_CAPS = (0, 1, 2)          # no plane test at caps 0 and 1, exactly one at cap 2


def scene_a(l_range=None):
    _, pos, fwd, up, focal, res, lr = D.SCENES["A"]
    return D.scene_from("ellis", pos, fwd, up, focal, res, l_range or lr)


def full_cap_rays(step):
    """scene A under a step form at the cap no ray reaches"""
    S, integrator = STEP_WALKS[step]
    return D.scene_rays("A", S=S, integrator=integrator)


def beside_caps(step):
    """the two caps beside a disc hit: the median step count of the step form's disc rays at the full cap, and that + 1"""
    full = full_cap_rays(step)
    n = np.sort(full["steps"][full["code"] == D.DISC])
    m = int(n[len(n) // 2])
    return m, m + 1


def capped_frame(step, cap):
    """(frame, counters, rays) of scene A under a step form at a cap: nearest lookup, perspective"""
    S, integrator = STEP_WALKS[step]
    sc = scene_a()
    rays = _walk(("cap", S, integrator, cap), sc, S, integrator, "perspective", True, cap, R)
    key = ("cap frame", S, integrator, cap)
    if key not in _cache:
        _cache[key] = compose(rays, sc[5], "nearest")
    return _cache[key] + (rays,)


def cap_conditions(step, cap):
    """(rays that end on the disc in the last iteration, steps == cap - 1: the count is k - 1 where an escaping lane's is k;
    rays that end on the disc with steps == cap under the full cap and are not escaped under this one: no plane test between
    y_{cap-1} and y_cap)"""
    full, rays = full_cap_rays(step), capped_frame(step, cap)[2]
    last = (rays["code"] == D.DISC) & (rays["steps"] == cap - 1)
    missed = (full["code"] == D.DISC) & (full["steps"] == cap) & (rays["code"] == O.NOT_ESCAPED)
    return int(last.sum()), int(missed.sum())


# The first iteration has no previous state and makes no plane test.  Scene D mirrored in the equatorial plane: the camera is BELOW it
# (cos(theta_0) < 0, the sign a zero-initialised previous cosine does not have) and the disc spans the throat, so that a plane test
# against a previous state of zeros would interpolate to l = 0, inside the disc, and end every ray where it starts.
BELOW = ("ellis", (0.0, 2.5, np.pi - 1.15, 0.0), (-1.0, 0.0, 0.3), (0.0, 0.0, 1.0), 9.0, (21, 13), (-3.0, 4.0))


def below_scene():
    return D.scene_from(*BELOW)


def below_frame(step):
    """(frame, counters, rays) of the scene below the plane under a step form: nearest lookup, perspective"""
    S, integrator = STEP_WALKS[step]
    sc = below_scene()
    rays = _walk(("below", S, integrator), sc, S, integrator, "perspective", True, CAP, R)
    key = ("below frame", S, integrator)
    if key not in _cache:
        _cache[key] = compose(rays, sc[5], "nearest")
    return _cache[key] + (rays,)


def first_iteration_hit():
    """the opaque texel a plane test of the first iteration would find against a previous state of zeros, or None"""
    sc = below_scene()
    pos, dsc = sc[3].pos, sc[5]
    s0, c0 = RC.Walk(D.stepper_of(sc[1], sc[2])).sincos(pos[2])
    hit = D.crossing(0.0, c0, s0, 0.0, pos[1], 0.0, pos[3], dsc.l_in, dsc.l_out, dsc.w, dsc.h)
    return hit if hit is not None and dsc.alpha[hit[1]][hit[0]] >= 128 else None


BALLOT_R, BALLOT_RANGE = 7.0, (1.5, 6.9)


def ballot_frame():
    """(frame, counters, rays) of scene A's pose with an escape radius of 7 and a disc l in [1.5, 6.9]: rays end on the disc where their
    neighbours escape"""
    sc = scene_a(BALLOT_RANGE)
    rays = _walk(("ballot",), sc, 0, 0, "perspective", True, CAP, BALLOT_R)
    if "ballot frame" not in _cache:
        _cache["ballot frame"] = compose(rays, sc[5], "nearest")
    return _cache["ballot frame"] + (rays,)


def ballot_pairs(rays):
    """(tile, k) of every 8 x 8 tile -- a wave -- that holds a disc ray with count k and an escaped ray with count k + 1: both leave the
    loop in iteration k + 1, through one ballot"""
    code, steps = rays["code"], rays["steps"]
    H, W = code.shape
    out = []
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            c, s = code[ty:ty + 8, tx:tx + 8], steps[ty:ty + 8, tx:tx + 8]
            on_disc = set(s[c == D.DISC].tolist())
            escaped = set(s[(c == O.POSITIVE) | (c == O.NEGATIVE)].tolist())
            out += [((tx // 8, ty // 8), k) for k in sorted(on_disc) if k + 1 in escaped]
    return out
