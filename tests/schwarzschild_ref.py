"""References for the Schwarzschild kind (CURVIS_METRIC_SCHWARZSCHILD), which the CPU oracle does not know.  They are composed from two
sources: the library's HOST accessors, which run the strict (IEEE) step compiled for x86 -- curvis_new_photon, curvis_walk_ray (the
kernels' loop over curvis_update_relativistic_object / curvis_heun_step / curvis_step_delta), curvis_vector_to_direction,
curvis_sky_texel_index --, and the oracle's metric-independent primitives (rotations, interpolation, the sky lookup), put together
by tests/ref_compose.py's compositions in their whole-ray mode: every ray here is walked by curvis_walk_ray, the anchor that
tests/test_kernel_matrix_host.py pins ref_compose's per-step walk to.  A comparison of a GPU result with these is x86 strict step against gfx950
fast step: it checks the guard, the device math and the plumbing; the formulas themselves are pinned by the mpmath tests of
tests/test_schwarzschild_host.py."""
import ctypes as C

import numpy as np

import curvis_amd
import oracle_lib as O
import projection_ref as PR
import ref_compose as RC
from curvis_amd import _abi

COUNTERS = PR.COUNTERS
HALF_PI = float.fromhex("0x1.921fb54442d18p+0")


def metric(mass=1.0):
    return curvis_amd.SchwarzschildMetric(mass)


_dp = O._dp


def new_photon(pm, pos, direction):
    x, p = np.zeros(4), np.zeros(4)
    RC.host_new_photon(pm._c(), pos, direction, x, p)
    return x, p


def walk(pm, x, p, delta, cap, max_radius, step_scale=0, integrator=0):
    """the ray (x, p) walked in place to escape, capture or the cap with the strict step: (steps, code)"""
    code, steps = RC.host_walk_ray(pm._c(), x, p, delta, step_scale, integrator, cap, max_radius)
    return steps, code


def _texel_of(sky_shapes):
    """raw (tx, ty) of the nearest lookup on a sky of (w, h) texels with the identity orientation"""
    tx, ty = C.c_uint32(0), C.c_uint32(0)

    def texel(code, d):
        w, h = sky_shapes[0 if code == 1 else 1]
        _abi.lib().curvis_sky_texel_index(w, h, None, _dp(d), C.byref(tx), C.byref(ty))
        return tx.value, ty.value
    return texel


def _walked(pm, cam, dirs, delta, cap, max_radius, step_scale, integrator):
    return RC.compose_brute(RC.HostStepper(pm), cam.pos, dirs, cap, max_radius, delta, step_scale, integrator, whole=True)


def debug_dump(pm, cam, dirs, sky_shapes, delta, cap, max_radius, step_scale=0, integrator=0):
    """what curvis_render_brute_debug records for the rays along the world-space directions dirs [H, W, 3] from the oracle camera cam"""
    return RC.debug_records(_walked(pm, cam, dirs, delta, cap, max_radius, step_scale, integrator), _abi.RAY_DEBUG, _texel_of(sky_shapes))


def compose_brute(pm, cam, dirs, sky_pos, sky_neg, cap, max_radius, delta, step_scale=0, integrator=0):
    """RelativisticSystem::render_image over dirs, every ray walked by curvis_walk_ray: (frame, counters, codes)"""
    rays = _walked(pm, cam, dirs, delta, cap, max_radius, step_scale, integrator)
    rgb, cnt = RC.frame_nearest(rays, None, (sky_pos, sky_neg))
    return rgb, cnt[:6], rays["code"]


def evaluator(pm, l, delta, cap, max_radius, step_scale=0, integrator=0):
    """ref_compose's escape-angle evaluator, the photon walked by curvis_walk_ray"""
    return RC.EscapeAngle(RC.HostStepper(pm), l, delta, step_scale, integrator, cap, max_radius, whole=True)


def compute_escape_angle(pm, l, alpha, delta, cap, max_radius, step_scale=0, integrator=0):
    """(code, angle, steps) of one alpha; code -2 where the reference panics"""
    return evaluator(pm, l, delta, cap, max_radius, step_scale, integrator)(alpha)


def compose_direct(pm, cam, dirs, sky_pos, sky_neg, cap, max_radius, delta, step_scale=0, integrator=0):
    """"direct" mode, the escape angle per pixel from the evaluator above: (frame, counters, codes)"""
    f = evaluator(pm, cam.pos[1], delta, cap, max_radius, step_scale, integrator)

    def angle(alpha):
        out = f(alpha)
        assert out[0] != O.PANIC
        return out
    rays = RC.compose_direct(angle, cam, dirs)
    rgb, cnt = RC.frame_nearest(rays, None, (sky_pos, sky_neg))
    return rgb, cnt[:6], rays["code"]


def compose_efficient_from_table(cam, dirs, sky_pos, sky_neg, table):
    """steps 2, 4 and 5 of render_image_efficient over dirs from a given sample table (alpha, escape angle, escape space: the
    refinement logic that builds it does not depend on the metric and has its own tests): (frame, (rays, n_pos, n_neg, n_none, n_oob))"""
    rgb, cnt = RC.frame_nearest(RC.compose_efficient([table[k] for k in ("a", "e", "s")], cam, dirs), None, (sky_pos, sky_neg))
    return rgb, (cnt[0],) + cnt[2:6]


# ---- the scene of the GPU tests ----------------------------------------------------------------------------------------------------
MASS, L_CAM, R, DELTA, CAP = 1.0, 8.0, 25.0, 0.05, 4096
FOCAL, DIAG = 15.0, 43.0
SKY_SHAPES = ((333, 177), (129, 301))       # +l, -l (w, h)
SKY_SALTS = (0x7A3C1B, 0xDEA5C4)
FRAMES = ((24, 16), (32, 24))


def scene(res):
    """camera at l = 8 M on the equator looking 20 degrees off the hole: (product metric, oracle camera, product camera)"""
    a = np.deg2rad(20.0)
    pos, fwd, up = (0.0, L_CAM, HALF_PI, 0.0), (-float(np.cos(a)), float(np.sin(a)), 0.05), (0.0, 0.0, 1.0)
    return metric(MASS), O.camera(pos, fwd, up, FOCAL, DIAG, res), curvis_amd.Camera(pos, fwd, up, FOCAL, DIAG, res[0], res[1])


def index_skies():
    return RC.index_skies(SKY_SHAPES, SKY_SALTS)


memo = RC.memo
