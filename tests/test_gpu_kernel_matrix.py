"""Every form of the brute renderer's kernels on the GPU, exact against tests/kernel_matrix_ref.py: the 384 DISC forms of the fused
static kernel, its 384 plain forms and the 96 forms of the relay kernel -- metric kind x step form x supersample x lookup x projection.
Every pixel and every counter of every cell, no tolerance anywhere.  A test is one (kind, step) and loops over its cells of
supersample x lookup x projection, which share two reference walks per projection; each test first asserts, from the reference alone,
the ray classes its cells rely on (tests/test_kernel_matrix_host.py does the same without a GPU), and prints how many cells it compared.

Then the edges of the disc loop: the cap beside a disc hit -- a ray that ends on the disc in the last iteration counts cap - 1 steps, and
no plane test is made between the last two states --, caps 0, 1 and 2, a camera below the plane, where a plane test in the first
iteration (which has no previous state) would end every ray, and a wave in which one lane ends on the disc with count k while
another escapes with count k + 1, through one ballot."""
import contextlib

import numpy as np
import pytest

import disc_ref as D
import kernel_matrix_ref as K
import projection_ref as P
import step_scale_ref as SR
import curvis_amd

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = dict(projection=0, sky_filter=0, sky_mipmap=0, supersample=1, step_scale=0, integrator=0, fast_math=1, variant=-1, fuse_shade=1)
KIND_STEPS = [(kind, step) for kind in K.KINDS for step in K.STEPS]
RELAY_GROUPS = sorted({(c[0], c[1], c[3]) for c in K.relay_cells()})      # (kind, step, lookup): eight cells each


@contextlib.contextmanager
def options(ctx, **kw):
    saved = {k: ctx.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


@pytest.fixture()
def ctx(gpu_ctx):
    for k, img in enumerate(SR.index_skies()):
        gpu_ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))
    yield gpu_ctx
    gpu_ctx.set_disc(None)
    for key, value in OPTION_DEFAULTS.items():
        gpu_ctx.set_option(key, value)


def product_disc(d):
    return curvis_amd.Disc(np.array(d.rgba), d.l_in, d.l_out)


def counters(ctx, st, frame=0):
    """the seven counters of a render: the call's statistics and the frame's n_disc"""
    return tuple(int(getattr(st, k)) for k in P.COUNTERS) + (ctx.frame_disc_hits(frame),)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def assert_render(ctx, pm, pc, want, what, cap=K.CAP, max_radius=K.R, relay=False):
    """one render against (frame, seven counters): every pixel, the counters of the call and of the frame, their sum, and which kernel
    rendered"""
    rgb, st = ctx.render_brute(pm, pc, cap, max_radius, K.DELTA)
    got = counters(ctx, st)
    assert_frame(rgb, want[0], what)
    assert got == want[1], (what, got, want[1])
    assert got == tuple(int(getattr(ctx.frame_stats(0), k)) for k in P.COUNTERS) + (got[6],), what
    assert got[0] == got[2] + got[3] + got[4] + got[6], (what, "rays = n_pos + n_neg + n_none + n_disc")
    if relay:
        assert ctx.get_option("last_relay_launches") >= 1, (what, "the relay kernel renders")
        assert ctx.get_option("relay_mismatches") == 0 and ctx.get_option("relay_disabled") == 0, what
    else:
        assert ctx.get_option("last_relay_launches") == 0, (what, "the static kernel renders")


def run_cells(ctx, kind, step, inner, disc, relay=False, **extra):
    """the cells (supersample, lookup, projection) of one (kind, step): the number compared"""
    for n, _, projection in inner:
        K.assert_cell_classes(kind, step, n, projection, disc)
    for n, lookup, projection in inner:
        _, _, pm, _, pc, dsc = K.cell_scene(kind, n)
        ctx.set_disc(product_disc(dsc) if disc else None)
        with options(ctx, **K.cell_options(step, n, lookup, projection), **extra):
            assert_render(ctx, pm, pc, K.cell_frame(kind, step, n, lookup, projection, disc),
                          ("disc" if disc else "relay" if relay else "plain", kind, step, "supersample %d" % n, lookup, projection), relay=relay)
    return len(inner)


# ---- 1. the 384 DISC forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,step", KIND_STEPS)
def test_disc_cells(ctx, kind, step):
    n = run_cells(ctx, kind, step, K.inner_cells(), True)
    print("kernel matrix, disc, %s %s: %d cells compared" % (kind, step, n))
    assert n == 24


# ---- 2. the 384 plain forms of the fused static kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,step", KIND_STEPS)
def test_plain_cells(ctx, kind, step):
    n = run_cells(ctx, kind, step, K.inner_cells(), False, variant=1)
    print("kernel matrix, plain, %s %s: %d cells compared" % (kind, step, n))
    assert n == 24


# ---- 3. the 96 forms of the relay kernel: the plain cell's frame and counters -----------------------------------------------------------
@pytest.mark.parametrize("kind,step,lookup", RELAY_GROUPS)
def test_relay_cells(ctx, kind, step, lookup):
    inner = [c[2:] for c in K.relay_cells() if (c[0], c[1], c[3]) == (kind, step, lookup)]
    n = run_cells(ctx, kind, step, inner, False, relay=True, variant=2, relay_min_blocks=0)
    print("kernel matrix, relay, %s %s %s: %d cells compared" % (kind, step, lookup, n))
    assert n == 8 and len(RELAY_GROUPS) == 12


# ---- 4. everything at once, and the equirectangular projection, per kind ---------------------------------------------------------------
@pytest.mark.parametrize("disc", [True, False], ids=["disc", "plain"])
@pytest.mark.parametrize("kind", K.KINDS)
def test_all_options_at_once(ctx, kind, disc):
    """scaled Heun steps, supersample 2, fisheye, the bilinear filter on the mip pyramid"""
    sc = K.cell_scene(kind, 2)
    rays = D.walk_rays(D.stepper_of(sc[1], sc[2]), sc[3].pos, SR.world_dirs(sc[3], P.FISHEYE), sc[5] if disc else None, K.CAP, K.R, K.DELTA,
                       K.STEP_SCALE, 1)
    K.assert_walk_classes(rays, (kind, "everything", disc), disc)
    assert rays["steps"].sum() not in (K.walk(kind, "scaled", "fisheye", K.GRIDS[2], disc)["steps"].sum(), K.walk(kind, "heun", "fisheye", K.GRIDS[2], disc)["steps"].sum())
    fine, cnt = K.compose(rays, sc[5] if disc else None, "mipmap")
    ctx.set_disc(product_disc(sc[5]) if disc else None)
    with options(ctx, step_scale=K.STEP_SCALE, integrator=1, projection=2, sky_filter=1, sky_mipmap=1, supersample=2, variant=-1 if disc else 1):
        assert_render(ctx, sc[2], sc[4], (SR.box_average(fine, 2), cnt), (kind, "everything", "disc" if disc else "plain"))


@pytest.mark.parametrize("kind", K.EQUIRECTANGULAR_KINDS)
def test_equirectangular_disc_cell(ctx, kind):
    """the kernel form is the fisheye one; ray_init differs"""
    K.assert_walk_classes(K.walk(kind, "fast", "equirectangular", K.GRIDS[1], True), (kind, "equirectangular"), True)
    _, _, pm, _, pc, dsc = K.cell_scene(kind, 1)
    ctx.set_disc(product_disc(dsc))
    with options(ctx, projection=1):
        assert_render(ctx, pm, pc, K.cell_frame(kind, "fast", 1, "nearest", "equirectangular", True), ("disc", kind, "equirectangular"))


# ---- 5. the edges of the disc loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", K.STEPS)
def test_cap_beside_a_disc_hit(ctx, step):
    caps = K.beside_caps(step)
    for cap in caps:
        last, missed = K.cap_conditions(step, cap)
        assert last >= 1 and missed >= 1, (step, cap, last, missed)
    _, _, pm, _, pc, dsc = K.scene_a()
    ctx.set_disc(product_disc(dsc))
    with options(ctx, **K.STEP_OPTIONS[step]):
        for cap in caps + K.LOW_CAPS:
            want = K.capped_frame(step, cap)
            print("cap", cap, step, "reference counters", want[1])
            assert_render(ctx, pm, pc, want, ("cap beside a hit", step, cap), cap=cap)


@pytest.mark.parametrize("step", K.STEPS)
def test_first_iteration_makes_no_plane_test(ctx, step):
    """the camera below the plane, the disc across the throat: a plane test against the zero-initialised previous state would end every
    ray on one texel before its first step"""
    assert K.first_iteration_hit() is not None
    want = K.below_frame(step)
    D.assert_classes(want[2], ("below the plane", step))
    _, _, pm, _, pc, dsc = K.below_scene()
    ctx.set_disc(product_disc(dsc))
    with options(ctx, **K.STEP_OPTIONS[step]):
        assert_render(ctx, pm, pc, want, ("camera below the plane", step))


@pytest.mark.parametrize("step", ["fast", "strict"])
def test_disc_hit_and_escape_in_one_ballot(ctx, step):
    want = K.ballot_frame()
    pairs = K.ballot_pairs(want[2])
    assert len(pairs) >= 1, "a wave with a disc ray of count k and an escaped ray of count k + 1"
    D.assert_classes(want[2], "ballot scene")
    _, _, pm, _, pc, dsc = K.scene_a(K.BALLOT_RANGE)
    ctx.set_disc(product_disc(dsc))
    with options(ctx, **K.STEP_OPTIONS[step]):
        assert_render(ctx, pm, pc, want, ("hit and escape in one ballot", step, pairs), max_radius=K.BALLOT_R)
