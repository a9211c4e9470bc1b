"""Every form of the direct and the efficient renderer's kernels on the GPU, exact against tests/efficient_matrix_ref.py: the 384 forms of
direct_kernel, the 16 + 16 forms of the two table kernels (host-paced and device sampler), the 28 forms of the efficient pixel kernels
behind either sampler, a three-frame batch through all 28, everything at once, and the direct loop's cap.  Every pixel, every counter and
every table entry bit for bit, no tolerance anywhere.  A test first asserts, from the reference alone, the classes its cells rely on
(tests/test_efficient_matrix_host.py does the same without a GPU), asserts which sampler and which pixel enumeration really ran before it
compares anything, and prints how many cells it compared."""
import numpy as np
import pytest

import common
import efficient_matrix_ref as E
import kernel_matrix_ref as K
import projection_ref as P
import step_scale_ref as SR
import curvis_amd
from test_gpu_kernel_matrix import OPTION_DEFAULTS, KIND_STEPS, options, assert_frame

pytestmark = pytest.mark.gpu

EXTRA_DEFAULTS = ("pixel_tiled", "device_sampler", "sampling_speculation")
DEVICE = dict(device_sampler=1)


@pytest.fixture()
def ctx(gpu_ctx):
    saved = {k: gpu_ctx.get_option(k) for k in EXTRA_DEFAULTS}
    for k, img in enumerate(SR.index_skies()):
        gpu_ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))
    gpu_ctx.set_disc(None)
    yield gpu_ctx
    for key, value in OPTION_DEFAULTS.items():
        gpu_ctx.set_option(key, value)
    for key, value in saved.items():
        gpu_ctx.set_option(key, value)


def six(st):
    return tuple(int(getattr(st, k)) for k in P.COUNTERS)


def assert_direct(ctx, pm, pc, want, what, cap=K.CAP):
    """one render_direct against (frame, six counters): every pixel, the counters of the call and of the frame, and their sum"""
    rgb, st = ctx.render_direct(pm, pc, cap, K.R, K.DELTA)
    assert_frame(rgb, want[0], what)
    got = six(st)
    assert got == want[1], (what, got, want[1])
    assert six(ctx.frame_stats(0)) == want[1], (what, "frame statistics", six(ctx.frame_stats(0)), want[1])
    assert got[0] == got[2] + got[3] + got[4], (what, "rays = n_pos + n_neg + n_none")


def assert_table(ctx, frame, want, what):
    """the sample table and the sampler's bookkeeping of a frame, as test_gpu_efficient_oracle.check_vs_oracle compares them"""
    si = ctx.sampling_info(frame)
    got = (si.n_samples, si.calls, si.steps, si.rounds, si.warned_max_iterations)
    assert got == E.bookkeeping(want), (what, "sampling info", got, E.bookkeeping(want))
    for name, arr in zip("aes", ctx.samples(frame)):
        assert np.array_equal(common.bits(arr), common.bits(want[name])), (what, "sample table", name)


def assert_efficient(ctx, pm, cams, want, what, sampler, pixel_tiled, thr=E.TIGHT):
    """one render_efficient against [(frame, six counters)]: which sampler and which enumeration ran, then every pixel of every frame,
    the frames' statistics, and their sum against the call's"""
    rgb, st = ctx.render_efficient(pm, cams, *E.efficient_args(thr=thr))
    assert ctx.get_option("last_sampler_path") == sampler, (what, "sampler path", ctx.get_option("last_sampler_path"))
    if sampler == 1:
        assert ctx.get_option("last_sampling_launches") == 1, what
    assert ctx.get_option("last_pixel_tiled") == pixel_tiled, (what, "pixel enumeration", ctx.get_option("last_pixel_tiled"))
    total = np.zeros(6, np.int64)
    for f, (w_rgb, w_cnt) in enumerate(want):
        assert_frame(rgb[f], w_rgb, (what, "frame", f))
        got = six(ctx.frame_stats(f))
        assert got == w_cnt, (what, "frame statistics", f, got, w_cnt)
        assert got[0] == got[2] + got[3] + got[4], (what, f)
        total += np.array(w_cnt, np.int64)
    assert six(st) == tuple(int(v) for v in total), (what, "call statistics", six(st), total.tolist())


def form_tiled(n, lookup, pixel_tiled):
    """what last_pixel_tiled reports for a form: the tile enumeration whenever it is supersampled, mip-mapped or asked for"""
    return int(n > 1 or lookup == "mipmap" or pixel_tiled == 1)


def products(kind, n):
    """(product metric, product camera) of a direct cell"""
    return E.metrics_of(kind)[1], E.cameras(kind, K.GRIDS[n], n)[1]


# ---- a. the 384 forms of direct_kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,step", KIND_STEPS)
def test_direct_cells(ctx, kind, step):
    inner = K.inner_cells()
    for n, _, projection in inner:
        E.assert_cell_classes("direct", kind, step, n, projection)
    for n, lookup, projection in inner:
        pm, pc = products(kind, n)
        with options(ctx, **K.cell_options(step, n, lookup, projection)):
            assert_direct(ctx, pm, pc, E.direct_cell(kind, step, n, lookup, projection), ("direct", kind, step, "supersample %d" % n, lookup, projection))
    print("efficient matrix, direct, %s %s: %d cells compared" % (kind, step, len(inner)))
    assert len(inner) == 24


# ---- b. the 32 forms of the table kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [0, 1], ids=["host-paced", "device"])
@pytest.mark.parametrize("kind,step", KIND_STEPS)
def test_tables(ctx, kind, step, sampler):
    """the table at the cells' thresholds through either sampler.  Where that table outgrows the device sampler the call reports path 2 and
    the table compared is the host-paced sampler's: the device leg then runs again at the looser thresholds of E.device_thresholds, at
    which the device sampler completes, and it is that table which counts as the form's"""
    want = E.table(kind, step)
    assert want["n"] >= 100 and want["rounds"] >= 2 and want["warned"] == 0
    pm, pc = products(kind, 8)
    path, thr = E.sampler_path([want], sampler), E.device_thresholds(kind, step) if sampler else E.TIGHT
    with options(ctx, device_sampler=sampler, **K.STEP_OPTIONS[step]):
        ctx.render_efficient(pm, pc, *E.efficient_args())
        assert ctx.get_option("last_sampler_path") == path, (kind, step, sampler, ctx.get_option("last_sampler_path"), path, want["peak"])
        if path == 1:
            assert ctx.get_option("last_sampling_launches") == 1
        assert_table(ctx, 0, want, (kind, step, sampler))
        assert (path == 2) == (thr != E.TIGHT)
        if path == 2:
            fits = E.table(kind, step, thr=thr)
            assert fits["n"] >= 100 and fits["rounds"] >= 2 and fits["warned"] == 0 and fits["peak"] <= E.SAMPLER_CAP
            ctx.render_efficient(pm, pc, *E.efficient_args(thr=thr))
            assert ctx.get_option("last_sampler_path") == 1 and ctx.get_option("last_sampling_launches") == 1, (kind, step, thr)
            assert_table(ctx, 0, fits, (kind, step, sampler, thr))
    print("efficient matrix, table, %s %s %s, thresholds %g: 1 form compared" % (kind, step, "device sampler" if sampler else "host-paced sampler", thr[0]))


# ---- c. the 28 forms of the pixel kernels ---------------------------------------------------------------------------------------------------------
def run_pixel_forms(ctx, kind, step, forms, sampler):
    """behind the device sampler at E.device_thresholds(kind, step): the device sampler's table is the one the pixels read (path 1)"""
    thr = E.device_thresholds(kind, step) if sampler else E.TIGHT
    for n, _, projection, _ in forms:
        E.assert_cell_classes("efficient", kind, step, n, projection, thr)
    for n, lookup, projection, pixel_tiled in forms:
        pm, pc = E.metrics_of(kind)[1], E.efficient_camera(kind, step, n, projection, thr)
        with options(ctx, device_sampler=sampler, pixel_tiled=pixel_tiled, **K.cell_options(step, n, lookup, projection)):
            assert_efficient(ctx, pm, [pc], [E.efficient_cell(kind, step, n, lookup, projection, thr)],
                             ("efficient", kind, step, "supersample %d" % n, lookup, projection, "pixel_tiled %d" % pixel_tiled, "sampler %d" % sampler, thr),
                             sampler, form_tiled(n, lookup, pixel_tiled), thr)
    return len(forms), thr


@pytest.mark.parametrize("kind,step", KIND_STEPS)
def test_pixel_cells_device_sampler(ctx, kind, step):
    n, thr = run_pixel_forms(ctx, kind, step, [f[:4] for f in E.pixel_forms()], 1)
    print("efficient matrix, pixels, device sampler, %s %s, thresholds %g: %d cells compared" % (kind, step, thr[0], n))
    assert n == 28


@pytest.mark.parametrize("kind,step", KIND_STEPS)
def test_pixel_cells_host_paced_sampler(ctx, kind, step):
    n, _ = run_pixel_forms(ctx, kind, step, E.HOST_PACED_FORMS, 0)
    print("efficient matrix, pixels, host-paced sampler, %s %s: %d cells compared" % (kind, step, n))
    assert n == 4


# ---- d. the three-frame batch through all 28 pixel forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", K.STEPS)
def test_batch_cells(ctx, step):
    kind = E.BATCH_KINDS[step]
    pm = E.metrics_of(kind)[1]
    forms = [f[:4] for f in E.pixel_forms()]
    ls = E.batch_radii(kind)
    assert ls[0] == ls[2] != ls[1]
    thr = E.device_thresholds(kind, step, ls[:2])
    for grid in (K.GRIDS[1], K.GRIDS[8]):
        assert E.optical_axis_pixels(kind, "perspective", grid, E.batch_poses(kind)[0]) == (1, 1), "frame 0 holds the pixel with the NaN rotation axis"
    for n, lookup, projection, pixel_tiled in forms:
        want = E.batch_cell(kind, step, n, lookup, projection, thr)
        assert all(cnt[2] + cnt[3] >= 8 for _, cnt in want), (kind, step, n, lookup, projection, [cnt for _, cnt in want])
        with options(ctx, pixel_tiled=pixel_tiled, **DEVICE, **K.cell_options(step, n, lookup, projection)):
            what = ("batch", kind, step, "supersample %d" % n, lookup, projection, "pixel_tiled %d" % pixel_tiled, thr)
            assert_efficient(ctx, pm, E.batch_cameras(kind, n), want, what, 1, form_tiled(n, lookup, pixel_tiled), thr)
            for f, l in enumerate(ls):
                assert_table(ctx, f, E.table(kind, step, l, thr=thr), what + ("frame", f))
    print("efficient matrix, batch, %s %s, thresholds %g: %d cells compared" % (kind, step, thr[0], len(forms)))
    assert len(forms) == 28


# ---- e. everything at once, and the equirectangular projection, per kind and renderer ----------------------------------------------------------------
@pytest.mark.parametrize("renderer", ["direct", "efficient"])
@pytest.mark.parametrize("kind", K.KINDS)
def test_all_options_at_once(ctx, kind, renderer):
    """scaled Heun steps, supersample 2, fisheye, the bilinear filter on the mip pyramid"""
    grid = K.GRIDS[2]
    if renderer == "direct":
        thr = None
        fine_of = E.direct_fine
        E.assert_classes(E.direct_rays(kind, E.EVERYTHING, "fisheye", grid), kind, renderer, (kind, "everything"))
        pm, pc = products(kind, 2)
    else:
        thr = E.device_thresholds(kind, E.EVERYTHING)

        def fine_of(*a):
            return E.efficient_fine(*a, thr=thr)
        E.assert_classes(E.efficient_rays(kind, E.EVERYTHING, "fisheye", grid, thr=thr), kind, renderer, (kind, "everything"))
        pm, pc = E.metrics_of(kind)[1], E.efficient_camera(kind, E.EVERYTHING, 2, "fisheye", thr)
    want = E._resolve(fine_of(kind, E.EVERYTHING, "fisheye", grid, "mipmap"), 2)
    assert want[1][1] not in (fine_of(kind, "scaled", "fisheye", grid, "mipmap")[1][1], fine_of(kind, "heun", "fisheye", grid, "mipmap")[1][1])
    with options(ctx, step_scale=K.STEP_SCALE, integrator=1, projection=2, sky_filter=1, sky_mipmap=1, supersample=2, **DEVICE):
        if renderer == "direct":
            assert_direct(ctx, pm, pc, want, (kind, "everything", "direct"))
        else:
            assert_efficient(ctx, pm, [pc], [want], (kind, "everything", "efficient", thr), 1, 1, thr)
            assert_table(ctx, 0, E.table(kind, E.EVERYTHING, thr=thr), (kind, "everything"))
    print("efficient matrix, everything at once, %s %s: 1 cell compared" % (kind, renderer))


@pytest.mark.parametrize("renderer", ["direct", "efficient"])
@pytest.mark.parametrize("kind", K.KINDS)
def test_equirectangular_cell(ctx, kind, renderer):
    """the kernel form is the fisheye one; the pixel's vector differs"""
    thr = E.device_thresholds(kind, "fast") if renderer == "efficient" else E.TIGHT
    E.assert_equirectangular_classes(renderer, kind, thr)
    pm, pc = E.metrics_of(kind)[1], E.cameras(kind, E.EQUI_GRIDS[kind])[1]
    want = E.equirectangular_cell(renderer, kind, thr)
    with options(ctx, projection=1, **DEVICE):
        if renderer == "direct":
            assert_direct(ctx, pm, pc, want, (kind, "equirectangular", "direct"))
        else:
            assert_efficient(ctx, pm, [pc], [want], (kind, "equirectangular", "efficient", thr), 1, 0, thr)
    print("efficient matrix, equirectangular, %s %s: 1 cell compared" % (kind, renderer))


# ---- f. the direct loop's cap -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", K.STEPS)
def test_direct_cap_beside_the_median_escape(ctx, step):
    """lanes of one wave leave the per-lane loop at different times: at the two caps beside the median escape some 8 x 8 tile holds a ray
    that escapes in the last iteration and one that does not escape; then caps 0 and 1.  Then black lanes in the other store epilogues:
    the median cap under a mip-mapped and under a resolved form"""
    caps = E.median_caps(step)
    for cap in caps:
        assert len(E.mixed_tiles(step, cap)) >= 1, (step, cap)
    pm, pc = products(E.EDGE_KIND, 1)
    with options(ctx, **K.STEP_OPTIONS[step]):
        for cap in caps + E.LOW_CAPS:
            want = E.capped_cell(step, cap)
            print("direct cap", cap, step, "reference counters", want[1])
            assert_direct(ctx, pm, pc, want[:2], ("direct cap", step, cap), cap=cap)
    print("efficient matrix, edge, %s: %d cells compared" % (step, len(caps + E.LOW_CAPS)))
    assert len(caps + E.LOW_CAPS) == 4
    for n, lookup, projection in E.CAPPED_EXTRA:
        want = E.capped_cell(step, caps[0], n, lookup, projection)
        assert want[1][4] >= 8 and want[1][2] + want[1][3] >= 8, ("black and escaped rays in one frame", step, n, lookup, projection, want[1])
        with options(ctx, **K.cell_options(step, n, lookup, projection)):
            assert_direct(ctx, pm, E.cameras(E.EDGE_KIND, E.EDGE_GRID, n)[1], want[:2], ("direct cap", step, caps[0], n, lookup, projection), cap=caps[0])
    print("efficient matrix, capped direct forms, %s: %d cells compared" % (step, len(E.CAPPED_EXTRA)))
