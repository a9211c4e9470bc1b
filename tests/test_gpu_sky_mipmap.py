"""Mip-mapped sky lookup (library option "sky_mipmap" = 1 on top of "sky_filter" = 1) against its definition, through every renderer.

The definition (include/curvis_hip.h, restated in numpy integers in tests/sky_mipmap_ref.py) is in terms of the (Xc, Yc) of the
bilinear definition.  So, exactly as in test_gpu_sky_filter.py, the oracle (O.CV) renders the scene over INDEX skies of 256 w x 256 h
texels, every pixel of its frame is decoded to (which sky, Xc, Yc), the reference applies footprint, level and colour on the real
w x h skies, and the GPU's frame must equal the result in every pixel and every counter.

Scene: sky_filter_ref's (skies of 13 x 7 and 16 x 5 hashed texels, orientations A and B, camera at l = 5 and at l = -3, max_radius 10,
delta 0.05, cap 340) in three frames -- 24 x 16 at focal 15, 21 x 13 at focal 15 (odd sizes: partners outside the frame, partial
tiles), 20 x 12 at focal 6 (wide: strong minification, several levels).  Every oracle-based test first asserts, from the reference's own
intermediate values, that the classes it relies on are there."""
import contextlib
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import common
import oracle_lib as O
import refpaths
import sky_filter_ref as F
import sky_mipmap_ref as M
import curvis_amd
from curvis_amd import _abi, pngio, rendering

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")

KINDS = ("ellis", "interstellar")
ORIENTS = ("A", "B")
R, DELTA, CAP = F.R, F.DELTA, F.CAP
FRAMES = (((24, 16), 15.0), ((21, 13), 15.0), ((20, 12), 6.0))
EFF = dict(cap=CAP, n0=100, maxit=100, t1=1e-5, t2=1e-5)    # the cap of the other two renderers: the efficient frames hold capped rays too
COUNTERS = ("rays", "steps", "n_pos", "n_neg", "n_none", "n_oob")
BATCH_LS = (5.0, 4.0, -3.0)
MESSAGE = "sky_mipmap must be 0 (off) or 1 (on)"
ON = dict(sky_filter=1, sky_mipmap=1)


def counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS)


def efficient_args(cap=CAP):
    return (cap, R, DELTA, EFF["n0"], EFF["maxit"], EFF["t1"], EFF["t2"])


def scene(kind, res, focal, l=5.0, fwd=(-1.0, 0.0, 0.0)):
    return common.scene(kind, res=res, pos=(0.0, l, F.HALF_PI, 0.0), fwd=fwd, focal=focal)


@functools.lru_cache(maxsize=None)
def oracle_fine(renderer, kind, orient, res, focal, l=5.0, n=1, eff_cap=CAP):
    """the oracle's frame over the fine index skies at n times the resolution: (frame, counters, steps of the sampler or None)"""
    om, oc, _, _ = scene(kind, (res[0] * n, res[1] * n), focal, l)
    sp, sn = F.oracle_fine_skies(orient)
    steps = None
    if renderer == "brute":
        rgb, _, st = O.render_image(O.CV, om, oc, sp, sn, CAP, R, DELTA)
    elif renderer == "direct":
        rgb, st = O.render_image_direct(O.CV, om, oc, sp, sn, CAP, R, DELTA)
    else:
        rgb, smp, st = O.render_image_efficient(O.CV, om, oc, sp, sn, *efficient_args(eff_cap))
        steps = smp["steps"]
    rgb.setflags(write=False)
    return rgb, counters(st), steps


def frame_classes(which, rho, k, f, seen):
    """what the reference did with a frame's rays, from its own intermediate values"""
    sky = which >= 0
    frac = sky & (f != 0)
    return dict(level0=int((sky & (rho < 256)).sum()), frac_levels=set(k[frac].tolist()), fractions=set(f[frac].tolist()),
                whole_above_0=int((sky & (f == 0) & (k > 0)).sum()), levels=set(k[sky].tolist()), **seen)


@functools.lru_cache(maxsize=None)
def expected(renderer, kind, orient, res, focal, l=5.0, n=1, eff_cap=CAP):
    """(the frame by the definition, the oracle's counters, sampler steps, classes, the bilinear frame)"""
    fine, st, steps = oracle_fine(renderer, kind, orient, res, focal, l, n, eff_cap)
    which, Xc, Yc = F.decode(fine)
    assert int((which < 0).sum()) == st[4], (renderer, kind, orient, res, l, st)   # black pixels are the capped rays, nothing else
    want, rho, k, f, seen = M.mip_frame(which, Xc, Yc, F.real_skies())
    bilinear = F.filtered_frame(fine)[0]
    if n > 1:
        want, bilinear = F.box_average(want, n), F.box_average(bilinear, n)
    want.setflags(write=False)
    return want, st, steps, frame_classes(which, rho, k, f, seen), bilinear


def merged_classes(renderer, kind, n=1, frames=FRAMES, ls=(5.0, -3.0), eff_cap=CAP):
    total = dict(level0=0, frac_levels=set(), fractions=set(), whole_above_0=0, levels=set(), outside=0, capped=0, other_sky=0, wrapped=0, used=0)
    for res, focal in frames:
        for orient in ORIENTS:
            for l in ls:
                cl = expected(renderer, kind, orient, res, focal, l, n, eff_cap)[3]
                for key, v in cl.items():
                    total[key] = total[key] | v if isinstance(v, set) else total[key] + v
    return total


def assert_classes_present(renderer, kind, n=1):
    """over the frames a test compares: a ray at level 0 with rho < 256; rays with f != 0 at two or more different k; partners on the
    other sky, capped ones, ones outside the frame, and ones across the seam (a wrapped difference).  A ray with f = 0 and k > 0 needs
    rho = 256 * 2^k exactly: the frames of this scene hold some (asserted), and the device selftest drives every such rho."""
    F.assert_salts()
    cl = merged_classes(renderer, kind, n)
    who = (renderer, kind, n, {k: (sorted(v) if isinstance(v, set) else v) for k, v in cl.items() if k != "fractions"})
    assert cl["level0"] >= 1 and len(cl["frac_levels"]) >= 2 and cl["whole_above_0"] >= 1, who
    assert cl["other_sky"] >= 1 and cl["capped"] >= 1 and cl["outside"] >= 1 and cl["wrapped"] >= 1, who


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


def bind(ctx, orient, images=None):
    for k, img in enumerate(images or F.real_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img), *(F.ORIENT[orient][k] if orient else ())))


@pytest.fixture()
def ctx(gpu_ctx):
    assert gpu_ctx.get_option("sky_mipmap") == 0 and gpu_ctx.get_option("sky_filter") == 0 and gpu_ctx.get_option("supersample") == 1
    yield gpu_ctx
    for key, value in (("sky_mipmap", 0), ("sky_filter", 0), ("supersample", 1), ("projection", 0), ("step_scale", 0), ("integrator", 0),
                       ("pixel_tiled", 0)):
        gpu_ctx.set_option(key, value)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


# ---- 1. the pyramid ----------------------------------------------------------------------------------------------------------------
PYRAMID_SIZES = ((1, 1), (2, 2), (3, 2), (13, 7), (16, 5), (1, 37), (37, 1), (333, 777), (1024, 512))


def assert_chain(ctx, which, T, what):
    want = M.pyramid(T)
    for k, lv in enumerate(want):
        got = ctx.sky_mip_level(which, k)
        assert got.shape == lv.shape and np.array_equal(got, lv), (what, k, got.shape, lv.shape)
    with pytest.raises(curvis_amd.CurvisError) as e:
        ctx.sky_mip_level(which, len(want))
    assert e.value.code == _abi.E_INVALID


@pytest.mark.parametrize("size", PYRAMID_SIZES, ids=lambda s: "%dx%d" % s)
def test_pyramid_every_byte_of_every_level(ctx, size):
    w, h = size
    T = F.texture(w, h, 0x9A7 + w)
    ctx.set_sky(0, curvis_amd.SphericalImage(T))                               # an uploaded sky
    assert_chain(ctx, 0, T, ("uploaded", size))
    other = F.texture(h + 2, w + 1, 0x5B1 + h)                                 # replaced by one of another size: rebuilt, not reused
    ctx.set_sky(0, curvis_amd.SphericalImage(other))
    assert_chain(ctx, 0, other, ("replaced", size))
    ctx.upload_frames(T.reshape(-1))                                           # a borrowed device sky: the frame buffer's bytes
    ptr, nbytes = ctx.framebuffer()
    assert nbytes >= T.size
    ctx.set_sky_device(1, ptr, w, h, copy=False)
    assert_chain(ctx, 1, T, ("borrowed", size))
    assert np.array_equal(ctx.read_sky(1, 0, T.size), T.reshape(-1))           # level 0 stays the caller's buffer, untouched
    bind(ctx, None)


# ---- 2. the per-ray function alone on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1))
def test_selftest_per_ray_function(gpu_ctx, k):
    w, h = F.SHAPES[k]
    T = F.real_skies()[k]
    levels = M.pyramid(np.array(T))
    rng = np.random.default_rng(1234 + k)
    rhos = M.directed_rhos()
    xs = [0, 127, 128, 129, 128 * w, 256 * w - 129, 256 * w - 128, 256 * w - 1]
    ys = [0, 127, 128, 128 * h, 256 * h - 129, 256 * h - 128, 256 * h - 1]
    directed = np.array([(x, y, r) for x in xs for y in ys for r in rhos], np.int64)
    n = 100_000
    random = np.stack([rng.integers(0, 256 * w, n), rng.integers(0, 256 * h, n),
                       np.where(rng.random(n) < 0.5, rng.integers(0, 1 << 14, n), rng.integers(0, 1 << 32, n))], axis=1)
    triples = np.concatenate([directed, random])
    want, ks, fs = M.colour(levels, triples[:, 0], triples[:, 1], triples[:, 2])
    assert set(ks.tolist()) == set(range(len(levels))) and ((fs == 0) & (ks > 0) & (ks < len(levels) - 1)).any() and (fs == 255).any()
    got = gpu_ctx.selftest_sky_mip(np.array(T), triples.astype(np.uint32))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [(triples[i].tolist(), got[i].tolist(), want[i].tolist(), int(ks[i]), int(fs[i])) for i in bad[:4]])


# ---- 3. every renderer against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_brute_vs_definition(ctx, kind, fast_math):
    assert_classes_present("brute", kind)
    pm = scene(kind, *FRAMES[0])[2]
    for orient in ORIENTS:
        bind(ctx, orient)
        for res, focal in FRAMES:
            for l in (5.0, -3.0):
                want, want_st = expected("brute", kind, orient, res, focal, l)[:2]
                for variant in (-1, 1, 2):                     # whatever the variant asks for, the static kernel renders
                    with options(ctx, fast_math=fast_math, variant=variant, relay_min_blocks=0, **ON):
                        rgb, st = ctx.render_brute(pm, scene(kind, res, focal, l)[3], CAP, R, DELTA)
                        assert ctx.get_option("last_relay_launches") == 0
                    what = (kind, orient, res, focal, l, fast_math, variant)
                    assert_frame(rgb, want, what)
                    assert counters(st) == want_st == counters(ctx.frame_stats(0)), what


@pytest.mark.parametrize("kind", KINDS)
def test_efficient_vs_definition(ctx, kind):
    assert_classes_present("efficient", kind)
    pm = scene(kind, *FRAMES[0])[2]
    for orient in ORIENTS:
        bind(ctx, orient)
        for res, focal in FRAMES:
            for l in (5.0, -3.0):
                want, want_st, want_steps = expected("efficient", kind, orient, res, focal, l)[:3]
                for sampler, opts in ((0, dict(device_sampler=0)), (1, dict(device_sampler=1, device_sampler_min_frames=1))):
                    pc = scene(kind, res, focal, l)[3]
                    with options(ctx, **opts):
                        _, st0 = ctx.render_efficient(pm, pc, *efficient_args())
                        assert ctx.get_option("last_pixel_tiled") == 0
                        with options(ctx, **ON):
                            rgb, st = ctx.render_efficient(pm, pc, *efficient_args())
                            assert ctx.get_option("last_pixel_tiled") == 1 and ctx.get_option("last_sampler_path") == sampler
                    what = (kind, orient, res, focal, l, sampler)
                    assert_frame(rgb, want, what)
                    assert counters(st) == counters(st0) and counters(st)[2:] == want_st[2:] and st.steps == want_steps, what


@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_direct_vs_definition(ctx, kind, fast_math):
    assert_classes_present("direct", kind)
    pm = scene(kind, *FRAMES[0])[2]
    for orient in ORIENTS:
        bind(ctx, orient)
        for res, focal in FRAMES:
            for l in (5.0, -3.0):
                want, want_st = expected("direct", kind, orient, res, focal, l)[:2]
                with options(ctx, fast_math=fast_math, **ON):
                    rgb, st = ctx.render_direct(pm, scene(kind, res, focal, l)[3], CAP, R, DELTA)
                assert_frame(rgb, want, (kind, orient, res, focal, l, fast_math))
                assert counters(st) == want_st


# ---- 4. combinations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_supersampled(ctx, kind):
    """supersample = 2: the quads are those of the fine grid, the box average is taken over the mip-filtered sub-rays.  (The efficient
    renderer at a cap of 4096 here: at 340 its fine Interstellar frame stays on level 0.)"""
    n, eff_cap = 2, 4096
    res, focal = FRAMES[2]
    pm, pc = scene(kind, res, focal)[2:]
    for renderer in ("brute", "efficient", "direct"):
        cl = merged_classes(renderer, kind, n, frames=(FRAMES[2],), ls=(5.0,), eff_cap=eff_cap)
        # fine-grid quads on level 0, on a level above 1 with a fraction, and with a partner that does not count
        assert cl["level0"] >= 1 and len(cl["frac_levels"]) >= 1 and max(cl["levels"]) >= 2 and cl["other_sky"] + cl["capped"] >= 1, (renderer, kind, cl)
    for orient in ORIENTS:
        bind(ctx, orient)
        with options(ctx, supersample=n, **ON):
            rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
            want, want_st = expected("brute", kind, orient, res, focal, 5.0, n)[:2]
            assert_frame(rgb, want, ("brute", kind, orient))
            assert counters(st) == want_st
            rgb, st = ctx.render_efficient(pm, pc, *efficient_args(eff_cap))
            want, want_st = expected("efficient", kind, orient, res, focal, 5.0, n, eff_cap)[:2]
            assert_frame(rgb, want, ("efficient", kind, orient))
            assert counters(st)[2:] == want_st[2:] and st.rays == n * n * res[0] * res[1]
            rgb, st = ctx.render_direct(pm, pc, CAP, R, DELTA)
            want, want_st = expected("direct", kind, orient, res, focal, 5.0, n)[:2]
            assert_frame(rgb, want, ("direct", kind, orient))
            assert counters(st) == want_st


def mip_of_fine(fine):
    which, Xc, Yc = F.decode(fine)
    want, rho, k, f, seen = M.mip_frame(which, Xc, Yc, F.real_skies())
    assert ((which >= 0) & (rho >= 256)).any() and seen["used"] >= 50, "the case exercises the pyramid"
    return want


def test_with_projection(ctx):
    import projection_ref as P
    skies = F.oracle_fine_skies("A")
    fine, fine_st, _ = P.expected("brute", "ellis", P.EQUIRECTANGULAR, skies=skies, n=1)
    pm, pc = P.scene("ellis", P.RES[P.EQUIRECTANGULAR])[2:]
    bind(ctx, "A")
    with options(ctx, projection=P.EQUIRECTANGULAR, **ON):
        rgb, st = ctx.render_brute(pm, pc, P.CAP, P.R, P.DELTA)
    assert_frame(rgb, mip_of_fine(fine), "projection = 1")
    assert counters(st) == fine_st


def test_with_step_scale(ctx):
    import gpu_step_scale_cases as CASES
    import step_scale_ref as SR
    # the filtered case of the option's own tests, from the pose whose rays cross the poles and at 20 x 12: the facing pose stays below
    # one texel per pixel at this scene's escape radius (largest rho 146)
    case = dict(CASES.FILTERED, pose="tilted", res=(20, 12))
    assert case["S"] == 1024
    fine = SR.expected("brute", case["kind"], case["pose"], case["S"], case.get("res", SR.RES), case.get("cap", 4096),
                       case.get("projection", 0), case.get("skies", "index"))
    bind(ctx, None)
    pm, pc = SR.metrics(case["kind"])[1], SR.cameras(case["pose"], case.get("res", SR.RES))[1]
    with options(ctx, step_scale=case["S"], **ON):
        rgb, st = ctx.render_brute(pm, pc, 4096, SR.R, SR.DELTA)
    assert_frame(rgb, mip_of_fine(fine[0]), "step_scale = 1024")
    assert counters(st) == fine[1]


def test_with_heun_integrator(ctx):
    import gpu_integrator_cases as CASES
    import integrator_ref as IR
    import step_scale_ref as SR
    case = dict(CASES.FILTERED, pose="tilted", res=(20, 12))   # as in test_with_step_scale
    fine = IR.expected_case(case)
    bind(ctx, None)
    pm, pc = SR.metrics(case["kind"])[1], SR.cameras(case["pose"], case.get("res", SR.RES))[1]
    with options(ctx, integrator=1, step_scale=case["S"], **ON):
        rgb, st = ctx.render_brute(pm, pc, 4096, SR.R, IR.DELTA)
    assert_frame(rgb, mip_of_fine(fine[0]), "integrator = 1")
    assert counters(st) == fine[1]


@pytest.mark.parametrize("renderer", ("brute", "efficient"))
def test_batch_of_three_radii(ctx, renderer):
    res, focal = FRAMES[2]
    pm = scene("ellis", res, focal)[2]
    cams = [scene("ellis", res, focal, l)[3] for l in BATCH_LS]
    bind(ctx, "A")
    want = [expected(renderer, "ellis", "A", res, focal, l) for l in BATCH_LS]
    with options(ctx, **ON):
        if renderer == "brute":
            rgb, st = ctx.render_brute(pm, cams, CAP, R, DELTA)
        else:
            rgb, st = ctx.render_efficient(pm, cams, *efficient_args())
        for f in range(3):
            assert_frame(rgb[f], want[f][0], (renderer, "batch frame", f))
            if renderer == "brute":
                assert counters(ctx.frame_stats(f)) == want[f][1], ("batch frame", f)
            else:
                assert counters(ctx.frame_stats(f))[2:] == want[f][1][2:], ("batch frame", f)


# ---- 5. row bands -------------------------------------------------------------------------------------------------------------------
def test_row_bands(ctx):
    res, focal = FRAMES[1]                                   # 21 x 13: the frame ends on an odd row count
    pm, pc = scene("ellis", res, focal)[2:]
    bind(ctx, "A")
    want, want_st = expected("brute", "ellis", "A", res, focal)[:2]
    with options(ctx, **ON):
        for bands in (((0, 6), (6, 7)), ((0, 8), (8, 4), (12, 1))):
            total = np.zeros(6, np.uint64)
            for begin, count in bands:
                band, st = ctx.render_brute_rows(pm, pc, begin, count, CAP, R, DELTA)
                assert_frame(band, want[begin:begin + count], ("rows", begin, count))
                total += np.array(counters(st), np.uint64)
            assert tuple(int(v) for v in total) == want_st, bands
        for begin, count in ((1, 4), (5, 8), (0, 7), (2, 3)):  # an odd first row; an odd count that does not end the frame
            with pytest.raises(curvis_amd.CurvisError) as e:
                ctx.render_brute_rows(pm, pc, begin, count, CAP, R, DELTA)
            assert e.value.code == _abi.E_INVALID and "sky_mipmap" in str(e.value), (begin, count, str(e.value))
            assert ctx.get_option("sky_mipmap") == 1
    with options(ctx, sky_filter=1):
        ctx.render_brute_rows(pm, pc, 1, 4, CAP, R, DELTA)   # the filter alone takes any band
    # supersample = 2: every band of output rows begins on an even fine row and holds an even number of them
    res, focal = FRAMES[2]
    pm, pc = scene("ellis", res, focal)[2:]
    want, want_st = expected("brute", "ellis", "A", res, focal, 5.0, 2)[:2]
    with options(ctx, supersample=2, **ON):
        total = np.zeros(6, np.uint64)
        for begin, count in ((0, 5), (5, 3), (8, 4)):
            band, st = ctx.render_brute_rows(pm, pc, begin, count, CAP, R, DELTA)
            assert_frame(band, want[begin:begin + count], ("supersampled rows", begin, count))
            total += np.array(counters(st), np.uint64)
        assert tuple(int(v) for v in total) == want_st


# ---- 6. degenerate cases -----------------------------------------------------------------------------------------------------------------
def renders(ctx, kind="ellis", res=F.RES, focal=15.0, fwd=(-1.0, 0.0, 0.0)):
    pm, pc = scene(kind, res, focal, fwd=fwd)[2:]
    return [ctx.render_brute(pm, pc, CAP, R, DELTA)[0], ctx.render_efficient(pm, pc, *efficient_args())[0],
            ctx.render_direct(pm, pc, CAP, R, DELTA)[0]]


AWAY = (1.0, 0.0, 0.0)


def test_all_footprints_below_one_texel_is_the_bilinear_frame(ctx):
    """a magnified frame: every rho < 256, so every ray takes level 0 with f = 0 -- the sky_filter = 1 frame of the same call bit for
    bit.  The 24 x 16 frame that faces the wormhole does not qualify at any focal length tried (at focal 60 its largest rho is 2048, next
    to the ring); the same camera turned away from the wormhole does, at focal 15 already (largest rho 28)."""
    res, focal = F.RES, 15.0
    om, oc, pm, pc = scene("ellis", res, focal, fwd=AWAY)
    sp, sn = (O.sky(img) for img in F.fine_skies())
    fine = O.render_image(O.CV, om, oc, sp, sn, CAP, R, DELTA)[0]
    which, Xc, Yc = F.decode(fine)
    want, rho, k, f, seen = M.mip_frame(which, Xc, Yc, F.real_skies())
    assert (which >= 0).sum() == res[0] * res[1] and seen["used"] == 2 * res[0] * res[1]       # the premise: every ray has both partners,
    assert 0 < rho.max() < 256 and (rho > 0).sum() > 300 and not k.any() and not f.any()         # lands elsewhere, and stays on level 0
    bind(ctx, None)
    with options(ctx, sky_filter=1):
        frames = renders(ctx, res=res, focal=focal, fwd=AWAY)
        with options(ctx, sky_mipmap=1):
            for name, got, bilinear in zip(("brute", "efficient", "direct"), renders(ctx, res=res, focal=focal, fwd=AWAY), frames):
                assert_frame(got, bilinear, ("rho < 256 everywhere", name))
    assert_frame(frames[0], want, "and the definition's")


def test_constant_and_one_texel_skies(ctx):
    colour = np.array([10, 200, 77, 255], np.uint8)
    res, focal = FRAMES[2]
    for shape in ((7, 13), (1, 1)):
        bind(ctx, "B", [np.broadcast_to(colour, shape + (4,)).copy()] * 2)
        nearest = renders(ctx, res=res, focal=focal)
        with options(ctx, **ON):
            for got, want in zip(renders(ctx, res=res, focal=focal), nearest):
                assert_frame(got, want, ("a constant sky comes back constant", shape))
                assert set(map(tuple, got.reshape(-1, 3).tolist())) <= {(10, 200, 77), (0, 0, 0)}
    bind(ctx, "A", [F.texture(1, 1, 5), F.texture(1, 1, 6)])   # a 1 x 1 sky of any colour: the frame of the nearest lookup
    nearest = renders(ctx, res=res, focal=focal)
    with options(ctx, **ON):
        for got, want in zip(renders(ctx, res=res, focal=focal), nearest):
            assert_frame(got, want, "1 x 1 skies")


def test_switched_off_again_is_todays_frame_and_todays_kernels(ctx):
    res, focal = FRAMES[2]
    bind(ctx, "A")
    with options(ctx, sky_filter=1):
        before = renders(ctx, res=res, focal=focal)
        assert ctx.get_option("last_pixel_tiled") == 0          # the efficient renderer's linear efficient_pixel_kernel
        with options(ctx, sky_mipmap=1):
            mipped = renders(ctx, res=res, focal=focal)
            assert ctx.get_option("last_pixel_tiled") == 1
        after = renders(ctx, res=res, focal=focal)
        assert ctx.get_option("last_pixel_tiled") == 0
        with options(ctx, variant=2, relay_min_blocks=0):       # and the brute renderer takes the relay kernel again
            relay = ctx.render_brute(*scene("ellis", res, focal)[2:], CAP, R, DELTA)[0]
            assert ctx.get_option("last_relay_launches") >= 1
    for b, m, a in zip(before, mipped, after):
        assert b.tobytes() == a.tobytes()
        assert (b != m).any()                                    # and the pyramid did something in between
    assert relay.tobytes() == before[0].tobytes()


def test_tile_enumeration_alone_is_the_linear_kernels_frame(ctx):
    """option "pixel_tiled" = 1 (the measurement switch of tools/gpu_sky_mipmap_cost.py): the efficient renderer enumerates pixels by 8 x 8
    tiles under the nearest and the bilinear lookup too, and renders the frames and counters of the linear kernel"""
    res, focal = FRAMES[1]                                   # 21 x 13: partial tiles
    pm, pc = scene("ellis", res, focal)[2:]
    cams = [scene("ellis", res, focal, l)[3] for l in BATCH_LS]
    bind(ctx, "B")
    for filt in (0, 1):
        with options(ctx, sky_filter=filt):
            linear, st0 = ctx.render_efficient(pm, cams, *efficient_args())
            assert ctx.get_option("last_pixel_tiled") == 0
            per0 = [counters(ctx.frame_stats(f)) for f in range(3)]
            with options(ctx, pixel_tiled=1):
                tiled, st1 = ctx.render_efficient(pm, cams, *efficient_args())
                assert ctx.get_option("last_pixel_tiled") == 1
                assert [counters(ctx.frame_stats(f)) for f in range(3)] == per0 and counters(st1) == counters(st0)
            for f in range(3):
                assert_frame(tiled[f], linear[f], ("pixel_tiled", filt, f))


# ---- 7. refusals and front ends -----------------------------------------------------------------------------------------------------------
def test_option_and_refusals(ctx):
    bind(ctx, "A")
    res, focal = FRAMES[0]
    pm, pc = scene("ellis", res, focal)[2:]
    for order in (("sky_mipmap", "sky_filter"), ("sky_filter", "sky_mipmap")):   # setting it is always allowed, in either order
        for key in order:
            ctx.set_option(key, 1)
        for key in order:
            ctx.set_option(key, 0)
    ctx.set_option("sky_mipmap", 1)
    for bad in (2, -1, 256):
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.set_option("sky_mipmap", bad)
        assert e.value.code == _abi.E_INVALID and MESSAGE in str(e.value)
        assert ctx.get_option("sky_mipmap") == 1
    # on top of the bilinear filter only
    for call in (lambda: ctx.render_brute(pm, pc, CAP, R, DELTA), lambda: ctx.render_efficient(pm, pc, *efficient_args()),
                 lambda: ctx.render_direct(pm, pc, CAP, R, DELTA), lambda: ctx.render_brute_rows(pm, pc, 0, 4, CAP, R, DELTA)):
        with pytest.raises(curvis_amd.CurvisError) as e:
            call()
        assert e.value.code == _abi.E_INVALID and "sky_mipmap" in str(e.value) and "sky_filter" in str(e.value), str(e.value)
        assert ctx.get_option("sky_mipmap") == 1 and ctx.get_option("sky_filter") == 0
    ctx.set_option("sky_filter", 1)
    want = expected("brute", "ellis", "A", res, focal)[0]
    refused = [("debug dump", {}, dict(debug=True)), ("variant = 0", dict(variant=0), {}), ("fuse_shade = 0", dict(fuse_shade=0), {})]
    for words, opts, kw in refused:
        with options(ctx, **opts):
            with pytest.raises(curvis_amd.CurvisError) as e:
                ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)
            assert e.value.code == _abi.E_INVALID and "sky_mipmap" in str(e.value) and words in str(e.value), (words, str(e.value))
            assert ctx.get_option("sky_mipmap") == 1
            with options(ctx, sky_mipmap=0, sky_filter=0):
                ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)           # works with both off
    assert_frame(ctx.render_brute(pm, pc, CAP, R, DELTA)[0], want, "after the refusals")


CLI_RES = (24, 14)
SIM = ("escape_radius = 10.0\nray_integration_max_itarations = 4096\nray_integration_step = 0.05\n"
       "sampling_initial_nums = 100\nsampling_max_iterations = 50\n"
       "sampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 2e-5\n")


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_sky_mipmap")
    sp, sn = F.real_skies()
    pngio.write_png(d / "pos.png", np.array(sp))
    pngio.write_png(d / "neg.png", np.array(sn))
    (d / "sim.toml").write_text(SIM)
    (d / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = 43.0\nfocal_length = 6.0\n" % CLI_RES)
    return d


def test_binary_image_and_python_keyword(ctx, cli_files):
    d = cli_files
    _, _, pm, pc = common.scene("ellis", res=CLI_RES, focal=6.0)      # the binary's default pose
    sp, sn = (curvis_amd.SphericalImage(np.array(t)) for t in F.real_skies())
    system = curvis_amd.RelativisticSystem(pm, sp, sn, pc, context=ctx)
    api = {"brute": lambda **kw: system.render_image(4096, 10.0, 0.05, **kw),
           "efficient": lambda **kw: system.render_image_efficient(4096, 10.0, 0.05, 100, 100, 1e-5, 2e-5, **kw),
           "direct": lambda **kw: system.render_image_direct(4096, 10.0, 0.05, **kw)}
    lib = {"brute": lambda: ctx.render_brute(pm, pc, 4096, 10.0, 0.05)[0],
           "efficient": lambda: ctx.render_efficient(pm, pc, 4096, 10.0, 0.05, 100, 100, 1e-5, 2e-5)[0],
           "direct": lambda: ctx.render_direct(pm, pc, 4096, 10.0, 0.05)[0]}
    for mode in ("efficient", "brute", "direct"):
        out = d / ("img_" + mode)
        out.mkdir()
        r = run("image", d / "pos.png", d / "neg.png", out, "-s", d / "sim.toml", "-c", d / "cam.toml", "--mode", mode,
                "--sky-filter", "bilinear", "--sky-mipmap", "on")
        assert r.returncode == 0, r.stderr
        bilinear = api[mode](sky_filter="bilinear")
        keyword = api[mode](sky_filter="bilinear", sky_mipmap=True)
        assert ctx.get_option("sky_mipmap") == 0 and ctx.get_option("sky_filter") == 0      # the keyword puts the options back
        with options(ctx, **ON):
            library = lib[mode]()
        assert_frame(keyword, library, ("Python keyword", mode))
        assert_frame(pngio.read_png(out / "output_image.png"), library, ("curvis image --sky-mipmap on", mode))
        assert (library != bilinear).any()
        assert_frame(api[mode](sky_filter="bilinear", sky_mipmap=False), bilinear, ("sky_mipmap=False", mode))
    r = run("image", d / "pos.png", d / "neg.png", d / "refused", "-s", d / "sim.toml", "-c", d / "cam.toml", "--sky-mipmap", "on")
    assert r.returncode != 0 and "sky_mipmap" in r.stderr                  # without --sky-filter bilinear the library refuses the call


def test_binary_video_and_rendering_systems(ctx, cli_files, tmp_path):
    d = cli_files
    orbit = refpaths.reference_path_file("path_orbit.csv")
    (d / "vid.toml").write_text('video_name = "v"\nframe_rate = 0.05\nfilepath_to_camera_path = "%s"\n' % orbit)
    out = d / "vid"
    out.mkdir()
    r = run("video", d / "pos.png", d / "neg.png", out, "-v", d / "vid.toml", "-s", d / "sim.toml", "-c", d / "cam.toml",
            "--mode", "efficient", "--sky-filter=bilinear", "--sky-mipmap=on")
    assert r.returncode == 0, r.stderr
    it = rendering.Interpolator.from_file(orbit)
    times = rendering.times_of_frames(it.min_time(), it.max_time(), 0.05)
    assert len(times) == 3
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 6.0, 43.0, CLI_RES[0], CLI_RES[1])
            for t in times]
    bind(ctx, None)
    metric = curvis_amd.EllisMetric(1.0)
    with options(ctx, **ON):
        rgb, _ = ctx.render_efficient(metric, cams, 4096, 10.0, 0.05, 100, 100, 1e-5, 1e-5)   # the video loop passes threshold_1 twice
    with options(ctx, sky_filter=1):
        bilinear, _ = ctx.render_efficient(metric, cams, 4096, 10.0, 0.05, 100, 100, 1e-5, 1e-5)
    assert (rgb != bilinear).any()
    for k in range(3):
        assert_frame(pngio.read_png(out / "tmp" / ("frame_%d.png" % k)), rgb[k], ("curvis video --sky-mipmap=on, frame", k))
    # the Python rendering systems
    vs = rendering.VideoRenderingSettings(0.05, CLI_RES[0], CLI_RES[1], 43.0, 6.0, orbit, d / "pos.png", d / "neg.png", tmp_path / "v",
                                          escape_radius=10.0, max_iterations_propagation=4096, ray_integration_step=0.05, alphas_num=100,
                                          max_iterations_sampling=100, sampling_convergence_threshold_1=1e-5)
    video = rendering.VideoRenderingSystem.new(metric, vs, context=ctx, sky_filter="bilinear", sky_mipmap=True)
    frames = {}
    video.render(on_frame=lambda index, frame, stats: frames.__setitem__(index, np.array(frame)))
    assert ctx.get_option("sky_mipmap") == 0 and ctx.get_option("sky_filter") == 0
    for k in range(3):
        assert_frame(frames[k], rgb[k], ("VideoRenderingSystem, frame", k))
    pos, fwd, up = (0.0, 5.0, F.HALF_PI, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
    st = rendering.ImageRenderingSettings(d / "pos.png", d / "neg.png", tmp_path / "img", "one", pos, fwd, up, camera_focal_length=6.0,
                                          resolution_x=CLI_RES[0], resolution_y=CLI_RES[1], escape_radius=10.0,
                                          max_iterations_propagation=4096, alphas_num=100, max_iterations_sampling=100)
    image = rendering.ImageRenderingSystem.new(metric, st, context=ctx, sky_filter="bilinear", sky_mipmap=True)
    path = image.render()
    assert ctx.get_option("sky_mipmap") == 0 and ctx.get_option("sky_filter") == 0
    with options(ctx, **ON):                                   # the system has bound its own (unrotated) skies
        want = ctx.render_efficient(metric, curvis_amd.Camera(pos, fwd, up, 6.0, 43.0, CLI_RES[0], CLI_RES[1]), 4096, 10.0, 0.05, 100, 100,
                                    1e-5, 1e-5)[0]
    assert_frame(pngio.read_png(path), want, "ImageRenderingSystem")
