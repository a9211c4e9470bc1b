"""Camera projections (library option "projection": 1 equirectangular, 2 fisheye) against their definition, through every renderer.

The definition (include/curvis_hip.h) is restated in numpy FP64 in tests/projection_ref.py, which also composes each renderer's frame
per pixel from primitives of the CPU oracle (O.CV); tests/test_projection_host.py pins those compositions against the oracle's own
renders with the perspective vector.  Everything here is compared exactly.

Scene: camera at (0, 1.0, pi/2, 0) looking along (-1, 0.3, 0.2), up (0, 0, 1), focal 7, diagonal 43; Ellis rho = 1 and Interstellar
(0.1, 1e-4, 1); max_radius 10, delta 0.05, cap 240; index skies of 333 x 777 (+l) and 1000 x 500 (-l) texels; equirectangular frames
of 32 x 16 and fisheye frames of 20 x 14 pixels.  Every oracle-based test first asserts, from the composition, at least 8 rays to
either sky and 8 capped ones (brute), or 8 pixels on either sky (efficient, direct)."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import projection_ref as P
import refpaths
import sky_filter_ref as F
import curvis_amd
from curvis_amd import _abi, pngio, rendering

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
PROJECTIONS = (P.EQUIRECTANGULAR, P.FISHEYE)
BATCH_LS = (1.0, 1.5, -0.8)
R, DELTA, CAP = P.R, P.DELTA, P.CAP
MESSAGE = "projection must be 0 (perspective), 1 (equirectangular) or 2 (fisheye)"


def counters(st):
    return tuple(int(getattr(st, k)) for k in P.COUNTERS)


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


def bind(ctx, images=None, orient=None):
    for k, img in enumerate(images or P.index_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img), *(F.ORIENT[orient][k] if orient else ())))


@pytest.fixture()
def ctx(gpu_ctx):
    assert gpu_ctx.get_option("projection") == 0 and gpu_ctx.get_option("sky_filter") == 0 and gpu_ctx.get_option("supersample") == 1
    yield gpu_ctx
    for key, value in (("projection", 0), ("sky_filter", 0), ("supersample", 1)):
        gpu_ctx.set_option(key, value)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


KERNELS = (("default", {}), ("static", dict(variant=1)), ("relay", dict(variant=2, relay_min_blocks=0)))


# ---- 1. brute renderer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("projection", PROJECTIONS, ids=P.NAMES[1:])
def test_brute_vs_definition(ctx, projection, kind, fast_math):
    P.assert_classes("brute", kind, projection)
    bind(ctx)
    res = P.RES[projection]
    pm = P.scene(kind, res)[2]
    cams = [P.scene(kind, res, l=l)[3] for l in BATCH_LS]
    want = [P.expected("brute", kind, projection, l=l) for l in BATCH_LS]
    for name, opts in KERNELS:
        with options(ctx, projection=projection, fast_math=fast_math, **opts):
            what = (P.NAMES[projection], kind, fast_math, name)
            rgb, st = ctx.render_brute(pm, cams[0], CAP, R, DELTA)
            if name != "default":
                assert (ctx.get_option("last_relay_launches") >= 1) == (name == "relay"), what
            assert_frame(rgb, want[0][0], what)
            assert counters(st) == want[0][1] == counters(ctx.frame_stats(0)), what
            assert ctx.get_option("relay_mismatches") == 0 and ctx.get_option("relay_disabled") == 0
    # a batch of nine frames (more than "relay_max_frames": the static kernel) with three different cameras
    with options(ctx, projection=projection, fast_math=fast_math):
        rgb, st = ctx.render_brute(pm, [cams[f % 3] for f in range(9)], CAP, R, DELTA)
        assert ctx.get_option("last_relay_launches") == 0
        for f in range(9):
            assert_frame(rgb[f], want[f % 3][0], (P.NAMES[projection], kind, fast_math, "batch frame", f))
            assert counters(ctx.frame_stats(f)) == want[f % 3][1], (P.NAMES[projection], kind, fast_math, "batch frame", f)
        assert counters(st) == tuple(3 * sum(w[1][k] for w in want) for k in range(6))


@pytest.mark.parametrize("kind", P.KINDS)
def test_brute_odd_fisheye_frame_has_the_axis_pixel(ctx, kind):
    """21 x 15: the centre pixel's rho is 0 and its vector (1, 0, 0)"""
    P.assert_classes("brute", kind, P.FISHEYE, P.RES_ODD)
    oc, pm, pc = P.scene(kind, P.RES_ODD)[1:]
    vec = P.pixel_vectors(oc, P.FISHEYE, np.array([10]), np.array([7]))
    assert vec[0].tolist() == [1.0, 0.0, 0.0]
    bind(ctx)
    want, want_st, _ = P.expected("brute", kind, P.FISHEYE, P.RES_ODD)
    for name, opts in KERNELS[1:]:
        with options(ctx, projection=P.FISHEYE, **opts):
            rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
        assert_frame(rgb, want, ("odd fisheye", kind, name))
        assert counters(st) == want_st


# ---- 2. a row band ----------------------------------------------------------------------------------------------------------------
def test_rows_of_the_equirectangular_frame(ctx):
    P.assert_classes("brute", "ellis", P.EQUIRECTANGULAR)
    bind(ctx)
    pm, pc = P.scene("ellis", P.RES[P.EQUIRECTANGULAR])[2:]
    want = P.expected("brute", "ellis", P.EQUIRECTANGULAR)[0]
    with options(ctx, projection=P.EQUIRECTANGULAR):
        full, _ = ctx.render_brute(pm, pc, CAP, R, DELTA)
        band, st = ctx.render_brute_rows(pm, pc, 5, 6, CAP, R, DELTA)
    assert_frame(full, want, "full frame")
    assert_frame(band, full[5:11], "rows [5, 11)")
    assert st.rays == 6 * P.RES[P.EQUIRECTANGULAR][0]


# ---- 3. efficient renderer, both samplers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("projection", PROJECTIONS, ids=P.NAMES[1:])
def test_efficient_vs_definition(ctx, projection, kind):
    P.assert_classes("efficient", kind, projection)
    bind(ctx)
    res = P.RES[projection]
    pm = P.scene(kind, res)[2]
    cams = [P.scene(kind, res, l=l)[3] for l in BATCH_LS]
    want = [P.expected("efficient", kind, projection, l=l) for l in BATCH_LS]
    with options(ctx, projection=projection, device_sampler=0):
        rgb, st = ctx.render_efficient(pm, cams[0], *P.efficient_args())
        assert ctx.get_option("last_sampler_path") == 0
    assert_frame(rgb, want[0][0], (P.NAMES[projection], kind, "host-paced sampler"))
    assert counters(st)[2:] == want[0][1][2:] and st.rays == res[0] * res[1]
    with options(ctx, projection=projection, device_sampler=1, device_sampler_min_frames=1):
        rgb, st = ctx.render_efficient(pm, cams, *P.efficient_args())
        assert ctx.get_option("last_sampler_path") == 1
        for f in range(3):
            assert_frame(rgb[f], want[f][0], (P.NAMES[projection], kind, "device sampler", f))
            assert counters(ctx.frame_stats(f))[2:] == want[f][1][2:]


# ---- 4. direct renderer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("projection", PROJECTIONS, ids=P.NAMES[1:])
def test_direct_vs_definition(ctx, projection, kind, fast_math):
    P.assert_classes("direct", kind, projection)
    bind(ctx)
    pm, pc = P.scene(kind, P.RES[projection])[2:]
    want, want_st, _ = P.expected("direct", kind, projection)
    with options(ctx, projection=projection, fast_math=fast_math):
        rgb, st = ctx.render_direct(pm, pc, CAP, R, DELTA)
    assert_frame(rgb, want, (P.NAMES[projection], kind, fast_math))
    assert counters(st) == want_st


# ---- 5. supersample = 2 x bilinear: the box average of the filtered fine frame of the composition ----------------------------------
_fine = {}


def fine_oracle_skies():
    if "A" not in _fine:
        _fine["A"] = F.oracle_fine_skies("A")
    return _fine["A"]


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("projection", PROJECTIONS, ids=P.NAMES[1:])
def test_supersampled_and_filtered(ctx, projection, kind):
    n = 2
    F.assert_salts()
    skies = fine_oracle_skies()
    pm, pc = P.scene(kind, P.RES[projection])[2:]
    bind(ctx, F.real_skies(), "A")
    for renderer in ("brute", "efficient"):
        P.assert_classes(renderer, kind, projection, skies=skies, n=n)
        fine, fine_st, _ = P.expected(renderer, kind, projection, skies=skies, n=n)
        want = F.box_average(F.filtered_frame(fine)[0], n)
        with options(ctx, projection=projection, sky_filter=1, supersample=n):
            if renderer == "brute":
                for name, opts in KERNELS[1:]:
                    with options(ctx, **opts):
                        rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
                    assert_frame(rgb, want, (renderer, name, P.NAMES[projection], kind))
                    assert counters(st) == fine_st
            else:
                rgb, st = ctx.render_efficient(pm, pc, *P.efficient_args())
                assert_frame(rgb, want, (renderer, P.NAMES[projection], kind))
                assert counters(st)[2:] == fine_st[2:] and st.rays == fine_st[0]


# ---- 6. switched off again ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fresh_ctx():
    """a context of its own: what the relay seat belt has checked so far is this test's doing alone"""
    c = curvis_amd.Context(0)
    yield c
    c.close()


def test_switched_off_again_is_todays_frame(fresh_ctx):
    ctx = fresh_ctx
    bind(ctx)
    res = P.RES[P.EQUIRECTANGULAR]
    om, oc, pm, pc = P.scene("ellis", res)
    sp, sn = (O.sky(np.array(t)) for t in P.index_skies())
    today = [O.render_image(O.CV, om, oc, sp, sn, CAP, R, DELTA)[0], O.render_image_efficient(O.CV, om, oc, sp, sn, *P.efficient_args())[0],
             O.render_image_direct(O.CV, om, oc, sp, sn, CAP, R, DELTA)[0]]

    def renders():
        brute = ctx.render_brute(pm, pc, CAP, R, DELTA)[0]
        assert ctx.get_option("last_relay_launches") >= 1      # read before the other renderers' calls reset it
        return [brute, ctx.render_efficient(pm, pc, *P.efficient_args())[0], ctx.render_direct(pm, pc, CAP, R, DELTA)[0]]
    with options(ctx, variant=2, relay_min_blocks=0):
        checks = [ctx.get_option("relay_checks")]
        for projection in (0, 1, 0, 2, 1, 0):
            with options(ctx, projection=projection):
                frames = renders()
            checks.append(ctx.get_option("relay_checks"))
            if projection == 0:
                for got, want, name in zip(frames, today, ("brute", "efficient", "direct")):
                    assert_frame(got, want, ("projection 0 after a projected render", name))
            else:
                for got, was, name in zip(frames, today, ("brute", "efficient", "direct")):
                    assert_frame(got, P.expected(name, "ellis", projection, res)[0], (P.NAMES[projection], name))
                    assert (got != was).any()
        assert ctx.get_option("relay_mismatches") == 0 and ctx.get_option("relay_disabled") == 0
    # the launch shape carries the projection: the first equirectangular and the first fisheye launch were checked on their own,
    # the repeats of a shape were not
    steps = [b - a for a, b in zip(checks, checks[1:])]
    assert steps == [1, 1, 0, 1, 0, 0], checks


# ---- 7. option and refusals ------------------------------------------------------------------------------------------------------
def test_option_and_refusals(ctx):
    bind(ctx)
    res = P.RES[P.FISHEYE]
    pm, pc = P.scene("ellis", res)[2:]
    for value in (1, 2, 0, 2):
        ctx.set_option("projection", value)
        assert ctx.get_option("projection") == value
    for bad in (3, -1):
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.set_option("projection", bad)
        assert e.value.code == _abi.E_INVALID and MESSAGE in str(e.value)
        assert ctx.get_option("projection") == 2
    want = P.expected("brute", "ellis", P.FISHEYE)[0]
    refused = [("debug dump", {}, dict(debug=True)), ("variant = 0", dict(variant=0), {}), ("fuse_shade = 0", dict(fuse_shade=0), {})]
    for words, opts, kw in refused:
        with options(ctx, **opts):
            with pytest.raises(curvis_amd.CurvisError) as e:
                ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)
            assert e.value.code == _abi.E_INVALID and "projection" in str(e.value) and words in str(e.value), (words, str(e.value))
            assert ctx.get_option("projection") == 2
            with options(ctx, projection=0):
                ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)           # works with the option off
    assert_frame(ctx.render_brute(pm, pc, CAP, R, DELTA)[0], want, "after the refusals")
    # the fisheye's range: half the diagonal over the focal length beyond pi
    short = P.scene("ellis", res, focal=3.0)[3]
    assert not P.fisheye_in_range(P.scene("ellis", res, focal=3.0)[1]) and P.fisheye_in_range(P.scene("ellis", res)[1])
    for call in (lambda c: ctx.render_brute(pm, c, CAP, R, DELTA), lambda c: ctx.render_efficient(pm, c, *P.efficient_args()),
                 lambda c: ctx.render_direct(pm, c, CAP, R, DELTA), lambda c: ctx.render_brute(pm, [pc, c], CAP, R, DELTA)):
        with pytest.raises(curvis_amd.CurvisError) as e:
            call(short)
        assert e.value.code == _abi.E_INVALID and "fisheye" in str(e.value), str(e.value)
        call(pc)                                                          # the same call with focal 7
        for other in (0, 1):                                              # the other projections do not read the focal length's range
            with options(ctx, projection=other):
                call(short)


# ---- 8. the binary and the Python keywords -----------------------------------------------------------------------------------------
CLI_RES = (24, 14)
SIM = ("escape_radius = 10.0\nray_integration_max_itarations = 4096\nray_integration_step = 0.05\n"
       "sampling_initial_nums = 100\nsampling_max_iterations = 50\n"
       "sampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 2e-5\n")


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_projection")
    sp, sn = P.index_skies()
    pngio.write_png(d / "pos.png", np.array(sp))
    pngio.write_png(d / "neg.png", np.array(sn))
    (d / "sim.toml").write_text(SIM)
    (d / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = 43.0\nfocal_length = 7.0\n" % CLI_RES)
    return d


def test_binary_image_and_python_keywords(ctx, cli_files):
    import common
    d = cli_files
    _, _, pm, pc = common.scene("ellis", res=CLI_RES, focal=7.0)      # the binary's default pose
    sp, sn = (curvis_amd.SphericalImage(np.array(t)) for t in P.index_skies())
    system = curvis_amd.RelativisticSystem(pm, sp, sn, pc, context=ctx)
    api = {"brute": lambda **kw: system.render_image(4096, 10.0, 0.05, **kw),
           "efficient": lambda **kw: system.render_image_efficient(4096, 10.0, 0.05, 100, 50, 1e-5, 2e-5, **kw)}
    lib = {"brute": lambda: ctx.render_brute(pm, pc, 4096, 10.0, 0.05)[0],
           "efficient": lambda: ctx.render_efficient(pm, pc, 4096, 10.0, 0.05, 100, 50, 1e-5, 2e-5)[0]}
    for mode in ("efficient", "brute"):
        out = d / ("img_" + mode)
        out.mkdir()
        r = run("image", d / "pos.png", d / "neg.png", out, "-s", d / "sim.toml", "-c", d / "cam.toml", "--mode", mode,
                "--projection", "equirectangular")
        assert r.returncode == 0, r.stderr
        perspective = api[mode]()
        keyword = api[mode](projection="equirectangular")
        assert ctx.get_option("projection") == 0              # the keyword puts the context's option back
        with options(ctx, projection=P.EQUIRECTANGULAR):
            library = lib[mode]()
        assert_frame(keyword, library, ("Python keyword", mode))
        assert_frame(pngio.read_png(out / "output_image.png"), library, ("curvis image --projection equirectangular", mode))
        assert (library != perspective).any()
        assert_frame(api[mode](projection="perspective"), perspective, ("projection='perspective'", mode))
        with options(ctx, projection=P.FISHEYE):
            assert_frame(api[mode](projection="fisheye"), lib[mode](), ("projection='fisheye'", mode))


def test_binary_video(ctx, cli_files):
    d = cli_files
    orbit = refpaths.reference_path_file("path_orbit.csv")
    (d / "vid.toml").write_text('video_name = "v"\nframe_rate = 0.05\nfilepath_to_camera_path = "%s"\n' % orbit)
    out = d / "vid"
    out.mkdir()
    r = run("video", d / "pos.png", d / "neg.png", out, "-v", d / "vid.toml", "-s", d / "sim.toml", "-c", d / "cam.toml",
            "--mode", "efficient", "--projection=fisheye")
    assert r.returncode == 0, r.stderr
    it = rendering.Interpolator.from_file(orbit)
    times = rendering.times_of_frames(it.min_time(), it.max_time(), 0.05)
    assert len(times) == 3
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 7.0, 43.0, CLI_RES[0], CLI_RES[1])
            for t in times]
    bind(ctx)
    with options(ctx, projection=P.FISHEYE):
        # the video loop passes threshold_1 twice (src/rendering.rs:305-306)
        rgb, _ = ctx.render_efficient(curvis_amd.EllisMetric(1.0), cams, 4096, 10.0, 0.05, 100, 50, 1e-5, 1e-5)
    perspective, _ = ctx.render_efficient(curvis_amd.EllisMetric(1.0), cams, 4096, 10.0, 0.05, 100, 50, 1e-5, 1e-5)
    assert (rgb != perspective).any()
    for k in range(3):
        assert_frame(pngio.read_png(out / "tmp" / ("frame_%d.png" % k)), rgb[k], ("curvis video --projection=fisheye, frame", k))
