"""The moving camera (curvis_ctx_set_camera_velocities) on the GPU, through every renderer, exact against compositions over the boosted
directions of tests/camera_boost_ref.py: pixels and all six counters, no tolerance anywhere.

Scene: projection_ref's -- camera at (0, 1.0, pi/2, 0) looking along (-1, 0.3, 0.2), focal 7, diagonal 43; Ellis rho = 1 and
Interstellar (0.1, 1e-4, 1); max_radius 10, delta 0.05, cap 240; index skies of 333 x 777 (+l) and 1000 x 500 (-l) texels; perspective
frames of 24 x 16, equirectangular ones of 32 x 16.  Velocities (0.3, -0.4, 0.5) and (0, 0, 0.9).  Every comparison first asserts, from
the composition, at least 8 rays to either sky and 8 capped ones (brute), or 8 pixels on either sky (efficient, direct)."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import camera_boost_ref as B
import disc_ref as D
import oracle_lib as O
import projection_ref as P
import ref_compose as RC
import refpaths
import schwarzschild_ref as SCH
import step_scale_ref as SR
import curvis_amd
from curvis_amd import _abi, pngio, rendering, systems

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
R, DELTA, CAP = P.R, P.DELTA, P.CAP
V, V_PHI = B.VELOCITY, B.VELOCITY_PHI
PERSPECTIVE, EQUIRECTANGULAR = P.PERSPECTIVE, P.EQUIRECTANGULAR
CASE_IDS = ["perspective", "equirectangular"]
OPTION_DEFAULTS = dict(projection=0, sky_filter=0, sky_mipmap=0, supersample=1, step_scale=0, integrator=0, fast_math=1, variant=-1, fuse_shade=1,
                       device_sampler=-1)
RELAY = dict(variant=2, relay_min_blocks=0)


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


@contextlib.contextmanager
def velocities(ctx, beta):
    ctx.set_camera_velocities(beta)
    try:
        yield
    finally:
        ctx.set_camera_velocities(None)


def bind(ctx, images=None):
    for k, img in enumerate(images or P.index_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_camera_velocities(None)
    yield gpu_ctx
    gpu_ctx.set_camera_velocities(None)
    gpu_ctx.set_disc(None)
    for key, value in OPTION_DEFAULTS.items():
        gpu_ctx.set_option(key, value)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def still(renderer, kind, projection, l=P.POS[1]):
    """the composition of the same frame with the camera at rest"""
    return P.expected(renderer, kind, projection, res=B.RES[projection], l=l)


# ---- 1. brute renderer ---------------------------------------------------------------------------------------------------------------
def brute_case(ctx, projection, beta, kind, fast_math):
    B.assert_classes("brute", kind, projection, beta)
    bind(ctx)
    pm, pc = P.scene(kind, B.RES[projection])[2:]
    want, want_st, _ = B.expected("brute", kind, projection, beta)
    assert (want != still("brute", kind, projection)[0]).any(axis=-1).sum() >= 100
    with velocities(ctx, [beta]):
        for name, opts in (("default", {}), ("static", dict(variant=1)), ("relay asked for", RELAY)):
            with options(ctx, projection=projection, fast_math=fast_math, **opts):
                rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
                assert ctx.get_option("last_relay_launches") == 0, name      # the static kernel, whatever was asked for
            what = (P.NAMES[projection], beta, kind, fast_math, name)
            assert_frame(rgb, want, what)
            assert counters(st) == want_st == counters(ctx.frame_stats(0)), what


@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("projection", [PERSPECTIVE, EQUIRECTANGULAR], ids=CASE_IDS[:2])
def test_brute_vs_definition(ctx, projection, kind, fast_math):
    brute_case(ctx, projection, V, kind, fast_math)


@pytest.mark.parametrize("kind", P.KINDS)
def test_brute_velocity_along_phi(ctx, kind):
    brute_case(ctx, PERSPECTIVE, V_PHI, kind, 1)


# ---- 2. efficient renderer, both samplers, and the direct renderer ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("projection", [PERSPECTIVE, EQUIRECTANGULAR], ids=CASE_IDS[:2])
def test_efficient_vs_definition(ctx, projection, kind):
    B.assert_classes("efficient", kind, projection, V)
    bind(ctx)
    res = B.RES[projection]
    pm, pc = P.scene(kind, res)[2:]
    want, want_st, _ = B.expected("efficient", kind, projection, V)
    assert (want != still("efficient", kind, projection)[0]).any()
    with velocities(ctx, [V]):
        for device_sampler in (0, 1):
            with options(ctx, projection=projection, device_sampler=device_sampler, device_sampler_min_frames=1):
                rgb, st = ctx.render_efficient(pm, pc, *P.efficient_args())
                assert ctx.get_option("last_sampler_path") == device_sampler
            assert_frame(rgb, want, (P.NAMES[projection], kind, "device sampler", device_sampler))
            assert counters(st)[2:] == want_st[2:] and st.rays == res[0] * res[1]


@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("projection", [PERSPECTIVE, EQUIRECTANGULAR], ids=CASE_IDS[:2])
def test_direct_vs_definition(ctx, projection, kind, fast_math):
    B.assert_classes("direct", kind, projection, V)
    bind(ctx)
    pm, pc = P.scene(kind, B.RES[projection])[2:]
    want, want_st, _ = B.expected("direct", kind, projection, V)
    with velocities(ctx, [V]), options(ctx, projection=projection, fast_math=fast_math):
        rgb, st = ctx.render_direct(pm, pc, CAP, R, DELTA)
    assert_frame(rgb, want, (P.NAMES[projection], kind, fast_math))
    assert counters(st) == want_st


# ---- 3. one Schwarzschild frame: against the library's own strict step on the host ----------------------------------------------------------
def test_schwarzschild_frame(ctx):
    res = (24, 16)
    pm, oc, pc = SCH.scene(res)
    sp, sn = (O.sky(np.array(t)) for t in SCH.index_skies())
    dirs = B.outward_vectors(oc, PERSPECTIVE, V)[1]
    want, want_st, _ = SCH.memo(("camera boost", res, V), lambda: SCH.compose_brute(pm, oc, dirs, sp, sn, SCH.CAP, SCH.R, SCH.DELTA))
    assert want_st[2] >= 8 and want_st[3] >= 8, want_st        # rays that miss the hole and rays it captures
    for k, img in enumerate(SCH.index_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))
    with velocities(ctx, [V]):
        rgb, st = ctx.render_brute(pm, pc, SCH.CAP, SCH.R, SCH.DELTA)
    assert_frame(rgb, want, "Schwarzschild, brute")
    assert counters(st) == want_st
    rgb0, _ = ctx.render_brute(pm, pc, SCH.CAP, SCH.R, SCH.DELTA)
    assert (rgb0 != rgb).any()


# ---- 4. batches: every frame its own velocity and camera ----------------------------------------------------------------------------------
BATCH = ((1.0, V), (1.5, (0.0, 0.0, 0.0)), (-0.8, V_PHI))


def batch_expected(renderer, kind, beta_of=None):
    out = []
    for l, beta in BATCH:
        beta = beta_of or beta
        out.append(B.expected(renderer, kind, PERSPECTIVE, beta, l=l) if any(beta) else still(renderer, kind, PERSPECTIVE, l=l))
    return out


@pytest.mark.parametrize("kind", P.KINDS)
def test_brute_batch(ctx, kind):
    B.assert_classes("brute", kind, PERSPECTIVE, V)
    bind(ctx)
    res = B.RES[PERSPECTIVE]
    pm = P.scene(kind, res)[2]
    cams = [P.scene(kind, res, l=l)[3] for l, _ in BATCH]
    want = batch_expected("brute", kind)
    with velocities(ctx, [beta for _, beta in BATCH]):
        rgb, st = ctx.render_brute(pm, cams, CAP, R, DELTA)
        for f in range(3):
            assert_frame(rgb[f], want[f][0], (kind, "batch frame", f))
            assert counters(ctx.frame_stats(f)) == want[f][1], (kind, "batch frame", f)
        assert counters(st) == tuple(sum(w[1][k] for w in want) for k in range(6))
    # n = 1: the one triple for every frame; n = 2 for three frames: refused, nothing rendered
    want = batch_expected("brute", kind, V)
    with velocities(ctx, [V]):
        rgb, _ = ctx.render_brute(pm, cams, CAP, R, DELTA)
    for f in range(3):
        assert_frame(rgb[f], want[f][0], (kind, "broadcast frame", f))
    with velocities(ctx, [V, V_PHI]):
        for call in (lambda: ctx.render_brute(pm, cams, CAP, R, DELTA), lambda: ctx.render_efficient(pm, cams, *P.efficient_args()),
                     lambda: ctx.render_brute(pm, cams[0], CAP, R, DELTA), lambda: ctx.render_direct(pm, cams[0], CAP, R, DELTA)):
            with pytest.raises(curvis_amd.CurvisError) as e:
                call()
            assert e.value.code == _abi.E_INVALID and "camera velocity" in str(e.value), str(e.value)
        ctx.render_brute(pm, cams[:2], CAP, R, DELTA)          # two frames: taken


@pytest.mark.parametrize("kind", P.KINDS)
def test_efficient_batch(ctx, kind):
    bind(ctx)
    res = B.RES[PERSPECTIVE]
    pm = P.scene(kind, res)[2]
    cams = [P.scene(kind, res, l=l)[3] for l, _ in BATCH]
    want = batch_expected("efficient", kind)
    with velocities(ctx, [beta for _, beta in BATCH]):
        for device_sampler in (1, 0):
            with options(ctx, device_sampler=device_sampler, device_sampler_min_frames=1):
                rgb, _ = ctx.render_efficient(pm, cams, *P.efficient_args())
                for f in range(3):
                    assert_frame(rgb[f], want[f][0], (kind, "sampler", device_sampler, "batch frame", f))
                    assert counters(ctx.frame_stats(f))[2:] == want[f][1][2:]


# ---- 5. row bands ----------------------------------------------------------------------------------------------------------------------
def test_two_bands_are_the_frame(ctx):
    B.assert_classes("brute", "ellis", PERSPECTIVE, V)
    bind(ctx)
    pm, pc = P.scene("ellis", B.RES[PERSPECTIVE])[2:]
    want = B.expected("brute", "ellis", PERSPECTIVE, V)[0]
    with velocities(ctx, [V]):
        top, st_top = ctx.render_brute_rows(pm, pc, 0, 7, CAP, R, DELTA)
        bottom, st_bottom = ctx.render_brute_rows(pm, pc, 7, 9, CAP, R, DELTA)
    assert_frame(np.concatenate([top, bottom]), want, "rows [0, 7) and [7, 16)")
    assert st_top.rays == 7 * 24 and st_bottom.rays == 9 * 24


# ---- 6. every option together ------------------------------------------------------------------------------------------------------------
S, HEUN = 4 * 256, 1
COMBINED = dict(supersample=2, sky_filter=1, sky_mipmap=1, step_scale=S, integrator=HEUN)


def test_every_option_together(ctx, kind="ellis"):
    """supersample 2, the mip-mapped bilinear lookup, scaled Heun steps: the box average of the boosted 24 x 16 composition.  The Ellis
    scene: under scaled Heun steps its walk keeps the three ray classes (asserted below); the Interstellar walk keeps 3 capped rays of
    its 64, fewer than the 8 a brute comparison asks for."""
    fine_res = (24, 16)
    om, oc = P.scene(kind, fine_res)[:2]
    pm, pc = P.scene(kind, (12, 8))[2:]
    images = P.index_skies()
    oracle_skies = tuple(O.sky(np.array(t)) for t in images)
    dirs = B.outward_vectors(oc, PERSPECTIVE, V)[1]
    bind(ctx)

    def brute():
        rays = RC.compose_brute(RC.OracleStepper(om), oc.pos, dirs, CAP, R, DELTA, S, HEUN)
        return RC.frame(rays, None, "mipmap", images, oracle_skies)

    def efficient():
        f = RC.EscapeAngle(RC.OracleStepper(om), oc.pos[1], DELTA, S, HEUN, CAP, R, memo=True)
        table = RC.sample_table(f, P.EFF["n0"], P.EFF["maxit"], P.EFF["t1"], P.EFF["t2"])
        return RC.frame(RC.compose_efficient(table, oc, dirs), None, "mipmap", images, oracle_skies, steps=f.steps)
    fine, cnt = RC.memo(("camera boost, all options, brute", kind), brute)
    assert min(cnt[2:5]) >= 8, cnt
    with velocities(ctx, [V]), options(ctx, **COMBINED):
        rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
    assert_frame(rgb, SR.box_average(fine, 2), (kind, "brute"))
    assert counters(st) == cnt[:6]
    fine, cnt = RC.memo(("camera boost, all options, efficient", kind), efficient)
    assert min(cnt[2:4]) >= 8, cnt
    with velocities(ctx, [V]), options(ctx, **COMBINED):
        rgb, st = ctx.render_efficient(pm, pc, *P.efficient_args())
    assert_frame(rgb, SR.box_average(fine, 2), (kind, "efficient"))
    assert counters(st)[2:] == cnt[2:6] and st.rays == cnt[0]


# ---- 7. a disc -----------------------------------------------------------------------------------------------------------------------------
def test_static_disc_and_velocity(ctx):
    """disc_ref's scene A, its walk fed the boosted directions"""
    _, om, pm, oc, pc, disc = D.scene("A")
    dirs = B.outward_vectors(oc, PERSPECTIVE, V)[1]
    rays = RC.memo(("camera boost, disc A",), lambda: D.walk_rays(RC.OracleStepper(om), oc.pos, dirs, disc, D.CAP, D.R, D.DELTA))
    D.assert_classes(rays, "A, moving camera")
    want, want_cnt = RC.frame(rays, disc, "nearest", SR.index_skies(), SR.oracle_skies())
    for k, img in enumerate(SR.index_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))
    ctx.set_disc(curvis_amd.Disc(np.array(disc.rgba), disc.l_in, disc.l_out))
    with velocities(ctx, [V]):
        rgb, st = ctx.render_brute(pm, pc, D.CAP, D.R, D.DELTA)
        assert counters(st) + (ctx.frame_disc_hits(0),) == want_cnt
    assert_frame(rgb, want, "disc A")
    assert (rgb != D.scene_frame("A")[0]).any()


def test_moving_disc_and_velocity_is_refused(ctx):
    pm, _, pc, disc = D.schwarzschild_scene()
    for k, img in enumerate(SR.index_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))
    ctx.set_disc(curvis_amd.Disc(np.array(disc.rgba), disc.l_in, disc.l_out, motion="prograde"))
    with velocities(ctx, [V]):
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.render_brute(pm, pc, 64, D.R, D.DELTA)
        assert e.value.code == _abi.E_INVALID and "camera velocity" in str(e.value) and "disc" in str(e.value), str(e.value)
    with velocities(ctx, [(0.0, 0.0, 0.0)]):
        ctx.render_brute(pm, pc, 64, D.R, D.DELTA)               # a camera at rest: taken
    ctx.set_disc_motion("static")
    with velocities(ctx, [V]):
        ctx.render_brute(pm, pc, 64, D.R, D.DELTA)               # a disc at rest: taken


# ---- 8. zero, cleared, refused -----------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fresh_ctx():
    """a context of its own: what the relay seat belt has checked so far is this test's doing alone"""
    c = curvis_amd.Context(0)
    yield c
    c.close()


def test_zero_and_cleared_are_todays_frames(fresh_ctx):
    ctx = fresh_ctx
    bind(ctx)
    res = B.RES[PERSPECTIVE]
    om, oc, pm, pc = P.scene("ellis", res)
    sp, sn = (O.sky(np.array(t)) for t in P.index_skies())
    today = [O.render_image(O.CV, om, oc, sp, sn, CAP, R, DELTA)[0], O.render_image_efficient(O.CV, om, oc, sp, sn, *P.efficient_args())[0],
             O.render_image_direct(O.CV, om, oc, sp, sn, CAP, R, DELTA)[0]]

    def renders(relay):
        brute = ctx.render_brute(pm, pc, CAP, R, DELTA)[0]
        assert (ctx.get_option("last_relay_launches") >= 1) == relay      # read before the other renderers' calls reset it
        return [brute, ctx.render_efficient(pm, pc, *P.efficient_args())[0], ctx.render_direct(pm, pc, CAP, R, DELTA)[0]]
    with options(ctx, **RELAY):
        for beta in (None, [V], [(0.0, 0.0, 0.0)], [V_PHI], None, [(-0.0, 0.0, 0.0)] * 1):
            ctx.set_camera_velocities(beta)
            moving = beta is not None and any(beta[0])
            frames = renders(relay=not moving)          # at rest the relay kernel renders the call again: the PROJ = 0 form of before
            for got, want, name in zip(frames, today, ("brute", "efficient", "direct")):
                if moving:
                    assert_frame(got, B.expected(name, "ellis", PERSPECTIVE, beta[0])[0], (beta, name))
                    assert (got != want).any()
                else:
                    assert_frame(got, want, ("at rest", beta, name))
        assert ctx.get_option("relay_mismatches") == 0 and ctx.get_option("relay_disabled") == 0


def test_refusals(ctx):
    bind(ctx)
    pm, pc = P.scene("ellis", B.RES[PERSPECTIVE])[2:]
    L = _abi.lib()
    for bad in ([(1.0, 0.0, 0.0)], [V, (0.6, 0.8, 0.1)], [(np.nan, 0.0, 0.0)]):
        ctx.set_camera_velocities([V_PHI])
        with pytest.raises(ValueError, match="camera velocity"):
            ctx.set_camera_velocities(bad)
        # the former state stays
        assert_frame(ctx.render_brute(pm, pc, CAP, R, DELTA)[0], B.expected("brute", "ellis", PERSPECTIVE, V_PHI)[0], "after a refused setting")
    assert L.curvis_ctx_set_camera_velocities(ctx._h, None, 3) == 0          # NULL clears, whatever n says
    assert_frame(ctx.render_brute(pm, pc, CAP, R, DELTA)[0], still("brute", "ellis", PERSPECTIVE)[0], "cleared")
    want = B.expected("brute", "ellis", PERSPECTIVE, V)[0]
    refused = [("debug dump", {}, dict(debug=True)), ("variant = 0", dict(variant=0), {}), ("fuse_shade = 0", dict(fuse_shade=0), {})]
    with velocities(ctx, [V]):
        for words, opts, kw in refused:
            with options(ctx, **opts):
                with pytest.raises(curvis_amd.CurvisError) as e:
                    ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)
                assert e.value.code == _abi.E_INVALID and "camera velocity" in str(e.value) and words in str(e.value), (words, str(e.value))
        assert_frame(ctx.render_brute(pm, pc, CAP, R, DELTA)[0], want, "after the refusals")
    for words, opts, kw in refused:                                # and with a camera at rest every one of them works
        with velocities(ctx, [(0.0, 0.0, 0.0)]), options(ctx, **opts):
            ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)


# ---- 9. the Python keywords and the binary -------------------------------------------------------------------------------------------------
CLI_RES = (32, 18)
SIM = ("escape_radius = 10.0\nray_integration_max_itarations = 4096\nray_integration_step = 0.05\n"
       "sampling_initial_nums = 100\nsampling_max_iterations = 50\n"
       "sampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 2e-5\n")


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_camera_boost")
    sp, sn = P.index_skies()
    pngio.write_png(d / "pos.png", np.array(sp))
    pngio.write_png(d / "neg.png", np.array(sn))
    (d / "sim.toml").write_text(SIM)
    (d / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = 43.0\nfocal_length = 7.0\n" % CLI_RES)
    return d


def test_python_keyword_and_binary_image(ctx, cli_files):
    import common
    d = cli_files
    _, _, pm, pc = common.scene("ellis", res=CLI_RES, focal=7.0)      # the binary's default pose
    sp, sn = (curvis_amd.SphericalImage(np.array(t)) for t in P.index_skies())
    system = curvis_amd.RelativisticSystem(pm, sp, sn, pc, context=ctx)
    api = {"brute": lambda **kw: system.render_image(4096, 10.0, 0.05, **kw),
           "efficient": lambda **kw: system.render_image_efficient(4096, 10.0, 0.05, 100, 50, 1e-5, 2e-5, **kw),
           "direct": lambda **kw: system.render_image_direct(4096, 10.0, 0.05, **kw)}
    lib = {"brute": lambda: ctx.render_brute(pm, pc, 4096, 10.0, 0.05)[0],
           "efficient": lambda: ctx.render_efficient(pm, pc, 4096, 10.0, 0.05, 100, 50, 1e-5, 2e-5)[0],
           "direct": lambda: ctx.render_direct(pm, pc, 4096, 10.0, 0.05)[0]}
    for mode in ("efficient", "brute", "direct"):
        at_rest = api[mode]()
        keyword = api[mode](velocity=V)
        assert_frame(api[mode](), at_rest, ("the keyword clears the context's velocities", mode))
        with velocities(ctx, [V]):
            library = lib[mode]()
        assert_frame(keyword, library, ("Python keyword", mode))
        assert (library != at_rest).any()
        if mode == "direct":
            continue
        out = d / ("img_" + mode)
        out.mkdir()
        r = run("image", d / "pos.png", d / "neg.png", out, "-s", d / "sim.toml", "-c", d / "cam.toml", "--mode", mode,
                "--camera-velocity", "%r,%r,%r" % V)
        assert r.returncode == 0, r.stderr
        assert_frame(pngio.read_png(out / "output_image.png"), library, ("curvis image --camera-velocity", mode))
    with pytest.raises(ValueError, match="velocity"):
        system.render_image(4096, 10.0, 0.05, velocity=(1.0, 0.0, 0.0))


@pytest.mark.parametrize("name", ("path_through.csv", "path_orbit.csv"))
def test_binary_and_python_video_on_a_path(ctx, cli_files, name):
    d = cli_files
    path = refpaths.reference_path_file(name)
    it = rendering.Interpolator.from_file(path)
    rate = 5.5 / (it.max_time() - it.min_time())        # six frames, the last one well before the path's last segment
    times = rendering.times_of_frames(it.min_time(), it.max_time(), rate)
    assert len(times) == 6
    tag = name.split(".")[0]
    (d / (tag + ".toml")).write_text('video_name = "v"\nframe_rate = %r\nfilepath_to_camera_path = "%s"\n' % (rate, path))
    out = d / ("vid_" + tag)
    out.mkdir()
    r = run("video", d / "pos.png", d / "neg.png", out, "-v", d / (tag + ".toml"), "-s", d / "sim.toml", "-c", d / "cam.toml",
            "--mode", "efficient", "--camera-motion", "path", "--light-speed", "1", "--stats", out / "stats.jsonl")
    assert r.returncode == 0, r.stderr
    pm = curvis_amd.EllisMetric(1.0)
    poses = [np.concatenate(([t], it.camera_position(t)[1:4])) for t in times]
    beta = [systems.camera_path_velocity(pm, poses[max(k - 1, 0)], poses[k], poses[min(k + 1, 5)], 1.0) for k in range(6)]
    assert all(0.05 < sum(b * b for b in v) ** 0.5 < 1.0 for v in beta), beta
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 7.0, 43.0, CLI_RES[0], CLI_RES[1]) for t in times]
    bind(ctx)
    with velocities(ctx, beta):
        # the video loop passes threshold_1 twice (src/rendering.rs:305-306)
        rgb, _ = ctx.render_efficient(pm, cams, 4096, 10.0, 0.05, 100, 50, 1e-5, 1e-5)
    at_rest, _ = ctx.render_efficient(pm, cams, 4096, 10.0, 0.05, 100, 50, 1e-5, 1e-5)
    assert (rgb != at_rest).any()
    for k in range(6):
        assert_frame(pngio.read_png(out / "tmp" / ("frame_%d.png" % k)), rgb[k], ("curvis video --camera-motion path, frame", k))
    import json
    lines = [json.loads(s) for s in (out / "stats.jsonl").read_text().splitlines() if s.strip()]
    frames = {int(s["frame"]): s for s in lines if "frame" in s}
    for k in range(6):
        assert [float(v) for v in frames[k]["beta"]] == list(beta[k]), (k, frames[k].get("beta"), beta[k])
    # the Python mirror
    video = rendering.VideoRenderingSystem(pm, ctx, it, rate, CLI_RES, 43.0, 7.0, 10.0, 4096, 0.05, batch=4, sampling_initial_nums=100,
                                           sampling_convergence_threshold_1=1e-5, camera_motion="path", light_speed=1.0)
    video.max_iterations_sampling = 50
    got = {}
    stats = video.render(on_frame=lambda k, frame, s: got.__setitem__(k, np.array(frame)))
    for k in range(6):
        assert_frame(got[k], rgb[k], ("VideoRenderingSystem(camera_motion='path'), frame", k))
        assert stats[k]["beta"] == beta[k]
    assert_frame(ctx.render_efficient(pm, cams[0], 4096, 10.0, 0.05, 100, 50, 1e-5, 1e-5)[0], at_rest[0], "the velocities are cleared afterwards")
    if name == "path_through.csv":
        # ten times slower light: the fly-through exceeds it, and the run stops with the frame's number before anything is rendered
        out2 = d / "vid_too_fast"
        out2.mkdir()
        r = run("video", d / "pos.png", d / "neg.png", out2, "-v", d / (tag + ".toml"), "-s", d / "sim.toml", "-c", d / "cam.toml",
                "--mode", "efficient", "--camera-motion", "path", "--light-speed", "0.1")
        first = min(k for k in range(6) if sum((10.0 * b) ** 2 for b in beta[k]) >= 1.0)       # beta is linear in 1 / light_speed
        assert r.returncode != 0 and ("frame %d" % first) in r.stderr and "light" in r.stderr, r.stderr
        assert not (out2 / "tmp" / "frame_0.png").exists()
        slow = rendering.VideoRenderingSystem(pm, ctx, it, rate, CLI_RES, 43.0, 7.0, 10.0, 4096, 0.05, camera_motion="path", light_speed=0.1)
        with pytest.raises(ValueError, match="frame %d " % first):
            slow.render()
