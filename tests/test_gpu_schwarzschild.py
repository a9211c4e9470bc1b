"""The Schwarzschild kind (CURVIS_METRIC_SCHWARZSCHILD) on the GPU, through every renderer, against references composed in
tests/schwarzschild_ref.py from the library's host accessors (the strict step on x86) and the oracle's metric-independent primitives.
Everything is compared exactly.

Scene: M = 1, camera at l = 8 on the equator looking 20 degrees off the hole, max_radius 25, delta 0.05, cap 4096; frames of 24 x 16
and 32 x 24; index skies of 333 x 177 (+l) and 129 x 301 (-l, "the horizon") texels.  The shadow covers part of the frame, so rays
cross, graze and miss the photon sphere (asserted from the reference: rays to either side)."""
import contextlib
import math
import os
import subprocess

import numpy as np
import pytest

import common
import oracle_lib as O
import projection_ref as PR
import schwarzschild_ref as SR
import sky_filter_ref as F
import sky_mipmap_ref as MIP
import curvis_amd
from curvis_amd import _abi, pngio, rendering

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
R, DELTA, CAP = SR.R, SR.DELTA, SR.CAP
EFF = (CAP, R, DELTA, 100, 100, 1e-5, 1e-5)
OPTION_DEFAULTS = dict(projection=0, sky_filter=0, sky_mipmap=0, supersample=1, step_scale=0, integrator=0, fast_math=1, variant=-1, device_sampler=-1)


def counters(st):
    return tuple(int(getattr(st, k)) for k in SR.COUNTERS)


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
    yield gpu_ctx
    for key in ("sky_mipmap", "sky_filter", "projection", "supersample", "integrator", "step_scale", "fast_math", "variant", "device_sampler"):
        gpu_ctx.set_option(key, OPTION_DEFAULTS[key])


def bind(ctx, images=None):
    for k, img in enumerate(images or SR.index_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))


def oracle_skies():
    return tuple(O.sky(np.array(t)) for t in SR.index_skies())


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def expected(renderer, res, step_scale=0, integrator=0):
    def make():
        pm, oc, _ = SR.scene(res)
        dirs = PR.outward_vectors(oc, PR.PERSPECTIVE)[1]
        sp, sn = oracle_skies()
        compose = SR.compose_brute if renderer == "brute" else SR.compose_direct
        out = compose(pm, oc, dirs, sp, sn, CAP, R, DELTA, step_scale, integrator)
        assert out[1][2] >= 8 and out[1][3] >= 8, (renderer, res, out[1])   # rays that miss the hole and rays it captures
        return out
    return SR.memo((renderer, res, step_scale, integrator), make)


# ---- G1: the debug dump ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", SR.FRAMES)
@pytest.mark.parametrize("opts", [dict(), dict(fast_math=0), dict(step_scale=4 * 256), dict(integrator=1)], ids=["fast", "strict", "scaled", "heun"])
def test_debug_dump_equals_the_host_walk(ctx, res, opts):
    bind(ctx)
    pm, oc, pc = SR.scene(res)
    S, integ = opts.get("step_scale", 0), opts.get("integrator", 0)
    want = SR.memo(("dump", res, S, integ), lambda: SR.debug_dump(pm, oc, PR.outward_vectors(oc, PR.PERSPECTIVE)[1], SR.SKY_SHAPES, DELTA, CAP, R, S, integ))
    assert (want["code"] == 1).sum() >= 8 and (want["code"] == -1).sum() >= 8
    with options(ctx, **opts):
        _, st, dbg = ctx.render_brute(pm, pc, CAP, R, DELTA, debug=True)
    common.assert_debug_equal(dbg, want)
    assert st.steps == int(want["steps"].sum()) and st.n_neg == int((want["code"] == -1).sum())


# ---- G2: fused frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", SR.FRAMES)
@pytest.mark.parametrize("fast_math", [1, 0])
def test_brute_frames(ctx, res, fast_math):
    bind(ctx)
    pm, _, pc = SR.scene(res)
    want, want_st, _ = expected("brute", res)
    for name, opts in (("default", {}), ("static", dict(variant=1)), ("relay asked for", dict(variant=2, relay_min_blocks=0))):
        with options(ctx, fast_math=fast_math, **opts):
            rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
            assert ctx.get_option("last_relay_launches") == 0, name     # the static kernel, whatever was asked for
        assert_frame(rgb, want, (res, fast_math, name))
        assert counters(st) == want_st == counters(ctx.frame_stats(0)), (res, fast_math, name)
    with options(ctx, fast_math=fast_math):
        rgb, st = ctx.render_brute(pm, [pc] * 3, CAP, R, DELTA)
    for f in range(3):
        assert_frame(rgb[f], want, (res, fast_math, "batch", f))
    assert counters(st) == tuple(3 * v for v in want_st)


@pytest.mark.parametrize("res", SR.FRAMES)
@pytest.mark.parametrize("fast_math", [1, 0])
def test_direct_frames(ctx, res, fast_math):
    bind(ctx)
    pm, _, pc = SR.scene(res)
    want, want_st, _ = expected("direct", res)
    with options(ctx, fast_math=fast_math):
        rgb, st = ctx.render_direct(pm, pc, CAP, R, DELTA)
    assert_frame(rgb, want, (res, fast_math))
    assert counters(st) == want_st


@pytest.mark.parametrize("res", SR.FRAMES)
@pytest.mark.parametrize("device_sampler", [0, 1])
def test_efficient_frames_and_sample_tables(ctx, res, device_sampler):
    bind(ctx)
    pm, oc, pc = SR.scene(res)
    with options(ctx, device_sampler=device_sampler, device_sampler_min_frames=1):
        rgb, st = ctx.render_efficient(pm, pc, *EFF)
        assert ctx.get_option("last_sampler_path") == device_sampler
        a, e, s = ctx.samples(0)
    # every entry of the table against compute_escape_angle at that alpha, independently of the refinement logic
    assert len(a) >= 100 and (s == 1.0).sum() >= 8 and (s == -1.0).sum() >= 8
    for k in range(len(a)):
        code, ang, _ = SR.compute_escape_angle(pm, SR.L_CAM, float(a[k]), DELTA, CAP, R)
        assert code in (1, -1) and s[k] == float(code), (k, a[k], s[k], code)
        assert np.float64(ang).view(np.uint64) == np.float64(e[k]).view(np.uint64), (k, a[k], e[k], ang)
    sp, sn = oracle_skies()
    want, want_cnt = SR.compose_efficient_from_table(oc, PR.outward_vectors(oc, PR.PERSPECTIVE)[1], sp, sn, dict(a=a, e=e, s=s))
    assert want_cnt[1] >= 8 and want_cnt[2] >= 8
    assert_frame(rgb, want, (res, device_sampler))
    assert (st.rays, st.n_pos, st.n_neg, st.n_none, st.n_oob) == want_cnt


# ---- G3: the options together ---------------------------------------------------------------------------------------------------------
G3 = dict(supersample=2, sky_filter=1, sky_mipmap=1, projection=PR.FISHEYE, integrator=1, step_scale=4 * 256)
G3_RES = (24, 16)


def _fine_scene():
    pm, _, pc = SR.scene(G3_RES)
    oc_fine = SR.scene((G3_RES[0] * 2, G3_RES[1] * 2))[1]
    return pm, oc_fine, pc, PR.outward_vectors(oc_fine, PR.FISHEYE)[1]


def _g3_frame(fine_rgb, n_none):
    which, Xc, Yc = F.decode(fine_rgb)
    assert int((which < 0).sum()) == n_none
    want = MIP.mip_frame(which, Xc, Yc, F.real_skies())[0]
    return F.box_average(want, 2)


@pytest.mark.parametrize("renderer", ["brute", "direct", "efficient"])
def test_all_options_in_one_render(ctx, renderer):
    """supersample 2, bilinear filter on a mip pyramid, fisheye, Heun and scaled steps together: the rays of the 2 x 2 finer fisheye
    grid are walked on the host over the fine index skies (256 times the real ones), and the filters' integer steps are
    tests/sky_filter_ref.py's and tests/sky_mipmap_ref.py's"""
    F.assert_salts()
    assert PR.fisheye_in_range(SR.scene(G3_RES)[1])
    pm, oc_fine, pc, dirs = _fine_scene()
    fine = tuple(O.sky(img) for img in F.fine_skies())
    for k, img in enumerate(F.real_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))
    S, integ = G3["step_scale"], G3["integrator"]
    with options(ctx, **G3):
        if renderer == "brute":
            fine_rgb, cnt, _ = SR.memo("g3 brute", lambda: SR.compose_brute(pm, oc_fine, dirs, fine[0], fine[1], CAP, R, DELTA, S, integ))
            rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
            assert ctx.get_option("last_relay_launches") == 0
            assert counters(st) == cnt
        elif renderer == "direct":
            fine_rgb, cnt, _ = SR.memo("g3 direct", lambda: SR.compose_direct(pm, oc_fine, dirs, fine[0], fine[1], CAP, R, DELTA, S, integ))
            rgb, st = ctx.render_direct(pm, pc, CAP, R, DELTA)
            assert counters(st) == cnt
        else:
            rgb, st = ctx.render_efficient(pm, pc, *EFF)
            a, e, s = ctx.samples(0)
            for k in range(0, len(a), 7):   # the table under Heun and scaled steps (every entry without them: the test above)
                code, ang, _ = SR.compute_escape_angle(pm, SR.L_CAM, float(a[k]), DELTA, CAP, R, S, integ)
                assert s[k] == float(code) and np.float64(ang).view(np.uint64) == np.float64(e[k]).view(np.uint64), (k, a[k])
            fine_rgb, c5 = SR.compose_efficient_from_table(oc_fine, dirs, fine[0], fine[1], dict(a=a, e=e, s=s))
            cnt = (c5[0], None, c5[1], c5[2], c5[3], c5[4])
            assert (st.rays, st.n_pos, st.n_neg, st.n_none, st.n_oob) == c5
    assert cnt[2] >= 8 and cnt[3] >= 8
    assert_frame(rgb, _g3_frame(fine_rgb, cnt[4]), renderer)


# ---- G4: the step and the solver, device against host -----------------------------------------------------------------------------------
def adversarial_states(mass):
    """(l, theta, p_l, p_theta, p_phi): l at and around 0, deep in the funnel, the photon sphere and the doubles next to it, up to and
    beyond 2^90; sin(theta) tiny; p_phi = 0"""
    l_ps = 2.0 * mass * (1.5 + math.log(0.5))
    ls = [0.0, -0.0, 5e-324, -5e-324, 1e-120, -1e-120, 2.0 ** -100, 2.0 ** -101, -2.0 ** -99, 1e-9, -1e-9, -3.0 * mass, -24.0 * mass, 0.3 * mass,
          2.0 * mass, 8.0 * mass, 24.99 * mass, 2.0 ** 89, 1.9 * 2.0 ** 89, 2.0 ** 90, -2.0 ** 90, 2.0 ** 91, 1e300]
    v = l_ps
    for _ in range(6):
        v = math.nextafter(v, 0.0)
    for _ in range(13):
        ls.append(v)
        v = math.nextafter(v, math.inf)
    out = []
    for l in ls:
        for th in (1.2, SR.HALF_PI, 1e-9, 1e-70, 3.141592653589, -0.4, 7.0):
            for p3 in (0.7 * mass, 0.0, -2.5e-3 * mass):
                for p1 in (-0.9, 0.8):
                    out.append((l, th, p1, 0.3, p3))
    return np.array(out)


@pytest.mark.parametrize("mass", [1.0, 0.37, 2.0 ** -20, 1000.0])
def test_fast_step_on_adversarial_states(gpu_ctx, mass):
    pm = SR.metric(mass)
    states = adversarial_states(mass)
    delta = 0.05 * mass
    # the fast step's contract is |l| < 2^90 (the escape test with max_radius < 2^90, or the Heun stage's own test): with max_radius = 2^89
    # the kernel's guard admits every state below that; the states at and beyond 2^90 are no input of the fast step in any loop, and are
    # compared through the strict step alone
    _, fast, strict, took_fast = gpu_ctx.selftest_fast_step(pm, states, delta=delta, max_radius=2.0 ** 89)
    inside = np.abs(states[:, 0]) < 2.0 ** 90
    assert (took_fast & inside).sum() >= len(states) // 4 and (~took_fast).sum() >= 16

    def same_bits(a, b):
        return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    bad = ~same_bits(fast, strict).all(axis=1) & inside
    print("fast != strict on the device at %d of %d states inside the contract%s" % (bad.sum(), inside.sum(), "".join(
        "\n  state %r took_fast %r\n   fast   %r\n   strict %r" % (states[i].tolist(), bool(took_fast[i]), fast[i].tolist(), strict[i].tolist()) for i in np.argwhere(bad)[:6, 0])))
    assert not bad.any()
    # ... and the host's strict step of the same text: (l, theta, phi - phi0, p_l, p_theta)
    m = pm._c()
    host = np.zeros_like(fast)
    for i, (l, th, p1, p2, p3) in enumerate(states):
        x, p = np.array([0.0, l, th, 0.0]), np.array([1.0, p1, p2, p3])
        assert _abi.lib().curvis_update_relativistic_object(m, SR._dp(x), SR._dp(p), delta) == 0
        host[i] = (x[1], x[2], x[3], p[1], p[2])
    bad = ~same_bits(strict, host).all(axis=1)
    print("device strict != host strict at %d of %d states%s" % (bad.sum(), len(states), "".join(
        "\n  state %r\n   device %r\n   host   %r" % (states[i].tolist(), strict[i].tolist(), host[i].tolist()) for i in np.argwhere(bad)[:6, 0])))
    assert not bad.any()


@pytest.mark.parametrize("mass", [2.0 ** -20, 0.37, 1.0, 1000.0])
def test_solver_sweep_device_equals_host(gpu_ctx, mass):
    """the metric functions over the arguments of the mpmath sweep (tests/test_schwarzschild_host.py), device against host: one step
    from (l, pi/2, p_l = 0, p_theta = 1, p_phi = 0) moves theta by delta / R^2 and p_l by delta R' / R^3 -- R and R' enter alone"""
    import test_schwarzschild_host as H
    pm = SR.metric(mass)
    ls = np.array([float(v) * mass for v in H.sweep_l_over_m()])
    ls = ls[np.abs(ls) < 2.0 ** 90]
    states = np.stack([ls, np.full(ls.size, 1.2), np.zeros(ls.size), np.ones(ls.size), np.zeros(ls.size)], axis=1)
    _, fast, strict, _ = gpu_ctx.selftest_fast_step(pm, states, delta=1.0, max_radius=2.0 ** 89)
    m = pm._c()
    host = np.zeros_like(strict)
    for i, l in enumerate(ls):
        x, p = np.array([0.0, l, 1.2, 0.0]), np.array([1.0, 0.0, 1.0, 0.0])
        assert _abi.lib().curvis_update_relativistic_object(m, SR._dp(x), SR._dp(p), 1.0) == 0
        host[i] = (x[1], x[2], x[3], p[1], p[2])
    assert np.array_equal(strict.view(np.uint64), host.view(np.uint64))
    assert np.array_equal(fast.view(np.uint64), host.view(np.uint64))
    assert len(set(host[:, 3].tolist())) > ls.size // 2   # p_l really carries R' / R^3


# ---- G5: the picture ------------------------------------------------------------------------------------------------------------------
PIC_RES, PIC_R_CAM, PIC_FOCAL, PIC_DIAG = 64, 10.0, 15.0, 43.0


def _picture_masks():
    """pixels surely inside the shadow (their angle from the frame's centre below psi_c minus one pixel) and surely outside (above
    psi_c plus one pixel), for a camera at r = 10 M that looks straight at the hole"""
    psi_c = math.asin(3.0 * math.sqrt(3.0) * math.sqrt(1.0 - 2.0 / PIC_R_CAM) / PIC_R_CAM)
    sensor = PIC_DIAG / math.sqrt(2.0)   # 64 x 64: width = height
    py, px = np.meshgrid(np.arange(PIC_RES), np.arange(PIC_RES), indexing="ij")
    y, z = -sensor * (px / PIC_RES - 0.5), sensor * (0.5 - py / PIC_RES)
    psi = np.arctan2(np.sqrt(y * y + z * z), PIC_FOCAL)
    pixel = sensor / PIC_RES / PIC_FOCAL   # the angle a pixel subtends at the centre of the frame, where it is largest
    return psi < psi_c - pixel, psi > psi_c + pixel


def test_the_picture_python_and_binary(ctx, tmp_path):
    pm = SR.metric(1.0)
    sky = np.zeros((16, 32, 3), np.uint8)
    sky[...] = (200, 180, 90)
    sky[::2, ::2] = (90, 200, 180)          # no black texel on the +l sky
    bg = tmp_path / "sky.png"
    pngio.write_png(bg, sky)
    l_cam = pm.l_of_radius(PIC_R_CAM)
    inside, outside = _picture_masks()
    assert inside.sum() > 300 and outside.sum() > 1500
    # through ImageRenderingSystem: no -l background named
    for mode in ("brute", "efficient"):
        st = rendering.ImageRenderingSettings(str(bg), None, str(tmp_path / ("py_" + mode)), "hole", (0.0, l_cam, SR.HALF_PI, 0.0), (-1.0, 0.0, 0.0),
                                              (0.0, 0.0, 1.0), PIC_FOCAL, PIC_DIAG, PIC_RES, PIC_RES, 30.0, 40000, 0.05)
        system = rendering.ImageRenderingSystem(pm, st, context=ctx, mode=mode)
        img = pngio.read_png(system.render())[..., :3]
        black = (img == 0).all(axis=-1)
        assert black[inside].all() and not black[outside].any(), mode
        stats = system.relativistic_system.last_stats
        assert stats.n_neg == int(black.sum()) and stats.n_none == 0, (mode, stats.n_neg, int(black.sum()))
    # through the binary: a metric file with `mass`, one background
    (tmp_path / "hole.toml").write_text("mass = 1.0\n")
    (tmp_path / "image.toml").write_text('image_name = "hole"\nt = 0.0\nl = %r\ntheta = %r\nphi = 0.0\nforward_x = -1.0\nforward_y = 0.0\nforward_z = 0.0\n'
                                         'up_x = 0.0\nup_y = 0.0\nup_z = 1.0\n' % (l_cam, SR.HALF_PI))
    (tmp_path / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = %r\nfocal_length = %r\n" % (PIC_RES, PIC_RES, PIC_DIAG, PIC_FOCAL))
    (tmp_path / "sim.toml").write_text("escape_radius = 30.0\nray_integration_max_itarations = 40000\nray_integration_step = 0.05\nsampling_initial_nums = 100\n"
                                       "sampling_max_iterations = 50\nsampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 1e-5\n")
    out = tmp_path / "bin"
    out.mkdir()
    r = subprocess.run([BIN, "image", str(bg), str(out), "-m", str(tmp_path / "hole.toml"), "-i", str(tmp_path / "image.toml"), "-c", str(tmp_path / "cam.toml"),
                        "-s", str(tmp_path / "sim.toml"), "--mode", "brute"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = pngio.read_png(out / "hole.png")[..., :3]
    black = (img == 0).all(axis=-1)
    assert black[inside].all() and not black[outside].any()
    assert np.array_equal(img, pngio.read_png(tmp_path / "py_brute" / "hole.png")[..., :3])


# ---- G6: refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    bind(ctx)
    pm, _, pc = SR.scene((24, 16))
    with options(ctx, variant=0):
        with pytest.raises(curvis_amd.CurvisError, match="variant = 0"):
            ctx.render_brute(pm, pc, CAP, R, DELTA)
        with pytest.raises(curvis_amd.CurvisError, match="variant = 0"):
            ctx.render_brute(pm, pc, CAP, R, DELTA, debug=True)
    for l in (0.0, -0.0, -3.0):
        cam = curvis_amd.Camera((0.0, l, SR.HALF_PI, 0.0), (-1.0, 0.2, 0.0), (0.0, 0.0, 1.0), SR.FOCAL, SR.DIAG, 24, 16)
        for call in (lambda: ctx.render_brute(pm, cam, CAP, R, DELTA), lambda: ctx.render_direct(pm, cam, CAP, R, DELTA),
                     lambda: ctx.render_efficient(pm, cam, *EFF), lambda: ctx.render_brute(pm, [pc, cam], CAP, R, DELTA)):
            with pytest.raises(curvis_amd.CurvisError, match="greater than 0") as err:
                call()
            assert err.value.code == _abi.E_INVALID
    # the other kinds keep their cameras at l <= 0
    rgb, st = ctx.render_brute(curvis_amd.EllisMetric(1.0), curvis_amd.Camera((0.0, -3.0, SR.HALF_PI, 0.0), (1.0, 0.2, 0.0), (0.0, 0.0, 1.0), SR.FOCAL, SR.DIAG, 24, 16),
                               CAP, R, DELTA)
    assert st.rays == 24 * 16
    rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)   # and the context still renders the kind
    assert counters(st) == expected("brute", (24, 16))[1]
