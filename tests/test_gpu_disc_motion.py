"""The disc's emission shift on the GPU (include/curvis_hip.h, curvis_ctx_set_disc_motion; the DISC = 2 kernels): every pixel and every
counter against tests/disc_motion_ref.py, which composes the frame per ray from the definition in Python doubles over disc_ref's
Schwarzschild scene (24 x 16, SCHW_*, CAP, R, DELTA).  What a case relies on -- rays with F = 0, saturated channels, g on both sides of
1, camera factors that differ -- is asserted from the reference alone before anything is compared."""
import contextlib
import json
import os
import subprocess

import numpy as np
import pytest

import disc_motion_ref as DM
import disc_ref as D
import projection_ref as P
import step_scale_ref as SR
import curvis_amd
from curvis_amd import _abi, pngio, rendering, skies

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
OPTION_DEFAULTS = dict(projection=0, sky_filter=0, sky_mipmap=0, supersample=1, step_scale=0, integrator=0, fast_math=1, variant=-1, fuse_shade=1)
R, DELTA, CAP = DM.R, DM.DELTA, DM.CAP
NAMES = {1: "prograde", -1: "retrograde", 0: "static"}


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
    gpu_ctx.set_disc(None)      # the motion goes with it: static, gain 1
    for key, value in OPTION_DEFAULTS.items():
        gpu_ctx.set_option(key, value)


def product_disc(d, sigma=0, gain=1.0):
    return curvis_amd.Disc(np.array(d.rgba), d.l_in, d.l_out, motion=NAMES[sigma], gain=gain)


def counters(ctx, st, frame=0):
    return tuple(int(getattr(st, k)) for k in P.COUNTERS) + (ctx.frame_disc_hits(frame),)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def assert_render(ctx, pm, pc, want, what):
    rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
    got = counters(ctx, st)
    print(what, "counters", got, "reference", want[1])
    assert_frame(rgb, want[0], what)
    assert got == want[1], (what, got, want[1])
    assert got[0] == got[2] + got[3] + got[4] + got[6], (what, "rays = n_pos + n_neg + n_none + n_disc")
    assert ctx.get_option("last_relay_launches") == 0, (what, "the static kernel renders a disc")
    return rgb, st


def assert_engaged(want, static, what):
    """a moving disc's reference frame differs from the static disc's in disc pixels only; codes, steps and counters are the static disc's"""
    on = want[2]["code"] == D.DISC
    assert on.sum() >= 8 and (want[0][on] != static[0][on]).any(), what
    assert np.array_equal(want[0][~on], static[0][~on]) and want[1] == static[1], what


# ---- 1. the two motions, both step flavours ----------------------------------------------------------------------------------------------
def test_the_static_reference_is_disc_refs():
    """sigma = 0 through disc_motion_ref's walk is disc_ref's Schwarzschild frame: the walk that hands out l_hit and p_phi is the old walk"""
    mine, theirs = DM.scene_frame(0), D.schwarzschild_frame()
    assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1]
    assert np.array_equal(mine[2]["code"], theirs[2]["code"]) and np.array_equal(mine[2]["steps"], theirs[2]["steps"])


@pytest.mark.parametrize("fast_math", [1, 0])
def test_prograde_and_retrograde(ctx, fast_math):
    static, pro, retro = DM.scene_frame(0), DM.scene_frame(1), DM.scene_frame(-1)
    dsc = DM.scene()[3]
    for sigma, want in ((1, pro), (-1, retro)):
        zero, sat, above, below = DM.conditions(want[2], want[3], 1.0, dsc)
        print(NAMES[sigma], "disc rays with F = 0: %d, saturated: %d, g > 1: %d, g < 1: %d" % (zero, sat, above, below))
        assert above >= 1 and below >= 1, "the approaching side is brighter than its texel, the receding side dimmer"
        assert_engaged(want, static, NAMES[sigma])
    on = pro[2]["code"] == D.DISC
    assert (pro[0][on] != retro[0][on]).any() and np.array_equal(pro[0][~on], retro[0][~on])
    pm, _, pc, _ = DM.scene()
    with options(ctx, fast_math=fast_math):
        for sigma, want in ((1, pro), (-1, retro), (0, static)):
            ctx.set_disc(product_disc(dsc, sigma))
            assert_render(ctx, pm, pc, want, (NAMES[sigma], fast_math))


@pytest.mark.parametrize("gain", [0.25, 4.0])
def test_gain(ctx, gain):
    want, unit = DM.scene_frame(1, gain), DM.scene_frame(1)
    dsc = DM.scene()[3]
    zero, sat, above, below = DM.conditions(want[2], want[3], gain, dsc)
    print("gain", gain, "F = 0: %d, saturated: %d, g > 1: %d, g < 1: %d" % (zero, sat, above, below))
    if gain == 4.0:
        assert sat >= 1, "a channel below 255 that the shift saturates"
    assert (want[0] != unit[0]).any() and want[1] == unit[1]
    pm, _, pc, _ = DM.scene()
    ctx.set_disc(product_disc(dsc, 1, gain))
    assert_render(ctx, pm, pc, want, ("gain", gain))


def test_inner_edge_inside_the_photon_sphere(ctx):
    """l_inner = 0: rays end on the disc at and inside r = 3M, where there is no circular orbit -- painted black, still counted"""
    want, static = DM.scene_frame(-1, l_inner=0.0), DM.scene_frame(0, l_inner=0.0)
    dsc = DM.scene(l_inner=0.0)[3]
    zero, sat, above, below = DM.conditions(want[2], want[3], 1.0, dsc)
    print("l_inner = 0: F = 0: %d, saturated: %d, g > 1: %d, g < 1: %d" % (zero, sat, above, below))
    assert zero >= 1 and above >= 1 and below >= 1
    black = (want[2]["code"] == D.DISC) & (want[3] == 0.0)
    assert (want[0][black] == 0).all() and (static[0][black] != 0).any()
    assert_engaged(want, static, "l_inner = 0")
    assert want[1][6] > DM.scene_frame(0)[1][6], "more rays end on the wider disc"
    pm, _, pc, _ = DM.scene(l_inner=0.0)
    ctx.set_disc(product_disc(dsc, -1))
    assert_render(ctx, pm, pc, want, "l_inner = 0")


# ---- 2. the options ------------------------------------------------------------------------------------------------------------------
def test_scaled_heun_steps(ctx):
    kw = dict(S=4 * 256, integrator=1)
    want, static = DM.scene_frame(1, **kw), DM.scene_frame(0, **kw)
    assert_engaged(want, static, "scaled Heun")
    assert want[1][1] != DM.scene_frame(1)[1][1], "the options change the walk"
    pm, _, pc, dsc = DM.scene()
    ctx.set_disc(product_disc(dsc, 1))
    with options(ctx, step_scale=4 * 256, integrator=1):
        assert_render(ctx, pm, pc, want, "scaled Heun")


def test_supersampled(ctx):
    """supersample = 2: the box average of the reference at 48 x 32; shaded sub-rays on the disc are averaged with sub-rays on the sky"""
    fine, static = DM.scene_frame(1, res=(48, 32)), DM.scene_frame(0, res=(48, 32))
    assert_engaged(fine, static, "fine")
    on_disc = (fine[2]["code"].reshape(16, 2, 24, 2) == D.DISC).sum(axis=(1, 3))
    assert ((on_disc > 0) & (on_disc < 4)).sum() >= 4, "pixels whose sub-rays are partly on the disc"
    pm, _, pc, dsc = DM.scene(res=(48, 32), product_res=D.SCHW_RES)
    ctx.set_disc(product_disc(dsc, 1))
    with options(ctx, supersample=2):
        assert_render(ctx, pm, pc, (SR.box_average(fine[0], 2), fine[1]), "supersample 2")


@pytest.mark.parametrize("mipmap", [0, 1])
def test_filtered(ctx, mipmap):
    """sky_filter = 1 (and sky_mipmap = 1 on top, a separate epilogue): sky rays are filtered, a disc ray takes its own SHADED colour"""
    lookup = "mipmap" if mipmap else "bilinear"
    want, static, nearest = DM.scene_frame(1, lookup=lookup), DM.scene_frame(0, lookup=lookup), DM.scene_frame(1)
    assert_engaged(want, static, lookup)
    on = want[2]["code"] == D.DISC
    assert np.array_equal(want[0][on], nearest[0][on]) and (want[0][~on] != nearest[0][~on]).any()
    pm, _, pc, dsc = DM.scene()
    ctx.set_disc(product_disc(dsc, 1))
    with options(ctx, sky_filter=1, sky_mipmap=mipmap):
        assert_render(ctx, pm, pc, want, lookup)


def test_fisheye(ctx):
    want, static = DM.scene_frame(-1, projection=P.FISHEYE), DM.scene_frame(0, projection=P.FISHEYE)
    assert_engaged(want, static, "fisheye")
    assert (want[0] != DM.scene_frame(-1)[0]).any()
    pm, _, pc, dsc = DM.scene()
    ctx.set_disc(product_disc(dsc, -1))
    with options(ctx, projection=2):
        assert_render(ctx, pm, pc, want, "fisheye")


# ---- 3. bands, batches, back to static ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [(8, 8), (6, 10)])
def test_row_bands(ctx, split):
    want = DM.scene_frame(1)
    pm, _, pc, dsc = DM.scene()
    ctx.set_disc(product_disc(dsc, 1))
    begin, total, parts = 0, np.zeros(7, np.int64), []
    for count in split:
        band, st = ctx.render_brute_rows(pm, pc, begin, count, CAP, R, DELTA)
        got = counters(ctx, st)
        assert got[0] == got[2] + got[3] + got[4] + got[6] == count * 24
        assert got[6] == (want[2]["code"][begin:begin + count] == D.DISC).sum()
        total += got
        parts.append(band)
        begin += count
    assert_frame(np.concatenate(parts), want[0], ("bands", split))
    assert tuple(int(v) for v in total) == want[1]


def test_a_batch_of_three_cameras_at_three_l(ctx):
    """every frame is shaded with its OWN camera's factor: the cameras sit at l = 7.5, 8 and 11 (from l = 6, inside the disc's inner edge
    at l_of_radius(6 M) = 7.39, no ray ends on the disc)"""
    ls = (7.5, 8.0, 11.0)
    wants = [DM.scene_frame(1, l_cam=l) for l in ls]
    mc = DM.scene()[0]._c()
    A = [DM.u_of_l(mc, l) / (1.0 + DM.u_of_l(mc, l)) for l in ls]
    assert len(set(A)) == 3, "camera factors that differ"
    # a frame shaded with another frame's camera would differ: the same rays under the neighbour's factor
    for k, l in enumerate(ls):
        other = DM.factors(wants[k][2], ls[(k + 1) % 3], 1, 1.0)
        on = wants[k][2]["code"] == D.DISC
        assert on.sum() >= 8 and (other[on] != wants[k][3][on]).all()
    scenes = [DM.scene(l_cam=l) for l in ls]
    pm, dsc = scenes[0][0], scenes[0][3]
    ctx.set_disc(product_disc(dsc, 1))
    rgb, st = ctx.render_brute(pm, [s[2] for s in scenes], CAP, R, DELTA)
    assert ctx.frame_disc_hits() == [w[1][6] for w in wants]
    for f in range(3):
        assert_frame(rgb[f], wants[f][0], ("batch frame", f))
        got = tuple(int(getattr(ctx.frame_stats(f), k)) for k in P.COUNTERS) + (ctx.frame_disc_hits(f),)
        assert got == wants[f][1], ("batch frame", f, got, wants[f][1])
    assert tuple(int(getattr(st, k)) for k in P.COUNTERS) == tuple(sum(w[1][k] for w in wants) for k in range(6))
    # and in the other order, in launches of one: the factor travels with the frame
    for f in (2, 0):
        assert_render(ctx, pm, scenes[f][2], wants[f], ("single", ls[f]))


def test_set_motion_render_set_static_render(ctx):
    """the second frame and its counters are those of a context that never had a motion"""
    pm, _, pc, dsc = DM.scene()
    L = _abi.lib()
    ctx.set_disc(product_disc(dsc))
    assert L.curvis_ctx_set_disc_motion(ctx._h, 1, 4.0) == 0
    moving, _ = assert_render(ctx, pm, pc, DM.scene_frame(1, 4.0), "moving")
    # the setting survives curvis_ctx_set_disc ...
    assert L.curvis_ctx_set_disc(ctx._h, np.array(dsc.rgba).ctypes.data, dsc.w, dsc.h, dsc.l_in, dsc.l_out) == 0
    assert_render(ctx, pm, pc, DM.scene_frame(1, 4.0), "after set_disc")
    # ... a refused call leaves it ...
    for motion, gain in ((2, 1.0), (-2, 1.0), (1, -1.0), (1, float("nan")), (1, float("inf"))):
        assert L.curvis_ctx_set_disc_motion(ctx._h, motion, gain) == _abi.E_INVALID
        assert "disc motion" in L.curvis_last_error(ctx._h).decode()
    assert_render(ctx, pm, pc, DM.scene_frame(1, 4.0), "after refused calls")
    # ... and static is static whatever the gain
    assert L.curvis_ctx_set_disc_motion(ctx._h, 0, 4.0) == 0
    after, st_after = assert_render(ctx, pm, pc, DM.scene_frame(0), "static again")
    fresh = curvis_amd.Context(0)
    try:
        for k, img in enumerate(SR.index_skies()):
            fresh.set_sky(k, curvis_amd.SphericalImage(np.array(img)))
        fresh.set_disc(product_disc(dsc))
        never, st_never = fresh.render_brute(pm, pc, CAP, R, DELTA)
        assert_frame(after, never, "after the motion")
        assert counters(ctx, st_after) == counters(fresh, st_never)
    finally:
        fresh.close()
    assert (after != moving).any()
    # without a disc the motion does nothing
    ctx.set_disc(None)
    assert L.curvis_ctx_set_disc_motion(ctx._h, 1, 1.0) == 0
    rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
    assert ctx.frame_disc_hits(0) == 0 and st.n_pos + st.n_neg + st.n_none == st.rays


def test_refused_with_an_ellis_metric(ctx):
    _, _, pm, _, pc, disc = D.scene("A")
    ctx.set_disc(product_disc(disc))
    L = _abi.lib()
    assert L.curvis_ctx_set_disc_motion(ctx._h, 1, 1.0) == 0
    for call in (lambda: ctx.render_brute(pm, pc, CAP, R, DELTA), lambda: ctx.render_brute(pm, [pc, pc], CAP, R, DELTA),
                 lambda: ctx.render_brute_rows(pm, pc, 0, 8, CAP, R, DELTA)):
        with pytest.raises(curvis_amd.CurvisError) as e:
            call()
        assert e.value.code == _abi.E_INVALID and "disc motion" in str(e.value), str(e.value)
    # every existing refusal stays, under its own message
    with options(ctx, fuse_shade=0):
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.render_brute(pm, pc, CAP, R, DELTA)
        assert "fuse_shade" in str(e.value)
    # the context is usable: static again, scene A's frame
    assert L.curvis_ctx_set_disc_motion(ctx._h, 0, 1.0) == 0
    want = D.scene_frame("A")
    rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
    assert_frame(rgb, want[0], "scene A after the refusal")
    assert counters(ctx, st) == want[1]
    with pytest.raises(ValueError, match="motion"):      # Python refuses early, before the context is touched
        curvis_amd.RelativisticSystem(pm, None, None, pc, context=ctx, disc=product_disc(disc, 1))


# ---- 4. the rendering systems and the binary ---------------------------------------------------------------------------------------------
def test_image_rendering_system_with_a_moving_disc(ctx, tmp_path):
    want = DM.scene_frame(1, 4.0)
    pm, _, _, dsc = DM.scene()
    for k, img in enumerate(SR.index_skies()):
        pngio.write_png(tmp_path / ("sky%d.png" % k), np.array(img))
    st = rendering.ImageRenderingSettings(str(tmp_path / "sky0.png"), str(tmp_path / "sky1.png"), str(tmp_path / "out"), "a", D.SCHW_POS, D.SCHW_FWD,
                                          D.SCHW_UP, camera_focal_length=D.SCHW_FOCAL, camera_diagonal=D.DIAG, resolution_x=D.SCHW_RES[0],
                                          resolution_y=D.SCHW_RES[1], escape_radius=R, max_iterations_propagation=CAP, ray_integration_step=DELTA)
    system = rendering.ImageRenderingSystem.new(pm, st, context=ctx, mode="brute", disc=product_disc(dsc, 1, 4.0))
    assert_frame(pngio.read_png(system.render())[..., :3], want[0], "ImageRenderingSystem with a moving disc")
    assert ctx.frame_disc_hits(0) == want[1][6]


def test_the_picture_python_and_binary(ctx, tmp_path):
    pm = curvis_amd.SchwarzschildMetric(1.0)
    res, focal, diag, l_cam, theta = 48, 12.0, 43.0, 10.0, 1.35
    l_in, l_out = pm.l_of_radius(6.0), 16.0
    tex = skies.ring_texture(256, 32)
    sky = skies.checker(256, 128, seed=0xC0FFEE)
    pngio.write_png(tmp_path / "sky.png", sky)
    pngio.write_png(tmp_path / "ring.png", tex)
    cam = curvis_amd.Camera((0.0, l_cam, theta, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), focal, diag, res, res)
    frames = {}
    for motion, gain in (("static", 1.0), ("prograde", 1.0), ("retrograde", 1.0), ("retrograde", 0.5)):
        system = curvis_amd.RelativisticSystem(pm, curvis_amd.SphericalImage(sky), None, cam, context=ctx,
                                               disc=curvis_amd.Disc(tex, l_in, l_out, motion=motion, gain=gain))
        frames[motion, gain] = system.render_image(40000, 30.0, 0.05)
        n_disc = ctx.frame_disc_hits(0)
    assert n_disc > 50 and (frames["prograde", 1.0] != frames["static", 1.0]).any() and (frames["retrograde", 1.0] != frames["retrograde", 0.5]).any()
    # the side that approaches under one motion recedes under the other: prograde minus retrograde is positive in one half of the
    # frame and negative in the other.  The camera's vectors are (l, theta, phi) components: forward is -l and up is +phi, so phi runs
    # along the image's vertical axis and the halves are the upper and the lower one
    lum = frames["prograde", 1.0].astype(np.int64).sum(axis=2) - frames["retrograde", 1.0].astype(np.int64).sum(axis=2)
    assert lum[:res // 2].sum() * lum[res // 2:].sum() < 0, "one half brighter, the other dimmer"
    (tmp_path / "hole.toml").write_text("mass = 1.0\n")
    (tmp_path / "image.toml").write_text('image_name = "disc"\nt = 0.0\nl = %r\ntheta = %r\nphi = 0.0\nforward_x = -1.0\nforward_y = 0.0\nforward_z = 0.0\n'
                                         'up_x = 0.0\nup_y = 0.0\nup_z = 1.0\n' % (l_cam, theta))
    (tmp_path / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = %r\nfocal_length = %r\n" % (res, res, diag, focal))
    (tmp_path / "sim.toml").write_text("escape_radius = 30.0\nray_integration_max_itarations = 40000\nray_integration_step = 0.05\nsampling_initial_nums = 100\n"
                                       "sampling_max_iterations = 50\nsampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 1e-5\n")
    out = tmp_path / "out"
    out.mkdir()
    common_args = [BIN, "image", str(tmp_path / "sky.png"), str(out), "-m", str(tmp_path / "hole.toml"), "-i", str(tmp_path / "image.toml"),
                   "-c", str(tmp_path / "cam.toml"), "-s", str(tmp_path / "sim.toml"), "--disc", str(tmp_path / "ring.png"),
                   "--disc-inner", repr(l_in), "--disc-outer", repr(l_out), "--stats", str(tmp_path / "stats.jsonl"), "--mode", "brute"]
    for flags, motion in ((["--disc-motion", "prograde"], ("prograde", 1.0)), (["--disc-motion", "retrograde", "--disc-gain", "0.5"], ("retrograde", 0.5)),
                          (["--disc-motion", "static", "--disc-gain", "3"], ("static", 1.0))):
        r = subprocess.run(common_args + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert_frame(pngio.read_png(out / "disc.png")[..., :3], frames[motion], ("the binary's PNG", flags))
        line = json.loads((tmp_path / "stats.jsonl").read_text().splitlines()[0])
        assert line["n_disc"] == n_disc
