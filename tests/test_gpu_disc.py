"""The accretion disc on the GPU, exact against tests/disc_ref.py: every pixel, rays, steps, n_pos, n_neg, n_none, n_oob and n_disc, no
tolerance anywhere.  The disc's texture is an index texture with gaps (disc_ref.disc_texture) and the skies are step_scale_ref's index
skies, so a pixel comparison is a texel comparison and a which-surface comparison.  Each case first asserts, from the reference alone,
the ray classes it relies on (tests/test_disc_host.py does the same without a GPU): at least 8 disc rays, 8 +l rays and 4 rays that
passed a gap and went on, and, where the case is about theta outside [0, pi] (scenes C, D, F), at least 3 crossings inside [l_in, l_out]
with s_k < 0, where the azimuth is shifted by pi.  Scenes D and F have 3 and 6 of them, D at 42 x 26 has 5; scene C has 11 plane crossings
with s_k < 0 and one of them inside its range, and asserts that one (disc_ref.SNEG_IN_RANGE_MIN)."""
import contextlib
import json
import os
import subprocess

import numpy as np
import pytest

import common
import disc_ref as D
import oracle_lib as O
import projection_ref as P
import step_scale_ref as SR
import curvis_amd
from curvis_amd import _abi, pngio, rendering, skies

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
OPTION_DEFAULTS = dict(projection=0, sky_filter=0, sky_mipmap=0, supersample=1, step_scale=0, integrator=0, fast_math=1, variant=-1, fuse_shade=1)
R, DELTA, CAP = D.R, D.DELTA, D.CAP


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


def assert_render(ctx, pm, pc, want, what, cap=CAP, delta=DELTA):
    want_rgb, want_cnt = want[0], want[1]
    rgb, st = ctx.render_brute(pm, pc, cap, R, delta)
    got = counters(ctx, st)
    print(what, "counters", got, "reference", want_cnt)
    assert_frame(rgb, want_rgb, what)
    assert got == want_cnt, (what, got, want_cnt)
    assert got == tuple(int(getattr(ctx.frame_stats(0), k)) for k in P.COUNTERS) + (got[6],), what
    assert got[0] == got[2] + got[3] + got[4] + got[6], (what, "rays = n_pos + n_neg + n_none + n_disc")
    assert ctx.get_option("last_relay_launches") == 0, (what, "the static kernel renders a disc")
    return rgb, st


# ---- 1. the five scenes, both step flavours against one reference ---------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("name", sorted(D.SCENES))
def test_scenes(ctx, name, fast_math):
    want = D.scene_frame(name)
    D.assert_classes(want[2], name, sneg_in_range=D.SNEG_IN_RANGE_MIN.get(name, 0))
    _, _, pm, _, pc, disc = D.scene(name)
    ctx.set_disc(product_disc(disc))
    for variant in ((-1, 1, 2) if fast_math else (-1,)):   # whatever the variant asks for, the static kernel renders
        with options(ctx, fast_math=fast_math, variant=variant, relay_min_blocks=0):
            assert_render(ctx, pm, pc, want, (name, fast_math, variant))
    # the disc engages: another frame and other counters than the same call without it
    ctx.set_disc(None)
    rgb0, st0 = ctx.render_brute(pm, pc, CAP, R, DELTA)
    assert (rgb0 != want[0]).any() and st0.steps != want[1][1] and ctx.frame_disc_hits(0) == 0


# ---- 2. the options ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(step_scale=4 * 256), dict(integrator=1), dict(step_scale=4 * 256, integrator=1)], ids=["scaled", "heun", "scaled-heun"])
def test_scene_a_under_the_step_options(ctx, opts):
    want = D.scene_frame("A", S=opts.get("step_scale", 0), integrator=opts.get("integrator", 0))
    D.assert_classes(want[2], ("A", opts))
    plain = D.scene_frame("A")
    assert want[1][1] != plain[1][1], "the option changes the walk"
    _, _, pm, _, pc, disc = D.scene("A")
    ctx.set_disc(product_disc(disc))
    with options(ctx, **opts):
        assert_render(ctx, pm, pc, want, ("A", opts))


def test_scene_d_supersampled(ctx):
    """supersample = 2: the box average of the reference at 42 x 26; sub-rays on the disc are averaged with sub-rays on the sky"""
    fine = D.scene_frame("D", res=(42, 26))
    D.assert_classes(fine[2], "D fine", sneg_in_range=D.SNEG_IN_RANGE_MIN["D"])
    code = fine[2]["code"].reshape(13, 2, 21, 2)
    on_disc = (code == D.DISC).sum(axis=(1, 3))
    assert ((on_disc > 0) & (on_disc < 4)).sum() >= 4, "pixels whose sub-rays are partly on the disc"
    _, _, pm, _, pc, disc = D.scene("D")
    ctx.set_disc(product_disc(disc))
    with options(ctx, supersample=2):
        assert_render(ctx, pm, pc, (SR.box_average(fine[0], 2), fine[1]), "D supersample 2")


def test_scene_a_fisheye(ctx):
    want = D.scene_frame("A", projection=P.FISHEYE)
    D.assert_classes(want[2], "A fisheye")
    assert (want[0] != D.scene_frame("A")[0]).any()
    _, _, pm, _, pc, disc = D.scene("A")
    ctx.set_disc(product_disc(disc))
    with options(ctx, projection=2):
        assert_render(ctx, pm, pc, want, "A fisheye")


@pytest.mark.parametrize("mipmap", [0, 1])
def test_scene_a_filtered(ctx, mipmap):
    """sky_filter = 1 (and sky_mipmap = 1 on top): sky rays are filtered as sky_filter_ref / sky_mipmap_ref define it, a disc ray keeps
    its own texel and is a quad partner that saw no sky"""
    want = D.scene_frame("A", "mipmap" if mipmap else "bilinear")
    D.assert_classes(want[2], ("A filtered", mipmap))
    nearest = D.scene_frame("A")
    on_disc = want[2]["code"] == D.DISC
    assert np.array_equal(want[0][on_disc], nearest[0][on_disc]) and (want[0][~on_disc] != nearest[0][~on_disc]).any()
    if mipmap:
        assert (want[0] != D.scene_frame("A", "bilinear")[0]).any(), "the pyramid engages"
        # sky rays with a disc ray for a quad partner
        c = want[2]["code"]
        sky = (c == O.POSITIVE) | (c == O.NEGATIVE)
        h = sky & np.roll(c == D.DISC, 1, axis=1)
        assert h[:, 1::2].sum() + (sky & np.roll(c == D.DISC, -1, axis=1))[:, 0::2].sum() >= 4
    _, _, pm, _, pc, disc = D.scene("A")
    ctx.set_disc(product_disc(disc))
    with options(ctx, sky_filter=1, sky_mipmap=mipmap):
        assert_render(ctx, pm, pc, want, ("A filtered", mipmap))


def test_all_options_at_once(ctx):
    """scaled Heun steps, supersample 2, fisheye, bilinear filter on the mip pyramid: the reference at 48 x 32, quads of the fine grid"""
    kw = dict(S=4 * 256, integrator=1, projection=P.FISHEYE, res=(48, 32))
    fine = D.scene_frame("A", "mipmap", **kw)
    D.assert_classes(fine[2], "A everything")
    _, _, pm, _, pc, disc = D.scene("A")
    ctx.set_disc(product_disc(disc))
    with options(ctx, step_scale=4 * 256, integrator=1, projection=2, sky_filter=1, sky_mipmap=1, supersample=2):
        assert_render(ctx, pm, pc, (SR.box_average(fine[0], 2), fine[1]), "A everything")


# ---- 3. Schwarzschild: the disc bent over and under the hole ---------------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
def test_schwarzschild(ctx, fast_math):
    want_rgb, want_cnt, rays = D.schwarzschild_frame()
    D.assert_classes(rays, "schwarzschild")
    code = rays["code"]
    shadow_rows = np.nonzero((code == O.NEGATIVE).any(axis=1))[0]
    assert len(shadow_rows) >= 3, "the hole's shadow"
    centre = 0.5 * (shadow_rows.min() + shadow_rows.max())
    rows = np.nonzero(code == D.DISC)[0]
    print("schwarzschild: shadow rows %d..%d, disc rays above %d, below %d" % (shadow_rows.min(), shadow_rows.max(), (rows < centre).sum(), (rows > centre).sum()))
    assert (rows < centre).sum() >= 4 and (rows > centre).sum() >= 4, "the far side of the disc over the hole, and under it"
    pm, _, pc, disc = D.schwarzschild_scene()
    ctx.set_disc(product_disc(disc))
    with options(ctx, fast_math=fast_math):
        assert_render(ctx, pm, pc, (want_rgb, want_cnt), ("schwarzschild", fast_math))


# ---- 4. bands, batches, removal --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [(8, 8), (6, 10)])
def test_scene_a_as_row_bands(ctx, split):
    want = D.scene_frame("A")
    _, _, pm, _, pc, disc = D.scene("A")
    ctx.set_disc(product_disc(disc))
    begin, total, parts = 0, np.zeros(7, np.int64), []
    for count in split:
        band, st = ctx.render_brute_rows(pm, pc, begin, count, CAP, R, DELTA)
        got = counters(ctx, st)
        assert got[0] == got[2] + got[3] + got[4] + got[6] == count * 24
        code = want[2]["code"][begin:begin + count]
        assert got[6] == (code == D.DISC).sum() and got[1] == want[2]["steps"][begin:begin + count].sum()
        total += got
        parts.append(band)
        begin += count
    assert_frame(np.concatenate(parts), want[0], ("bands", split))
    assert tuple(int(v) for v in total) == want[1]


def test_scene_a_as_a_batch_of_three(ctx):
    phis = (0.0, 0.7, -2.1)
    wants = [D.scene_frame("A", phi=p) for p in phis]
    assert (wants[0][0] != wants[1][0]).any() and (wants[1][0] != wants[2][0]).any()
    scenes = [D.scene("A", phi=p) for p in phis]
    pm, disc = scenes[0][2], scenes[0][5]
    ctx.set_disc(product_disc(disc))
    singles = []
    for s, w in zip(scenes, wants):
        rgb, st = assert_render(ctx, pm, s[4], w, ("single", s[4]))
        singles.append((rgb, counters(ctx, st)))
    rgb, st = ctx.render_brute(pm, [s[4] for s in scenes], CAP, R, DELTA)
    assert ctx.frame_disc_hits() == [w[1][6] for w in wants]
    for f in range(3):
        assert_frame(rgb[f], singles[f][0], ("batch frame", f))
        got = tuple(int(getattr(ctx.frame_stats(f), k)) for k in P.COUNTERS) + (ctx.frame_disc_hits(f),)
        assert got == singles[f][1] == wants[f][1], ("batch frame", f)
        assert got[0] == got[2] + got[3] + got[4] + got[6]
    assert tuple(int(getattr(st, k)) for k in P.COUNTERS) == tuple(sum(w[1][k] for w in wants) for k in range(6))


def test_set_render_remove_render(ctx):
    """the second frame and its counters are those of a context that never had a disc"""
    _, _, pm, _, pc, disc = D.scene("A")
    ctx.set_disc(product_disc(disc))
    with_disc, _ = ctx.render_brute(pm, pc, CAP, R, DELTA)
    assert ctx.frame_disc_hits(0) == D.SCENE_COUNTS["A"][0]
    ctx.set_disc(None)
    after, st_after = ctx.render_brute(pm, pc, CAP, R, DELTA)
    after_cnt = counters(ctx, st_after)
    fresh = curvis_amd.Context(0)
    try:
        for k, img in enumerate(SR.index_skies()):
            fresh.set_sky(k, curvis_amd.SphericalImage(np.array(img)))
        never, st_never = fresh.render_brute(pm, pc, CAP, R, DELTA)
        assert_frame(after, never, "after removal")
        assert after_cnt == counters(fresh, st_never) and after_cnt[6] == 0
    finally:
        fresh.close()
    assert (after != with_disc).any()
    no_disc = D.scene_frame("A", disc=False)
    assert_frame(after, no_disc[0], "no disc: the reference without one")
    assert after_cnt == no_disc[1]


# ---- 5. refusals, each leaving the context usable ---------------------------------------------------------------------------------------
def test_refusals(ctx):
    want = D.scene_frame("A")
    _, _, pm, _, pc, disc = D.scene("A")
    L, h = _abi.lib(), ctx._h
    tex = np.array(disc.rgba)
    bad = [(tex.ctypes.data, 0, 53, 1.5, 5.0), (tex.ctypes.data, 97, 0, 1.5, 5.0), (tex.ctypes.data, 97, 53, float("nan"), 5.0),
           (tex.ctypes.data, 97, 53, 1.5, float("inf")), (tex.ctypes.data, 97, 53, 5.0, 5.0), (tex.ctypes.data, 97, 53, 5.0, 1.5)]
    ctx.set_disc(product_disc(disc))
    for args in bad:      # a refused call leaves the disc that was set
        assert L.curvis_ctx_set_disc(h, *args) == _abi.E_INVALID, args
        assert "disc" in L.curvis_last_error(h).decode()
    assert_render(ctx, pm, pc, want, "after refused set_disc calls")
    eff = (CAP, R, DELTA, 50, 50, 1e-5, 1e-5)
    calls = [("efficient", lambda: ctx.render_efficient(pm, pc, *eff)), ("efficient batch", lambda: ctx.render_efficient(pm, [pc, pc], *eff)),
             ("prefetch", lambda: ctx.prefetch_efficient(pm, [pc], *eff)), ("direct", lambda: ctx.render_direct(pm, pc, CAP, R, DELTA)),
             ("debug", lambda: ctx.render_brute(pm, pc, CAP, R, DELTA, debug=True))]
    for what, call in calls:
        with pytest.raises(curvis_amd.CurvisError) as e:
            call()
        assert e.value.code == _abi.E_INVALID and "disc" in str(e.value), (what, str(e.value))
        assert_render(ctx, pm, pc, want, ("after the refusal of", what))
    for key, value in (("variant", 0), ("fuse_shade", 0)):
        with options(ctx, **{key: value}):
            with pytest.raises(curvis_amd.CurvisError) as e:
                ctx.render_brute(pm, pc, CAP, R, DELTA)
            assert e.value.code == _abi.E_INVALID and "disc" in str(e.value) and key in str(e.value)
        assert_render(ctx, pm, pc, want, ("after the refusal of", key))
    # the Python systems: a shared context does not leak one system's disc into another's frame
    sp, sn = (curvis_amd.SphericalImage(np.array(t)) for t in SR.index_skies())
    with_disc = curvis_amd.RelativisticSystem(pm, sp, sn, pc, context=ctx, disc=product_disc(disc))
    without = curvis_amd.RelativisticSystem(pm, sp, sn, pc, context=ctx)
    assert_frame(with_disc.render_image(CAP, R, DELTA), want[0], "RelativisticSystem with a disc")
    assert_frame(without.render_image(CAP, R, DELTA), D.scene_frame("A", disc=False)[0], "RelativisticSystem without, same context")
    with pytest.raises(ValueError):
        with_disc.render_image_direct(CAP, R, DELTA)
    without.render_image_direct(CAP, R, DELTA)        # unbinds: served


# ---- 6. the rendering systems ------------------------------------------------------------------------------------------------------------
class Poses:
    """stands where an Interpolator would: scene A's camera at one azimuth per second"""

    def __init__(self, phis):
        self.phis = phis

    def min_time(self):
        return 0.0

    def max_time(self):
        return len(self.phis) - 0.5

    def camera_position(self, t):
        return D.SCENES["A"][1][:3] + (self.phis[int(t)],)

    def camera_forward(self, t):
        return D.SCENES["A"][2]

    def camera_up(self, t):
        return D.SCENES["A"][3]


def video_system(ctx, pm, phis, disc):
    focal, res = D.SCENES["A"][4], D.SCENES["A"][5]
    return rendering.VideoRenderingSystem(pm, ctx, Poses(phis), 1.0, res, D.DIAG, focal, R, CAP, DELTA, batch=2, mode="brute", disc=disc)


def test_video_rendering_system_counts_n_disc_per_frame(ctx):
    """three frames in launches of two and one: every frame and its statistics are those of a single render, n_disc is read at the
    frame's place within its launch; a system without a disc on the same context then renders without one"""
    phis = (0.0, 0.7, -2.1)
    wants = [D.scene_frame("A", phi=p) for p in phis]
    assert len({w[1][6] for w in wants}) == 3, "three different n_disc: a frame that read another's would show"
    _, _, pm, _, _, disc = D.scene("A")
    frames = {}
    stats = video_system(ctx, pm, phis, product_disc(disc)).render(on_frame=lambda k, rgb, d: frames.__setitem__(k, np.array(rgb)))
    assert [d["frame"] for d in stats] == [0, 1, 2] and [d["batch_frames"] for d in stats] == [2, 2, 1]
    for f, (d, w) in enumerate(zip(stats, wants)):
        assert_frame(frames[f], w[0], ("video frame", f))
        got = tuple(d[k] for k in P.COUNTERS) + (d["n_disc"],)
        assert got == w[1], ("video frame", f, got, w[1])
        assert d["rays"] == d["n_pos"] + d["n_neg"] + d["n_none"] + d["n_disc"]
    no_disc = D.scene_frame("A", disc=False)
    stats = video_system(ctx, pm, phis[:1], None).render(on_frame=lambda k, rgb, d: frames.__setitem__(k, np.array(rgb)))
    assert_frame(frames[0], no_disc[0], "video frame without a disc, same context")
    assert "n_disc" not in stats[0] and tuple(stats[0][k] for k in P.COUNTERS) == no_disc[1][:6]


def test_image_rendering_system_with_a_disc(ctx, tmp_path):
    want = D.scene_frame("A")
    _, pos, fwd, up, focal, res, _ = D.SCENES["A"]
    _, _, pm, _, _, disc = D.scene("A")
    for k, img in enumerate(SR.index_skies()):
        pngio.write_png(tmp_path / ("sky%d.png" % k), np.array(img))
    st = rendering.ImageRenderingSettings(str(tmp_path / "sky0.png"), str(tmp_path / "sky1.png"), str(tmp_path / "out"), "a", pos, fwd, up,
                                                     camera_focal_length=focal, camera_diagonal=D.DIAG, resolution_x=res[0], resolution_y=res[1],
                                                     escape_radius=R, max_iterations_propagation=CAP, ray_integration_step=DELTA)
    system = rendering.ImageRenderingSystem.new(pm, st, context=ctx, mode="brute", disc=product_disc(disc))
    assert_frame(pngio.read_png(system.render())[..., :3], want[0], "ImageRenderingSystem with a disc")
    assert ctx.frame_disc_hits(0) == want[1][6]


# ---- 7. the picture: Python and the binary ------------------------------------------------------------------------------------------------
def test_the_picture_python_and_binary(ctx, tmp_path):
    pm = curvis_amd.SchwarzschildMetric(1.0)
    res, focal, diag, l_cam, theta = 48, 12.0, 43.0, 10.0, 1.35
    l_in, l_out = pm.l_of_radius(6.0), 16.0
    tex = skies.ring_texture(256, 32)
    sky = skies.checker(256, 128, seed=0xC0FFEE)
    pngio.write_png(tmp_path / "sky.png", sky)
    pngio.write_png(tmp_path / "ring.png", tex)
    cam = curvis_amd.Camera((0.0, l_cam, theta, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), focal, diag, res, res)
    system = curvis_amd.RelativisticSystem(pm, curvis_amd.SphericalImage(sky), None, cam, context=ctx, disc=curvis_amd.Disc(tex, l_in, l_out))
    py = system.render_image(40000, 30.0, 0.05)
    n_disc = ctx.frame_disc_hits(0)
    assert n_disc > 50
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
                   "--disc-inner", repr(l_in), "--disc-outer", repr(l_out), "--stats", str(tmp_path / "stats.jsonl")]
    r = subprocess.run(common_args + ["--mode", "brute"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert_frame(pngio.read_png(out / "disc.png")[..., :3], py, "the binary's PNG")
    line = json.loads((tmp_path / "stats.jsonl").read_text().splitlines()[0])
    assert line["n_disc"] == n_disc > 0 and line["rays"] == line["n_pos"] + line["n_neg"] + line["n_none"] + line["n_disc"]
    # --devices 3: every context gets the disc, three row bands make the one frame and n_disc is the sum of theirs
    r = subprocess.run(common_args + ["--mode", "brute", "--devices", "3"], capture_output=True, text=True, timeout=120, env=common.share_env(3))
    assert r.returncode == 0, r.stderr
    assert_frame(pngio.read_png(out / "disc.png")[..., :3], py, "the binary's PNG from three row bands")
    bands = json.loads((tmp_path / "stats.jsonl").read_text().splitlines()[0])
    assert all(bands[k] == line[k] for k in ("rays", "steps", "n_pos", "n_neg", "n_none", "n_oob", "n_disc")), (bands, line)
    r = subprocess.run(common_args, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--disc needs --mode brute" in r.stderr
    # without a disc the line has no such field
    r = subprocess.run(common_args[:12] + common_args[18:] + ["--mode", "brute"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "n_disc" not in (tmp_path / "stats.jsonl").read_text(), r.stderr


def test_binary_video_with_a_disc(ctx, tmp_path):
    """curvis video --mode brute --batch 2 --disc: three frames, each frame and its n_disc those of the library's batch"""
    d = tmp_path
    _, _, fwd, up, focal, res, (l_in, l_out) = D.SCENES["A"]
    for k, img in enumerate(SR.index_skies()):
        pngio.write_png(d / ("sky%d.png" % k), np.array(img))
    pngio.write_png(d / "disc.png", np.array(D.disc_texture()))
    rows = ["t,l,theta,phi,fx,fy,fz,upx,upy,upz"] + ["%r,6.0,1.25,%r,%r,%r,%r,%r,%r,%r" % ((float(t), 0.7 * t) + fwd + up) for t in range(4)]
    (d / "path.csv").write_text("\n".join(rows) + "\n")
    (d / "vid.toml").write_text('video_name = "v"\nframe_rate = 1.0\nfilepath_to_camera_path = "%s"\n' % (d / "path.csv"))
    (d / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = %r\nfocal_length = %r\n" % (res + (D.DIAG, focal)))
    (d / "sim.toml").write_text("escape_radius = %r\nray_integration_max_itarations = %d\nray_integration_step = %r\nsampling_initial_nums = 100\n"
                                "sampling_max_iterations = 50\nsampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 1e-5\n" % (R, CAP, DELTA))
    out = d / "out"
    out.mkdir()
    r = subprocess.run([BIN, "video", str(d / "sky0.png"), str(d / "sky1.png"), str(out), "-v", str(d / "vid.toml"), "-s", str(d / "sim.toml"),
                        "-c", str(d / "cam.toml"), "--mode", "brute", "--batch", "2", "--disc", str(d / "disc.png"), "--disc-inner", repr(l_in),
                        "--disc-outer", repr(l_out), "--stats", str(d / "st.jsonl")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    it = rendering.Interpolator.from_file(str(d / "path.csv"))
    times = rendering.times_of_frames(it.min_time(), it.max_time(), 1.0)
    assert len(times) == 3
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), focal, D.DIAG, res[0], res[1]) for t in times]
    ctx.set_disc(product_disc(D.scene("A")[5]))
    rgb, _ = ctx.render_brute(curvis_amd.EllisMetric(1.0), cams, CAP, R, DELTA)
    hits = ctx.frame_disc_hits()
    assert min(hits) >= 8 and len(set(hits)) == 3, hits
    lines = sorted((json.loads(l) for l in (d / "st.jsonl").read_text().splitlines()), key=lambda l: l["frame"])
    assert [l["frame"] for l in lines] == [0, 1, 2]
    for k, l in enumerate(lines):
        assert_frame(pngio.read_png(out / "tmp" / ("frame_%d.png" % k))[..., :3], rgb[k], ("curvis video --disc, frame", k))
        assert l["n_disc"] == hits[k] and l["rays"] == l["n_pos"] + l["n_neg"] + l["n_none"] + l["n_disc"], (k, l, hits)
