"""Bilinear sky filtering (library option "sky_filter" = 1) against its definition, through every renderer.

The definition (include/curvis_hip.h, restated in numpy integers in tests/sky_filter_ref.py) is in terms of what the nearest lookup
returns on a sky of 256 w x 256 h texels.  So the oracle (O.CV) renders the scene over INDEX skies of that size, every pixel of its
frame is decoded to (which sky, Xc, Yc), steps 3-5 of the definition are applied to the real w x h sky in numpy, and the GPU's
filtered frame must equal the result in every pixel.  Nothing new is needed from the oracle.

Scene: common.scene(kind, res=(24, 16)), camera at l = 5 (and at l = -3, from where every ray ends on the -l sky), max_radius 10,
delta 0.05, cap 340 for the brute and direct renderers; skies of 13 x 7 (+l) and 16 x 5 (-l) texels with hashed colours, in two
orientations A and B that put the seam and opposite poles into the frame (B also an out-of-bounds ray on the pole axis).  Every
oracle-based test first asserts, from the decoded indices, that the classes it relies on are there: wraps on the left and on the
right of the seam, a clamp at the top and one at the bottom over A and B, a seam-and-pole corner, interior rays with both weights
non-zero, and the out-of-bounds ray in B."""
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
import curvis_amd
from curvis_amd import _abi, pngio, rendering

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")

KINDS = ("ellis", "interstellar")
ORIENTS = ("A", "B")
RES, R, DELTA, CAP = F.RES, F.R, F.DELTA, F.CAP
EFF = dict(cap=4096, n0=100, maxit=100, t1=1e-5, t2=1e-5)   # the supersample test's settings for the efficient renderer
COUNTERS = ("rays", "steps", "n_pos", "n_neg", "n_none", "n_oob")
BATCH_LS = (5.0, 4.0, -3.0)
MESSAGE = "sky_filter must be 0 (nearest) or 1 (bilinear)"


def counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS)


def efficient_args():
    return (EFF["cap"], R, DELTA, EFF["n0"], EFF["maxit"], EFF["t1"], EFF["t2"])


@functools.lru_cache(maxsize=None)
def oracle_fine(renderer, kind, orient, l=5.0, n=1):
    """the oracle's frame over the fine index skies at n times the resolution: (frame, counters, steps of the sampler or None);
    read-only, shared by the tests"""
    om, oc, _, _ = F.scene(kind, (RES[0] * n, RES[1] * n), l)
    sp, sn = F.oracle_fine_skies(orient)
    steps = None
    if renderer == "brute":
        rgb, _, st = O.render_image(O.CV, om, oc, sp, sn, CAP, R, DELTA)
    elif renderer == "direct":
        rgb, st = O.render_image_direct(O.CV, om, oc, sp, sn, CAP, R, DELTA)
    else:
        rgb, smp, st = O.render_image_efficient(O.CV, om, oc, sp, sn, *efficient_args())
        steps = smp["steps"]
    rgb.setflags(write=False)
    return rgb, counters(st), steps


@functools.lru_cache(maxsize=None)
def expected(renderer, kind, orient, l=5.0, n=1):
    """(the filtered frame by the definition, the oracle's counters, sampler steps, classes of the +l sky's rays, of the -l sky's)"""
    fine, st, steps = oracle_fine(renderer, kind, orient, l, n)
    want, which, Xc, Yc = F.filtered_frame(fine)
    assert int((which < 0).sum()) == st[4], (renderer, kind, orient, l, st)   # black pixels are the capped rays, nothing else
    if n > 1:
        want = F.box_average(want, n)
    want.setflags(write=False)
    return want, st, steps, F.classes(which, Xc, Yc, 0), F.classes(which, Xc, Yc, 1)


def assert_classes_present(renderer, kind, n=1):
    """over the frames a test compares -- orientations A and B, camera at l = 5 and at l = -3 -- every class the comparison relies on"""
    F.assert_salts()
    total = dict(left=0, right=0, top=0, bottom=0, corner=0, interior=0)
    for orient in ORIENTS:
        _, st, _, pos, neg = expected(renderer, kind, orient, 5.0, n)
        # the +l sky at l = 5: the seam (at least one side per frame), a pole, and a few hundred interior rays with many different weights
        assert pos["left"] + pos["right"] >= 1 and pos["top"] + pos["bottom"] >= 1, (renderer, kind, orient, pos)
        assert pos["interior"] >= 250 * n * n and pos["fx_values"] >= 100 and pos["fy_values"] >= 50, (renderer, kind, orient, pos)
        if n == 1:
            assert st[5] == (1 if orient == "B" else 0), ("the out-of-bounds ray on the pole axis of orientation B", renderer, kind, st)
        _, st3, _, pos3, neg3 = expected(renderer, kind, orient, -3.0, n)
        assert pos3["n"] == 0 and neg3["n"] == n * n * RES[0] * RES[1], (renderer, kind, orient, st3)
        assert neg3["left"] >= 1 and neg3["right"] >= 1 and neg3["top"] + neg3["bottom"] >= 1, (renderer, kind, orient, neg3)
        for cl in (pos, neg, pos3, neg3):
            for k in total:
                total[k] += cl[k]
    assert all(v >= 1 for v in total.values()), (renderer, kind, total)
    top = [expected(renderer, kind, o, 5.0, n)[3]["top"] > expected(renderer, kind, o, 5.0, n)[3]["bottom"] for o in ORIENTS]
    assert top[0] != top[1], ("A and B clamp mostly at opposite poles", renderer, kind, top)


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
    assert gpu_ctx.get_option("sky_filter") == 0 and gpu_ctx.get_option("supersample") == 1
    yield gpu_ctx
    gpu_ctx.set_option("sky_filter", 0)
    gpu_ctx.set_option("supersample", 1)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


# ---- 1. brute renderer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_brute_vs_definition(ctx, kind, fast_math):
    assert_classes_present("brute", kind)
    pm = F.scene(kind)[2]
    cams = [F.scene(kind, l=l)[3] for l in BATCH_LS]
    for orient in ORIENTS:
        bind(ctx, orient)
        want = [expected("brute", kind, orient, l) for l in BATCH_LS]
        for name, opts in (("static", dict(variant=1)), ("relay", dict(variant=2, relay_min_blocks=0))):
            with options(ctx, sky_filter=1, fast_math=fast_math, **opts):
                what = (name, kind, orient, fast_math)
                for cam, w in ((cams[0], want[0]), (cams[2], want[2])):    # l = 5, and l = -3: every ray on the -l sky
                    rgb, st = ctx.render_brute(pm, cam, CAP, R, DELTA)
                    assert (ctx.get_option("last_relay_launches") >= 1) == (name == "relay"), what
                    assert_frame(rgb, w[0], what)
                    assert counters(st) == w[1] == counters(ctx.frame_stats(0)), what
                assert ctx.get_option("relay_mismatches") == 0 and ctx.get_option("relay_disabled") == 0
                # rows in two bands
                total = np.zeros(6, np.uint64)
                for begin, count in ((0, 7), (7, 9)):
                    band, st = ctx.render_brute_rows(pm, cams[0], begin, count, CAP, R, DELTA)
                    assert_frame(band, want[0][0][begin:begin + count], what + ("rows", begin, count))
                    total += np.array(counters(st), np.uint64)
                assert tuple(int(v) for v in total) == want[0][1], what
                # a batch of three frames with different l
                rgb, st = ctx.render_brute(pm, cams, CAP, R, DELTA)
                for f in range(3):
                    assert_frame(rgb[f], want[f][0], what + ("batch frame", f))
                    assert counters(ctx.frame_stats(f)) == want[f][1], what + ("batch frame", f)
                assert counters(st) == tuple(sum(w[1][k] for w in want) for k in range(6)), what


# ---- 2. efficient renderer: both samplers; counters and sample tables are the nearest render's ----------------------------------
def sampler_record(ctx, n_frames):
    out = []
    for f in range(n_frames):
        si = ctx.sampling_info(f)
        out.append(((si.n_samples, si.rounds, si.calls, si.steps, si.warned_max_iterations),
                    tuple(common.bits(a).tobytes() for a in ctx.samples(f)), counters(ctx.frame_stats(f))))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_efficient_vs_definition(ctx, kind):
    assert_classes_present("efficient", kind)
    pm = F.scene(kind)[2]
    cams = [F.scene(kind, l=l)[3] for l in BATCH_LS]
    for orient in ORIENTS:
        bind(ctx, orient)
        want = [expected("efficient", kind, orient, l) for l in BATCH_LS]
        for sampler, opts in ((0, dict(device_sampler=0)), (1, dict(device_sampler=1, device_sampler_min_frames=1))):
            with options(ctx, **opts):
                for batch in ([cams[0]], cams):
                    what = (kind, orient, "device sampler" if sampler else "host-paced sampler", len(batch))
                    one = batch[0] if len(batch) == 1 else batch
                    _, st0 = ctx.render_efficient(pm, one, *efficient_args())
                    nearest = sampler_record(ctx, len(batch))
                    with options(ctx, sky_filter=1):
                        rgb, st = ctx.render_efficient(pm, one, *efficient_args())
                        assert ctx.get_option("last_sampler_path") == sampler, what
                        assert sampler_record(ctx, len(batch)) == nearest and counters(st) == counters(st0), what
                    frames = [rgb] if len(batch) == 1 else rgb
                    for f in range(len(batch)):
                        assert_frame(frames[f], want[f][0], what + (f,))
                        assert nearest[f][2][2:] == want[f][1][2:] and nearest[f][2][1] == want[f][2], what + (f,)


# ---- 3. direct renderer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_direct_vs_definition(ctx, kind, fast_math):
    assert_classes_present("direct", kind)
    pm = F.scene(kind)[2]
    for orient in ORIENTS:
        bind(ctx, orient)
        for l in (5.0, -3.0):
            want, want_st, _, _, _ = expected("direct", kind, orient, l)
            with options(ctx, sky_filter=1, fast_math=fast_math):
                rgb, st = ctx.render_direct(pm, F.scene(kind, l=l)[3], CAP, R, DELTA)
                assert counters(ctx.frame_stats(0)) == want_st
            assert_frame(rgb, want, (kind, orient, l, fast_math))
            assert counters(st) == want_st


# ---- 4. supersample = 2 x bilinear: the box average of the filtered fine frame, the oracle at 48 x 32 ------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_supersampled_and_filtered(ctx, kind):
    n = 2
    pm, pc = F.scene(kind)[2:]
    for renderer in ("brute", "efficient", "direct"):
        assert_classes_present(renderer, kind, n)
    for orient in ORIENTS:
        bind(ctx, orient)
        with options(ctx, sky_filter=1, supersample=n):
            for name, opts in (("static", dict(variant=1)), ("relay", dict(variant=2, relay_min_blocks=0))):
                with options(ctx, **opts):
                    rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
                want, want_st = expected("brute", kind, orient, 5.0, n)[:2]
                assert_frame(rgb, want, ("brute", name, kind, orient))
                assert counters(st) == want_st
            for sampler, opts in ((0, dict(device_sampler=0)), (1, dict(device_sampler=1, device_sampler_min_frames=1))):
                with options(ctx, **opts):
                    rgb, st = ctx.render_efficient(pm, pc, *efficient_args())
                want, want_st = expected("efficient", kind, orient, 5.0, n)[:2]
                assert_frame(rgb, want, ("efficient", sampler, kind, orient))
                assert counters(st)[2:] == want_st[2:] and st.rays == n * n * RES[0] * RES[1]
            rgb, st = ctx.render_direct(pm, pc, CAP, R, DELTA)
            want, want_st = expected("direct", kind, orient, 5.0, n)[:2]
            assert_frame(rgb, want, ("direct", kind, orient))
            assert counters(st) == want_st


# ---- 5. switched off again; skies on which the filter is the identity or one-dimensional ----------------------------------------
def renders(ctx, kind="ellis"):
    pm, pc = F.scene(kind)[2:]
    return [ctx.render_brute(pm, pc, CAP, R, DELTA)[0], ctx.render_efficient(pm, pc, *efficient_args())[0],
            ctx.render_direct(pm, pc, CAP, R, DELTA)[0]]


def test_switched_off_again_is_todays_frame(ctx):
    bind(ctx, "A")
    before = renders(ctx)
    with options(ctx, sky_filter=1):
        filtered = renders(ctx)
    after = renders(ctx)
    for b, f, a in zip(before, filtered, after):
        assert b.tobytes() == a.tobytes()
        assert (b != f).any()              # and the filter did something in between


def test_constant_and_one_texel_skies(ctx):
    colour = np.array([10, 200, 77, 255], np.uint8)
    for shape in ((7, 13), (1, 1)):
        bind(ctx, "B", [np.broadcast_to(colour, shape + (4,)).copy()] * 2)
        nearest = renders(ctx)
        with options(ctx, sky_filter=1):
            for got, want in zip(renders(ctx), nearest):
                assert_frame(got, want, ("a constant sky comes back constant", shape))
                assert set(map(tuple, got.reshape(-1, 3).tolist())) <= {(10, 200, 77), (0, 0, 0)}
    # a 1 x 1 sky of any colour: the frame of the nearest lookup
    bind(ctx, "A", [F.texture(1, 1, 5), F.texture(1, 1, 6)])
    nearest = renders(ctx)
    with options(ctx, sky_filter=1):
        for got, want in zip(renders(ctx), nearest):
            assert_frame(got, want, "1 x 1 skies")


def test_one_column_sky_is_exact(ctx):
    """skies of 1 x 9 and 1 x 1 texels: x0 = x1 = 0 whatever the longitude; the rows blend, and clamp at the poles"""
    shapes, salts = ((1, 9), (1, 1)), (0x017A3C, 0x02DEA5)
    real = [F.texture(w, h, 77 + k) for k, (w, h) in enumerate(shapes)]
    fine = [common.index_sky(256 * w, 256 * h, s) for (w, h), s in zip(shapes, salts)]
    F.assert_salts(shapes, salts, fine)
    for orient in ORIENTS:
        bind(ctx, orient, real)
        om, oc, pm, pc = F.scene("ellis")
        sp, sn = (O.sky(img, F.inverse_rotation(*F.ORIENT[orient][k])) for k, img in enumerate(fine))
        rgb, _, st = O.render_image(O.CV, om, oc, sp, sn, CAP, R, DELTA)
        want, which, Xc, Yc = F.filtered_frame(rgb, shapes, real, salts)
        fy = (Yc[which == 0] - 128) & 255
        assert (which == 0).sum() > 300 and len(set(fy.tolist())) > 50 and st.n_neg > 0
        with options(ctx, sky_filter=1):
            got, gst = ctx.render_brute(pm, pc, CAP, R, DELTA)
        assert_frame(got, want, ("1 x 9 and 1 x 1", orient))
        assert counters(gst) == counters(st)


# ---- 6. the two per-ray functions alone on the device, both instantiations -------------------------------------------------------
@pytest.mark.parametrize("size", F.SELFTEST_SIZES, ids=lambda s: "%dx%d" % s)
def test_selftest_sky_bilinear(gpu_ctx, size):
    w, h = size
    T = F.texture(w, h, 0xB11)
    rng = np.random.default_rng(977 + w)
    directed = F.directed_directions()
    orientations = [None] if w * h > 1 << 20 else [None, F.ORIENT["A"][0], ((0.3, -0.8, 0.52), (0.1, 0.2, 1.0))]
    for orient in orientations:
        inv = None if orient is None else F.inverse_rotation(*orient)
        dirs = np.concatenate([directed, F.random_directions(rng, F.N_RANDOM)])
        want_taps, want_raw, oob, want_rgb = F.expected_taps_and_colours(T, inv, dirs)
        taps, rgb = gpu_ctx.selftest_sky_bilinear(T, dirs, inv)
        for k, name in enumerate(("plain", "shared reciprocals")):
            bad = np.nonzero((taps[:, k] != want_taps).any(axis=1) | (rgb[:, k] != want_rgb).any(axis=1))[0]
            assert len(bad) == 0, (name, size, orient, len(bad), [(dirs[i].tolist(), taps[i, k].tolist(), want_taps[i].tolist(),
                                                                  rgb[i, k].tolist(), want_rgb[i].tolist()) for i in bad[:3]])
        if size == F.DIRECTED_SKY and orient is None:      # the directed inputs do what they are there for
            x0, x1, y0, y1, fx, fy = (want_taps[:len(directed), c] for c in range(6))
            assert ((x0 == w - 1) & (x1 == 0)).any() and ((y0 == 0) & (fy == 0)).any() and ((y0 == h - 1) & (y1 == h - 1)).any()
            assert (fx == 0).any() and (fx == 255).any() and (fy == 0).any() and (fy == 255).any() and (fx == 128).any() and oob.any()
            assert set(x0.tolist()) == set(range(w)) and set(y0.tolist()) == set(range(h))


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_option_and_refusals(ctx):
    bind(ctx, "A")
    pm, pc = F.scene("ellis")[2:]
    ctx.set_option("sky_filter", 1)
    for bad in (2, -1):
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.set_option("sky_filter", bad)
        assert e.value.code == _abi.E_INVALID and MESSAGE in str(e.value)
        assert ctx.get_option("sky_filter") == 1
    want = expected("brute", "ellis", "A")[0]
    refused = [("debug dump", {}, dict(debug=True)), ("variant = 0", dict(variant=0), {}), ("fuse_shade = 0", dict(fuse_shade=0), {})]
    for words, opts, kw in refused:
        with options(ctx, **opts):
            with pytest.raises(curvis_amd.CurvisError) as e:
                ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)
            assert e.value.code == _abi.E_INVALID and "sky_filter" in str(e.value) and words in str(e.value), (words, str(e.value))
            assert ctx.get_option("sky_filter") == 1
            with options(ctx, sky_filter=0):
                ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)           # works with the filter off
    assert_frame(ctx.render_brute(pm, pc, CAP, R, DELTA)[0], want, "after the refusals")
    # a sky of 2^23 + 1 texels in either dimension: 256 w is no u32 any more
    small = F.real_skies()[1]
    for shape in ((1, F.MAX_SIDE + 1), (F.MAX_SIDE + 1, 1)):
        big = np.zeros(shape + (4,), np.uint8)
        for which in (0, 1):
            ctx.set_sky(which, curvis_amd.SphericalImage(big))
            ctx.set_sky(1 - which, curvis_amd.SphericalImage(np.array(small)))
            for call in (lambda: ctx.render_brute(pm, pc, CAP, R, DELTA), lambda: ctx.render_efficient(pm, pc, *efficient_args()),
                         lambda: ctx.render_direct(pm, pc, CAP, R, DELTA)):
                with pytest.raises(curvis_amd.CurvisError) as e:
                    call()
                assert e.value.code == _abi.E_INVALID and "2^23" in str(e.value), str(e.value)
                assert ctx.get_option("sky_filter") == 1
        with options(ctx, sky_filter=0):
            ctx.render_brute(pm, pc, CAP, R, DELTA)                      # the nearest lookup takes such a sky
        with pytest.raises(curvis_amd.CurvisError):
            ctx.selftest_sky_bilinear(big, np.array([[1.0, 0.0, 0.0]]))
    bind(ctx, "A")
    assert_frame(ctx.render_brute(pm, pc, CAP, R, DELTA)[0], want, "after the oversized skies")


# ---- 8. the binary and the Python keywords -------------------------------------------------------------------------------------------
CLI_RES = (24, 14)
SIM = ("escape_radius = 10.0\nray_integration_max_itarations = 4096\nray_integration_step = 0.05\n"
       "sampling_initial_nums = 100\nsampling_max_iterations = 50\n"
       "sampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 2e-5\n")


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_sky_filter")
    sp, sn = F.real_skies()
    pngio.write_png(d / "pos.png", np.array(sp))
    pngio.write_png(d / "neg.png", np.array(sn))
    (d / "sim.toml").write_text(SIM)
    (d / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = 43.0\nfocal_length = 15.0\n" % CLI_RES)
    return d


def test_binary_image_and_python_keywords(ctx, cli_files):
    d = cli_files
    _, _, pm, pc = common.scene("ellis", res=CLI_RES)      # the binary's default pose
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
                "--sky-filter", "bilinear", "--stats", out / "st.json")
        assert r.returncode == 0, r.stderr
        nearest = api[mode]()
        keyword = api[mode](sky_filter="bilinear")
        assert ctx.get_option("sky_filter") == 0              # the keyword puts the context's option back
        with options(ctx, sky_filter=1):
            library = lib[mode]()
        assert_frame(keyword, library, ("Python keyword", mode))
        assert_frame(pngio.read_png(out / "output_image.png"), library, ("curvis image --sky-filter bilinear", mode))
        assert (library != nearest).any()
        assert_frame(api[mode](sky_filter="nearest"), nearest, ("sky_filter='nearest'", mode))
        st = json.loads((out / "st.json").read_text())
        assert st["sky_filter"] == "bilinear" and st["mode"] == mode and st["rays"] == CLI_RES[0] * CLI_RES[1]


def test_binary_video(ctx, cli_files):
    d = cli_files
    orbit = refpaths.reference_path_file("path_orbit.csv")
    (d / "vid.toml").write_text('video_name = "v"\nframe_rate = 0.05\nfilepath_to_camera_path = "%s"\n' % orbit)
    out = d / "vid"
    out.mkdir()
    r = run("video", d / "pos.png", d / "neg.png", out, "-v", d / "vid.toml", "-s", d / "sim.toml", "-c", d / "cam.toml",
            "--mode", "efficient", "--sky-filter=bilinear", "--stats", out / "st.jsonl")
    assert r.returncode == 0, r.stderr
    it = rendering.Interpolator.from_file(orbit)
    times = rendering.times_of_frames(it.min_time(), it.max_time(), 0.05)
    assert len(times) == 3
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 15.0, 43.0, CLI_RES[0], CLI_RES[1])
            for t in times]
    bind(ctx, None)
    with options(ctx, sky_filter=1):
        # the video loop passes threshold_1 twice (src/rendering.rs:305-306)
        rgb, _ = ctx.render_efficient(curvis_amd.EllisMetric(1.0), cams, 4096, 10.0, 0.05, 100, 100, 1e-5, 1e-5)
    nearest, _ = ctx.render_efficient(curvis_amd.EllisMetric(1.0), cams, 4096, 10.0, 0.05, 100, 100, 1e-5, 1e-5)
    assert (rgb != nearest).any()
    for k in range(3):
        assert_frame(pngio.read_png(out / "tmp" / ("frame_%d.png" % k)), rgb[k], ("curvis video --sky-filter=bilinear, frame", k))
    lines = [json.loads(ln) for ln in (out / "st.jsonl").read_text().splitlines()]
    assert sorted(ln["frame"] for ln in lines) == [0, 1, 2] and all(ln["sky_filter"] == "bilinear" for ln in lines)
