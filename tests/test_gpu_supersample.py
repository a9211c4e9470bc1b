"""Supersampling (library option "supersample" = N in {2, 4, 8}) against the CPU oracle (CVO_CV), through every renderer.

The definition under test: with supersampling N a render call for cameras of W x H pixels returns W x H frames, and with A the
frame the SAME renderer produces with supersampling 1 for the same camera at N W x N H,

    out[y][x][c] = (sum over the N x N block of A[N y + j][N x + i][c] + N^2 / 2) >> (2 log2 N)

(8-bit channel values, round half up, black sub-rays count as 0); every counter of the call and of every frame is that of the
fine render.  A is taken from the oracle, so each comparison is exact: one differing sub-ray texel moves a channel sum.

Base scene: common.scene(metric, res=(13, 9)) -- camera at l = 5 looking at the throat -- with max_radius 10, delta 0.05 and a
cap of 340 steps, over index skies (colour = texel index) of 333 x 777 (+l) and 1000 x 500 (-l).  At every N the fine render holds
all three ray classes, and a handful of the 117 output pixels mix classes inside one pixel, capped (black) rays among them: every
oracle-based test asserts that from the oracle's per-ray dump first, so that a scene change cannot make it vacuous."""
import contextlib
import functools
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import common
import oracle_lib as O
import refpaths
import curvis_amd
from curvis_amd import _abi, pngio, rendering

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")

RES = (13, 9)
R, DELTA, CAP = 10.0, 0.05, 340
FACTORS = (2, 4, 8)
KINDS = ("ellis", "interstellar")
SALTS = (0x1B2C3D, 0xC4A5E6)
EFF = dict(cap=4096, n0=100, maxit=100, t1=1e-5, t2=1e-5)   # the efficient renderer's settings (max_radius = 10 as well)
COUNTERS = ("rays", "steps", "n_pos", "n_neg", "n_none", "n_oob")


@functools.lru_cache(maxsize=None)
def _skies():
    return common.index_sky(333, 777, SALTS[0]), common.index_sky(1000, 500, SALTS[1])


def _scene(kind, res, l=5.0):
    return common.scene(kind, res=res, pos=(0.0, l, common.HALF_PI, 0.0))


def box_average(a, n):
    """the definition: a = [n H, n W, 3] uint8 -> [H, W, 3] uint8"""
    h, w = a.shape[0] // n, a.shape[1] // n
    s = a.astype(np.uint32).reshape(h, n, w, n, 3).sum(axis=(1, 3), dtype=np.uint32)
    return ((s + n * n // 2) >> (2 * (n.bit_length() - 1))).astype(np.uint8)


def counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS)


@functools.lru_cache(maxsize=None)
def oracle_brute(kind, res, n, l=5.0):
    """the oracle's fine render of the scene at res x n: (frame, per-ray classes, counters); read-only, shared by the tests"""
    om, oc, _, _ = _scene(kind, (res[0] * n, res[1] * n), l)
    sp, sn = _skies()
    rgb, dbg, st = O.render_image(O.CV, om, oc, O.sky(sp), O.sky(sn), CAP, R, DELTA, debug=True)
    rgb.setflags(write=False)
    return rgb, dbg["code"].copy(), counters(st)


@functools.lru_cache(maxsize=None)
def oracle_efficient(kind, res, n, l=5.0):
    om, oc, _, _ = _scene(kind, (res[0] * n, res[1] * n), l)
    sp, sn = _skies()
    rgb, smp, st = O.render_image_efficient(O.CV, om, oc, O.sky(sp), O.sky(sn), EFF["cap"], R, DELTA, EFF["n0"], EFF["maxit"],
                                            EFF["t1"], EFF["t2"])
    rgb.setflags(write=False)
    return rgb, smp, counters(st)


@functools.lru_cache(maxsize=None)
def oracle_direct(kind, res, n):
    om, oc, _, _ = _scene(kind, (res[0] * n, res[1] * n))
    sp, sn = _skies()
    rgb, st = O.render_image_direct(O.CV, om, oc, O.sky(sp), O.sky(sn), CAP, R, DELTA)
    rgb.setflags(write=False)
    return rgb, counters(st)


def assert_scene_mixes_classes(kind, n, l=5.0):
    """at least one output pixel of the base scene whose n x n rays are of more than one class, and one whose mix includes a
    capped ray: the averages under test are then not averages of one texel colour, and black takes part"""
    _, code, st = oracle_brute(kind, RES, n, l)
    assert st[2] > 0 and st[3] > 0 and st[4] > 0, ("the fine render must hold all three ray classes", kind, n, st)
    blocks = code.reshape(RES[1], n, RES[0], n).transpose(0, 2, 1, 3).reshape(RES[1], RES[0], n * n)
    mixed = blocks.min(axis=2) != blocks.max(axis=2)
    with_capped = mixed & (blocks == O.NOT_ESCAPED).any(axis=2)
    assert mixed.sum() >= 1 and with_capped.sum() >= 1, (kind, n, int(mixed.sum()), int(with_capped.sum()))


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
    sp, sn = _skies()
    gpu_ctx.set_sky(0, curvis_amd.SphericalImage(sp))
    gpu_ctx.set_sky(1, curvis_amd.SphericalImage(sn))
    assert gpu_ctx.get_option("supersample") == 1
    yield gpu_ctx
    gpu_ctx.set_option("supersample", 1)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


# ---- 1. brute renderer against the oracle: both kernels, both step flavours ---------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("n", FACTORS)
@pytest.mark.parametrize("kind", KINDS)
def test_brute_vs_oracle(ctx, kind, n, fast_math):
    assert_scene_mixes_classes(kind, n)
    fine, _, want_st = oracle_brute(kind, RES, n)
    want = box_average(fine, n)
    _, _, pm, pc = _scene(kind, RES)
    with options(ctx, supersample=n, fast_math=fast_math, variant=1):
        rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
        assert ctx.get_option("last_relay_launches") == 0
        assert_frame(rgb, want, ("static kernel", kind, n, fast_math))
        assert counters(st) == want_st and counters(ctx.frame_stats(0)) == want_st
        assert want_st[0] == n * n * RES[0] * RES[1]
    with options(ctx, supersample=n, fast_math=fast_math, variant=2, relay_min_blocks=0):
        rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
        assert ctx.get_option("last_relay_launches") >= 1     # the relay kernel's epilogue really ran
        assert ctx.get_option("relay_mismatches") == 0 and ctx.get_option("relay_disabled") == 0
        assert_frame(rgb, want, ("relay kernel", kind, n, fast_math))
        assert counters(st) == want_st and counters(ctx.frame_stats(0)) == want_st


# ---- 2. shapes: partial fine tiles on the right and bottom edges (N = 2, 4), one-pixel frames, whole tiles -----------------------
@pytest.mark.parametrize("n", FACTORS)
@pytest.mark.parametrize("res", [(1, 1), (8, 8), (13, 9), (3, 17)], ids=lambda r: "%dx%d" % r)
def test_shapes(ctx, res, n):
    fine, _, want_st = oracle_brute("ellis", res, n)
    want = box_average(fine, n)
    _, _, pm, pc = _scene("ellis", res)
    _, _, _, pc_fine = _scene("ellis", (res[0] * n, res[1] * n))
    with options(ctx, variant=1):
        own_fine, own_st = ctx.render_brute(pm, pc_fine, CAP, R, DELTA)     # supersample = 1 at n W x n H: the product's own A
        with options(ctx, supersample=n):
            rgb, st = ctx.render_brute(pm, pc, CAP, R, DELTA)
    assert_frame(rgb, want, ("against the oracle", res, n))
    assert counters(st) == want_st
    assert_frame(rgb, box_average(own_fine, n), ("against the product's own fine render", res, n))
    assert counters(st) == counters(own_st)


# ---- 3. row band ----------------------------------------------------------------------------------------------------------------
def test_row_band(ctx):
    n = 4
    assert_scene_mixes_classes("ellis", n)
    fine, _, want_st = oracle_brute("ellis", RES, n)
    want = box_average(fine, n)
    _, _, pm, pc = _scene("ellis", RES)
    with options(ctx, supersample=n):
        full, st_full = ctx.render_brute(pm, pc, CAP, R, DELTA)
        assert_frame(full, want, "full frame")
        total = np.zeros(6, np.uint64)
        for begin, count in ((0, 2), (2, 3), (5, 4)):
            band, st = ctx.render_brute_rows(pm, pc, begin, count, CAP, R, DELTA)
            assert_frame(band, full[begin:begin + count], ("rows", begin, count))
            assert st.rays == n * n * RES[0] * count
            total += np.array(counters(st), np.uint64)
    assert tuple(int(v) for v in total) == counters(st_full) == want_st


# ---- 4. batch: 13 x 9 x 3 bytes per frame is odd, frames 1 and 2 do not start on a dword boundary ----------------------------------
BATCH_LS = (5.0, 4.0, 3.0)


def batch_vs_oracle(ctx, kind, n, download=True):
    want, want_st = [], []
    for l in BATCH_LS:
        fine, _, st = oracle_brute(kind, RES, n, l)
        want.append(box_average(fine, n))
        want_st.append(st)
    pm = _scene(kind, RES)[2]
    cams = [_scene(kind, RES, l)[3] for l in BATCH_LS]
    with options(ctx, supersample=n):
        rgb, st = ctx.render_brute(pm, cams, CAP, R, DELTA, download=download)
        per = [counters(ctx.frame_stats(f)) for f in range(len(cams))]
    assert per == want_st
    assert counters(st) == tuple(sum(s[k] for s in want_st) for k in range(6))
    if download:
        for f in range(len(cams)):
            assert_frame(rgb[f], want[f], ("frame", f, kind, n))
    return want


@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_batch(ctx, kind, n):
    assert_scene_mixes_classes(kind, n)
    batch_vs_oracle(ctx, kind, n)


# ---- 5. efficient renderer: both samplers; the samplers must not notice --------------------------------------------------------
def efficient_args():
    return (EFF["cap"], R, DELTA, EFF["n0"], EFF["maxit"], EFF["t1"], EFF["t2"])


def sampler_record(ctx, n_frames):
    out = []
    for f in range(n_frames):
        si = ctx.sampling_info(f)
        out.append(((si.n_samples, si.rounds, si.calls, si.steps, si.warned_max_iterations),
                    tuple(common.bits(a).tobytes() for a in ctx.samples(f))))
    return out


@pytest.mark.parametrize("n", FACTORS)
@pytest.mark.parametrize("kind", KINDS)
def test_efficient_vs_oracle(ctx, kind, n):
    assert_scene_mixes_classes(kind, n)
    pm = _scene(kind, RES)[2]
    # one frame, host-paced sampler
    with options(ctx, device_sampler=0):
        _, _ = ctx.render_efficient(pm, _scene(kind, RES)[3], *efficient_args())
        plain = sampler_record(ctx, 1)
        with options(ctx, supersample=n):
            rgb, st = ctx.render_efficient(pm, _scene(kind, RES)[3], *efficient_args())
            assert ctx.get_option("last_sampler_path") == 0
            assert sampler_record(ctx, 1) == plain
            fs = counters(ctx.frame_stats(0))
    fine, smp, want_st = oracle_efficient(kind, RES, n)
    assert want_st[2] > 0 and want_st[3] > 0
    assert_frame(rgb, box_average(fine, n), ("host-paced sampler", kind, n))
    assert counters(st)[2:5] == want_st[2:5] and fs[2:5] == want_st[2:5]
    assert st.rays == fs[0] == n * n * RES[0] * RES[1] and st.steps == smp["steps"]
    # three radii, device-resident sampler
    cams = [_scene(kind, RES, l)[3] for l in BATCH_LS]
    with options(ctx, device_sampler=1, device_sampler_min_frames=1):
        ctx.render_efficient(pm, cams, *efficient_args())
        assert ctx.get_option("last_sampler_path") == 1
        plain = sampler_record(ctx, 3)
        with options(ctx, supersample=n):
            rgb, st = ctx.render_efficient(pm, cams, *efficient_args())
            assert ctx.get_option("last_sampler_path") == 1
            assert sampler_record(ctx, 3) == plain
            per = [counters(ctx.frame_stats(f)) for f in range(3)]
    for f, l in enumerate(BATCH_LS):
        fine, smp, want_st = oracle_efficient(kind, RES, n, l)
        assert_frame(rgb[f], box_average(fine, n), ("device sampler, frame", f, kind, n))
        assert per[f][2:5] == want_st[2:5] and per[f][0] == n * n * RES[0] * RES[1] and per[f][1] == smp["steps"]
    assert st.rays == 3 * n * n * RES[0] * RES[1]


# ---- 6. direct renderer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", [1, 0])
@pytest.mark.parametrize("n", FACTORS)
@pytest.mark.parametrize("kind", KINDS)
def test_direct_vs_oracle(ctx, kind, n, fast_math):
    assert_scene_mixes_classes(kind, n)
    fine, want_st = oracle_direct(kind, RES, n)
    assert want_st[2] > 0 and want_st[3] > 0 and want_st[4] > 0
    _, _, pm, pc = _scene(kind, RES)
    with options(ctx, supersample=n, fast_math=fast_math):
        rgb, st = ctx.render_direct(pm, pc, CAP, R, DELTA)
        assert counters(ctx.frame_stats(0)) == want_st
    assert_frame(rgb, box_average(fine, n), (kind, n, fast_math))
    assert counters(st) == want_st and st.rays == n * n * RES[0] * RES[1]


# ---- 7. the option and the call shapes it refuses -------------------------------------------------------------------------------
def test_option_surface(ctx):
    assert ctx.get_option("supersample") == 1
    _, _, pm, pc = _scene("ellis", RES)
    default, st0 = ctx.render_brute(pm, pc, CAP, R, DELTA)
    ctx.set_option("supersample", 1)
    again, st1 = ctx.render_brute(pm, pc, CAP, R, DELTA)
    assert default.tobytes() == again.tobytes() and counters(st0) == counters(st1)
    ctx.set_option("supersample", 4)
    for bad in (0, 3, 16, -1):
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.set_option("supersample", bad)
        assert e.value.code == _abi.E_INVALID and "supersample must be 1, 2, 4 or 8" in str(e.value)
        assert ctx.get_option("supersample") == 4
    ctx.set_option("supersample", 2)
    refused = [("debug dump", {}, dict(debug=True)), ("variant = 0", dict(variant=0), {}), ("fuse_shade = 0", dict(fuse_shade=0), {})]
    for words, opts, kw in refused:
        with options(ctx, **opts):
            with pytest.raises(curvis_amd.CurvisError) as e:
                ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)
            assert e.value.code == _abi.E_INVALID and "supersample" in str(e.value) and words in str(e.value), (words, str(e.value))
            with options(ctx, supersample=1):
                out = ctx.render_brute(pm, pc, CAP, R, DELTA, **kw)
                assert_frame(out[0], default, ("works again with supersample = 1", words))
    fine, _, _ = oracle_brute("ellis", RES, 2)
    assert_frame(ctx.render_brute(pm, pc, CAP, R, DELTA)[0], box_average(fine, 2), "after the refusals")


# ---- 8. PNG front end: the frames in HBM are W x H ------------------------------------------------------------------------------
def test_png_front_end(ctx):
    n = 2
    want = batch_vs_oracle(ctx, "ellis", n, download=False)
    streams, _ = ctx.deflate_frames(RES[0], RES[1], len(want))
    for f, z in enumerate(streams):
        rows = np.frombuffer(zlib.decompress(z), np.uint8).reshape(RES[1], RES[0] * 3 + 1)
        assert (rows[:, 0] == 2).all()     # filter type Up: a running sum mod 256 undoes it
        got = np.cumsum(rows[:, 1:].astype(np.uint32), axis=0).astype(np.uint8).reshape(RES[1], RES[0], 3)
        assert_frame(got, want[f], ("inflated stream of frame", f))
    assert_frame(ctx.download_frames(RES[0], RES[1], len(want))[1], want[1], "curvis_ctx_download")


# ---- 9. the binary ----------------------------------------------------------------------------------------------------------------
CLI_RES = (24, 14)
SIM = ("escape_radius = 10.0\nray_integration_max_itarations = 4096\nray_integration_step = 0.05\n"
       "sampling_initial_nums = 100\nsampling_max_iterations = 50\n"
       "sampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 2e-5\n")


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_supersample")
    sp, sn = _skies()
    pngio.write_png(d / "pos.png", sp)
    pngio.write_png(d / "neg.png", sn)
    (d / "sim.toml").write_text(SIM)
    (d / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = 43.0\nfocal_length = 15.0\n" % CLI_RES)
    return d


def test_binary_image(ctx, cli_files):
    d = cli_files
    _, _, pm, pc = common.scene("ellis", res=CLI_RES)      # the binary's default pose
    sp, sn = _skies()
    system = curvis_amd.RelativisticSystem(pm, curvis_amd.SphericalImage(sp), curvis_amd.SphericalImage(sn), pc, context=ctx)
    api = {"brute": lambda: system.render_image(4096, 10.0, 0.05, supersample=2),
           "efficient": lambda: system.render_image_efficient(4096, 10.0, 0.05, 100, 100, 1e-5, 2e-5, supersample=2),
           "direct": lambda: system.render_image_direct(4096, 10.0, 0.05, supersample=2)}
    for mode in ("efficient", "brute", "direct"):
        out = d / ("img_" + mode)
        out.mkdir()
        r = run("image", d / "pos.png", d / "neg.png", out, "-s", d / "sim.toml", "-c", d / "cam.toml", "--mode", mode,
                "--supersample", "2", "--stats", out / "st.json")
        assert r.returncode == 0, r.stderr
        assert_frame(pngio.read_png(out / "output_image.png"), api[mode](), ("curvis image --supersample 2", mode))
        st = json.loads((out / "st.json").read_text())
        assert st["supersample"] == 2 and st["mode"] == mode and st["rays"] == 4 * CLI_RES[0] * CLI_RES[1]
        assert st["rays"] == system.last_stats.rays and st["n_pos"] == system.last_stats.n_pos and st["n_none"] == system.last_stats.n_none
    assert ctx.get_option("supersample") == 1              # the keyword puts the context's option back


def test_binary_video(ctx, cli_files):
    d = cli_files
    orbit = refpaths.reference_path_file("path_orbit.csv")
    (d / "vid.toml").write_text('video_name = "v"\nframe_rate = 0.0625\nfilepath_to_camera_path = "%s"\n' % orbit)
    out = d / "vid"
    out.mkdir()
    r = run("video", d / "pos.png", d / "neg.png", out, "-v", d / "vid.toml", "-s", d / "sim.toml", "-c", d / "cam.toml",
            "--mode", "efficient", "--supersample", "4", "--stats", out / "st.jsonl")
    assert r.returncode == 0, r.stderr
    it = rendering.Interpolator.from_file(orbit)
    times = rendering.times_of_frames(it.min_time(), it.max_time(), 0.0625)
    assert len(times) == 4
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 15.0, 43.0, CLI_RES[0], CLI_RES[1])
            for t in times]
    with options(ctx, supersample=4):
        # the video loop passes threshold_1 twice (src/rendering.rs:305-306)
        rgb, _ = ctx.render_efficient(curvis_amd.EllisMetric(1.0), cams, 4096, 10.0, 0.05, 100, 100, 1e-5, 1e-5)
    for k in range(4):
        assert_frame(pngio.read_png(out / "tmp" / ("frame_%d.png" % k)), rgb[k], ("curvis video --supersample 4, frame", k))
    lines = [json.loads(ln) for ln in (out / "st.jsonl").read_text().splitlines()]
    assert sorted(ln["frame"] for ln in lines) == [0, 1, 2, 3]
    assert all(ln["supersample"] == 4 and ln["rays"] == 16 * CLI_RES[0] * CLI_RES[1] for ln in lines)
