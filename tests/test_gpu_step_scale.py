"""Distance-scaled Euler steps (library option "step_scale") on the GPU, exact against the composition of tests/step_scale_ref.py: the
oracle's own Euler step cvo_update under CVO_CV, called with the step delta_k of the option's definition (include/curvis_hip.h), ray by
ray.  tests/test_step_scale_host.py pins that composition to the oracle's entry points at S = 0 and asserts, without a GPU, that every
scene below holds the ray classes its case is about (tests/gpu_step_scale_cases.py is the list both files walk).

Debug dump: final state, step count, escape code and texel of every ray, bit for bit.  Fused static kernel, direct renderer, efficient
renderer (both samplers, and the sample table): every pixel and every counter.  In every exact case the option engages: fewer executed
steps than the same call at S = 0, and another frame."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import common
import gpu_step_scale_cases as CASES
import oracle_lib as O
import refpaths
import sky_filter_ref as F
import step_scale_ref as SR
import curvis_amd
from curvis_amd import _abi, pngio, rendering

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
COUNTERS = SR.COUNTERS
R, DELTA = SR.R, SR.DELTA


def counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS)


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


def bind(ctx, skies="index"):
    for k, img in enumerate(SR.index_skies() if skies == "index" else F.real_skies()):
        ctx.set_sky(k, curvis_amd.SphericalImage(np.array(img)))


@pytest.fixture()
def ctx(gpu_ctx):
    assert gpu_ctx.get_option("step_scale") == 0
    yield gpu_ctx
    for key, value in (("step_scale", 0), ("supersample", 1), ("sky_filter", 0), ("projection", 0)):
        gpu_ctx.set_option(key, value)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def assert_dump(got, want, what):
    """every field bit for bit; a NaN equals a NaN whatever its payload (x86 and gfx950 propagate payloads differently)"""
    for f in ("steps", "code", "tx", "ty"):
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (what, f, len(bad), bad[:3].tolist(), got[f][tuple(bad[0])], want[f][tuple(bad[0])])
    for f in ("x", "p"):
        same = (common.bits(got[f]) == common.bits(want[f])) | (np.isnan(got[f]) & np.isnan(want[f]))
        bad = np.argwhere(~same)
        assert len(bad) == 0, (what, f, len(bad), bad[:3].tolist(), got[f][tuple(bad[0])], want[f][tuple(bad[0])])


def scene(case, res=None):
    """(product metric, product camera, the composition) of a case"""
    res = res or case.get("res", SR.RES)
    pm = SR.metrics(case["kind"])[1]
    pc = SR.cameras(case["pose"], res)[1]
    return pm, pc


def want_of(case, renderer="brute"):
    return SR.expected(renderer, case["kind"], case["pose"], case["S"], case.get("res", SR.RES), case.get("cap", 4096),
                       case.get("projection", 0), case.get("skies", "index"))


def engaged(rgb, st, rgb0, st0, what):
    assert st.steps < st0.steps, (what, "no fewer steps than at step_scale = 0", st.steps, st0.steps)
    assert (rgb != rgb0).any(), (what, "the frame of step_scale = 0")


# ---- 1. debug dump and the plain fused frame -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES.DUMP, ids=lambda c: c["id"])
def test_dump_and_fused_frame(ctx, case):
    SR.assert_brute_classes(case["kind"], case["pose"], case["S"], case.get("res", SR.RES), case.get("cap", 4096),
                            capped=case.get("capped", False), neg=case["kind"] != "flat")
    bind(ctx)
    pm, pc = scene(case)
    cap = case.get("cap", 4096)
    want_rgb, want_cnt, want_dbg, _ = want_of(case)
    rgb0, st0 = ctx.render_brute(pm, pc, cap, R, DELTA)
    with options(ctx, step_scale=case["S"]):
        rgb, st, dbg = ctx.render_brute(pm, pc, cap, R, DELTA, debug=True)
        assert_dump(dbg, want_dbg, case["id"])
        assert_frame(rgb, want_rgb, (case["id"], "debug dump's frame"))
        assert counters(st) == want_cnt, case["id"]
        for variant in (-1, 1, 2):       # whatever the variant asks for, the static kernel renders
            with options(ctx, variant=variant, relay_min_blocks=0):
                rgb, st = ctx.render_brute(pm, pc, cap, R, DELTA)
                assert ctx.get_option("last_relay_launches") == 0
                assert_frame(rgb, want_rgb, (case["id"], "fused", variant))
                assert counters(st) == want_cnt == counters(ctx.frame_stats(0)), (case["id"], variant)
        with options(ctx, fuse_shade=0):   # the debug dump is never fused: served
            _, _, dbg = ctx.render_brute(pm, pc, cap, R, DELTA, debug=True)
            assert_dump(dbg, want_dbg, (case["id"], "fuse_shade = 0"))
    engaged(rgb, st, rgb0, st0, case["id"])


# ---- 2. batch, row band, and the three other options ---------------------------------------------------------------------------------
def test_batch_of_three_poses(ctx):
    bind(ctx)
    pm = SR.metrics("ellis")[1]
    cams = [scene(c)[1] for c in CASES.BATCH]
    want = [want_of(c) for c in CASES.BATCH]
    rgb0, st0 = ctx.render_brute(pm, cams, 4096, R, DELTA)
    with options(ctx, step_scale=1024):
        rgb, st = ctx.render_brute(pm, cams, 4096, R, DELTA)
        for f in range(3):
            assert_frame(rgb[f], want[f][0], ("batch frame", f))
            assert counters(ctx.frame_stats(f)) == want[f][1], ("batch frame", f)
        assert counters(st) == tuple(sum(w[1][k] for w in want) for k in range(6))
    engaged(rgb, st, rgb0, st0, "batch")


def test_row_band(ctx):
    bind(ctx)
    pm, pc = scene(CASES.BAND)
    want = want_of(CASES.BAND)
    bands = ((0, 7), (7, 17))
    fixed = [ctx.render_brute_rows(pm, pc, begin, count, 4096, R, DELTA) for begin, count in bands]
    with options(ctx, step_scale=CASES.BAND["S"]):
        total = np.zeros(6, np.uint64)
        for (begin, count), (band0, st0) in zip(bands, fixed):
            band, st = ctx.render_brute_rows(pm, pc, begin, count, 4096, R, DELTA)
            assert_frame(band, want[0][begin:begin + count], ("rows", begin, count))
            total += np.array(counters(st), np.uint64)
            engaged(band, st, band0, st0, ("rows", begin, count))
        assert tuple(int(v) for v in total) == want[1]


def test_supersampled(ctx):
    bind(ctx)
    case = CASES.SUPERSAMPLED
    pm, pc = scene(case, (SR.RES[0] // 2, SR.RES[1] // 2))
    fine = want_of(case)
    rgb0, st0 = None, None
    with options(ctx, supersample=2):
        rgb0, st0 = ctx.render_brute(pm, pc, 4096, R, DELTA)
        with options(ctx, step_scale=case["S"]):
            rgb, st = ctx.render_brute(pm, pc, 4096, R, DELTA)
    assert_frame(rgb, SR.box_average(fine[0], 2), "supersample = 2")
    assert counters(st) == fine[1]
    engaged(rgb, st, rgb0, st0, "supersample = 2")


def test_filtered(ctx):
    case = CASES.FILTERED
    SR.assert_brute_classes(case["kind"], case["pose"], case["S"], skies="fine")
    bind(ctx, "real")
    pm, pc = scene(case)
    fine = want_of(case)
    with options(ctx, sky_filter=1):
        rgb0, st0 = ctx.render_brute(pm, pc, 4096, R, DELTA)
        with options(ctx, step_scale=case["S"]):
            rgb, st = ctx.render_brute(pm, pc, 4096, R, DELTA)
    assert_frame(rgb, F.filtered_frame(fine[0])[0], "sky_filter = 1")
    assert counters(st) == fine[1]
    engaged(rgb, st, rgb0, st0, "sky_filter = 1")


def test_projected(ctx):
    case = CASES.PROJECTED
    SR.assert_brute_classes(case["kind"], case["pose"], case["S"], case["res"], projection=case["projection"])
    bind(ctx)
    pm, pc = scene(case)
    want = want_of(case)
    with options(ctx, projection=case["projection"]):
        rgb0, st0 = ctx.render_brute(pm, pc, 4096, R, DELTA)
        with options(ctx, step_scale=case["S"]):
            rgb, st = ctx.render_brute(pm, pc, 4096, R, DELTA)
    assert_frame(rgb, want[0], "projection = 1")
    assert counters(st) == want[1]
    engaged(rgb, st, rgb0, st0, "projection = 1")


def test_all_three_options(ctx):
    case = CASES.ALL_THREE
    SR.assert_brute_classes(case["kind"], case["pose"], case["S"], case["res"], projection=case["projection"], skies="fine")
    bind(ctx, "real")
    pm, pc = scene(case, (case["res"][0] // 2, case["res"][1] // 2))
    fine = want_of(case)
    with options(ctx, projection=case["projection"], sky_filter=1, supersample=2):
        rgb0, st0 = ctx.render_brute(pm, pc, 4096, R, DELTA)
        with options(ctx, step_scale=case["S"]):
            rgb, st = ctx.render_brute(pm, pc, 4096, R, DELTA)
    assert_frame(rgb, SR.box_average(F.filtered_frame(fine[0])[0], 2), "all three")
    assert counters(st) == fine[1]
    engaged(rgb, st, rgb0, st0, "all three")


# ---- 3. direct and efficient renderers -----------------------------------------------------------------------------------------------
def efficient_args(cap=4096):
    return (cap, R, DELTA, SR.EFF["n0"], SR.EFF["maxit"], SR.EFF["t1"], SR.EFF["t2"])


@pytest.mark.parametrize("case", [c for c in CASES.ANGLE if c["renderer"] == "direct"], ids=lambda c: c["id"])
def test_direct(ctx, case):
    bind(ctx)
    pm, pc = scene(case)
    want = want_of(case, "direct")
    SR.assert_angle_classes(want[-1], case["kind"])
    rgb0, st0 = ctx.render_direct(pm, pc, 4096, R, DELTA)
    with options(ctx, step_scale=case["S"]):
        rgb, st = ctx.render_direct(pm, pc, 4096, R, DELTA)
    assert_frame(rgb, want[0], case["id"])
    assert counters(st) == want[1], case["id"]
    engaged(rgb, st, rgb0, st0, case["id"])


@pytest.mark.parametrize("case", [c for c in CASES.ANGLE if c["renderer"] == "efficient"], ids=lambda c: c["id"])
def test_efficient_both_samplers(ctx, case):
    bind(ctx)
    pm, pc = scene(case)
    want_rgb, want_cnt, table, f = want_of(case, "efficient")
    SR.assert_angle_classes(f, case["kind"])
    for sampler, opts in ((0, dict(device_sampler=0)), (1, dict(device_sampler=1, device_sampler_min_frames=1))):
        what = (case["id"], "device sampler" if sampler else "host-paced sampler")
        with options(ctx, **opts):
            rgb0, st0 = ctx.render_efficient(pm, pc, *efficient_args())
            with options(ctx, step_scale=case["S"]):
                rgb, st = ctx.render_efficient(pm, pc, *efficient_args())
                assert ctx.get_option("last_sampler_path") == sampler, what
                got = ctx.samples(0)
                si = ctx.sampling_info(0)
        for g, w, name in zip(got, table, ("alpha", "escape angle", "escape space")):
            assert common.bits(g).tobytes() == common.bits(w).tobytes(), what + (name, len(g), len(w))
        assert (si.calls, si.steps) == (f.calls, f.steps), what
        assert_frame(rgb, want_rgb, what)
        assert counters(st) == want_cnt, what
        engaged(rgb, st, rgb0, st0, what)


def test_prefetch_is_keyed_by_the_option(ctx):
    bind(ctx)
    case = CASES.ANGLE[2]
    assert case["renderer"] == "efficient" and case["kind"] == "ellis"
    pm, pc = scene(case)
    want = want_of(case, "efficient")[0]
    with options(ctx, device_sampler=1, device_sampler_min_frames=1):
        plain, _ = ctx.render_efficient(pm, pc, *efficient_args())
        assert (plain != want).any()
        # a prefetch made under S = 0 is not consumed by a render under S = 1024 ...
        ctx.prefetch_efficient(pm, pc, *efficient_args())
        with options(ctx, step_scale=case["S"]):
            rgb, _ = ctx.render_efficient(pm, pc, *efficient_args())
            assert ctx.get_option("last_sampling_prefetched") == 0
            assert_frame(rgb, want, "prefetched at 0, rendered at S")
            # ... nor the reverse ...
            ctx.prefetch_efficient(pm, pc, *efficient_args())
        rgb, _ = ctx.render_efficient(pm, pc, *efficient_args())
        assert ctx.get_option("last_sampling_prefetched") == 0
        assert_frame(rgb, plain, "prefetched at S, rendered at 0")
        # ... and one made under the same value is
        with options(ctx, step_scale=case["S"]):
            ctx.prefetch_efficient(pm, pc, *efficient_args())
            rgb, _ = ctx.render_efficient(pm, pc, *efficient_args())
            assert ctx.get_option("last_sampling_prefetched") == 1
            assert_frame(rgb, want, "prefetched and rendered at S")


def test_video_system_prefetches_under_the_option(ctx):
    """rendering.VideoRenderingSystem with step_scale: the sampler it starts one batch ahead runs under the option, so every batch finds
    its tables ready (the option is part of what identifies a sampler job), and the frames are the library's"""
    bind(ctx)
    it = rendering.Interpolator.from_file(refpaths.reference_path_file("path_through.csv"))
    pm = SR.metrics("ellis")[1]
    with options(ctx, device_sampler=1, device_sampler_min_frames=1):
        v = rendering.VideoRenderingSystem(pm, ctx, it, 1.5, SR.RES, 43.0, 15.0, R, 4096, DELTA, batch=7, mode="efficient",
                                           sampling_initial_nums=60, sampling_convergence_threshold_1=2e-5, step_scale=4.0)
        frames = {}
        hits, made = ctx.get_option("prefetch_hits"), ctx.get_option("prefetches")
        stats = v.render(on_frame=lambda k, rgb, d: frames.__setitem__(k, np.array(rgb)))
        assert ctx.get_option("step_scale") == 0                              # put back
        times = v.times_of_frames()
        assert len(times) == 30 == len(stats)
        assert ctx.get_option("prefetches") - made == 5 and ctx.get_option("prefetch_hits") - hits == 5   # batches of 7, 7, 7, 7, 2
        cams = [v.camera_at(times[k]) for k in (0, 13, 29)]
        with options(ctx, step_scale=1024):
            want, _ = ctx.render_efficient(pm, cams, 4096, R, DELTA, 60, 60, 2e-5, 2e-5)
        fixed, _ = ctx.render_efficient(pm, cams, 4096, R, DELTA, 60, 60, 2e-5, 2e-5)
        for f, k in enumerate((0, 13, 29)):
            assert_frame(frames[k], want[f], ("video frame", k))
        assert (want != fixed).any()


# ---- 4. S = 2^20 with R = 100: delta_k = delta on every step, so the ADAPT kernels must give today's bytes -----------------------------
def test_largest_scale_is_todays_frame(ctx):
    bind(ctx)
    pm, pc = SR.metrics("ellis")[1], SR.cameras("facing", (256, 144))[1]
    pi_, ps = SR.metrics("interstellar")[1], SR.cameras("tilted", (64, 36))[1]

    def renders():
        out = []
        for m, c in ((pm, pc), (pi_, ps)):
            rgb, st, dbg = ctx.render_brute(m, c, 4096, 100.0, DELTA, debug=True)
            out.append((rgb.tobytes(), counters(st), dbg.tobytes()))
            rgb, st = ctx.render_brute(m, c, 4096, 100.0, DELTA)
            out.append((rgb.tobytes(), counters(st)))
        rgb, st = ctx.render_direct(pi_, ps, 4096, 100.0, DELTA)
        out.append((rgb.tobytes(), counters(st)))
        for sampler in (0, 1):
            with options(ctx, device_sampler=sampler, device_sampler_min_frames=1):
                rgb, st = ctx.render_efficient(pi_, ps, 4096, 100.0, DELTA, 100, 100, 1e-5, 1e-5)
                out.append((rgb.tobytes(), counters(st), tuple(a.tobytes() for a in ctx.samples(0))))
        return out
    today = renders()
    with options(ctx, step_scale=1 << 20, variant=1):
        got = renders()
    assert len(got) == len(today)
    for k, (g, t) in enumerate(zip(got, today)):
        assert g == t, ("render", k, "differs from step_scale = 0")


# ---- 5. option, refusals, launch selection ---------------------------------------------------------------------------------------------
def test_option_and_refusals(ctx):
    bind(ctx)
    case = CASES.DUMP[0]
    pm, pc = scene(case)
    want = want_of(case)[0]
    for value in (1, 870, 0, 1 << 20, 1024):
        ctx.set_option("step_scale", value)
        assert ctx.get_option("step_scale") == value
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.set_option("step_scale", bad)
        assert e.value.code == _abi.E_INVALID and "step_scale" in str(e.value)
        assert ctx.get_option("step_scale") == 1024
    calls = {"brute": lambda **kw: ctx.render_brute(pm, pc, 4096, R, DELTA, **kw),
             "direct": lambda **kw: ctx.render_direct(pm, pc, 4096, R, DELTA),
             "efficient": lambda **kw: ctx.render_efficient(pm, pc, *efficient_args())}
    refused = [("fast_math = 0", dict(fast_math=0), "brute", {}), ("fast_math = 0", dict(fast_math=0), "brute", dict(debug=True)),
               ("fast_math = 0", dict(fast_math=0), "direct", {}), ("fast_math = 0", dict(fast_math=0), "efficient", {}),
               ("fast_math = 0", dict(fast_math=0, device_sampler=1, device_sampler_min_frames=1), "efficient", {}),
               ("variant = 0", dict(variant=0), "brute", {}), ("variant = 0", dict(variant=0), "brute", dict(debug=True)),
               ("fuse_shade = 0", dict(fuse_shade=0), "brute", {})]
    for words, opts, name, kw in refused:
        with options(ctx, **opts):
            with pytest.raises(curvis_amd.CurvisError) as e:
                calls[name](**kw)
            assert e.value.code == _abi.E_INVALID and "step_scale" in str(e.value) and words in str(e.value), (words, name, str(e.value))
            assert ctx.get_option("step_scale") == 1024
            with options(ctx, step_scale=0):
                calls[name](**kw)                                       # works with the option off
    with options(ctx, fast_math=0):                                     # the prefetch is refused in the same words
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.prefetch_efficient(pm, pc, *efficient_args())
        assert e.value.code == _abi.E_INVALID and "step_scale" in str(e.value)
    # a step that is not greater than 0
    for delta in (0.0, -0.05, float("nan")):
        for name in calls:
            with pytest.raises(curvis_amd.CurvisError) as e:
                {"brute": lambda: ctx.render_brute(pm, pc, 16, R, delta), "direct": lambda: ctx.render_direct(pm, pc, 16, R, delta),
                 "efficient": lambda: ctx.render_efficient(pm, pc, 16, R, delta, 100, 100, 1e-5, 1e-5)}[name]()
            assert e.value.code == _abi.E_INVALID and "step_scale" in str(e.value) and "delta" in str(e.value), (name, delta, str(e.value))
    assert_frame(ctx.render_brute(pm, pc, 4096, R, DELTA)[0], want, "after the refusals")
    # the functions that take their delta explicitly do not look at the option
    alphas = np.linspace(0.2, 2.9, 64)
    with_option = ctx.compute_escape_angles_range(pm, 5.0, alphas, DELTA, 4096, R)
    ctx.set_option("step_scale", 0)
    without = ctx.compute_escape_angles_range(pm, 5.0, alphas, DELTA, 4096, R)
    assert repr(with_option) == repr(without)


def test_relay_checks_do_not_move():
    """a single-frame 1080p-shaped call: with S = 0 the relay kernel takes it (and its first launch of the shape is checked), with
    S != 0 the static kernel does and the seat belt's counter stays where it is.  A context of its own: the counters are per context."""
    own = curvis_amd.Context(0)
    try:
        bind(own)
        pm, pc = SR.metrics("ellis")[1], SR.cameras("facing", (1920, 1080))[1]
        with options(own, step_scale=1024):
            before = own.get_option("relay_checks")
            _, st = own.render_brute(pm, pc, 4096, R, DELTA, download=False)
            assert own.get_option("last_relay_launches") == 0
            assert own.get_option("relay_checks") == before == 0 and own.get_option("relay_verified_shapes") == 0
        _, st0 = own.render_brute(pm, pc, 4096, R, DELTA, download=False)
        assert own.get_option("last_relay_launches") >= 1 and own.get_option("relay_checks") == 1
        assert st.steps < st0.steps and st.rays == st0.rays == 1920 * 1080
        with options(own, step_scale=1024):
            own.render_brute(pm, pc, 4096, R, DELTA, download=False)
            assert own.get_option("last_relay_launches") == 0 and own.get_option("relay_checks") == 1
        assert own.get_option("relay_mismatches") == 0 and own.get_option("relay_disabled") == 0
    finally:
        own.close()


# ---- 6. the binary and the Python keyword ----------------------------------------------------------------------------------------------
CLI_RES = (24, 14)
SIM = ("escape_radius = 30.0\nray_integration_max_itarations = 4096\nray_integration_step = 0.05\n"
       "sampling_initial_nums = 100\nsampling_max_iterations = 50\n"
       "sampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 2e-5\n")


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_step_scale")
    sp, sn = SR.index_skies()
    pngio.write_png(d / "pos.png", np.array(sp))
    pngio.write_png(d / "neg.png", np.array(sn))
    (d / "sim.toml").write_text(SIM)
    (d / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = 43.0\nfocal_length = 7.0\n" % CLI_RES)
    return d


def test_binary_image_and_python_keyword(ctx, cli_files):
    d = cli_files
    _, _, pm, pc = common.scene("ellis", res=CLI_RES, focal=7.0)      # the binary's default pose
    sp, sn = (curvis_amd.SphericalImage(np.array(t)) for t in SR.index_skies())
    system = curvis_amd.RelativisticSystem(pm, sp, sn, pc, context=ctx)
    api = {"brute": lambda **kw: system.render_image(4096, 30.0, 0.05, **kw),
           "efficient": lambda **kw: system.render_image_efficient(4096, 30.0, 0.05, 100, 50, 1e-5, 2e-5, **kw),
           "direct": lambda **kw: system.render_image_direct(4096, 30.0, 0.05, **kw)}
    lib = {"brute": lambda: ctx.render_brute(pm, pc, 4096, 30.0, 0.05)[0],
           "efficient": lambda: ctx.render_efficient(pm, pc, 4096, 30.0, 0.05, 100, 50, 1e-5, 2e-5)[0],
           "direct": lambda: ctx.render_direct(pm, pc, 4096, 30.0, 0.05)[0]}
    for mode in ("efficient", "brute", "direct"):
        out = d / ("img_" + mode)
        out.mkdir()
        r = run("image", d / "pos.png", d / "neg.png", out, "-s", d / "sim.toml", "-c", d / "cam.toml", "--mode", mode, "--step-scale", "3.3984375")
        assert r.returncode == 0, r.stderr
        fixed = api[mode]()
        keyword = api[mode](step_scale=3.3984375)
        assert ctx.get_option("step_scale") == 0               # the keyword puts the context's option back
        with options(ctx, step_scale=870):
            library = lib[mode]()
        assert_frame(keyword, library, ("Python keyword", mode))
        assert_frame(pngio.read_png(out / "output_image.png"), library, ("curvis image --step-scale 3.3984375", mode))
        assert (library != fixed).any()
        assert_frame(api[mode](step_scale=0), fixed, ("step_scale=0", mode))
    r = run("image", d / "pos.png", d / "neg.png", d / "nowhere", "-s", d / "sim.toml", "-c", d / "cam.toml", "--step-scale", "0.3")
    assert r.returncode == 2 and "--step-scale must be 0 or a multiple of 1/256" in r.stderr
    with pytest.raises(ValueError, match="multiple of 1/256"):
        api["brute"](step_scale=0.3)


def test_binary_video(ctx, cli_files):
    d = cli_files
    orbit = refpaths.reference_path_file("path_orbit.csv")
    (d / "vid.toml").write_text('video_name = "v"\nframe_rate = 0.05\nfilepath_to_camera_path = "%s"\n' % orbit)
    out = d / "vid"
    out.mkdir()
    r = run("video", d / "pos.png", d / "neg.png", out, "-v", d / "vid.toml", "-s", d / "sim.toml", "-c", d / "cam.toml",
            "--mode", "efficient", "--step-scale=4")
    assert r.returncode == 0, r.stderr
    it = rendering.Interpolator.from_file(orbit)
    times = rendering.times_of_frames(it.min_time(), it.max_time(), 0.05)
    assert len(times) == 3
    cams = [curvis_amd.Camera(it.camera_position(t), it.camera_forward(t), it.camera_up(t), 7.0, 43.0, CLI_RES[0], CLI_RES[1])
            for t in times]
    bind(ctx)
    with options(ctx, step_scale=1024):
        # the video loop passes threshold_1 twice (src/rendering.rs:305-306)
        rgb, _ = ctx.render_efficient(curvis_amd.EllisMetric(1.0), cams, 4096, 30.0, 0.05, 100, 50, 1e-5, 1e-5)
    fixed, _ = ctx.render_efficient(curvis_amd.EllisMetric(1.0), cams, 4096, 30.0, 0.05, 100, 50, 1e-5, 1e-5)
    assert (rgb != fixed).any()
    for k in range(3):
        assert_frame(pngio.read_png(out / "tmp" / ("frame_%d.png" % k)), rgb[k], ("curvis video --step-scale=4, frame", k))
