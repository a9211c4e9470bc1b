"""Heun's method (library option "integrator" = 1) on the GPU, exact against the composition of tests/integrator_ref.py: the oracle's
own Euler step cvo_update under CVO_CV, called twice per step from a saved state with the delta_k of "step_scale", and averaged, ray by
ray.  tests/test_integrator_host.py pins that composition's Euler form to step_scale_ref's and asserts, without a GPU, that every scene
below holds the ray classes its case is about (tests/gpu_integrator_cases.py is the list both files walk).

Debug dump: final state, t, step count, escape code and texel of every ray, bit for bit.  Fused static kernel, direct renderer,
efficient renderer (both samplers, and the sample table): every pixel and every counter.  In every exact case the option engages:
another frame and another step count than the same call under integrator = 0."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import common
import gpu_integrator_cases as CASES
import integrator_ref as IR
import sky_filter_ref as F
import step_scale_ref as SR
import curvis_amd
from curvis_amd import _abi, pngio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
COUNTERS = IR.COUNTERS
R = IR.R


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
    assert gpu_ctx.get_option("integrator") == 0
    yield gpu_ctx
    for key, value in (("integrator", 0), ("step_scale", 0), ("supersample", 1), ("sky_filter", 0), ("projection", 0)):
        gpu_ctx.set_option(key, value)


def assert_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def assert_dump(got, want, what):
    """every field bit for bit, x[0] = t included; a NaN equals a NaN whatever its payload (x86 and gfx950 propagate payloads differently)"""
    for f in ("steps", "code", "tx", "ty"):
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (what, f, len(bad), bad[:3].tolist(), got[f][tuple(bad[0])], want[f][tuple(bad[0])])
    for f in ("x", "p"):
        same = (common.bits(got[f]) == common.bits(want[f])) | (np.isnan(got[f]) & np.isnan(want[f]))
        bad = np.argwhere(~same)
        assert len(bad) == 0, (what, f, len(bad), bad[:3].tolist(), got[f][tuple(bad[0])], want[f][tuple(bad[0])])


def scene(case, res=None):
    """(product metric, product camera) of a case"""
    return SR.metrics(case["kind"])[1], SR.cameras(case["pose"], res or case.get("res", SR.RES))[1]


def heun(case):
    """the library options of a case"""
    return dict(integrator=1, step_scale=case["S"])


def engaged(rgb, st, rgb0, st0, what):
    """rgb0, st0: the same call under integrator = 0 (same delta, same step_scale), whose step count is the Euler composition's"""
    assert st.steps != st0.steps, (what, "the step count of integrator = 0", st.steps)
    assert (rgb != rgb0).any(), (what, "the frame of integrator = 0")


# ---- 1. debug dump and the plain fused frame -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES.DUMP, ids=lambda c: c["id"])
def test_dump_and_fused_frame(ctx, case):
    IR.assert_brute_classes(case)
    bind(ctx)
    pm, pc = scene(case)
    cap, delta = case.get("cap", 4096), case.get("delta", IR.DELTA)
    want_rgb, want_cnt, want_dbg, _, _ = IR.expected_case(case)
    with options(ctx, step_scale=case["S"]):
        rgb0, st0 = ctx.render_brute(pm, pc, cap, R, delta)
    with options(ctx, **heun(case)):
        rgb, st, dbg = ctx.render_brute(pm, pc, cap, R, delta, debug=True)
        assert_dump(dbg, want_dbg, case["id"])
        assert_frame(rgb, want_rgb, (case["id"], "debug dump's frame"))
        assert counters(st) == want_cnt, case["id"]
        for variant in (-1, 1, 2):       # whatever the variant asks for, the static kernel renders
            with options(ctx, variant=variant, relay_min_blocks=0):
                rgb, st = ctx.render_brute(pm, pc, cap, R, delta)
                assert ctx.get_option("last_relay_launches") == 0
                assert_frame(rgb, want_rgb, (case["id"], "fused", variant))
                assert counters(st) == want_cnt == counters(ctx.frame_stats(0)), (case["id"], variant)
        with options(ctx, fuse_shade=0):   # the debug dump is never fused: served
            _, _, dbg = ctx.render_brute(pm, pc, cap, R, delta, debug=True)
            assert_dump(dbg, want_dbg, (case["id"], "fuse_shade = 0"))
    engaged(rgb, st, rgb0, st0, case["id"])
    if case.get("delta") == SR.DELTA and not case.get("cap"):
        # the Euler composition itself (step_scale_ref's, shared with its own tests): other steps than Heun's
        euler = SR.expected("brute", case["kind"], case["pose"], case["S"], case.get("res", SR.RES))
        assert counters(st0) == euler[1] and st.steps != euler[1][1]


# ---- 2. batch, row band, and the three other options ---------------------------------------------------------------------------------
def test_batch_of_three_poses(ctx):
    bind(ctx)
    pm = SR.metrics("ellis")[1]
    cams = [scene(c)[1] for c in CASES.BATCH]
    want = [IR.expected_case(c) for c in CASES.BATCH]
    with options(ctx, step_scale=1024):
        rgb0, st0 = ctx.render_brute(pm, cams, 4096, R, IR.DELTA)
        with options(ctx, integrator=1):
            rgb, st = ctx.render_brute(pm, cams, 4096, R, IR.DELTA)
            for f in range(3):
                assert_frame(rgb[f], want[f][0], ("batch frame", f))
                assert counters(ctx.frame_stats(f)) == want[f][1], ("batch frame", f)
            assert counters(st) == tuple(sum(w[1][k] for w in want) for k in range(6))
    engaged(rgb, st, rgb0, st0, "batch")


def test_row_band(ctx):
    bind(ctx)
    pm, pc = scene(CASES.BAND)
    want = IR.expected_case(CASES.BAND)
    bands = ((0, 7), (7, 17))
    with options(ctx, step_scale=CASES.BAND["S"]):
        euler = [ctx.render_brute_rows(pm, pc, begin, count, 4096, R, IR.DELTA) for begin, count in bands]
    with options(ctx, **heun(CASES.BAND)):
        total = np.zeros(6, np.uint64)
        for (begin, count), (band0, st0) in zip(bands, euler):
            band, st = ctx.render_brute_rows(pm, pc, begin, count, 4096, R, IR.DELTA)
            assert_frame(band, want[0][begin:begin + count], ("rows", begin, count))
            total += np.array(counters(st), np.uint64)
            engaged(band, st, band0, st0, ("rows", begin, count))
        assert tuple(int(v) for v in total) == want[1]


def with_other_options(ctx, case, res, **others):
    """(Heun frame, its stats) of a brute call with the other options on, after the engagement check against integrator = 0"""
    pm, pc = scene(case, res)
    with options(ctx, step_scale=case["S"], **others):
        rgb0, st0 = ctx.render_brute(pm, pc, 4096, R, IR.DELTA)
        with options(ctx, integrator=1):
            rgb, st = ctx.render_brute(pm, pc, 4096, R, IR.DELTA)
    engaged(rgb, st, rgb0, st0, (case["id"], others))
    return rgb, st


def test_supersampled(ctx):
    bind(ctx)
    case = CASES.SUPERSAMPLED
    fine = IR.expected_case(case)
    rgb, st = with_other_options(ctx, case, (SR.RES[0] // 2, SR.RES[1] // 2), supersample=2)
    assert_frame(rgb, SR.box_average(fine[0], 2), "supersample = 2")
    assert counters(st) == fine[1]


def test_filtered(ctx):
    case = CASES.FILTERED
    IR.assert_brute_classes(case)
    bind(ctx, "real")
    fine = IR.expected_case(case)
    rgb, st = with_other_options(ctx, case, None, sky_filter=1)
    assert_frame(rgb, F.filtered_frame(fine[0])[0], "sky_filter = 1")
    assert counters(st) == fine[1]


def test_projected(ctx):
    case = CASES.PROJECTED
    IR.assert_brute_classes(case)
    bind(ctx)
    want = IR.expected_case(case)
    rgb, st = with_other_options(ctx, case, None, projection=case["projection"])
    assert_frame(rgb, want[0], "projection = 1")
    assert counters(st) == want[1]


def test_all_three_options_and_step_scale(ctx):
    case = CASES.ALL_THREE
    IR.assert_brute_classes(case)
    bind(ctx, "real")
    fine = IR.expected_case(case)
    rgb, st = with_other_options(ctx, case, (case["res"][0] // 2, case["res"][1] // 2), projection=case["projection"], sky_filter=1,
                                 supersample=2)
    assert_frame(rgb, SR.box_average(F.filtered_frame(fine[0])[0], 2), "all three")
    assert counters(st) == fine[1]


# ---- 3. direct and efficient renderers -----------------------------------------------------------------------------------------------
def efficient_args(cap=4096, delta=IR.DELTA):
    return (cap, R, delta, SR.EFF["n0"], SR.EFF["maxit"], SR.EFF["t1"], SR.EFF["t2"])


@pytest.mark.parametrize("case", [c for c in CASES.ANGLE if c["renderer"] == "direct"], ids=lambda c: c["id"])
def test_direct(ctx, case):
    IR.assert_angle_classes(case)
    bind(ctx)
    pm, pc = scene(case)
    want = IR.expected_case(case, "direct")
    with options(ctx, step_scale=case["S"]):
        rgb0, st0 = ctx.render_direct(pm, pc, 4096, R, IR.DELTA)
    with options(ctx, **heun(case)):
        rgb, st = ctx.render_direct(pm, pc, 4096, R, IR.DELTA)
    assert_frame(rgb, want[0], case["id"])
    assert counters(st) == want[1], case["id"]
    engaged(rgb, st, rgb0, st0, case["id"])


@pytest.mark.parametrize("case", [c for c in CASES.ANGLE if c["renderer"] == "efficient"], ids=lambda c: c["id"])
def test_efficient_both_samplers(ctx, case):
    IR.assert_angle_classes(case)
    bind(ctx)
    pm, pc = scene(case)
    want_rgb, want_cnt, table, f, _ = IR.expected_case(case, "efficient")
    for sampler, opts in ((0, dict(device_sampler=0)), (1, dict(device_sampler=1, device_sampler_min_frames=1))):
        what = (case["id"], "device sampler" if sampler else "host-paced sampler")
        with options(ctx, step_scale=case["S"], **opts):
            rgb0, st0 = ctx.render_efficient(pm, pc, *efficient_args())
            with options(ctx, integrator=1):
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


def test_prefetch_is_keyed_by_the_integrator(ctx):
    bind(ctx)
    case = CASES.ANGLE[3]
    assert case["renderer"] == "efficient" and case["kind"] == "ellis" and case["S"] == 1024
    pm, pc = scene(case)
    want = IR.expected_case(case, "efficient")[0]
    with options(ctx, device_sampler=1, device_sampler_min_frames=1, step_scale=case["S"]):
        euler, _ = ctx.render_efficient(pm, pc, *efficient_args())
        assert (euler != want).any()
        # a prefetch made under integrator = 0 is not consumed by a render under integrator = 1 ...
        ctx.prefetch_efficient(pm, pc, *efficient_args())
        with options(ctx, integrator=1):
            rgb, _ = ctx.render_efficient(pm, pc, *efficient_args())
            assert ctx.get_option("last_sampling_prefetched") == 0
            assert_frame(rgb, want, "prefetched under Euler, rendered under Heun")
            # ... nor the reverse ...
            ctx.prefetch_efficient(pm, pc, *efficient_args())
        rgb, _ = ctx.render_efficient(pm, pc, *efficient_args())
        assert ctx.get_option("last_sampling_prefetched") == 0
        assert_frame(rgb, euler, "prefetched under Heun, rendered under Euler")
        # ... and one made under the same value is
        with options(ctx, integrator=1):
            ctx.prefetch_efficient(pm, pc, *efficient_args())
            rgb, _ = ctx.render_efficient(pm, pc, *efficient_args())
            assert ctx.get_option("last_sampling_prefetched") == 1
            assert_frame(rgb, want, "prefetched and rendered under Heun")


def test_video_system_prefetches_under_the_integrator(ctx):
    """rendering.VideoRenderingSystem with integrator="heun": the sampler it starts one batch ahead runs under the option, so every
    batch finds its tables ready (the option is part of what identifies a sampler job), and the frames are the library's"""
    import refpaths
    from curvis_amd import rendering
    bind(ctx)
    it = rendering.Interpolator.from_file(refpaths.reference_path_file("path_through.csv"))
    pm = SR.metrics("ellis")[1]
    with options(ctx, device_sampler=1, device_sampler_min_frames=1):
        v = rendering.VideoRenderingSystem(pm, ctx, it, 1.5, SR.RES, 43.0, 15.0, R, 4096, IR.DELTA, batch=7, mode="efficient",
                                           sampling_initial_nums=60, sampling_convergence_threshold_1=2e-5, integrator="heun")
        frames = {}
        hits, made = ctx.get_option("prefetch_hits"), ctx.get_option("prefetches")
        stats = v.render(on_frame=lambda k, rgb, d: frames.__setitem__(k, np.array(rgb)))
        assert ctx.get_option("integrator") == 0                              # put back
        times = v.times_of_frames()
        assert len(times) == 30 == len(stats)
        assert ctx.get_option("prefetches") - made == 5 and ctx.get_option("prefetch_hits") - hits == 5   # batches of 7, 7, 7, 7, 2
        cams = [v.camera_at(times[k]) for k in (0, 13, 29)]
        with options(ctx, integrator=1):
            want, _ = ctx.render_efficient(pm, cams, 4096, R, IR.DELTA, 60, 60, 2e-5, 2e-5)
        euler, _ = ctx.render_efficient(pm, cams, 4096, R, IR.DELTA, 60, 60, 2e-5, 2e-5)
        for f, k in enumerate((0, 13, 29)):
            assert_frame(frames[k], want[f], ("video frame", k))
        assert (want != euler).any()


# ---- 4. option and refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1024])
def test_option_and_refusals(ctx, S):
    bind(ctx)
    case = CASES.DUMP[0]
    pm, pc = scene(case)
    want = IR.expected_case(case)[0]
    for value in (1, 0, 1):
        ctx.set_option("integrator", value)
        assert ctx.get_option("integrator") == value
    for bad in (-1, 2, 1 << 40):
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.set_option("integrator", bad)
        assert e.value.code == _abi.E_INVALID and "integrator" in str(e.value)
        assert ctx.get_option("integrator") == 1                         # the old value stays
    ctx.set_option("step_scale", S)
    name_of = "step_scale" if S else "integrator"                        # with both on, the refusal carries either name
    calls = {"brute": lambda **kw: ctx.render_brute(pm, pc, 4096, R, IR.DELTA, **kw),
             "direct": lambda **kw: ctx.render_direct(pm, pc, 4096, R, IR.DELTA),
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
            assert e.value.code == _abi.E_INVALID and name_of in str(e.value) and words in str(e.value), (words, name, str(e.value))
            assert ctx.get_option("integrator") == 1
            with options(ctx, integrator=0, step_scale=0):
                calls[name](**kw)                                       # works with the options off
    with options(ctx, fast_math=0):                                     # the prefetch is refused in the same words
        with pytest.raises(curvis_amd.CurvisError) as e:
            ctx.prefetch_efficient(pm, pc, *efficient_args())
        assert e.value.code == _abi.E_INVALID and name_of in str(e.value)
    # a step that is not greater than 0
    for delta in (0.0, -0.05, float("nan")):
        for name in calls:
            with pytest.raises(curvis_amd.CurvisError) as e:
                {"brute": lambda: ctx.render_brute(pm, pc, 16, R, delta), "direct": lambda: ctx.render_direct(pm, pc, 16, R, delta),
                 "efficient": lambda: ctx.render_efficient(pm, pc, 16, R, delta, 100, 100, 1e-5, 1e-5)}[name]()
            assert e.value.code == _abi.E_INVALID and name_of in str(e.value) and "delta" in str(e.value), (name, delta, str(e.value))
    # the context is usable after every refusal
    ctx.set_option("step_scale", case["S"])
    assert_frame(ctx.render_brute(pm, pc, 4096, R, IR.DELTA)[0], want, "after the refusals")
    # the functions that take their delta explicitly do not look at the option
    alphas = np.linspace(0.2, 2.9, 64)
    with_option = ctx.compute_escape_angles_range(pm, 5.0, alphas, IR.DELTA, 4096, R)
    ctx.set_option("integrator", 0)
    without = ctx.compute_escape_angles_range(pm, 5.0, alphas, IR.DELTA, 4096, R)
    assert repr(with_option) == repr(without)


# ---- 5. the binary and the Python keyword ----------------------------------------------------------------------------------------------
CLI_RES = (24, 14)
SIM = ("escape_radius = 30.0\nray_integration_max_itarations = 4096\nray_integration_step = 0.1\n"
       "sampling_initial_nums = 100\nsampling_max_iterations = 50\n"
       "sampling_convergence_threshold_1 = 1e-5\nsampling_convergence_threshold_2 = 2e-5\n")


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_binary_image_and_python_keyword(ctx, tmp_path):
    d = tmp_path
    sp, sn = SR.index_skies()
    pngio.write_png(d / "pos.png", np.array(sp))
    pngio.write_png(d / "neg.png", np.array(sn))
    (d / "sim.toml").write_text(SIM)
    (d / "cam.toml").write_text("resolution_x = %d\nresolution_y = %d\ndiagonal = 43.0\nfocal_length = 7.0\n" % CLI_RES)
    _, _, pm, pc = common.scene("ellis", res=CLI_RES, focal=7.0)      # the binary's default pose
    sp, sn = (curvis_amd.SphericalImage(np.array(t)) for t in SR.index_skies())
    system = curvis_amd.RelativisticSystem(pm, sp, sn, pc, context=ctx)
    api = {"brute": lambda **kw: system.render_image(4096, 30.0, 0.1, **kw),
           "efficient": lambda **kw: system.render_image_efficient(4096, 30.0, 0.1, 100, 50, 1e-5, 2e-5, **kw),
           "direct": lambda **kw: system.render_image_direct(4096, 30.0, 0.1, **kw)}
    lib = {"brute": lambda: ctx.render_brute(pm, pc, 4096, 30.0, 0.1)[0],
           "efficient": lambda: ctx.render_efficient(pm, pc, 4096, 30.0, 0.1, 100, 50, 1e-5, 2e-5)[0],
           "direct": lambda: ctx.render_direct(pm, pc, 4096, 30.0, 0.1)[0]}
    for mode in ("efficient", "brute", "direct"):
        out = d / ("img_" + mode)
        out.mkdir()
        r = run("image", d / "pos.png", d / "neg.png", out, "-s", d / "sim.toml", "-c", d / "cam.toml", "--mode", mode,
                "--integrator", "heun", "--step-scale", "4")
        assert r.returncode == 0, r.stderr
        euler = api[mode](step_scale=4.0)
        keyword = api[mode](step_scale=4.0, integrator="heun")
        assert ctx.get_option("integrator") == 0 and ctx.get_option("step_scale") == 0     # the keyword puts the context's options back
        with options(ctx, integrator=1, step_scale=1024):
            library = lib[mode]()
        assert_frame(keyword, library, ("Python keyword", mode))
        assert_frame(pngio.read_png(out / "output_image.png"), library, ("curvis image --integrator heun --step-scale 4", mode))
        assert (library != euler).any()
        assert_frame(api[mode](step_scale=4.0, integrator="euler"), euler, ("integrator='euler'", mode))
    r = run("image", d / "pos.png", d / "neg.png", d / "nowhere", "-s", d / "sim.toml", "-c", d / "cam.toml", "--integrator", "rk4")
    assert r.returncode == 2 and "--integrator must be euler or heun" in r.stderr
    with pytest.raises(ValueError, match="integrator must be"):
        api["brute"](integrator="rk4")
