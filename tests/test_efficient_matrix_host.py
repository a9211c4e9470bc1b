"""The kernel lattices of the direct and the efficient renderer (tests/efficient_matrix_ref.py), the parts that need no GPU: the
enumerations against the dispatch code, by reading it; the evaluator against the two evaluators that exist, bit for bit; the ray classes of
every walk and table that tests/test_gpu_efficient_matrix.py compares against, asserted from the reference alone; that every axis engages
in the reference; the conditions of the batch and of the capped direct loop; and pins of a few counters and frames."""
import os
import re
import zlib

import numpy as np
import pytest

import efficient_matrix_ref as E
import kernel_matrix_ref as K
import oracle_lib as O
import step_scale_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "curvis_amd", "csrc")
WALK_STEPS = ("fast", "scaled", "heun")        # the three step walks; strict shares fast's
BIG, SMALL = K.GRIDS[1], K.GRIDS[8]


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- the enumerations ------------------------------------------------------------------------------------------------------------------
def test_enumerations():
    assert len(E.direct_cells()) == 384 and len(set(E.direct_cells())) == 384
    assert len(E.table_forms()) == 16 and len(set(E.table_forms())) == 16
    forms = E.pixel_forms()
    kernels = [f[4] for f in forms]
    assert len(forms) == 28 and len(set(kernels)) == 28
    assert sorted(k for k in kernels if k[0] == "linear") == [("linear", f, p) for f in (0, 1) for p in (0, 1)]
    assert sorted(k for k in kernels if k[0] == "ss") == [("ss", n, f, p) for n in (1, 2, 4, 8) for f in (0, 1, 2) for p in (0, 1)]
    tiled = [f for f in forms if f[3] == 1]
    assert sorted(f[4] for f in tiled) == [("ss", 1, f, p) for f in (0, 1) for p in (0, 1)], "what option pixel_tiled alone reaches"
    assert [f[:3] for f in forms if f[3] == 0] == K.inner_cells()
    for n, lookup, projection, pixel_tiled in E.HOST_PACED_FORMS:
        assert (n, lookup, projection, pixel_tiled) in [f[:4] for f in forms]
    assert {(f[1], f[3]) for f in E.HOST_PACED_FORMS} == {(lookup, t) for lookup in ("nearest", "bilinear") for t in (0, 1)}
    assert {f[2] for f in E.HOST_PACED_FORMS} == set(K.PROJECTIONS)
    assert sorted(E.BATCH_KINDS) == sorted(K.STEPS) and sorted(E.BATCH_KINDS.values()) == sorted(K.KINDS)


def test_enumerations_match_the_dispatch_code():
    """by reading: with_launch_shape's axes, the three launches of direct_kernel, the four of the pixel kernels, the three of either
    table kernel"""
    rh, eh, ke = source("render_host.h"), source("efficient_host.h"), source("kernels_efficient.h")
    body = rh[rh.index("auto with_launch_shape("):rh.index("inline unsigned supersample_log2")]
    assert re.findall(r"case (\d+): return with_ss", body) == ["2", "4", "8"] and "default: return with_ss(std::integral_constant<int, 1>{})" in body
    shapes = set(re.findall(r"LaunchShape<KIND, FAST, SS, (\d), (\d)(, ADAPT)?>", body))
    assert shapes == {(f, p, a) for f in "012" for p in "01" for a in ("", ", ADAPT")}, "3 lookups x 2 projection forms, with and without ADAPT"
    assert "if constexpr (FAST)" in body and "adapt == 2 ? with_adapt(std::integral_constant<int, 2>{}) : with_adapt(std::integral_constant<int, 1>{})" in body
    kinds = rh[rh.index("auto with_kind("):rh.index("auto with_flag(")]
    assert len(re.findall(r"return f\(std::integral_constant<int, cvk::METRIC_", kinds)) == 4
    # 4 kinds x (strict | fast x ADAPT 0, 1, 2) x 4 factors x 3 lookups x 2 projection forms
    assert 4 * (1 + 3) * 4 * 3 * 2 == len(E.direct_cells())
    direct = eh[eh.index("int render_direct_impl("):]
    assert "with_launch_shape(metric->kind, ctx->fast_math != 0, ss, filter, shape.projection, shape.adapt" in direct
    assert re.findall(r"\(direct_kernel<([^>]*)>\)", direct) == ["T::KIND, T::FAST, T::SS, 2, T::PROJ, T::ADAPT", "T::KIND, T::FAST, T::SS, T::FILTER, T::PROJ, T::ADAPT",
                                                                 "T::KIND, T::FAST, T::SS, T::FILTER, T::PROJ"]
    assert "template <int KIND, bool FAST, int SS = 1, int FILTER = 0, int PROJ = 0, int ADAPT = 0>" in ke
    pixel = eh[eh.index("int launch_pixel_kernel("):eh.index("void efficient_statistics(")]
    assert "const bool tiled = ss > 1u || filter == 2u || ctx->pixel_tiled != 0;" in pixel
    assert "with_launch_shape(0, false, ss, filter, projection, false" in pixel
    assert re.findall(r"\((efficient_pixel(?:_ss)?_kernel<[^>]*>)\)", pixel) == [
        "efficient_pixel_ss_kernel<T::SS, 2, T::PROJ>", "efficient_pixel_ss_kernel<T::SS, T::FILTER, T::PROJ>",
        "efficient_pixel_ss_kernel<1, T::FILTER, T::PROJ>", "efficient_pixel_kernel<T::FILTER, T::PROJ>"]
    assert 4 * 1 * 2 + 3 * 2 * 2 + 2 * 2 + 2 * 2 == len(E.pixel_forms())      # mip: 4 factors; factors 2, 4, 8: 2 lookups; tiled; linear
    for kernel in ("escape_angle_kernel", "sampler_kernel"):
        assert re.findall(r"\(%s<([^>]*)>\)" % kernel, eh) == ["KIND, true, 2", "KIND, true, 1", "KIND, FAST"], kernel
        assert "template <int KIND, bool FAST, int ADAPT = 0>\n__global__ __launch_bounds__(%s) void %s(" % ("64" if kernel[0] == "e" else "kSamplerThreads", kernel) in ke
    assert 4 * (1 + 3) == len(E.table_forms())


def test_grids_hold_the_optical_axis_pixel():
    """both fine grids are even in W and H: under the perspective projection the pixel (W / 2, H / 2) looks along the optical axis exactly,
    in every cell and in every frame of the batch.  In frame 0 of the batch, which looks straight at the centre, its rotation axis
    cam_bg x out_bg is an exact zero and normalises to NaN"""
    for grid in (BIG, SMALL):
        assert grid[0] % 2 == 0 and grid[1] % 2 == 0
        for kind in K.KINDS:
            assert E.optical_axis_pixels(kind, "perspective", grid)[0] == 1, (kind, grid)
            pose = E.batch_poses(kind)[0]
            assert E.optical_axis_pixels(kind, "perspective", grid, pose) == (1, 1), (kind, grid)
            alphas, axes, _, _ = E.geometry(kind, "perspective", grid, pose)
            assert alphas[grid[1] // 2, grid[0] // 2] == np.pi and not axes[grid[1] // 2, grid[0] // 2].any(), "looks straight at the centre; the axis is zero"
            for k, pose in enumerate(E.batch_poses(kind)):
                assert E.optical_axis_pixels(kind, "perspective", grid, pose)[0] == 1, (kind, grid, k)
    assert E.BATCH_RES == (37, 19) and (E.BATCH_RES[0] * E.BATCH_RES[1] * 3) % 4 == 1 and (E.BATCH_RES[0] * E.BATCH_RES[1]) % 64 != 0
    for kind in K.KINDS:
        ls = E.batch_radii(kind)
        assert ls[0] == ls[2] != ls[1] and (ls[1] < 0) == (kind in ("ellis", "interstellar")) and abs(ls[1]) <= K.R


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------------
ALPHAS = np.linspace(E.A_MIN, E.A_MAX, 41)


@pytest.mark.parametrize("step", ["fast", "scaled"])
@pytest.mark.parametrize("kind", ["ellis", "interstellar", "flat"])
def test_evaluator_is_step_scale_refs(kind, step):
    S, integrator = K.STEP_WALKS[step]
    assert integrator == 0
    om, _ = E.metrics_of(kind)
    want = SR.evaluator(om, E.camera_radius(kind), K.DELTA, S, K.CAP, K.R)
    f = E.evaluator(kind, step)
    calls, steps = f.calls, f.steps
    codes = set()
    for a in ALPHAS:
        w, g = want(float(a)), f(float(a))
        codes.add(w[0])
        assert w[0] == g[0] and w[2] == g[2], (kind, step, a, w, g)
        if w[0] in (O.POSITIVE, O.NEGATIVE):
            assert float(w[1]).hex() == float(g[1]).hex(), (kind, step, a, w, g)
        else:
            assert g[1] != g[1]
    assert (f.calls - calls, f.steps - steps) == (want.calls, want.steps) and O.POSITIVE in codes
    assert kind == "flat" or O.NEGATIVE in codes


@pytest.mark.parametrize("step", WALK_STEPS)
def test_evaluator_is_schwarzschild_refs(step):
    import schwarzschild_ref as SW
    S, integrator = K.STEP_WALKS[step]
    om, pm = E.metrics_of("schwarzschild")
    assert om is None
    l = E.camera_radius("schwarzschild")
    f = E.evaluator("schwarzschild", step)
    calls = f.calls
    codes = set()
    for a in ALPHAS:
        w, g = SW.compute_escape_angle(pm, l, float(a), K.DELTA, K.CAP, K.R, S, integrator), f(float(a))
        codes.add(w[0])
        assert w[0] == g[0] and w[2] == g[2], (step, a, w, g)
        assert (w[1] != w[1] and g[1] != g[1]) or float(w[1]).hex() == float(g[1]).hex(), (step, a, w, g)
    assert {O.POSITIVE, O.NEGATIVE} <= codes
    assert f.calls - calls == len(ALPHAS) and f(float(ALPHAS[3])) == f(float(ALPHAS[3])) and f.calls - calls == len(ALPHAS) + 2, "a repeated alpha counts again"


@pytest.mark.parametrize("kind", ["ellis", "interstellar", "flat"])
def test_euler_table_is_the_oracles(kind):
    """the table, calls, steps, rounds and the warning of the oracle's own sampler, for the kinds and the step it knows"""
    om, _ = E.metrics_of(kind)
    oc = E.cameras(kind, SMALL, 1, E.aimed_pose(kind, "fast", "perspective", SMALL))[0]
    rgb, smp, st = O.render_image_efficient(O.CV, om, oc, *SR.oracle_skies(), *E.efficient_args())
    t = E.table(kind, "fast")
    for name in "aes":
        assert t[name].tobytes() == np.asarray(smp[name], dtype=np.float64).tobytes(), (kind, name)
    assert E.bookkeeping(t) == (len(smp["a"]), smp["calls"], smp["steps"], smp["rounds"], smp["warned_max_iterations"]), kind
    fine = E.efficient_fine(kind, "fast", "perspective", SMALL, "nearest")       # the cell's aimed pose: the oracle's frame holds its black pixel
    assert fine[1] == (st.rays, st.steps, st.n_pos, st.n_neg, st.n_none, st.n_oob) and np.array_equal(fine[0], rgb)
    assert kind == "flat" or st.n_none >= 1


# ---- the classes of every walk and table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", WALK_STEPS)
@pytest.mark.parametrize("kind", K.KINDS)
def test_tables(kind, step):
    t = E.table(kind, step)
    print(kind, step, "table", E.bookkeeping(t))
    assert t["n"] >= 100 and t["rounds"] >= 2 and t["warned"] == 0 and t["calls"] > E.EFF["n0"]
    assert (np.diff(t["a"]) > 0).all() and np.isfinite(t["e"]).all() and set(t["s"].tolist()) <= {1.0, -1.0}
    assert (t["s"] == 1.0).sum() >= 8
    if kind != "flat":
        assert (t["s"] == -1.0).sum() >= 8
    assert E.table(kind, "strict") is E.table(kind, "fast")
    if step != "fast":
        assert E.table(kind, step)["steps"] != E.table(kind, "fast")["steps"], "the step form changes the table"
    thr = E.device_thresholds(kind, step)
    if thr != E.TIGHT:
        fits = E.table(kind, step, thr=thr)
        print(kind, step, "table at the device sampler's thresholds", thr, E.bookkeeping(fits), fits["peak"])
        assert t["peak"] > E.SAMPLER_CAP >= fits["peak"] and fits["n"] >= 100 and fits["rounds"] >= 2 and fits["warned"] == 0
    if E.BATCH_KINDS.get(step) == kind or (step == "fast" and E.BATCH_KINDS["strict"] == kind):
        other = E.table(kind, step, E.batch_radii(kind)[1])
        print(kind, step, "batch table", E.bookkeeping(other))
        assert other["n"] >= 100 and other["warned"] == 0 and other["a"].tobytes() != t["a"].tobytes()


@pytest.mark.parametrize("projection", K.PROJECTIONS)
@pytest.mark.parametrize("step", WALK_STEPS)
@pytest.mark.parametrize("kind", K.KINDS)
def test_walks_hold_their_classes_and_every_axis_engages(kind, step, projection):
    for renderer, rays_of, fine_of in (("direct", E.direct_rays, E.direct_fine), ("efficient", E.efficient_rays, E.efficient_fine)):
        for grid in (BIG, SMALL):
            rays = rays_of(kind, step, projection, grid)
            print(renderer, kind, step, projection, grid, E.classes(rays), int(rays["steps"].sum()))
            E.assert_classes(rays, kind, renderer, (kind, step, projection, grid))
        nearest, bilinear, mipmap = (fine_of(kind, step, projection, BIG, lookup) for lookup in K.LOOKUPS)
        assert (bilinear[0] != nearest[0]).any(), "the filter engages"
        assert (mipmap[0] != bilinear[0]).any(), "the pyramid engages"
        assert nearest[1][:5] == bilinear[1][:5] == mipmap[1][:5] and nearest[1][0] == BIG[0] * BIG[1] == sum(nearest[1][2:5])
        if step != "fast":
            assert nearest[1][1] != fine_of(kind, "fast", projection, BIG, "nearest")[1][1], "the step form changes the steps"
        assert rays_of(kind, "strict", projection, BIG) is rays_of(kind, "fast", projection, BIG)
        if projection != "perspective":
            assert (nearest[0] != fine_of(kind, step, "perspective", BIG, "nearest")[0]).any(), "the projection engages"
    assert E.efficient_fine(kind, step, projection, BIG, "nearest")[1][1] == E.table(kind, step)["steps"]


@pytest.mark.parametrize("kind", K.KINDS)
def test_everything_at_once_and_equirectangular(kind):
    for renderer, fine_of in (("direct", E.direct_fine), ("efficient", E.efficient_fine)):
        rays = (E.direct_rays if renderer == "direct" else E.efficient_rays)(kind, E.EVERYTHING, "fisheye", K.GRIDS[2])
        E.assert_classes(rays, kind, renderer, (kind, "everything"))
        steps = fine_of(kind, E.EVERYTHING, "fisheye", K.GRIDS[2], "mipmap")[1][1]
        assert steps not in (fine_of(kind, "scaled", "fisheye", K.GRIDS[2], "mipmap")[1][1], fine_of(kind, "heun", "fisheye", K.GRIDS[2], "mipmap")[1][1])
        print(renderer, kind, "equirectangular", E.classes(E.equirectangular_rays(renderer, kind)))
        E.assert_equirectangular_classes(renderer, kind)
        if E.EQUI_GRIDS[kind] == BIG:
            assert (E.equirectangular_cell(renderer, kind)[0] != fine_of(kind, "fast", "fisheye", BIG, "nearest")[0]).any()


@pytest.mark.parametrize("step", K.STEPS)
def test_batch_frames_hold_their_classes(step):
    kind = E.BATCH_KINDS[step]
    for projection in K.PROJECTIONS:
        for grid in (E.BATCH_RES, BIG, SMALL):
            frames = [E.efficient_fine(kind, step, projection, grid, "nearest", pose) for pose in E.batch_poses(kind)]
            print("batch", kind, step, projection, grid, [f[1] for f in frames])
            for k, (rgb, cnt) in enumerate(frames):
                assert cnt[0] == grid[0] * grid[1] == sum(cnt[2:5]) and cnt[2] + cnt[3] >= 8, (kind, step, projection, grid, k, cnt)
            assert frames[0][1][1] == frames[2][1][1] != frames[1][1][1], "frames 0 and 2 share a table, frame 1 has its own"
            assert (frames[0][0] != frames[2][0]).any(), "the frames of the shared table differ"
            if kind in ("ellis", "interstellar"):
                assert frames[1][1][3] >= 8 or frames[1][1][2] >= 8


# ---- the direct loop's cap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", K.STEPS)
def test_caps_beside_the_median_escape(step):
    caps = E.median_caps(step)
    for cap in caps:
        tiles = E.mixed_tiles(step, cap)
        _, cnt, rays = E.capped_cell(step, cap)
        print(step, "cap", cap, "tiles with a ray that escapes in the last iteration and one that does not escape:", tiles, cnt)
        assert len(tiles) >= 1, (step, cap)
        assert cnt[4] >= 1 and cnt[2] + cnt[3] >= 1 and int(rays["steps"].max()) == cap
    for n, lookup, projection in E.CAPPED_EXTRA:
        cnt = E.capped_cell(step, caps[0], n, lookup, projection)[1]
        assert cnt[4] >= 8 and cnt[2] + cnt[3] >= 8, (step, n, lookup, projection, cnt)
    for cap in E.LOW_CAPS:
        _, cnt, rays = E.capped_cell(step, cap)
        assert cnt == (rays["code"].size, cap * rays["code"].size, 0, 0, rays["code"].size, 0), (step, cap, cnt)


# ---- pins: a silent change of the reference shows up ----------------------------------------------------------------------------------------
def crc(frame):
    return zlib.crc32(np.ascontiguousarray(frame).tobytes())


def test_pins():
    got = {
        "table ellis fast": E.bookkeeping(E.table("ellis", "fast")),
        "table interstellar scaled": E.bookkeeping(E.table("interstellar", "scaled")),
        "table schwarzschild heun": E.bookkeeping(E.table("schwarzschild", "heun")),
        "direct ellis fast 1 nearest perspective": (E.direct_cell("ellis", "fast", 1, "nearest", "perspective")[1], crc(E.direct_cell("ellis", "fast", 1, "nearest", "perspective")[0])),
        "direct schwarzschild heun 4 mipmap fisheye": (E.direct_cell("schwarzschild", "heun", 4, "mipmap", "fisheye")[1], crc(E.direct_cell("schwarzschild", "heun", 4, "mipmap", "fisheye")[0])),
        "efficient interstellar scaled 1 bilinear fisheye": (E.efficient_cell("interstellar", "scaled", 1, "bilinear", "fisheye")[1],
                                                             crc(E.efficient_cell("interstellar", "scaled", 1, "bilinear", "fisheye")[0])),
        "efficient flat fast 2 mipmap perspective": (E.efficient_cell("flat", "fast", 2, "mipmap", "perspective")[1], crc(E.efficient_cell("flat", "fast", 2, "mipmap", "perspective")[0])),
        "median caps": tuple(E.median_caps(step) for step in K.STEPS),
    }
    print(got)
    assert got == PINS


# measured when the reference was written
PINS = {
    "table ellis fast": (712, 746, 542284, 18, 0),
    "table interstellar scaled": (1571, 1656, 794311, 26, 0),
    "table schwarzschild heun": (791, 822, 714645, 17, 0),
    "direct ellis fast 1 nearest perspective": ((240, 170954, 222, 18, 0, 0), 4127719932),
    "direct schwarzschild heun 4 mipmap fisheye": ((240, 172589, 205, 35, 0, 0), 3898000556),
    "efficient interstellar scaled 1 bilinear fisheye": ((240, 794311, 208, 28, 4, 0), 2209520725),
    "efficient flat fast 2 mipmap perspective": ((240, 950715, 240, 0, 0, 0), 2681724823),
    "median caps": ((709, 710), (709, 710), (345, 346), (722, 723)),
}
