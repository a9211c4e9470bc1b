"""The efficient renderer (what `curvis image` / `curvis video` run by default) against the CPU oracle on BOTH of its samplers:
the host-paced one (cv_sampler.h, efficient_host.h) and the device-resident one (sampler_kernel, cv_sampler_dev.h), forced with the
option "device_sampler" -- left alone, a call of fewer than device_sampler_min_frames frames always takes the host-paced path.

Every frame of every call is compared with cvo_render_image_efficient for its own camera: the sample table (alpha, escape angle,
escape space) bit for bit, the sampler's bookkeeping (table size, integrator calls, Euler steps, rounds, the max-iterations
warning), the pixels and the frame's statistics.  Which outcome is right is the oracle's: a call it completes must complete, and
one where it panics must raise CURVIS_E_SAMPLING, on both paths.  The path a call really took is asserted before anything else,
so that a silent fall-back cannot make the device leg compare the host-paced sampler with the oracle twice."""
import collections
import functools

import numpy as np
import pytest

import common
import oracle_lib as O
import curvis_amd
from curvis_amd import _abi

pytestmark = pytest.mark.gpu

RES = (96, 54)           # even W and H: the optical-axis pixel (alpha = 0, NaN rotation axis) is one of the frame's
R, DELTA = 100.0, 0.05
SAMPLER_CAP = 1536       # cv_sampler_dev.h kSamplerCap: samples a device table may hold
PEND_CAP = 1024          # cv_sampler_dev.h kSamplerPendCap: alpha_nums beyond it never reach the device sampler
OPTIONS = ("device_sampler", "fast_math", "sampling_speculation")

# one render call: metric, the camera radius l of every frame, max_iterations_propagation, alpha_nums, max_iterations_sampling,
# the two convergence thresholds, the fast (1) or strict (0) Euler step
Case = collections.namedtuple("Case", "kind ls cap n0 maxit t1 t2 fast", defaults=(1,))


@functools.lru_cache(maxsize=None)
def _skies():
    return common.make_skies(256, 128, "check")


def _metrics(kind):
    if kind == "ellis":
        return O.ellis(1.0), curvis_amd.EllisMetric(1.0)
    if kind == "interstellar":
        return O.interstellar(0.1, 1e-4, 1.0), curvis_amd.InterstellarMetric(0.1, 1e-4, 1.0)
    return O.flat(), curvis_amd.FlatSphericalMetric()


def _pose(k, l):
    """frame k of a call: at radius l, looking towards the throat, tilted and turned a little more with every k"""
    return (0.0, l, common.HALF_PI + 0.05 * k, 0.3 * k), (-1.0 if l > 0 else 1.0, 0.1 * k, 0.02 * k)


def _cameras(ls):
    return [curvis_amd.Camera(*_pose(k, l), (0.0, 0.0, 1.0), 15.0, 43.0, RES[0], RES[1]) for k, l in enumerate(ls)]


@functools.lru_cache(maxsize=None)
def _oracle_frame(kind, k, l, cap, n0, maxit, t1, t2):
    """(rgb, sample table and bookkeeping, stats) of the oracle, or None where it panics; shared by the two paths' legs"""
    om, _ = _metrics(kind)
    pos, fwd = _pose(k, l)
    oc = O.camera(pos, fwd, (0.0, 0.0, 1.0), 15.0, 43.0, RES)
    sp, sn = _skies()
    try:
        rgb, smp, st = O.render_image_efficient(O.CV, om, oc, O.sky(sp), O.sky(sn), cap, R, DELTA, n0, maxit, t1, t2)
    except RuntimeError:
        return None
    return rgb, smp, (st.rays, st.steps, st.n_pos, st.n_neg, st.n_none, st.n_oob)


def oracle(case):
    return [_oracle_frame(case.kind, k, l, case.cap, case.n0, case.maxit, case.t1, case.t2) for k, l in enumerate(case.ls)]


def check_vs_oracle(ctx, case, device_sampler, expect_path=None, speculation=None, prefetch=(), expect_prefetched=0):
    """Render `case` in ONE call with option "device_sampler" = `device_sampler` and compare every frame with the oracle.
    expect_path: the "last_sampler_path" the call must report (default: `device_sampler`; 2 = the device sampler ran out of room
    and the host-paced one took the call).  prefetch: cases to hand to curvis_ctx_prefetch_efficient first, under the same options.
    Returns the oracle's frames."""
    want = oracle(case)
    _, pm = _metrics(case.kind)
    sp, sn = _skies()
    args = (case.cap, R, DELTA, case.n0, case.maxit, case.t1, case.t2)
    expect_path = device_sampler if expect_path is None else expect_path
    saved = {k: ctx.get_option(k) for k in OPTIONS}
    try:
        ctx.set_sky(0, curvis_amd.SphericalImage(sp))
        ctx.set_sky(1, curvis_amd.SphericalImage(sn))
        ctx.set_option("device_sampler", device_sampler)
        ctx.set_option("fast_math", case.fast)
        if speculation is not None:
            ctx.set_option("sampling_speculation", speculation)
        for p in prefetch:
            ctx.prefetch_efficient(_metrics(p.kind)[1], _cameras(p.ls), p.cap, R, DELTA, p.n0, p.maxit, p.t1, p.t2)
        cams = _cameras(case.ls)
        if case.n0 == 0 or any(w is None for w in want):
            # alpha_nums == 0 is refused before a sampler is chosen (the reference's `0usize - 1` panics; the oracle's C wraps)
            with pytest.raises(curvis_amd.CurvisError) as e:
                ctx.render_efficient(pm, cams, *args)
            if case.n0 > 0:
                assert ctx.get_option("last_sampler_path") == expect_path
            assert e.value.code == _abi.E_SAMPLING, str(e.value)
            return want
        rgb, st = ctx.render_efficient(pm, cams, *args)
        assert ctx.get_option("last_sampler_path") == expect_path
        if expect_path == 1:
            assert ctx.get_option("last_sampling_launches") == 1
            assert ctx.get_option("last_sampling_prefetched") == expect_prefetched
        total = np.zeros(6, np.uint64)
        for f, (w_rgb, w, w_st) in enumerate(want):
            si = ctx.sampling_info(f)
            got = (si.n_samples, si.calls, si.steps, si.rounds, si.warned_max_iterations)
            assert got == (len(w["a"]), w["calls"], w["steps"], w["rounds"], w["warned_max_iterations"]), ("sampling info", f, case.ls[f])
            for name, arr in zip("aes", ctx.samples(f)):
                assert np.array_equal(common.bits(arr), common.bits(w[name])), ("sample table", name, f, case.ls[f])
            bad = np.argwhere((rgb[f] != w_rgb).any(axis=2))
            assert len(bad) == 0, ("pixels", f, case.ls[f], len(bad), bad[:4].tolist())
            fs = ctx.frame_stats(f)
            assert (fs.rays, fs.steps, fs.n_pos, fs.n_neg, fs.n_none, fs.n_oob) == w_st, ("frame statistics", f, case.ls[f])
            total += np.array(w_st, np.uint64)
        assert (st.rays, st.steps, st.n_pos, st.n_neg, st.n_none, st.n_oob) == tuple(int(v) for v in total)
        return want
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


PATHS = [pytest.param(0, None, id="host-sampler"), pytest.param(1, None, id="device-sampler"),
         pytest.param(1, 0, id="device-sampler-no-speculation")]

# the union of test_gpu_parity's device-vs-host cases and test_efficient_twin's hard control-flow settings
HARD = {
    "ellis-radii": Case("ellis", (5.0, 3.0, -2.5, 0.3, 40.0), 4096, 100, 100, 1e-5, 1e-5),
    "interstellar-radii-and-throat": Case("interstellar", (5.0, -4.0, 0.01, 5e-5, -0.5), 8192, 100, 100, 1e-5, 2e-5),
    "interstellar-n0=50-thr=1e-6": Case("interstellar", (-3.0, 2.0), 8192, 50, 100, 1e-6, 1e-5),
    "flat": Case("flat", (5.0, 2.0), 4096, 100, 100, 1e-2, 1e-2),
    "n0=3": Case("ellis", (5.0, 3.0), 4096, 3, 50, 1e-5, 1e-5),
    "cap=2000-nan-samples": Case("ellis", (5.0, 1.0, 7.0), 2000, 100, 100, 1e-5, 1e-5),
    "maxit=0-warned": Case("ellis", (5.0, 2.0), 4096, 100, 0, 1e-5, 1e-5),
    "maxit=1-warned": Case("ellis", (5.0, 2.0), 4096, 100, 1, 1e-5, 1e-5),
    "maxit=3-l=0.3": Case("ellis", (0.3,), 4096, 100, 3, 1e-5, 1e-5),
    "thr=10-refine-nothing": Case("ellis", (5.0, 2.0), 4096, 100, 100, 10.0, 10.0),
    "strict-step-interstellar": Case("interstellar", (3.0, -3.0, 0.2), 8192, 60, 100, 1e-5, 1e-5, 0),
}


@pytest.mark.parametrize("device_sampler,speculation", PATHS)
@pytest.mark.parametrize("name", sorted(HARD))
def test_hard_sampler_settings_vs_oracle(gpu_ctx, name, device_sampler, speculation):
    want = check_vs_oracle(gpu_ctx, HARD[name], device_sampler, speculation=speculation)
    assert all(w is not None for w in want)        # (each of these completes in the oracle)
    if name.endswith("-warned"):
        assert all(w[1]["warned_max_iterations"] == 1 for w in want)


@pytest.mark.parametrize("device_sampler", [0, 1])
@pytest.mark.parametrize("kind", ["ellis", "interstellar"])
def test_tiny_tables_vs_oracle(gpu_ctx, kind, device_sampler):
    """tables of 0, 1 and 2 samples (max_iterations_sampling = 0) reach the per-pixel kernel's n_samples == 0 / == 1 branches, the
    sampler kernel's one-point interpolation table and a two-entry bucket grid; the rows where the oracle panics raise"""
    for n0, cap, maxit, n_want in common.EFF_TINY_TABLES:
        case = Case(kind, (5.0,), cap, n0, maxit, 1e-5, 1e-5)
        want = check_vs_oracle(gpu_ctx, case, device_sampler)
        if n_want is None:
            assert want == [None], case
        else:
            assert len(want[0][1]["a"]) == n_want, case


@pytest.mark.parametrize("device_sampler", [0, 1])
def test_alpha_nums_zero_is_refused(gpu_ctx, device_sampler):
    """compute_uniform_range's `alpha_nums - 1` (src/sampling.rs:133) panics in the reference's default build"""
    for maxit in (0, 100):
        check_vs_oracle(gpu_ctx, Case("ellis", (5.0,), 4096, 0, maxit, 1e-5, 1e-5), device_sampler)


@pytest.mark.parametrize("device_sampler", [0, 1])
@pytest.mark.parametrize("n0,maxit", common.EFF_EXACT_GRID)
def test_grid_points_on_zero_and_pi_vs_oracle(gpu_ctx, n0, maxit, device_sampler):
    """uniform grids with points exactly on alpha = 0.0 (and pi): the optical-axis pixel of a camera that looks straight at the
    throat has alpha = pi (l > 0) or 0.0 (l < 0) and queries a sample abscissa exactly"""
    for l, axis_alpha in ((5.0, np.pi), (-2.5, 0.0)):
        want = check_vs_oracle(gpu_ctx, Case("ellis", (l,), 4096, n0, maxit, 1e-5, 1e-5), device_sampler)
        a = want[0][1]["a"]
        assert 0.0 in a and (axis_alpha in a) == (n0 == 109 or axis_alpha == 0.0), (l, n0, maxit)


@pytest.mark.parametrize("device_sampler", [0, 1])
def test_device_sampler_capacity_edges_vs_oracle(gpu_ctx, device_sampler):
    """the largest grid the device sampler takes, the first it does not (the host-paced sampler runs), and a table that outgrows
    its arrays mid-way (the call falls back to the host-paced sampler: path 2) -- each equal to the oracle"""
    want = check_vs_oracle(gpu_ctx, Case("ellis", (5.0,), 4096, PEND_CAP, 0, 1e-5, 1e-5), device_sampler)
    assert len(want[0][1]["a"]) == PEND_CAP
    check_vs_oracle(gpu_ctx, Case("ellis", (5.0,), 4096, PEND_CAP + 1, 0, 1e-5, 1e-5), device_sampler, expect_path=0)
    want = check_vs_oracle(gpu_ctx, Case("ellis", (5.0, 3.0), 4096, 7, 100, 1e-9, 1e-9), device_sampler, expect_path=2 * device_sampler)
    assert len(want[0][1]["a"]) > SAMPLER_CAP


@pytest.mark.parametrize("device_sampler", [0, 1])
def test_sampler_panics_where_the_oracle_does(gpu_ctx, device_sampler):
    """a refinement round that starts with fewer than 3 finite samples: two grid points, and a cap at which nothing escapes"""
    for case in (Case("ellis", (5.0, 3.0), 4096, 2, 1, 1e-5, 1e-5), Case("ellis", (5.0, 3.0), 10, 100, 100, 1e-5, 1e-5)):
        assert oracle(case) == [None, None]
        check_vs_oracle(gpu_ctx, case, device_sampler)


BATCHES = {   # nine frames, radii repeated (frames share a device job) and on both sides of the throat
    "ellis": Case("ellis", (5.0, 3.0, 3.0, -2.5, 5.0, -2.5, 0.3, 3.0, 40.0), 4096, 100, 100, 1e-5, 1e-5),
    "interstellar": Case("interstellar", (-3.0, 5.0, -3.0, 0.01, 0.01, 2.0, -0.5, 5.0, 2.0), 8192, 100, 100, 1e-5, 2e-5),
}


@pytest.mark.parametrize("device_sampler", [0, 1])
@pytest.mark.parametrize("kind", sorted(BATCHES))
def test_batch_with_repeated_radii_vs_oracle(gpu_ctx, kind, device_sampler):
    check_vs_oracle(gpu_ctx, BATCHES[kind], device_sampler)


def test_prefetched_batches_vs_oracle(gpu_ctx):
    """curvis_ctx_prefetch_efficient for two batches (both slots), then the two calls: each consumes its prefetched tables.  A
    prefetch with alpha_nums < 3 is a no-op: that call samples itself"""
    b0, b1 = BATCHES["interstellar"], BATCHES["ellis"]
    check_vs_oracle(gpu_ctx, b0, 1, prefetch=(b0, b1), expect_prefetched=1)
    check_vs_oracle(gpu_ctx, b1, 1, expect_prefetched=1)
    tiny = Case("ellis", (5.0, 3.0), 1925, 3, 0, 1e-5, 1e-5)
    check_vs_oracle(gpu_ctx, tiny, 1, prefetch=(tiny,), expect_prefetched=1)
    tiny = Case("ellis", (5.0, 3.0), 4096, 2, 0, 1e-5, 1e-5)
    check_vs_oracle(gpu_ctx, tiny, 1, prefetch=(tiny,), expect_prefetched=0)
