"""Distance-scaled Euler steps (library option "step_scale"), the parts that need no GPU: the compositions of tests/step_scale_ref.py with
S = 0 pinned against the oracle's own entry points, bit for bit; curvis_step_delta against the definition in Python doubles; whole rays
walked with curvis_step_delta + curvis_update_relativistic_object to the composed reference's final state; the ray classes every case of
tests/test_gpu_step_scale.py relies on, asserted from the composed reference alone, so that an unsuitable scene is found without a GPU;
the binary's --step-scale flag and the Python keyword; and step_delta with the host accessor's body under AddressSanitizer and UBSan in
a stand-alone program."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import common
import oracle_lib as O
import projection_ref as P
import ref_compose as RC
import step_scale_ref as SR
import curvis_amd
from curvis_amd import _abi, rendering, systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
MESSAGE = "step_scale must be 0 \\(off\\) or a multiple of 1/256 up to 4096"
FLAG_MESSAGE = "--step-scale must be 0 or a multiple of 1/256 up to 4096"
KINDS = ("ellis", "interstellar", "flat")


# ---- 1. with S = 0 the compositions are the oracle's own entry points ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_walk_reproduces_escape_photon(kind):
    om = SR.metrics(kind)[0]
    rng = np.random.default_rng(11)
    w = RC.Walk(RC.OracleStepper(om))
    seen = set()
    for trial in range(60):
        l = float(rng.uniform(-6.0, 6.0)) if kind != "flat" else float(rng.uniform(0.5, 6.0))
        pos = np.array([0.0, l, float(rng.uniform(0.3, 2.8)), float(rng.uniform(-3.0, 3.0))])
        d = rng.normal(size=3)
        cap = 300 if trial % 5 == 0 else 4096
        code, steps, x, p = O.escape_photon(O.CV, om, pos, d, SR.DELTA, cap, SR.R)
        O.lib().cvo_new_photon(O.CV, w.mp, O._dp(pos), O._dp(d), w.xp, w.pp)
        got = w.run(SR.DELTA, 0, 0, cap, SR.R)
        assert got[:2] == (code, steps) and got.plain == steps
        assert common.bits(w.x).tobytes() == common.bits(x).tobytes() and common.bits(w.p).tobytes() == common.bits(p).tobytes()
        seen.add(code)
    assert O.NOT_ESCAPED in seen and O.POSITIVE in seen and (kind == "flat" or O.NEGATIVE in seen)


@pytest.mark.parametrize("kind", KINDS)
def test_escape_angle_reproduces_the_oracle(kind):
    om = SR.metrics(kind)[0]
    l = 3.0
    f = SR.evaluator(om, l, SR.DELTA, 0, 1500, SR.R)
    alphas = np.linspace(-0.1 * np.pi, 1.1 * np.pi, 2001)
    sides = {O.POSITIVE: 0, O.NEGATIVE: 0, O.NOT_ESCAPED: 0, O.PANIC: 0}
    for a in alphas:
        want = O.compute_escape_angle(O.CV, om, l, float(a), SR.DELTA, 1500, SR.R)
        got = f(float(a))
        assert got[0] == want[0] and got[2] == want[2], (kind, a, got, want)
        if want[0] in (O.POSITIVE, O.NEGATIVE):
            assert common.bits(got[1]) == common.bits(want[1]), (kind, a, got, want)
        sides[want[0]] += 1
    assert sides[O.POSITIVE] >= 100 and (kind == "flat" or sides[O.NEGATIVE] >= 100), sides


@pytest.mark.parametrize("kind", ("ellis", "interstellar"))
def test_sample_table_reproduces_the_oracle(kind):
    om = SR.metrics(kind)[0]
    args = (1500, SR.R, SR.EFF["n0"], SR.EFF["maxit"], SR.EFF["t1"], SR.EFF["t2"])
    smp = O.Samples()
    assert O.lib().cvo_doubly_sample(O.CV, C.byref(om), 3.0, SR.DELTA, args[0], args[1], -0.1 * np.pi, 1.1 * np.pi, *args[2:], C.byref(smp)) == 0
    want = [np.ctypeslib.as_array(getattr(smp, k), (smp.n,)).copy() for k in "aes"]
    calls, steps = int(smp.calls), int(smp.steps)
    O.lib().cvo_samples_free(C.byref(smp))
    f = SR.evaluator(om, 3.0, SR.DELTA, 0, *args[:2])
    a, e, s = RC.sample_table(f, *args[2:])
    for got, w in zip((a, e, s), want):
        assert common.bits(got).tobytes() == common.bits(w).tobytes()
    assert (f.calls, f.steps) == (calls, steps)


@pytest.mark.parametrize("kind", ("ellis", "interstellar"))
def test_frames_reproduce_the_oracle(kind):
    om = SR.metrics(kind)[0]
    oc = SR.cameras("facing", (13, 9))[0]
    sp, sn = SR.oracle_skies()
    dirs = SR.world_dirs(oc)
    cap = 1500
    want, wdbg, st = O.render_image(O.CV, om, oc, sp, sn, cap, SR.R, SR.DELTA, debug=True)
    got, cnt, dbg, _, _ = SR.brute(om, oc, dirs, sp, sn, cap, SR.R, SR.DELTA, 0)
    assert got.tobytes() == want.tobytes() and cnt == tuple(int(getattr(st, k)) for k in SR.COUNTERS)
    common.assert_debug_equal(dbg, wdbg)
    eff = (cap, SR.R, SR.DELTA, SR.EFF["n0"], SR.EFF["maxit"], SR.EFF["t1"], SR.EFF["t2"])
    want, smp, st = O.render_image_efficient(O.CV, om, oc, sp, sn, *eff)
    got, cnt, tab, _, _ = SR.efficient(om, oc, dirs, sp, sn, cap, SR.R, SR.DELTA, 0, *eff[3:])
    assert got.tobytes() == want.tobytes() and cnt == tuple(int(getattr(st, k)) for k in SR.COUNTERS)
    assert common.bits(tab[0]).tobytes() == common.bits(smp["a"]).tobytes()
    want, st = O.render_image_direct(O.CV, om, oc, sp, sn, cap, SR.R, SR.DELTA)
    got, cnt, _, _ = SR.direct(om, oc, dirs, sp, sn, cap, SR.R, SR.DELTA, 0)
    assert got.tobytes() == want.tobytes() and cnt == tuple(int(getattr(st, k)) for k in SR.COUNTERS)


# ---- 2. curvis_step_delta is the definition -------------------------------------------------------------------------------------------
def host_step_delta(delta, S, l):
    out = C.c_double(-1.0)
    assert _abi.lib().curvis_step_delta(float(delta), int(S), float(l), C.byref(out)) == 0, (delta, S, l)
    return out.value


def _same(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


@pytest.mark.parametrize("S", [1, 256, 870, 1024, 4097, 1 << 20])
@pytest.mark.parametrize("delta", [0.05, 0.0125, 1.0])
def test_step_delta_directed(S, delta):
    L0 = S / 256.0
    inf, nan = float("inf"), float("nan")
    up, down = float(np.nextafter(L0, inf)), float(np.nextafter(L0, 0.0))
    ls = [0.0, -0.0, L0, -L0, nan, inf, -inf, 5e-324, -2.5e-310, up, down, -up, -down, float(np.nextafter(up, inf)), float(np.nextafter(down, 0.0))]
    for l in ls:
        got, want = host_step_delta(delta, S, l), SR.step_delta(delta, S, l)
        assert _same(got, want), (S, delta, l, got, want)
        assert got >= delta
    # inside L0, at +-0, for NaN and for a subnormal the step is the reference's; far outside it is larger
    for l in (0.0, -0.0, nan, 5e-324, down / 2, -down / 2):
        assert _same(host_step_delta(delta, S, l), delta)
    assert host_step_delta(delta, S, 4.0 * L0 + 1.0) > delta and host_step_delta(delta, S, -inf) == inf
    # one ulp either side of delta: the products |l| kappa around L0 straddle it, and the compare is strict
    k = SR.kappa(delta, S)
    for l in (down, L0, up):
        a = abs(l) * k
        assert _same(host_step_delta(delta, S, l), a if a > delta else delta)
    assert _same(host_step_delta(delta, 0, 123.0), delta)     # off


def test_step_delta_with_an_inexact_kappa():
    # 870 / 256 is exact, 0.05 / (870 / 256) is not: the accessor's kappa is that one rounded quotient
    from fractions import Fraction
    k = SR.kappa(0.05, 870)
    assert Fraction(k) * Fraction(870, 256) != Fraction(0.05)
    for l in (3.4, 3.5, 17.25, -29.999):
        assert _same(host_step_delta(0.05, 870, l), max(abs(l) * k, 0.05))


def test_step_delta_random():
    rng = np.random.default_rng(5)
    n = 100000
    S = rng.integers(1, (1 << 20) + 1, n)
    delta = np.exp(rng.uniform(np.log(1e-4), np.log(10.0), n))
    l = rng.normal(size=n) * np.exp(rng.uniform(-3.0, 8.0, n))
    f = _abi.lib().curvis_step_delta
    out = C.c_double()
    for i in range(n):
        assert f(float(delta[i]), int(S[i]), float(l[i]), C.byref(out)) == 0
        want = SR.step_delta(float(delta[i]), int(S[i]), float(l[i]))
        assert out.value == want, (i, S[i], delta[i], l[i], out.value, want)


def test_step_delta_refusals():
    out = C.c_double(-1.0)
    f = _abi.lib().curvis_step_delta
    for delta, S in ((0.05, -1), (0.05, (1 << 20) + 1), (0.0, 1024), (-0.05, 1024), (float("nan"), 1024)):
        assert f(delta, S, 1.0, C.byref(out)) == _abi.E_INVALID and out.value == -1.0
    assert f(0.05, 1024, 1.0, None) == _abi.E_INVALID


# ---- 3. whole rays through the ABI's two host functions -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", [870, 1024])
def test_host_walk_reaches_the_composed_state(kind, S):
    om, pm = SR.metrics(kind)
    m = pm._c()
    rng = np.random.default_rng(S)
    w = RC.Walk(RC.OracleStepper(om))
    step, upd = _abi.lib().curvis_step_delta, _abi.lib().curvis_update_relativistic_object
    dk = C.c_double()
    both = 0
    for trial in range(12):
        l = float(rng.uniform(-6.0, 6.0)) if kind != "flat" else float(rng.uniform(0.5, 6.0))
        pos = np.array([0.0, l, float(rng.uniform(0.4, 2.7)), float(rng.uniform(-3.0, 3.0))])
        d = rng.normal(size=3)
        O.lib().cvo_new_photon(O.CV, w.mp, O._dp(pos), O._dp(d), w.xp, w.pp)
        x, p = w.x.copy(), w.p.copy()
        code, steps, plain = w.run(SR.DELTA, S, 0, 2000, SR.R)[:3]
        k = 0
        while k < 2000:
            assert step(SR.DELTA, S, float(x[1]), C.byref(dk)) == 0
            assert upd(C.byref(m), O._dp(x), O._dp(p), dk.value) == 0
            k += 1
            if abs(x[1]) > SR.R:
                break
        assert k == steps and common.bits(x).tobytes() == common.bits(w.x).tobytes() and common.bits(p).tobytes() == common.bits(w.p).tobytes()
        both += 0 < plain < steps
    assert both >= 3      # rays that took steps of both kinds


# ---- 4. the scenes of the GPU cases hold the ray classes they are meant to cover ----------------------------------------------------
import gpu_step_scale_cases as CASES  # noqa: E402  (the list both files walk)


@pytest.mark.parametrize("case", CASES.BRUTE, ids=lambda c: c["id"])
def test_brute_cases_hold_their_classes(case):
    SR.assert_brute_classes(case["kind"], case["pose"], case["S"], case.get("res", SR.RES), case.get("cap", 4096), case.get("projection", 0),
                            case.get("skies", "index"), capped=case.get("capped", False), neg=case["kind"] != "flat")


@pytest.mark.parametrize("case", CASES.ANGLE, ids=lambda c: c["id"])
def test_angle_cases_hold_their_classes(case):
    out = SR.expected(case["renderer"], case["kind"], case["pose"], case["S"], case.get("res", SR.RES))
    SR.assert_angle_classes(out[-1], case["kind"])
    assert out[1][2] >= 8 and out[1][3] >= 8, out[1]     # pixels of both skies


# ---- 5. the binary's flag and the Python keyword ---------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("sub", ["image", "video"])
@pytest.mark.parametrize("value", ["0.3", "-1", "4096.5", "abc", "", "nan", "inf", "1/256", "4 ", " 4", "+4", "0x4", "0x1p2"])
def test_binary_refuses_values_off_the_grid(sub, value, tmp_path):
    for spelled in (["--step-scale", value], ["--step-scale=" + value]):
        r = run(sub, tmp_path / "a.png", tmp_path / "b.png", *spelled)
        assert r.returncode == 2, (spelled, r.returncode, r.stderr)
        assert FLAG_MESSAGE in r.stderr


def test_binary_accepts_the_grid_and_lists_the_flag(tmp_path):
    for sub in ("image", "video"):
        for value in ("0", "4", "3.3984375", "0.00390625", "4096", "2.5e0"):
            r = run(sub, tmp_path / "a.png", tmp_path / "b.png", "--step-scale", value)
            assert r.returncode == 1 and "step-scale" not in r.stderr, (sub, value, r.stderr)   # fails later: the files do not exist
    r = run("image", tmp_path / "a.png", tmp_path / "b.png", "--step-scale")
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "[--step-scale L0]" in r.stdout


class NoContext:
    """stands where a Context would: any use of it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the context was touched (%s) before the value was checked" % name)


@pytest.mark.parametrize("bad", [0.3, -1.0, 4096.5, "4", None, True, float("nan"), float("inf"), 1e-3], ids=repr)
def test_python_keyword_refuses_values_off_the_grid(bad):
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, 8, 8)
    sky = curvis_amd.SphericalImage(np.zeros((4, 8, 4), np.uint8))
    system = curvis_amd.RelativisticSystem(curvis_amd.EllisMetric(1.0), sky, sky, cam, context=NoContext())
    for call in (lambda: system.render_image(100, 10.0, 0.05, step_scale=bad),
                 lambda: system.render_image_efficient(100, 10.0, 0.05, 100, 100, 1e-5, 1e-5, step_scale=bad),
                 lambda: system.render_image_direct(100, 10.0, 0.05, step_scale=bad)):
        with pytest.raises(ValueError, match=MESSAGE):
            call()
    vs = rendering.VideoRenderingSettings(1.0, 8, 8, 43.0, 15.0, "/nonexistent/path.csv", "/nonexistent/a.png", "/nonexistent/b.png",
                                          "/nonexistent/out")
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem.new(curvis_amd.EllisMetric(1.0), vs, context=NoContext(), step_scale=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 1.0, (8, 8), 43.0, 15.0, 10.0, 100, 0.05, step_scale=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.ImageRenderingSystem.new(curvis_amd.EllisMetric(1.0), object(), context=NoContext(), step_scale=bad)


def test_python_keyword_defaults_to_off():
    for f in (systems.RelativisticSystem.render_image, systems.RelativisticSystem.render_image_efficient,
              systems.RelativisticSystem.render_image_direct, rendering.ImageRenderingSystem.new, rendering.VideoRenderingSystem.new,
              rendering.ImageRenderingSystem.__init__, rendering.VideoRenderingSystem.__init__):
        assert inspect.signature(f).parameters["step_scale"].default == 0.0, f
    assert [systems.check_step_scale(v) for v in (0, 0.0, 4, 4.0, 3.3984375, 1 / 256, 4096, np.float64(2.5))] == [0, 0, 1024, 1024, 870, 1, 1 << 20, 640]


# ---- 6. step_delta and the accessor's body under the sanitizers -----------------------------------------------------------------------
def test_step_delta_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/san_step_scale.cpp: its own main, cv_device.h compiled for the host with -fsanitize=address,undefined"""
    exe = tmp_path / "san_step_scale"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_step_scale.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "step_scale ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
