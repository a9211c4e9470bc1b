"""Heun's method (library option "integrator" = 1), the parts that need no GPU: the compositions of tests/integrator_ref.py with
integrator = 0 pinned to tests/step_scale_ref.py's, bit for bit; curvis_heun_step against the composition's step on random and
directed states; whole rays walked with curvis_step_delta + curvis_heun_step to the composition's final state; the ray classes every
case of tests/test_gpu_integrator.py relies on, asserted from the composition alone, so that an unsuitable scene is found without a
GPU; the observed order of the method; the binary's --integrator flag and the Python keyword; and the step with the host accessor's
body under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import common
import gpu_integrator_cases as CASES
import integrator_ref as IR
import oracle_lib as O
import ref_compose as RC
import step_scale_ref as SR
import curvis_amd
from curvis_amd import _abi, rendering, systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
MESSAGE = "integrator must be 'euler' or 'heun'"
FLAG_MESSAGE = "--integrator must be euler or heun"
KINDS = ("ellis", "interstellar", "flat")


def same_bits(a, b):
    return common.bits(np.asarray(a, np.float64)).tobytes() == common.bits(np.asarray(b, np.float64)).tobytes()


# ---- 1. with integrator = 0 the compositions are step_scale_ref's -------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 870])
@pytest.mark.parametrize("kind", ("ellis", "interstellar"))
def test_euler_compositions_are_step_scale_refs(kind, S):
    om = SR.metrics(kind)[0]
    oc = SR.cameras("facing", (13, 9))[0]
    sp, sn = SR.oracle_skies()
    dirs = SR.world_dirs(oc)
    brute = (om, oc, dirs, sp, sn, 1500, SR.R, SR.DELTA, S)
    want, got = SR.brute(*brute), SR.brute(*brute, 0)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2].tobytes() == want[2].tobytes()
    assert (got[3] == want[3]).all() and (got[4] == 0).all()
    want, got = SR.direct(*brute), SR.direct(*brute, 0)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    eff = brute + (SR.EFF["n0"], SR.EFF["maxit"], SR.EFF["t1"], SR.EFF["t2"])
    want, got = SR.efficient(*eff), SR.efficient(*eff, 0)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    assert all(same_bits(g, w) for g, w in zip(got[2], want[2]))
    heun = SR.brute(*brute, 1)
    assert heun[1] != want[1] and heun[1][1] != SR.brute(*brute)[1][1]   # and the other walk is another walk


# ---- 2. curvis_heun_step is the composition's step --------------------------------------------------------------------------------------
def heun(m, x, p, delta):
    assert _abi.lib().curvis_heun_step(C.byref(m), O._dp(x), O._dp(p), float(delta)) == 0


def assert_state(x, p, w, what):
    same = (common.bits(x) == common.bits(w.x)) | (np.isnan(x) & np.isnan(w.x))
    assert same.all(), (what, "x", x.tolist(), w.x.tolist())
    same = (common.bits(p) == common.bits(w.p)) | (np.isnan(p) & np.isnan(w.p))
    assert same.all(), (what, "p", p.tolist(), w.p.tolist())


@pytest.mark.parametrize("kind", KINDS)
def test_heun_step_random_states(kind):
    om, pm = SR.metrics(kind)
    m = pm._c()
    w = RC.Walk(RC.OracleStepper(om))
    rng = np.random.default_rng(21)
    strict, outside, beyond, zero = 0, 0, 0, 0
    inner = SR.strict_radius(om)
    for trial in range(4000):
        scale = (0.5, 3.0, 35.0)[trial % 3]
        l = float(rng.normal() * scale)
        if kind == "flat":
            l = abs(l) + 0.05
        theta = float(rng.uniform(-1.0, 4.5)) if trial % 4 == 0 else float(rng.uniform(0.05, 3.09))
        x = np.array([float(rng.normal()), l, theta, float(rng.uniform(-7.0, 7.0))])
        p = np.array([1.0, float(rng.normal()), float(rng.normal() * 3.0), 0.0 if trial % 7 == 0 else float(rng.normal() * 4.0)])
        if trial % 5 == 4:                       # just inside the escape radius and heading out: the stage state lies beyond it
            side = 1.0 if kind == "flat" or trial % 2 else -1.0
            x[1], p[1] = side * float(rng.uniform(29.0, 30.0)), side * (1.0 + abs(p[1]))
            l = float(x[1])
        delta = float(np.exp(rng.uniform(np.log(0.01), np.log(2.0))))
        w.x[:], w.p[:] = x, p
        stage_l = w.heun(delta)
        heun(m, x, p, delta)
        assert_state(x, p, w, (kind, trial))
        strict += inner is not None and abs(l) < inner
        outside += not 0.0 <= theta <= np.pi
        beyond += abs(l) <= SR.R < stage_l
        zero += p[3] == 0.0
    assert outside >= 100 and beyond >= 8 and zero >= 100, (outside, beyond, zero)
    assert kind != "interstellar" or strict >= 100


@pytest.mark.parametrize("kind", KINDS)
def test_heun_step_keeps_the_constants_and_averages_the_time(kind):
    om, pm = SR.metrics(kind)
    m = pm._c()
    x, p = np.array([2.5, 3.0, 1.1, 0.4]), np.array([0.75, -0.9, 0.3, -0.0])
    x0, p0 = x.copy(), p.copy()
    heun(m, x, p, 0.1)
    t2 = (x0[0] + (p0[0] * (1.0 / -1.0)) * 0.1) + (p0[0] * (1.0 / -1.0)) * 0.1
    assert same_bits(x[0], (x0[0] + t2) * 0.5)
    assert same_bits(p[[0, 3]], p0[[0, 3]])                      # -0.0 included: kept, not recomputed
    # the definition from the ABI's own Euler step
    xe, pe = x0.copy(), p0.copy()
    upd = _abi.lib().curvis_update_relativistic_object
    assert upd(C.byref(m), O._dp(xe), O._dp(pe), 0.1) == 0 and upd(C.byref(m), O._dp(xe), O._dp(pe), 0.1) == 0
    assert same_bits(x, (x0 + xe) * 0.5) and same_bits(p[1:3], (p0[1:3] + pe[1:3]) * 0.5)
    assert _abi.lib().curvis_heun_step(None, O._dp(x), O._dp(p), 0.1) == _abi.E_INVALID
    assert _abi.lib().curvis_heun_step(C.byref(m), None, O._dp(p), 0.1) == _abi.E_INVALID


# ---- 3. whole rays through the ABI's two host functions -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", [0, 870, 1024])
def test_host_walk_reaches_the_composed_state(kind, S):
    om, pm = SR.metrics(kind)
    m = pm._c()
    rng = np.random.default_rng(100 + S)
    w = RC.Walk(RC.OracleStepper(om))
    step = _abi.lib().curvis_step_delta
    dk = C.c_double()
    both, escaped = 0, 0
    for trial in range(10):
        l = float(rng.uniform(-6.0, 6.0)) if kind != "flat" else float(rng.uniform(0.5, 3.5))     # flat: mostly inside either L0
        pos = np.array([0.0, l, float(rng.uniform(0.4, 2.7)), float(rng.uniform(-3.0, 3.0))])
        d = rng.normal(size=3)
        O.lib().cvo_new_photon(O.CV, w.mp, O._dp(pos), O._dp(d), w.xp, w.pp)
        x, p = w.x.copy(), w.p.copy()
        code, steps, plain = w.run(IR.DELTA, S, 1, 1000, SR.R)[:3]
        k = 0
        while k < 1000:
            assert step(IR.DELTA, S, float(x[1]), C.byref(dk)) == 0
            heun(m, x, p, dk.value)
            k += 1
            if abs(x[1]) > SR.R:
                break
        assert k == steps, (kind, S, trial, k, steps)
        assert_state(x, p, w, (kind, S, trial))
        both += 0 < plain < steps
        escaped += code in (O.POSITIVE, O.NEGATIVE)
    assert escaped >= 5 and (S == 0 or both >= 3)


# ---- 4. the scenes of the GPU cases hold the ray classes they are meant to cover ----------------------------------------------------
@pytest.mark.parametrize("case", CASES.BRUTE, ids=lambda c: c["id"])
def test_brute_cases_hold_their_classes(case):
    IR.assert_brute_classes(case)


@pytest.mark.parametrize("case", CASES.ANGLE, ids=lambda c: c["id"])
def test_angle_cases_hold_their_classes(case):
    IR.assert_angle_classes(case)


# ---- 5. the method is of second order ---------------------------------------------------------------------------------------------------
# Fixed steps, 16 x 9 rays of the "facing" pose (l = 5, looking at the throat), walked for the same affine parameter LAMBDA = 40 with
# every step size -- far enough to cross the throat and reach |l| ~ 35 -- and compared there: a comparison at the escape test would
# add the overshoot past the radius, which is of first order in delta for either method.  Error of a ray: the angle between the sky
# direction of its final state and that of a Heun run at delta / 16 (of the smaller delta).  The pair 0.2 / 0.1: the median errors
# are 4e-5 .. 3e-4 rad (Heun) and 8e-3 .. 2e-2 rad (Euler), nine orders of magnitude and more above the rounding of a few hundred
# steps (1e-16 each), so truncation decides.  Observed: 2.14 and 2.16 for Heun, 1.01 and 1.24 for Euler (Ellis, Interstellar).
ORDER_PAIR, LAMBDA = (0.2, 0.1), 40.0


@pytest.mark.parametrize("kind", ("ellis", "interstellar"))
def test_observed_order(kind):
    om = SR.metrics(kind)[0]
    oc = SR.cameras("facing", (16, 9))[0]
    dirs = SR.world_dirs(oc)

    def run(delta, integrator):
        n = int(round(LAMBDA / delta))
        codes, out, steps = IR.final_directions(om, oc, dirs, delta, 0, n, 1e30, integrator)
        assert (codes == O.NOT_ESCAPED).all() and (steps == n).all()
        return out
    yard = run(ORDER_PAIR[1] / 16, 1)
    order = {}
    for integrator in (0, 1):
        err = [float(np.median(IR.angles_between(run(d, integrator), yard))) for d in ORDER_PAIR]
        order[integrator] = float(np.log2(err[0] / err[1]))
        print("%s integrator %d: median error %.3e rad at delta %g, %.3e at %g: observed order %.3f" % (
            kind, integrator, err[0], ORDER_PAIR[0], err[1], ORDER_PAIR[1], order[integrator]))
        assert err[1] > 1e-9, "rounding, not truncation"
    assert order[1] > 1.5, order
    assert order[0] < 1.5, order


# ---- 6. the binary's flag and the Python keyword ---------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("sub", ["image", "video", "custom"])
@pytest.mark.parametrize("value", ["Heun", "rk4", "1", "", "heun ", "euler,heun"])
def test_binary_refuses_other_values(sub, value, tmp_path):
    for spelled in (["--integrator", value], ["--integrator=" + value]):
        r = run(sub, tmp_path / "a.png", tmp_path / "b.png", *spelled)
        assert r.returncode == 2, (spelled, r.returncode, r.stderr)
        assert FLAG_MESSAGE in r.stderr


def test_binary_accepts_both_values_and_lists_the_flag(tmp_path):
    for sub in ("image", "video"):
        for value in ("euler", "heun"):
            r = run(sub, tmp_path / "a.png", tmp_path / "b.png", "--integrator", value, "--step-scale", "4")
            assert r.returncode == 1 and "integrator" not in r.stderr, (sub, value, r.stderr)   # fails later: the files do not exist
    r = run("image", tmp_path / "a.png", tmp_path / "b.png", "--integrator")
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "[--integrator euler|heun]" in r.stdout


class NoContext:
    """stands where a Context would: any use of it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the context was touched (%s) before the value was checked" % name)


@pytest.mark.parametrize("bad", ["Heun", "rk4", 1, 0, None, True, b"heun", ""], ids=repr)
def test_python_keyword_refuses_other_values(bad):
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, 8, 8)
    sky = curvis_amd.SphericalImage(np.zeros((4, 8, 4), np.uint8))
    system = curvis_amd.RelativisticSystem(curvis_amd.EllisMetric(1.0), sky, sky, cam, context=NoContext())
    for call in (lambda: system.render_image(100, 10.0, 0.05, integrator=bad),
                 lambda: system.render_image_efficient(100, 10.0, 0.05, 100, 100, 1e-5, 1e-5, integrator=bad),
                 lambda: system.render_image_direct(100, 10.0, 0.05, integrator=bad)):
        with pytest.raises(ValueError, match=MESSAGE):
            call()
    vs = rendering.VideoRenderingSettings(1.0, 8, 8, 43.0, 15.0, "/nonexistent/path.csv", "/nonexistent/a.png", "/nonexistent/b.png",
                                          "/nonexistent/out")
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem.new(curvis_amd.EllisMetric(1.0), vs, context=NoContext(), integrator=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 1.0, (8, 8), 43.0, 15.0, 10.0, 100, 0.05, integrator=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.ImageRenderingSystem.new(curvis_amd.EllisMetric(1.0), object(), context=NoContext(), integrator=bad)


def test_python_keyword_defaults_to_euler():
    for f in (systems.RelativisticSystem.render_image, systems.RelativisticSystem.render_image_efficient,
              systems.RelativisticSystem.render_image_direct, rendering.ImageRenderingSystem.new, rendering.VideoRenderingSystem.new,
              rendering.ImageRenderingSystem.__init__, rendering.VideoRenderingSystem.__init__):
        params = inspect.signature(f).parameters
        assert params["integrator"].default == "euler", f
        assert "step_scale" in params, f                             # wherever step_scale= is accepted
    assert [systems.check_integrator(v) for v in ("euler", "heun")] == [0, 1]
    assert "curvis_heun_step" in _abi.SYMBOLS


# ---- 7. the Heun step and the accessor's body under the sanitizers ---------------------------------------------------------------------
def test_heun_step_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/san_integrator.cpp: its own main, cv_device.h compiled for the host with -fsanitize=address,undefined"""
    exe = tmp_path / "san_integrator"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_integrator.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "integrator ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
