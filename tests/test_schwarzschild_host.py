"""The Schwarzschild kind (CURVIS_METRIC_SCHWARZSCHILD, include/curvis_hip.h) on the CPU: validation and settings (A1), the metric
functions against mpmath (A2), the shadow's critical angle (A3) and the deflection integral (A4) through the library's host
accessors, and the fast step against the strict one under the sanitizers (A5, a stand-alone program).  The measuring functions are
shared with tools/schwarzschild_accuracy.py, which writes their figures to profiles/schwarzschild_accuracy.txt."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import curvis_amd
from curvis_amd import _abi, settings

import schwarzschild_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
MASSES = (2.0 ** -20, 0.37, 1.0, 1000.0)

# Maximum errors over the sweep of A2, in ulp of the computed value, as recorded in profiles/schwarzschild_accuracy.txt (the sweep is a
# sample: the tests assert twice these; the bound is measured, not derived)
RECORDED_MAX_ULP_R = 3.24
RECORDED_MAX_ULP_RD = 6424.0


def _metric_c(mass, kind=_abi.METRIC_SCHWARZSCHILD):
    return _abi.Metric(kind, 0, 0.0, mass, 0.0)


def functions(mass, l):
    m = _metric_c(mass)
    r, r2, rd, u = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    assert _abi.lib().curvis_metric_functions(C.byref(m), float(l), C.byref(r), C.byref(r2), C.byref(rd)) == 0
    assert _abi.lib().curvis_schwarzschild_u(C.byref(m), float(l), C.byref(u)) == 0
    return r.value, r2.value, rd.value, u.value


# ---- A1 ------------------------------------------------------------------------------------------------------------------------------
def test_validate_accepts_the_kind_iff_mass_is_positive():
    L = _abi.lib()
    for mass, ok in ((1.0, True), (5e-324, True), (1e300, True), (0.0, False), (-0.0, False), (-1.0, False), (float("nan"), False),
                     (float("inf"), True)):
        m = _metric_c(mass)
        m.rho, m.a = -3.0, float("nan")  # ignored
        assert (L.curvis_metric_validate(C.byref(m)) == 0) == ok, mass
    assert L.curvis_metric_validate(C.byref(_metric_c(1.0, 4))) != 0
    assert _abi.METRIC_SCHWARZSCHILD == 3
    assert C.sizeof(_abi.Metric) == 32  # the struct's layout is unchanged


def test_python_class_and_settings_round_trip(tmp_path):
    m = curvis_amd.SchwarzschildMetric(0.37)
    c = m._c()
    assert (c.kind, c.m) == (3, 0.37) and m.mass == 0.37
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            curvis_amd.SchwarzschildMetric(bad)
    assert m.r(3.0) == functions(0.37, 3.0)[0] and m.r_squared(3.0) == functions(0.37, 3.0)[1] and m.r_derivative(3.0) == functions(0.37, 3.0)[2]
    for r in (2.0001 * 0.74, 3 * 0.37, 10.0, 1e6):
        assert math.isclose(m.radius_of_l(m.l_of_radius(r)), r, rel_tol=1e-12), r
    assert math.isclose(m.l_of_radius(3 * 0.37), 0.37 * 2 * (1.5 + math.log(0.5)), rel_tol=1e-15)
    assert math.isclose(m.radius_of_l(-40.0), 0.74 * (1.0 + math.exp(-40.0 / 0.74 - 1.0)), rel_tol=1e-12)
    with pytest.raises(ValueError):
        m.l_of_radius(0.74)
    assert curvis_amd.SchwarzschildMetricSettings is settings.SchwarzschildMetricSettings
    f = tmp_path / "hole.toml"
    f.write_text("mass = 2.5\n")
    s = settings.metric_settings_from_toml_file(str(f))
    assert isinstance(s, settings.SchwarzschildMetricSettings) and s.mass == 2.5
    assert isinstance(s.metric(), curvis_amd.SchwarzschildMetric) and s.metric().mass == 2.5
    # every file the two existing forms read keeps its meaning
    f.write_text("rho = 2.0\nmass = 2.5\n")
    assert isinstance(settings.metric_settings_from_toml_file(str(f)), settings.EllisMetricSettings)
    f.write_text("m = 0.1\na = 0.2\nrho = 2.0\nmass = 2.5\n")
    assert isinstance(settings.metric_settings_from_toml_file(str(f)), settings.InterstellarMetricSettings)
    for text in ("mass = -1.0\n", "mass = \"one\"\n", "m = 1.0\n"):
        f.write_text(text)
        with pytest.raises(settings.SettingsError):
            settings.metric_settings_from_toml_file(str(f))


def test_binary_reads_a_mass_file(tmp_path):
    from curvis_amd import pngio
    a = tmp_path / "a.png"
    pngio.write_png(a, np.zeros((8, 16, 3), np.uint8))
    met = tmp_path / "hole.toml"
    met.write_text("mass = -1.0\n")
    run = lambda *args: subprocess.run([BIN] + [str(v) for v in args], capture_output=True, text=True, timeout=120)  # noqa: E731
    r = run("image", a, a, tmp_path, "-m", met)
    assert r.returncode == 101 and "metric parameters must be positive" in r.stderr, r.stderr  # read as the kind, refused by its validation
    r = run("image", a, tmp_path, "-m", met)  # no -l background: a complete command under this kind
    assert r.returncode == 101 and "metric parameters must be positive" in r.stderr, r.stderr
    ellis = tmp_path / "ellis.toml"
    ellis.write_text("rho = 1.0\n")
    r = run("image", a, "-m", ellis)  # ... and under no other
    assert r.returncode == 2 and "required arguments" in r.stderr, r.stderr
    met.write_text("m = 1.0\n")
    r = run("image", a, a, tmp_path, "-m", met)
    assert r.returncode == 1 and "Could not read the metric configuration file." in r.stderr


def test_walk_ray_is_the_step_accessors_loop():
    """curvis_walk_ray against a loop over curvis_step_delta and the one-step accessors, for the new kind and an old one"""
    L = _abi.lib()
    for pm in (SR.metric(1.0), curvis_amd.EllisMetric(1.0)):
        m = pm._c()
        for S, integ in ((0, 0), (1024, 0), (0, 1), (700, 1)):
            for d in ((-0.9, 0.2, 0.3), (-0.99, 0.05, 0.01), (0.5, 0.5, -0.5)):
                x, p = SR.new_photon(pm, (0.5, 8.0, 1.2, 0.3), d)
                wx, wp = x.copy(), p.copy()
                steps, code = SR.walk(pm, x, p, 0.05, 600, 25.0, S, integ)
                k, wcode = 0, 0
                while k < 600:
                    dk = C.c_double()
                    assert L.curvis_step_delta(0.05, S, wx[1], C.byref(dk)) == 0
                    step = L.curvis_heun_step if integ else L.curvis_update_relativistic_object
                    assert step(C.byref(m), SR._dp(wx), SR._dp(wp), dk.value) == 0
                    k += 1
                    if abs(wx[1]) > 25.0:
                        wcode = 1 if wx[1] > 0 else -1
                        break
                assert (steps, code) == (k, wcode)
                assert np.array_equal(x.view(np.uint64), wx.view(np.uint64)) and np.array_equal(p.view(np.uint64), wp.view(np.uint64))


# ---- A2 ------------------------------------------------------------------------------------------------------------------------------
def sweep_l_over_m():
    """l/M of A2: 0, +-tiny, 2001 points in [0, 6], 1000 log-spaced up to 2^80 -- and the photon sphere itself, 2 (3/2 + log(1/2)), so that
    the minimum of R over the sweep can be held against 3 sqrt(3) M"""
    tiny = [5e-324, -5e-324, 1e-300, -1e-300, 2.0 ** -100, -2.0 ** -100]
    return np.concatenate([[0.0], tiny, np.linspace(0.0, 6.0, 2001), np.logspace(math.log10(6.0), 80 * math.log10(2.0), 1000),
                           [2.0 * (1.5 + math.log(0.5))]])


def exact_functions(mass, l, mp):
    """(u, R, R') at 40 digits for the doubles mass and l >= 0"""
    y = mp.mpf(l) / (2 * mp.mpf(mass)) - 1
    if y < 500:
        u = mp.lambertw(mp.exp(y))
    else:  # e^y is beyond lambertw's comfort: Newton on u + log u = y at working precision, checked by its residual
        u = y - mp.log(y)
        for _ in range(8):
            u = u - (u + mp.log(u) - y) / (1 + 1 / u)
        assert abs(u + mp.log(u) - y) < mp.mpf(10) ** -35 * y
    R = 2 * mp.mpf(mass) * (1 + u) ** mp.mpf(1.5) / mp.sqrt(u)
    return u, R, (2 * u - 1) / (2 * mp.sqrt(u * (1 + u)))


def measure_metric_errors():
    """max ulp error of R and R' over the sweep and the masses: {"R": (ulp, mass, l), "Rd": (...), "min_R_ulp": worst over the masses}"""
    import mpmath as mp
    worst = {"R": (0.0, None, None), "Rd": (0.0, None, None), "min_R_ulp": 0.0}
    with mp.workdps(40):
        for mass in MASSES:
            r_min = math.inf
            for lm in sweep_l_over_m():
                l = float(lm) * mass
                r, r2, rd, u = functions(mass, l)
                _, R, Rd = exact_functions(mass, max(l, 0.0), mp)
                assert r2 == r * r
                eR = float(abs(mp.mpf(r) - R) / mp.mpf(math.ulp(r)))
                eD = float(abs(mp.mpf(rd) - Rd) / mp.mpf(math.ulp(rd))) if rd != 0.0 else float(abs(Rd) / mp.mpf(2.0 ** -54))
                if eR > worst["R"][0]:
                    worst["R"] = (eR, mass, l)
                if eD > worst["Rd"][0]:
                    worst["Rd"] = (eD, mass, l)
                r_min = min(r_min, r)
            e_min = float(abs(mp.mpf(r_min) - 3 * mp.sqrt(3) * mp.mpf(mass)) / mp.mpf(math.ulp(r_min)))
            worst["min_R_ulp"] = max(worst["min_R_ulp"], e_min)
    return worst


def test_metric_functions_against_mpmath():
    w = measure_metric_errors()
    print("max ulp error of R %.3f (M = %r, l = %r), of R' %.3f (M = %r, l = %r); min R against 3 sqrt(3) M: %.3f ulp" % (w["R"] + w["Rd"] + (w["min_R_ulp"],)))
    assert w["R"][0] <= 2 * RECORDED_MAX_ULP_R, w
    assert w["Rd"][0] <= 2 * RECORDED_MAX_ULP_RD, w
    assert w["min_R_ulp"] <= 2 * RECORDED_MAX_ULP_R, w


def test_metric_functions_exact_conditions():
    for mass in MASSES:
        signs = set()
        ls = [float(v) * mass for v in sweep_l_over_m()]
        l_ps = 2.0 * mass * (1.5 + math.log(0.5))
        v = l_ps
        for _ in range(8):
            v = math.nextafter(v, 0.0)
        for _ in range(17):  # the doubles around the photon sphere: u = 1/2 and its neighbours
            ls.append(v)
            v = math.nextafter(v, math.inf)
        for l in ls:
            r, r2, rd, u = functions(mass, l)
            t = 2.0 * u - 1.0
            assert (rd < 0) == (t < 0) and (rd > 0) == (t > 0) and (rd == 0) == (t == 0), (mass, l, rd, u)
            signs.add(-1 if rd < 0 else 1 if rd > 0 else 0)
        assert {-1, 1} <= signs
        at0 = functions(mass, 0.0)
        assert at0[2] < 0.0 and at0[3] < 0.2785
        for l in (-0.0, -5e-324, -1e-300, -1e-9 * mass, -mass, -25.0 * mass, -1e300, -math.inf):
            got = functions(mass, l)
            assert [math.copysign(1, g) for g in got] == [math.copysign(1, g) for g in at0]
            assert np.array_equal(np.array(got).view(np.uint64), np.array(at0).view(np.uint64)), (mass, l)


# ---- A3 ------------------------------------------------------------------------------------------------------------------------------
FAN_SPACING = 1e-11  # the bisection stops when the bracket around the flip is this narrow: the "fan" of alphas around the critical angle
SHADOW_DELTAS = (0.05, 0.025, 0.0125)   # the suite's step (DELTA of the GPU tests) and its halvings, in units of M


def flip_alpha(pm, l, delta, integrator, max_radius, lo, hi):
    """the alpha (convention of compute_escape_angle: from the OUTWARD radial direction) at which the escape side flips from +l to
    capture, bracketed to FAN_SPACING by bisection between lo (escapes) and hi (captured)"""
    def escapes(alpha):
        x, p = SR.new_photon(pm, (0.0, l, SR.HALF_PI, 0.0), (math.cos(alpha), 0.0, math.sin(alpha)))
        steps, code = SR.walk(pm, x, p, delta, 4000000, max_radius, 0, integrator)
        assert code != 0, "a ray of the fan ran into the step cap"
        return code == 1
    assert escapes(lo) and not escapes(hi)
    while hi - lo > FAN_SPACING:
        mid = 0.5 * (lo + hi)
        if escapes(mid):
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def shadow_figures(integrator=1, deltas=SHADOW_DELTAS):
    """per observer radius r/M: (closed form alpha_c, [flip alpha per delta])"""
    pm = SR.metric(1.0)
    out = {}
    for r in (3.5, 6.0, 20.0):
        psi_c = math.asin(3.0 * math.sqrt(3.0) * math.sqrt(1.0 - 2.0 / r) / r)   # from the INWARD radial direction
        alpha_c = math.pi - psi_c
        l = pm.l_of_radius(r)
        out[r] = (alpha_c, [flip_alpha(pm, l, d, integrator, l + 15.0, alpha_c - 0.2, alpha_c + 0.2) for d in deltas])
    return out


def order_check(values, exact, lo, hi, slack):
    d1, d2 = values[0] - values[1], values[1] - values[2]
    return d2 != 0.0 and lo <= d1 / d2 <= hi and abs(values[2] - exact) <= abs(d2) + slack, (d1, d2, d1 / d2 if d2 else math.nan, values[2] - exact)


def test_shadow_critical_angle_converges_at_second_order():
    for r, (alpha_c, flips) in shadow_figures().items():
        ok, figures = order_check(flips, alpha_c, 3.0, 5.0, FAN_SPACING)
        print("r = %g M: alpha_c %.12f, flips %s, differences %.3e %.3e ratio %.3f, finest - closed form %.3e" % ((r, alpha_c, flips) + figures))
        assert ok, (r, alpha_c, flips, figures)


# ---- A4 ------------------------------------------------------------------------------------------------------------------------------
# (b/M, r0/M): three impact parameters, from r = 20 M where that radius is reachable.  A ray of b = 30 M has its periapsis at 28.9 M and never reaches 20 M
# (R(20 M) = 21.1 M < b: no direction at that radius has this impact parameter), so that one starts from 40 M.
DEFLECTION_CASES = ((5.5, 20.0), (8.0, 20.0), (30.0, 40.0))
DEFLECTION_DELTAS = (0.05, 0.025, 0.0125)


def deflection_defects(integrator, deltas=DEFLECTION_DELTAS):
    """per b/M: [swept phi of the stepped ray - the integral over the same two legs (down to the periapsis, out to the radius the
    stepped ray stopped at), per delta]"""
    import mpmath as mp
    pm = SR.metric(1.0)
    out = {}
    with mp.workdps(30):
        for b, r0 in DEFLECTION_CASES:
            l0 = pm.l_of_radius(r0)
            sin_beta = b / pm.r(l0)     # b = p_phi / p_t = R(l0) sin(beta), beta from the radial direction
            beta = math.asin(sin_beta)
            f = lambda r: b / (r * r * mp.sqrt(abs(1 - b * b * (1 - 2 / r) / (r * r))))  # noqa: E731  (abs: the root r_p is rounded)
            r_p = max(mp.polyroots([1, 0, -b * b, 2 * b * b], maxsteps=200, extraprec=80), key=lambda z: mp.re(z)).real
            defects = []
            for d in deltas:
                x, p = SR.new_photon(pm, (0.0, l0, SR.HALF_PI, 0.0), (-math.cos(beta), 0.0, math.sin(beta)))
                steps, code = SR.walk(pm, x, p, d, 4000000, l0 + 15.0, 0, integrator)
                assert code == 1 and math.isclose(p[3], b, rel_tol=1e-14)
                r_end = pm.radius_of_l(x[1])
                exact = mp.quad(f, [r_p, r0]) + mp.quad(f, [r_p, r_end])
                defects.append(float(mp.mpf(x[3]) - exact))
            out[b] = defects
    return out


@pytest.mark.parametrize("integrator,lo,hi", [(1, 3.0, 5.0), (0, 1.6, 2.4)])
def test_deflection_against_the_integral(integrator, lo, hi):
    for b, defects in deflection_defects(integrator).items():
        ok, figures = order_check(defects, 0.0, lo, hi, 1e-11)   # 1e-11: radius_of_l and the quadrature, both good to ~1e-13
        print("b = %g M, %s: defects %s, differences %.3e %.3e ratio %.3f, finest %.3e" % ((b, "Heun" if integrator else "Euler", defects) + figures))
        assert ok, (b, integrator, defects, figures)


# ---- A5 ------------------------------------------------------------------------------------------------------------------------------
def test_fast_step_equals_strict_step_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/san_schwarzschild.cpp: its own main, cv_device.h compiled for the host with -fsanitize=address,undefined"""
    exe = tmp_path / "san_schwarzschild"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_schwarzschild.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "schwarzschild ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
