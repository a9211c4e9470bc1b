"""The disc's emission shift on the host (no GPU): curvis_disc_shift and curvis_disc_shade against the definition in Python doubles
(disc_motion_ref, written from include/curvis_hip.h) bit for bit, the physics of the factor, its accuracy against the closed form at
40 digits, the refusals that need no device, the binary's argument errors, and the two functions under ASan and UBSan."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import disc_motion_ref as DM
import disc_ref as D
import curvis_amd
from curvis_amd import _abi, rendering

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
INF, NAN = math.inf, math.nan
MASSES = (1.0, 0.37, 1.0 / 1024.0, 4096.0)


def metric(mass):
    return curvis_amd.SchwarzschildMetric(mass)._c()


def product(mc, l_hit, l_cam, motion, gain, p_phi):
    F = C.c_double(-1.0)
    assert _abi.lib().curvis_disc_shift(C.byref(mc), float(l_hit), float(l_cam), int(motion), float(gain), float(p_phi), C.byref(F)) == 0
    return F.value


def product_shade(texel, F):
    out = C.c_uint32(0)
    assert _abi.lib().curvis_disc_shade(int(texel), float(F), C.byref(out)) == 0
    return out.value


def same_bits(a, b):
    return (a != a and b != b) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def check(mc, mass, l_hit, l_cam, motion, gain, p_phi):
    want = DM.shift(mc, mass, l_hit, l_cam, motion, gain, p_phi)
    got = product(mc, l_hit, l_cam, motion, gain, p_phi)
    assert same_bits(got, want), (mass, l_hit, l_cam, motion, gain, p_phi, got, want)
    return want


TEXELS = (0xFF000000, 0x80FF01FE, 0xFFFEFF00, 0x8001FE01, 0xFFFFFFFF, 0xC0804020)


def check_shade(F):
    for t in TEXELS:
        got, want = product_shade(t, F), DM.shade(t, F)
        assert got == want and got >> 24 == t >> 24, (hex(t), F, hex(got), hex(want))


def photon_sphere_ls(mc, mass):
    """the doubles l around the photon sphere at which u_e is 1/2 and its two neighbours: {u: l}"""
    l = 2.0 * mass * (1.5 + math.log(0.5))
    for _ in range(256):
        l = np.nextafter(l, -INF)
    found = {}
    for _ in range(512):
        found.setdefault(DM.u_of_l(mc, l), float(l))
        l = np.nextafter(l, INF)
    return found


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", MASSES)
def test_disc_shift_directed(mass):
    mc = metric(mass)
    near = photon_sphere_ls(mc, mass)
    lo, hi = float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.5, 1.0))
    assert 0.5 in near and lo in near and hi in near, sorted(near)
    zero = sat = 0
    for u in (lo, 0.5, hi):
        for sigma in (1, -1):
            for p in (0.0, 3.0 * mass, -5.19 * mass):
                F = check(mc, mass, near[u], 8.0 * mass, sigma, 1.0, p)
                assert (F == 0.0) == (u <= 0.5), "at or inside the photon sphere F = 0; one ulp outside it is not"
                zero += F == 0.0
    for l_hit in (0.0, -0.0, -1.0 * mass, -1e300, 5e-324, 1.7 * mass, 2.0 * mass, 4.0 * mass, 14.0 * mass, 1e6 * mass):
        for l_cam in (8.0 * mass, 0.0, -3.0 * mass, 2.5 * mass, 1e6 * mass):
            for sigma in (1, -1):
                for gain in (1.0, 0.0, 0.25, 4.0, 1e300, 5e-324, 1e-300):
                    for p in (0.0, 4.0 * mass, -4.0 * mass, 1e3 * mass, -1e3 * mass, 1e300, -1e300):
                        F = check(mc, mass, l_hit, l_cam, sigma, gain, p)
                        if l_hit <= 0.0:
                            assert F == 0.0, "l_hit <= 0: the funnel, inside the photon sphere"
                        if gain == 0.0:
                            assert F == 0.0
                        check_shade(F)
                        zero += F == 0.0
                        sat += F > 255.0
    # den driven to 0 and below with an oversized p_phi: p_phi = -sigma / om, its neighbours, twice that
    for l_hit in (1.7 * mass, 3.0 * mass, 10.0 * mass):
        w = 1.0 + DM.u_of_l(mc, l_hit)
        om = DM._div(DM.inv_2m(mass), w * math.sqrt(2.0 * w))
        p = DM._div(1.0, om)
        for _ in range(8):
            p = float(np.nextafter(p, 0.0))
        signs = set()
        for _ in range(16):
            for sigma in (1, -1):
                F = check(mc, mass, l_hit, 8.0 * mass, sigma, 1.0, -sigma * p)
                signs.add(F == 0.0)
                check(mc, mass, l_hit, 8.0 * mass, sigma, 1.0, sigma * p)
            p = float(np.nextafter(p, INF))
        assert signs == {True, False}, "den on both sides of 0"
        assert check(mc, mass, l_hit, 8.0 * mass, 1, 1.0, -2.0 / om) == 0.0
    assert zero > 0 and sat > 0
    # motion 0: the factor that leaves a texel as it is
    assert product(mc, 4.0 * mass, 8.0 * mass, 0, 7.0, 1.0) == 1.0
    for t in TEXELS:
        assert product_shade(t, 1.0) == t


def test_disc_shift_random():
    rng = np.random.default_rng(0xD15C)
    n = 0
    for mass in MASSES:
        mc = metric(mass)
        for _ in range(2500):
            l_hit = mass * float(rng.choice([rng.uniform(-2.0, 30.0), 2.0 ** rng.uniform(-8.0, 20.0), rng.uniform(1.5, 1.75)]))
            l_cam = mass * float(rng.choice([rng.uniform(0.0, 30.0), 2.0 ** rng.uniform(0.0, 20.0)]))
            p = mass * float(rng.choice([rng.uniform(-40.0, 40.0), rng.normal(0.0, 5.0), 2.0 ** rng.uniform(0.0, 24.0)]))
            gain = float(rng.choice([1.0, rng.uniform(0.0, 8.0), 2.0 ** rng.uniform(-30.0, 30.0)]))
            F = check(mc, mass, l_hit, l_cam, int(rng.choice([1, -1])), gain, p)
            t = int(rng.integers(0, 1 << 32))
            assert product_shade(t, F) == DM.shade(t, F), (hex(t), F)
            n += 1
    assert n == 10000


def test_disc_shade_directed():
    lo, hi = float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0))
    for c in (0, 1, 254, 255):
        t = 0x80000000 | c | (c << 8) | (c << 16)
        for F in (0.0, -0.0, 0.5, 1.0, lo, hi, 254.5 / 254.0, 255.0 / 254.0, 254.49, 254.5, 255.0, 1e300, 5e-324, 1e-300, -1.0, INF, -INF, NAN, 0.25, 4.0):
            got, want = product_shade(t, F), DM.shade(t, F)
            assert got == want and got >> 24 == 0x80, (c, F, hex(got), hex(want))
    rng = np.random.default_rng(7)
    for _ in range(20000):
        t, F = int(rng.integers(0, 1 << 32)), float(rng.choice([rng.uniform(0.0, 3.0), 2.0 ** rng.uniform(-12.0, 12.0)]))
        assert product_shade(t, F) == DM.shade(t, F), (hex(t), F)
    # the rule itself: round to nearest with ties up, saturation at 255, alpha kept
    assert DM.shade(0xFF010101, 0.5) == 0xFF010101 and DM.shade(0xFF010101, 0.49) == 0xFF000000
    assert DM.shade(0x80FE00FE, 255.0 / 254.0) == 0x80FF00FF and DM.shade(0x12FFFFFF, 0.0) == 0x12000000


def test_accessors_refuse_null_and_other_kinds():
    L = _abi.lib()
    F, out = C.c_double(0.0), C.c_uint32(0)
    mc = metric(1.0)
    assert L.curvis_disc_shift(None, 4.0, 8.0, 1, 1.0, 0.0, C.byref(F)) == _abi.E_INVALID
    assert L.curvis_disc_shift(C.byref(mc), 4.0, 8.0, 1, 1.0, 0.0, None) == _abi.E_INVALID
    assert L.curvis_disc_shift(C.byref(mc), 4.0, 8.0, 2, 1.0, 0.0, C.byref(F)) == _abi.E_INVALID
    assert L.curvis_disc_shift(C.byref(mc), 4.0, 8.0, -2, 1.0, 0.0, C.byref(F)) == _abi.E_INVALID
    ellis = curvis_amd.EllisMetric(1.0)._c()
    assert L.curvis_disc_shift(C.byref(ellis), 4.0, 8.0, 1, 1.0, 0.0, C.byref(F)) == _abi.E_INVALID
    assert L.curvis_disc_shade(0xFF112233, 1.0, None) == _abi.E_INVALID
    # curvis_ctx_set_disc_motion without a context: refused, nothing dereferenced
    for motion, gain in ((1, 1.0), (0, 1.0), (2, 1.0), (1, -1.0), (1, NAN)):
        assert L.curvis_ctx_set_disc_motion(None, motion, gain) == _abi.E_INVALID


# ---- 2. the physics -------------------------------------------------------------------------------------------------------------------
def r_of(pm, l):
    return pm.radius_of_l(l)


@pytest.mark.parametrize("mass", MASSES)
def test_physics(mass):
    pm = curvis_amd.SchwarzschildMetric(mass)
    mc = pm._c()
    for l_hit in (2.0 * mass, 4.0 * mass, 9.0 * mass, 300.0 * mass):
        for l_cam in (3.0 * mass, 8.0 * mass, 1e4 * mass):
            r_e, r_c = r_of(pm, l_hit), r_of(pm, l_cam)
            # p_phi = 0: g^2 = (1 - 3M/r_e) / (1 - 2M/r_c), for either motion, exactly the same bits
            F1, Fm = product(mc, l_hit, l_cam, 1, 1.0, 0.0), product(mc, l_hit, l_cam, -1, 1.0, 0.0)
            g2 = (1.0 - 3.0 * mass / r_e) / (1.0 - 2.0 * mass / r_c)
            assert F1 == Fm and math.isclose(math.sqrt(F1), g2, rel_tol=1e-12), (l_hit, l_cam, math.sqrt(F1), g2)
            R = r_e / math.sqrt(1.0 - 2.0 * mass / r_e)
            for frac in (0.1, 0.5, 0.99):
                p = frac * R
                # swapping sigma together with the sign of p_phi leaves F unchanged exactly
                assert product(mc, l_hit, l_cam, 1, 1.0, p) == product(mc, l_hit, l_cam, -1, 1.0, -p)
                assert product(mc, l_hit, l_cam, 1, 1.0, -p) == product(mc, l_hit, l_cam, -1, 1.0, p)
                # prograde: p_phi < 0 (matter approaching along the traced, past-directed ray) is brighter than p_phi > 0
                assert product(mc, l_hit, l_cam, 1, 1.0, -p) > F1 > product(mc, l_hit, l_cam, 1, 1.0, p) > 0.0
                # the gain is one multiplication
                assert product(mc, l_hit, l_cam, 1, 4.0, p) == 4.0 * product(mc, l_hit, l_cam, 1, 1.0, p)


# ---- 3. against the closed form at 40 digits -------------------------------------------------------------------------------------------
# profiles/disc_motion_accuracy.txt (tools/disc_motion_accuracy.py, which calls measure_shift_errors below) records, for r_e >= 3.5 M,
# a maximum error of F / G of 8.226 ulp over this sweep; the file is one sample of inputs, the assertion takes twice its figure.
RECORDED_MAX_ULP = 8.226
RE_OVER_M = tuple(3.5 * (2.0 ** 20 / 3.5) ** (k / 23.0) for k in range(24))
RC_OVER_M = (4.0, 6.0, 10.0, 100.0, 65536.0, 2.0 ** 20)
P_FRACTIONS = (0.0, 0.3, -0.3, 0.7, -0.7, 1.0, -1.0)
NEAR_RE_OVER_M = (3.0 + 2.0 ** -40, 3.0 + 2.0 ** -30, 3.0 + 2.0 ** -20, 3.0 + 2.0 ** -10, 3.01, 3.1, 3.25, 3.49)


def exact_r(mp, l, mass):
    """r(l) of the kind at 40 digits: u + ln u = l / 2M - 1, r = 2M (1 + u), for the doubles l and M taken exactly"""
    y = mp.mpf(l) / (2 * mp.mpf(mass)) - 1
    return 2 * mp.mpf(mass) * (1 + mp.lambertw(mp.exp(y)).real)


def measure_shift_errors(re_over_m=RE_OVER_M):
    """{"max": (ulp, mass, r_e/M, r_c/M, fraction, sigma), "by_re": {r_e/M: worst ulp}}: curvis_disc_shift at G = 1 against
    g^4 = ((1 - 3M/r_e) / ((1 - 2M/r_c) (1 + sigma sqrt(M/r_e^3) p_phi)^2))^2 at 40 digits, fed the exact r_e = r(l_hit), r_c = r(l_camera)
    and the double p_phi = fraction * R(r_e)"""
    import mpmath as mp
    mp.mp.dps = 40
    worst, by_re = (0.0,), {}
    for mass in MASSES:
        pm = curvis_amd.SchwarzschildMetric(mass)
        mc = pm._c()
        cams = []
        for rc in RC_OVER_M:
            l_cam = pm.l_of_radius(rc * mass)
            cams.append((rc, l_cam, exact_r(mp, l_cam, mass)))
        for re in re_over_m:
            l_hit = pm.l_of_radius(re * mass)
            r_e = exact_r(mp, l_hit, mass)
            M = mp.mpf(mass)
            if not r_e > 3 * M:
                continue
            R = float(r_e / mp.sqrt(1 - 2 * M / r_e))
            omega = mp.sqrt(M / r_e ** 3)
            for frac in P_FRACTIONS:
                p = frac * R
                for sigma in (1, -1):
                    den = 1 + sigma * omega * mp.mpf(p)
                    if not den > mp.mpf(2) ** -20:      # |p_phi| = R next to r = 3M: the closed form's own pole, not a rounding question
                        continue
                    for rc, l_cam, r_c in cams:
                        exact = ((1 - 3 * M / r_e) / ((1 - 2 * M / r_c) * den ** 2)) ** 2
                        got = product(mc, l_hit, l_cam, sigma, 1.0, p)
                        ulp = float(np.spacing(np.float64(float(exact))))
                        err = float(abs(mp.mpf(got) - exact) / mp.mpf(ulp))
                        by_re[re] = max(by_re.get(re, 0.0), err)
                        if err > worst[0]:
                            worst = (err, mass, re, rc, frac, sigma)
    return {"max": worst, "by_re": by_re}


def test_agrees_with_the_closed_form_at_40_digits():
    w = measure_shift_errors()
    print("max error of F / G for r_e >= 3.5 M: %.3f ulp at (M, r_e/M, r_c/M, fraction of R, sigma) = %r; recorded %.1f" % (w["max"][0], w["max"][1:], RECORDED_MAX_ULP))
    assert len(w["by_re"]) == len(RE_OVER_M)
    assert w["max"][0] <= 2.0 * RECORDED_MAX_ULP, w["max"]


# ---- 4. Python's refusals ---------------------------------------------------------------------------------------------------------------
def test_disc_keywords():
    tex = np.array(D.disc_texture())
    d = curvis_amd.Disc(tex, 1.5, 6.0)
    assert (d.motion, d.gain) == ("static", 1.0)
    d = curvis_amd.Disc(tex, 1.5, 6.0, motion="prograde", gain=4)
    assert (d.motion, d.gain) == ("prograde", 4.0)
    assert curvis_amd.Disc(tex, 1.5, 6.0, "retrograde", 0.0).gain == 0.0
    for kw in (dict(motion="sideways"), dict(motion=1), dict(motion=None), dict(gain=-1.0), dict(gain=NAN), dict(gain=INF), dict(gain="2"), dict(gain=True)):
        with pytest.raises(ValueError):
            curvis_amd.Disc(tex, 1.5, 6.0, **kw)


class NoContext:
    """a context nothing may touch: the refusals below are made before one is used"""

    def __getattr__(self, name):
        raise AssertionError("the context was touched: " + name)


def test_systems_refuse_a_moving_disc_without_a_hole(tmp_path):
    tex = np.array(D.disc_texture())
    moving, static = curvis_amd.Disc(tex, 1.5, 6.0, motion="retrograde"), curvis_amd.Disc(tex, 1.5, 6.0)
    cam = curvis_amd.Camera((0.0, 6.0, 1.25, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, 8, 8)
    sky = curvis_amd.SphericalImage(np.zeros((2, 4, 4), np.uint8))
    for m in (curvis_amd.EllisMetric(1.0), curvis_amd.InterstellarMetric(1.0, 0.5, 1.0), curvis_amd.FlatSphericalMetric()):
        with pytest.raises(ValueError, match="motion"):
            curvis_amd.RelativisticSystem(m, sky, sky, cam, context=NoContext(), disc=moving)
        curvis_amd.RelativisticSystem(m, sky, sky, cam, context=NoContext(), disc=static)
        with pytest.raises(ValueError, match="motion"):
            rendering.VideoRenderingSystem(m, NoContext(), None, 1.0, (8, 8), 43.0, 15.0, 30.0, 100, 0.05, mode="brute", disc=moving)
        st = rendering.ImageRenderingSettings(str(tmp_path / "no.png"), str(tmp_path / "no.png"), str(tmp_path), "a", (0.0, 6.0, 1.25, 0.0),
                                              (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0))
        with pytest.raises(ValueError, match="motion"):      # before the settings' files are opened
            rendering.ImageRenderingSystem.new(m, st, context=NoContext(), mode="brute", disc=moving)
    hole = curvis_amd.SchwarzschildMetric(1.0)
    curvis_amd.RelativisticSystem(hole, sky, None, cam, context=NoContext(), disc=moving)
    rendering.VideoRenderingSystem(hole, NoContext(), None, 1.0, (8, 8), 43.0, 15.0, 30.0, 100, 0.05, mode="brute", disc=moving)


# ---- 5. the binary's flags (parsed before anything is opened) -----------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("sub", ["image", "video"])
def test_binary_flags(sub, tmp_path):
    base = (sub, tmp_path / "a.png", tmp_path / "b.png", "--mode", "brute")
    disc = ("--disc", "d.png", "--disc-inner", "1.5", "--disc-outer", "6")
    for flags in (["--disc-motion", "prograde"], ["--disc-gain", "2"], ["--disc-motion=static", "--disc-gain=1"]):
        r = run(*base, *flags)
        assert r.returncode == 2 and "need --disc" in r.stderr, (flags, r.stderr)
    for flags in (["--disc-motion", "sideways"], ["--disc-motion", "1"], ["--disc-motion", "Prograde"]):
        r = run(*base, *disc, *flags)
        assert r.returncode == 2 and "--disc-motion must be static, prograde or retrograde" in r.stderr, (flags, r.stderr)
    for gain in ("-1", "nan", "inf", "x", "2x"):
        r = run(*base, *disc, "--disc-gain=" + gain)
        assert r.returncode == 2 and "--disc-gain" in r.stderr, (gain, r.stderr)
    assert "--disc-motion" in run("--help").stdout and "--disc-gain" in run("--help").stdout


@pytest.mark.parametrize("sub", ["image", "video"])
def test_binary_refuses_a_motion_without_a_hole(sub, tmp_path):
    from curvis_amd import pngio
    pngio.write_png(tmp_path / "a.png", np.zeros((2, 4, 3), np.uint8))
    (tmp_path / "ellis.toml").write_text("rho = 1.0\n")
    disc = ("--disc", tmp_path / "a.png", "--disc-inner", "1.5", "--disc-outer", "6")
    for metric_args in ((), ("-m", tmp_path / "ellis.toml")):
        r = run(sub, tmp_path / "a.png", tmp_path / "a.png", tmp_path, "--mode", "brute", *disc, "--disc-motion", "prograde", *metric_args)
        assert r.returncode == 2 and "--disc-motion prograde needs a metric file with `mass`" in r.stderr, r.stderr
    # static is today's disc: no such refusal (the run then stops later, for want of a GPU or of settings, with another message)
    r = run(sub, tmp_path / "a.png", tmp_path / "a.png", tmp_path, "--mode", "brute", *disc, "--disc-motion", "static")
    assert "--disc-motion" not in r.stderr, r.stderr


# ---- 6. the two functions under the sanitizers ----------------------------------------------------------------------------------------------
def test_disc_shift_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/san_disc_motion.cpp: its own main, cv_device.h compiled for the host with -fsanitize=address,undefined (the flags
    of tests/sanitize/Makefile, as for san_disc)"""
    exe = tmp_path / "san_disc_motion"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_disc_motion.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "disc motion ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
