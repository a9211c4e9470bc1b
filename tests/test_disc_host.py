"""The accretion disc (include/curvis_hip.h, the disc's paragraph), the parts that need no GPU: curvis_disc_crossing -- the host
accessor of cv_device.h disc_crossing, the function the kernels call -- against tests/disc_ref.py on directed and on random inputs, bit
for bit; the reference's composition with no disc pinned to tests/step_scale_ref.py's; the ray counts of the GPU scenes
(disc_ref.SCENE_COUNTS), reproduced by the reference; the refusals of curvis_amd.Disc, RelativisticSystem and the rendering systems
that need no device; the binary's flags; and disc_crossing under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import disc_ref as D
import oracle_lib as O
import step_scale_ref as SR
import curvis_amd
from curvis_amd import _abi, rendering, skies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
TWO_PI = 2.0 * math.pi
INF, NAN = math.inf, math.nan


def product(a, w, h):
    """curvis_disc_crossing: (tx, ty) or None"""
    hit, tx, ty = C.c_int32(-1), C.c_uint32(0), C.c_uint32(0)
    assert _abi.lib().curvis_disc_crossing(*[float(v) for v in a], w, h, C.byref(hit), C.byref(tx), C.byref(ty)) == 0
    assert hit.value in (0, 1)
    return (tx.value, ty.value) if hit.value else None


def check(a, w, h):
    want = D.crossing(*a, w, h)
    got = product(a, w, h)
    assert got == want, (a, w, h, got, want)
    return want


def ulps(v):
    return (v, np.nextafter(v, INF), np.nextafter(v, -INF))


SIZES = ((97, 53), (1, 1), (1 << 23, 1 << 23), (1, 1 << 23), (1 << 23, 1))
TINY = 6.123233995736766e-17          # the cosine of fl(pi / 2)


def directed_inputs():
    """c one ulp either side of a sign change; t at 0 and 1; l_hit one ulp inside and outside each bound; phi_hit at 0, 2 pi +- ulp,
    negative and huge; s < 0; NaN and infinity in every argument"""
    out = []
    cs = [(TINY, -TINY), (-TINY, TINY), (0.3, -0.2), (-0.3, 0.2), (5e-324, -5e-324), (-5e-324, 1.0), (1.0, -5e-324), (1.0, -1.0),
          (0.25, 0.5), (-0.25, -0.5), (0.0, -0.0), (-0.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (-5e-324, 5e-324), (5e-324, 5e-324)]
    phis = [0.0, -0.0, 5e-324] + list(ulps(TWO_PI)) + list(ulps(-TWO_PI)) + [-1.0, 3.0, 1e300, -1e300, 4.0 * TWO_PI, -1e-320]
    for (c0, c1), s, (lin, lout) in itertools.product(cs, (1.0, -1.0, -1e-300), ((1.5, 5.0), (-6.0, -0.8), (-3.0, 4.0), (-1e300, 1e300))):
        for l in list(ulps(lin)) + list(ulps(lout)) + [0.5 * lin + 0.5 * lout]:
            for ph in phis:
                out.append((c0, c1, s, l, l, ph, ph, lin, lout))
        # t = 0 and t = 1 in effect: one cosine dwarfs the other, distinct end points
        out.append((5e-324, -1.0, s, lin, lout, 0.0, 6.0, lin, lout))
        out.append((1.0, -5e-324, s, lin, lout, 0.0, 6.0, lin, lout))
        out.append((0.5, -0.5, s, lin, lout, -1.0, 1.0, lin, lout))
    base = (0.3, -0.2, 1.0, 2.0, 2.5, 1.0, 1.1, 1.5, 5.0)
    for v in (NAN, INF, -INF):
        for i in range(9):
            out.append(base[:i] + (v,) + base[i + 1:])
        out.append((v,) * 9)
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_disc_crossing_directed(size):
    w, h = size
    hits = 0
    for a in directed_inputs():
        hits += check(a, w, h) is not None
    assert hits > 1000


def test_disc_crossing_directed_inputs_reach_every_branch():
    """from the reference alone: both compares of the range test fail and pass, s < 0 shifts the column, the column and the row clamp"""
    w, h = 97, 53
    res = [(a, D.crossing(*a, w, h)) for a in directed_inputs()]
    assert sum(r is None for _, r in res) > 1000 and sum(r is not None for _, r in res) > 1000
    inside = [(a, r) for a, r in res if r is not None]
    assert any(r[0] == w - 1 for _, r in inside) and any(r[1] == h - 1 for _, r in inside) and any(r == (0, 0) for _, r in inside)
    pairs = {}
    for a, r in inside:
        pairs.setdefault(a[:2] + a[3:], {})[a[2] < 0.0] = r
    assert sum(1 for v in pairs.values() if len(v) == 2 and v[True] != v[False]) > 100      # s < 0 moved the texel


def test_disc_crossing_random_1e5():
    rng = np.random.default_rng(20261019)
    n = 100_000
    c0 = rng.uniform(-1, 1, n) * np.exp2(rng.integers(-60, 1, n))
    c1 = -np.sign(c0) * rng.uniform(0, 1, n) * np.exp2(rng.integers(-60, 1, n))
    c1[rng.random(n) < 0.1] *= -1.0                      # a tenth does not cross
    s = rng.uniform(-1, 1, n)
    l0, l1 = rng.uniform(-8, 8, n), rng.uniform(-8, 8, n)
    near = rng.random(n) < 0.5
    l1[near] = l0[near] + rng.uniform(-0.06, 0.06, near.sum())   # steps of the size a render takes
    p0 = rng.uniform(-30, 30, n)
    p1 = p0 + rng.uniform(-0.5, 0.5, n)
    lin = rng.uniform(-7, 6, n)
    lout = lin + rng.uniform(1e-3, 9, n)
    ws, hs = rng.integers(1, 5000, n), rng.integers(1, 5000, n)
    hits = 0
    for i in range(n):
        hits += check((c0[i], c1[i], s[i], l0[i], l1[i], p0[i], p1[i], lin[i], lout[i]), int(ws[i]), int(hs[i])) is not None
    assert 10_000 < hits < 90_000, hits


def test_disc_crossing_refuses_null_and_empty():
    L = _abi.lib()
    hit, tx, ty = C.c_int32(0), C.c_uint32(0), C.c_uint32(0)
    args = [0.3, -0.2, 1.0, 2.0, 2.5, 1.0, 1.1, 1.5, 5.0]
    assert L.curvis_disc_crossing(*args, 0, 5, C.byref(hit), C.byref(tx), C.byref(ty)) == _abi.E_INVALID
    assert L.curvis_disc_crossing(*args, 5, 0, C.byref(hit), C.byref(tx), C.byref(ty)) == _abi.E_INVALID
    assert L.curvis_disc_crossing(*args, 5, 5, None, C.byref(tx), C.byref(ty)) == _abi.E_INVALID
    assert L.curvis_disc_crossing(*args, 5, 5, C.byref(hit), None, C.byref(ty)) == _abi.E_INVALID
    assert L.curvis_disc_crossing(*args, 5, 5, C.byref(hit), C.byref(tx), None) == _abi.E_INVALID
    assert _abi.DISC == D.DISC == 2


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", (0, 1))
@pytest.mark.parametrize("S", (0, 1024))
@pytest.mark.parametrize("name", ("A", "B"))
def test_without_a_disc_the_composition_is_step_scale_refs(name, S, integrator):
    """pinned first: frame, counters and final states, bit for bit (integrator_ref's composition under Heun)"""
    _, om, _, oc, _, _ = D.scene(name, res=(13, 9))
    dirs = SR.world_dirs(oc)
    rays = D.walk_rays(D.OracleStepper(om), oc.pos, dirs, None, D.CAP, D.R, D.DELTA, S, integrator)
    rgb, cnt = D.frame_nearest(rays, None, SR.oracle_skies())
    want = SR.brute(om, oc, dirs, *SR.oracle_skies(), D.CAP, D.R, D.DELTA, S, integrator)
    assert np.array_equal(rgb, want[0])
    assert cnt[:6] == want[1] and cnt[6] == 0
    assert rays["x"].tobytes() == want[2]["x"].tobytes() and rays["p"].tobytes() == want[2]["p"].tobytes()
    assert np.array_equal(rays["steps"], want[2]["steps"]) and np.array_equal(rays["code"], want[2]["code"])


@pytest.mark.parametrize("name", sorted(D.SCENES))
def test_scene_counts(name):
    """disc_ref.SCENE_COUNTS: disc, +l and -l rays, rays that passed a gap and went on, plane crossings with s_k < 0; and of the last
    those inside [l_in, l_out], disc_ref.SCENE_SNEG_IN_RANGE"""
    rays = D.scene_rays(name)
    print(name, D.classes(rays), "in-range s_k < 0 crossings:", int(rays["sneg"].sum()))
    assert D.classes(rays) == D.SCENE_COUNTS[name]
    assert int(rays["sneg"].sum()) == D.SCENE_SNEG_IN_RANGE[name]
    c = D.counters(rays, 0)
    assert c[0] == c[2] + c[3] + c[4] + c[6]
    D.assert_classes(rays, name, sneg_in_range=D.SNEG_IN_RANGE_MIN.get(name, 0))


def test_disc_texture_has_gaps_and_no_colour_of_a_sky():
    t = D.disc_texture()
    assert t.shape == (53, 97, 4) and D.DISC_SALT not in SR.SKY_SALTS
    assert 0.15 < (t[..., 3] == 0).mean() < 0.25 and set(np.unique(t[..., 3])) == {0, 255}


# ---- Python --------------------------------------------------------------------------------------------------------------------------
class NoContext:
    """stands where a Context would: any use of it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the context was touched (%s) before the disc was checked" % name)


IMG = np.zeros((4, 8, 4), np.uint8)


@pytest.mark.parametrize("args", [(np.zeros((4, 8), np.uint8), 1.0, 2.0), (np.zeros((4, 8, 2), np.uint8), 1.0, 2.0),
                                  (np.zeros((4, 8, 4), np.float32), 1.0, 2.0), (np.zeros((0, 8, 4), np.uint8), 1.0, 2.0),
                                  (np.zeros((4, 0, 3), np.uint8), 1.0, 2.0), (IMG, 2.0, 2.0), (IMG, 3.0, 2.0), (IMG, NAN, 2.0),
                                  (IMG, 1.0, INF), (IMG, -INF, 2.0), (IMG, "1", 2.0), (IMG, None, 2.0), (IMG, True, 2.0)], ids=repr)
def test_disc_refuses_what_the_abi_refuses(args):
    with pytest.raises(ValueError):
        curvis_amd.Disc(*args)


def test_disc_accepts_rgb_and_either_sign():
    d = curvis_amd.Disc(np.full((5, 7, 3), 9, np.uint8), -6, -0.8)
    assert d.rgba.shape == (5, 7, 4) and (d.rgba[..., 3] == 255).all() and (d.width_pixels, d.height_pixels) == (7, 5)
    assert (d.l_inner, d.l_outer) == (-6.0, -0.8)
    assert curvis_amd.Disc(IMG, -1.0, 1.0).rgba.dtype == np.uint8


def test_relativistic_system_refuses_the_other_renderers_before_it_touches_the_context():
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, 8, 8)
    sky = curvis_amd.SphericalImage(IMG)
    system = curvis_amd.RelativisticSystem(curvis_amd.EllisMetric(1.0), sky, sky, cam, context=NoContext(), disc=curvis_amd.Disc(IMG, 1.0, 2.0))
    for call in (lambda: system.render_image_efficient(100, 30.0, 0.05, 10, 10, 1e-5, 1e-5), lambda: system.render_image_direct(100, 30.0, 0.05),
                 lambda: system.render_image_debug(100, 30.0, 0.05)):
        with pytest.raises(ValueError, match="a disc is set"):
            call()
    with pytest.raises(ValueError, match="disc must be"):
        curvis_amd.RelativisticSystem(curvis_amd.EllisMetric(1.0), sky, sky, cam, context=NoContext(), disc=IMG)


def test_rendering_systems_require_their_brute_mode():
    disc = curvis_amd.Disc(IMG, 1.0, 2.0)
    for mode in ("efficient", "direct"):
        with pytest.raises(ValueError, match="mode='brute'"):
            rendering.ImageRenderingSystem.new(curvis_amd.EllisMetric(1.0), object(), context=NoContext(), mode=mode, disc=disc)
        with pytest.raises(ValueError, match="mode='brute'"):
            rendering.VideoRenderingSystem.new(curvis_amd.EllisMetric(1.0), object(), context=NoContext(), mode=mode, disc=disc)
        with pytest.raises(ValueError, match="mode='brute'"):
            rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 30, (8, 8), 43.0, 15.0, 30.0, 100, 0.05, mode=mode, disc=disc)
    with pytest.raises(ValueError, match="disc must be"):
        rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 30, (8, 8), 43.0, 15.0, 30.0, 100, 0.05, mode="brute", disc=IMG)
    v = rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 30, (8, 8), 43.0, 15.0, 30.0, 100, 0.05, mode="brute", disc=disc)
    assert v.disc is disc


def test_ring_texture():
    t = skies.ring_texture(256, 32, seed=7)
    assert t.shape == (32, 256, 4) and t.dtype == np.uint8 and np.array_equal(t, skies.ring_texture(256, 32, seed=7))
    assert not np.array_equal(t, skies.ring_texture(256, 32, seed=8))
    lum = t[..., :3].astype(np.int64).sum(axis=2).mean(axis=1)
    assert lum[0] > 2 * lum[-1]                                        # radial brightness falls outwards
    assert t[..., 0].std(axis=1).mean() > 5                            # azimuthal streaks
    gaps = (t[..., 3] == 0).all(axis=1)
    assert set(np.unique(t[..., 3])) <= {0, 255} and (t[..., 3][~gaps] == 255).all()
    assert 1 <= skies.ring_texture(256, 64, seed=7)[..., 3].min(axis=1).tolist().count(0) <= 16       # a few transparent gaps
    curvis_amd.Disc(t, 1.5, 6.0)
    with pytest.raises(ValueError):
        skies.ring_texture(0, 4)


# ---- the binary's flags (parsed before anything is opened) ----------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("sub", ["image", "video"])
def test_binary_wants_all_three_flags_or_none(sub, tmp_path):
    for flags in (["--disc", "d.png"], ["--disc-inner", "1"], ["--disc-outer", "2"], ["--disc", "d.png", "--disc-inner", "1"],
                  ["--disc-inner", "1", "--disc-outer", "2"], ["--disc", "d.png", "--disc-outer=2"]):
        r = run(sub, tmp_path / "a.png", tmp_path / "b.png", "--mode", "brute", *flags)
        assert r.returncode == 2 and "--disc, --disc-inner and --disc-outer are given together" in r.stderr, (flags, r.stderr)
    for inner, outer in (("2", "2"), ("3", "2"), ("nan", "2"), ("1", "inf"), ("x", "2"), ("1", "")):
        r = run(sub, tmp_path / "a.png", tmp_path / "b.png", "--mode", "brute", "--disc", "d.png", "--disc-inner=" + inner, "--disc-outer=" + outer)
        assert r.returncode == 2 and "--disc" in r.stderr, (inner, outer, r.stderr)


@pytest.mark.parametrize("sub", ["image", "video"])
@pytest.mark.parametrize("mode", [[], ["--mode", "efficient"], ["--mode", "direct"]], ids=lambda m: "-".join(m) or "default")
def test_binary_stops_without_mode_brute(sub, mode, tmp_path):
    r = run(sub, tmp_path / "a.png", tmp_path / "b.png", "--disc", "d.png", "--disc-inner", "1.5", "--disc-outer", "6", *mode)
    assert r.returncode != 0 and "--disc needs --mode brute" in r.stderr, r.stderr
    assert "--disc" in run("--help").stdout


# ---- disc_crossing under the sanitizers ----------------------------------------------------------------------------------------------
def test_disc_crossing_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/san_disc.cpp: its own main, cv_device.h compiled for the host with -fsanitize=address,undefined"""
    exe = tmp_path / "san_disc"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_disc.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "disc ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
