"""Mip-mapped sky lookup (library option "sky_mipmap"), the parts that need no GPU: the host accessors curvis_sky_mip_rho / _level /
_taps / _mix / _pyramid against the definition in numpy (tests/sky_mipmap_ref.py) on directed inputs; the binary's --sky-mipmap flag,
checked while the command line is parsed; the Python keyword, which accepts a bool only and refuses anything else before a context or a
file is touched; and the host instantiation of the per-ray functions under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import sky_filter_ref as F
import sky_mipmap_ref as M
import curvis_amd
from curvis_amd import _abi, rendering, systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
MESSAGE = "sky_mipmap must be False or True"
U32 = C.POINTER(C.c_uint32)


def u32(*v):
    return (C.c_uint32 * len(v))(*v)


# ---- level -------------------------------------------------------------------------------------------------------------------------
def host_level(rho, L):
    k, f = C.c_uint32(99), C.c_uint32(99)
    assert _abi.lib().curvis_sky_mip_level(int(rho), L, C.byref(k), C.byref(f)) == 0
    return k.value, f.value


def test_level_on_directed_rhos_for_every_pyramid_height():
    rhos = M.directed_rhos()
    assert {0, 255, 256, 257, 511, 512, 2 ** 32 - 1} <= set(rhos) and {256 * 2 ** 9 - 1, 256 * 2 ** 9 + 1} <= set(rhos)
    for L in range(1, 25):
        k, f = M.level(np.array(rhos), L)
        for r, kk, ff in zip(rhos, k.tolist(), f.tolist()):
            assert host_level(r, L) == (kk, ff), (r, L)
            assert kk < L and 0 <= ff < 256 and (kk < L - 1 or ff == 0)
    assert host_level(255, 24) == (0, 0) and host_level(256, 24) == (0, 0) and host_level(257, 24) == (0, 1)
    assert host_level(511, 24) == (0, 255) and host_level(512, 24) == (1, 0) and host_level(2 ** 32 - 1, 24) == (23, 0)
    assert host_level(2 ** 32 - 1, 25) == (23, 255)       # the function is total beyond the heights a sky can have
    assert _abi.lib().curvis_sky_mip_level(300, 0, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == _abi.E_INVALID


# ---- footprint ---------------------------------------------------------------------------------------------------------------------
def host_rho(w, own, hor, ok_h, ver, ok_v):
    out = C.c_uint32(0)
    assert _abi.lib().curvis_sky_mip_rho(w, u32(*own), u32(*hor), int(ok_h), u32(*ver), int(ok_v), C.byref(out)) == 0
    return out.value


def ref_rho(w, own, hor, ok_h, ver, ok_v):
    """one quad through the reference's footprint: a 2 x 2 frame with own at (0, 0); a partner that does not count is capped"""
    which = np.array([[0, 0 if ok_h else -1], [0 if ok_v else -1, -1]])
    Xc = np.array([[own[0], hor[0]], [ver[0], 0]])
    Yc = np.array([[own[1], hor[1]], [ver[1], 0]])
    return int(M.footprint(which, Xc, Yc, [w, w])[0][0, 0])


@pytest.mark.parametrize("w", [1, 2, 13, 16, 1000, 1 << 23])
def test_footprint_wraps_at_exactly_half_the_virtual_width(w):
    fw = 256 * w
    rng = np.random.default_rng(w)
    cases = [((0, 5), (128 * w, 5), (0, 5)), ((128 * w, 5), (0, 5), (128 * w, 5)),          # differences of exactly +-128 w
             ((fw - 1, 0), (0, 0), (fw - 1, 700)), ((0, 0), (fw - 1, 0), (0, 0)),            # across the seam: 1, not 256 w - 1
             ((3, 9), (3 + 128 * w - 1, 9), (3, 9)), ((3, 9), ((3 + 128 * w + 1) % fw, 9), (3, 9))]
    for _ in range(200):
        cases.append(tuple((int(rng.integers(0, fw)), int(rng.integers(0, 256 * 7))) for _ in range(3)))
    for own, hor, ver in cases:
        for ok_h in (0, 1):
            for ok_v in (0, 1):
                assert host_rho(w, own, hor, ok_h, ver, ok_v) == ref_rho(w, own, hor, ok_h, ver, ok_v), (w, own, hor, ver, ok_h, ok_v)
    assert host_rho(w, (0, 5), (128 * w, 5), 1, (0, 5), 1) == 128 * w == host_rho(w, (128 * w, 5), (0, 5), 1, (0, 5), 0)
    assert host_rho(w, (fw - 1, 0), (0, 0), 1, (0, 0), 0) == 1 and host_rho(w, (7, 7), (9, 9), 0, (1, 1), 0) == 0


# ---- pyramid, taps and colour on 1 x 1, 1 x n, n x 1 and odd skies --------------------------------------------------------------------
SIZES = ((1, 1), (2, 2), (3, 2), (13, 7), (16, 5), (1, 37), (37, 1), (33, 77))


def host_pyramid(T):
    h, w = T.shape[:2]
    img = np.ascontiguousarray(T)
    out = []
    for k in range(M.n_levels(w, h)):
        wl, hl = C.c_uint32(), C.c_uint32()
        assert _abi.lib().curvis_sky_mip_pyramid(img.ctypes.data, w, h, k, None, C.byref(wl), C.byref(hl)) == 0
        lv = np.zeros((hl.value, wl.value, 4), np.uint8)
        assert _abi.lib().curvis_sky_mip_pyramid(img.ctypes.data, w, h, k, lv.ctypes.data, C.byref(wl), C.byref(hl)) == 0
        out.append(lv)
    wl, hl = C.c_uint32(), C.c_uint32()
    assert _abi.lib().curvis_sky_mip_pyramid(img.ctypes.data, w, h, len(out), None, C.byref(wl), C.byref(hl)) == _abi.E_INVALID
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_pyramid_taps_and_mix_match_the_definition(size):
    w, h = size
    T = F.texture(w, h, 0x3117)
    want = M.pyramid(T)
    got = host_pyramid(T)
    assert len(got) == len(want) == M.n_levels(w, h) and got[-1].shape[:2] == (1, 1)
    for k, (g, wnt) in enumerate(zip(got, want)):
        assert g.shape == wnt.shape and np.array_equal(g, wnt), (size, k)
    rng = np.random.default_rng(7 * w + h)
    X = np.concatenate([[0, 127, 128, 256 * w - 129, 256 * w - 128, 256 * w - 1], rng.integers(0, 256 * w, 60)])
    Y = np.concatenate([[0, 127, 128, 256 * h - 129, 256 * h - 128, 256 * h - 1], rng.integers(0, 256 * h, 60)])
    rhos = np.array(M.directed_rhos())
    taps, sz = (C.c_uint32 * 6)(), (C.c_uint32 * 2)()
    for x, y in zip(X.tolist(), Y.tolist()):
        for k, lv in enumerate(want):
            assert _abi.lib().curvis_sky_mip_taps(w, h, k, x, y, taps, sz) == 0
            x0, x1, y0, y1, fx, fy, _, _, _ = F.taps(np.array([x >> k]), np.array([y >> k]), lv.shape[1], lv.shape[0])
            assert list(taps) == [int(v[0]) for v in (x0, x1, y0, y1, fx, fy)] and list(sz) == [lv.shape[1], lv.shape[0]], (size, x, y, k)
        # the whole colour: the accessors composed as the definition composes them, against the reference
        want_rgb, ks, fs = M.colour(want, np.full(len(rhos), x), np.full(len(rhos), y), rhos)
        for r, kk, ff, rgb in zip(rhos.tolist(), ks.tolist(), fs.tolist(), want_rgb.tolist()):
            assert host_level(r, len(want)) == (kk, ff)
            cols = []
            for lvl in ((kk, kk + 1) if ff else (kk,)):
                lv = want[lvl]
                assert _abi.lib().curvis_sky_mip_taps(w, h, lvl, x, y, taps, sz) == 0
                t = np.array(list(taps), np.int64)
                c = F.blend(lv, t[0:1], t[1:2], t[2:3], t[3:4], t[4:5], t[5:6])[0].astype(np.uint32)
                cols.append(int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16 | 0xFF000000)
            out = C.c_uint32()
            if ff:
                assert _abi.lib().curvis_sky_mip_mix(cols[0], cols[1], ff, C.byref(out)) == 0
            else:
                out.value = cols[0]
            assert [out.value & 255, (out.value >> 8) & 255, (out.value >> 16) & 255] == rgb, (size, x, y, r)
    assert _abi.lib().curvis_sky_mip_taps(w, h, len(want), 0, 0, taps, sz) == _abi.E_INVALID
    assert _abi.lib().curvis_sky_mip_taps(w, h, 0, 256 * w, 0, taps, sz) == _abi.E_INVALID
    assert _abi.lib().curvis_sky_mip_mix(0, 0, 256, C.byref(C.c_uint32())) == _abi.E_INVALID


def test_odd_sizes_count_the_last_column_twice():
    T = np.zeros((1, 3, 4), np.uint8)
    T[0, :, 0] = (10, 20, 201)
    T[..., 3] = 255
    lv = host_pyramid(T)
    assert [l.shape[:2] for l in lv] == [(1, 3), (1, 2), (1, 1)]
    assert lv[1][0, :, 0].tolist() == [(10 + 20 + 10 + 20 + 2) >> 2, 201] and lv[2][0, 0, 0] == (15 + 201 + 15 + 201 + 2) >> 2


# ---- the binary's flag ----------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("sub", ["image", "video"])
@pytest.mark.parametrize("value", ["1", "0", "On", "true", "off ", ""])
def test_binary_refuses_other_values(sub, value, tmp_path):
    # (the backgrounds do not exist: the flag is refused before anything is opened)
    for spelled in (["--sky-mipmap", value], ["--sky-mipmap=" + value]):
        r = run(sub, tmp_path / "a.png", tmp_path / "b.png", *spelled)
        assert r.returncode == 2, (spelled, r.returncode, r.stderr)
        assert "--sky-mipmap must be on or off" in r.stderr


def test_binary_accepts_the_values_and_lists_the_flag(tmp_path):
    for sub in ("image", "video"):
        for spelled in (["--sky-mipmap", "on"], ["--sky-mipmap", "off"], ["--sky-mipmap=on"], ["--sky-mipmap=off"]):
            r = run(sub, tmp_path / "a.png", tmp_path / "b.png", "--sky-filter", "bilinear", *spelled)
            assert r.returncode == 1 and "sky-mipmap" not in r.stderr, (sub, spelled, r.stderr)   # fails later: the files do not exist
    r = run("image", tmp_path / "a.png", tmp_path / "b.png", "--sky-mipmap")
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "[--sky-mipmap on|off]" in r.stdout


# ---- the Python keyword ----------------------------------------------------------------------------------------------------------
class NoContext:
    """stands where a Context would: any use of it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the context was touched (%s) before the value was checked" % name)


BAD = [1, 0, "on", "True", None, 1.0, b"\x01", np.bool_(True), np.int64(1)]


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_python_keyword_accepts_a_bool_only(bad):
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, 8, 8)
    sky = curvis_amd.SphericalImage(np.zeros((4, 8, 4), np.uint8))
    system = curvis_amd.RelativisticSystem(curvis_amd.EllisMetric(1.0), sky, sky, cam, context=NoContext())
    for call in (lambda: system.render_image(100, 10.0, 0.05, sky_filter="bilinear", sky_mipmap=bad),
                 lambda: system.render_image_efficient(100, 10.0, 0.05, 100, 100, 1e-5, 1e-5, sky_filter="bilinear", sky_mipmap=bad),
                 lambda: system.render_image_direct(100, 10.0, 0.05, sky_filter="bilinear", sky_mipmap=bad)):
        with pytest.raises(ValueError, match=MESSAGE):
            call()
    vs = rendering.VideoRenderingSettings(1.0, 8, 8, 43.0, 15.0, "/nonexistent/path.csv", "/nonexistent/a.png", "/nonexistent/b.png",
                                          "/nonexistent/out")
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem.new(curvis_amd.EllisMetric(1.0), vs, context=NoContext(), sky_mipmap=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 1.0, (8, 8), 43.0, 15.0, 10.0, 100, 0.05,
                                       sky_mipmap=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.ImageRenderingSystem.new(curvis_amd.EllisMetric(1.0), object(), context=NoContext(), sky_mipmap=bad)


def test_python_keyword_defaults_to_false():
    for f in (systems.RelativisticSystem.render_image, systems.RelativisticSystem.render_image_efficient,
              systems.RelativisticSystem.render_image_direct, rendering.ImageRenderingSystem.new, rendering.VideoRenderingSystem.new,
              rendering.ImageRenderingSystem.__init__, rendering.VideoRenderingSystem.__init__):
        assert inspect.signature(f).parameters["sky_mipmap"].default is False, f
    assert systems.check_sky_mipmap(False) == 0 and systems.check_sky_mipmap(True) == 1
    assert inspect.signature(systems._Supersampled.__init__).parameters["sky_mipmap"].default == 0


def test_supersampled_sets_and_restores_the_option():
    class Recorder:
        def __init__(self):
            self.opts = dict(supersample=1, sky_filter=0, projection=0, step_scale=0, integrator=0, sky_mipmap=0)
            self.log = []

        def get_option(self, key):
            return self.opts[key]

        def set_option(self, key, value):
            self.opts[key] = value
            self.log.append((key, value))
    ctx = Recorder()
    with systems._Supersampled(ctx, 1, 1, 0, 0, 0, 1):
        assert ctx.opts["sky_mipmap"] == 1 and ctx.opts["sky_filter"] == 1
    assert ctx.opts["sky_mipmap"] == 0 and ctx.opts["sky_filter"] == 0
    assert ctx.log == [("sky_filter", 1), ("sky_mipmap", 1), ("sky_filter", 0), ("sky_mipmap", 0)]


# ---- the per-ray functions' host instantiation under the sanitizers ----------------------------------------------------------------
def test_per_ray_functions_are_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/san_sky_mipmap.cpp: its own main, cv_device.h compiled for the host with -fsanitize=address,undefined; every gather
    of every level read from a heap block of exactly w_k x h_k texels"""
    exe = tmp_path / "san_sky_mipmap"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_sky_mipmap.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sky mipmap ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
