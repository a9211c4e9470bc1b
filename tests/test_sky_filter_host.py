"""Bilinear sky filtering (library option "sky_filter"), the parts that need no GPU: curvis_sky_bilinear_taps against the definition in
numpy (tests/sky_filter_ref.py) fed by the oracle's nearest lookup on the 256 times finer sky; the binary's --sky-filter flag, checked
while the command line is parsed; the Python keywords, which refuse a bad value before they touch a context; and the host
instantiation of the two per-ray functions under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sky_filter_ref as F
import curvis_amd
from curvis_amd import _abi, rendering

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
MESSAGE = "sky_filter must be 'nearest' or 'bilinear'"


# ---- curvis_sky_bilinear_taps ------------------------------------------------------------------------------------------------------
def host_taps(w, h, inv, dirs):
    """curvis_sky_bilinear_taps over n directions: (taps [n, 6], raw [n, 2], return codes [n])"""
    f = _abi.lib().curvis_sky_bilinear_taps
    d = np.ascontiguousarray(dirs, dtype=np.float64)
    taps, raw, rc = np.zeros((len(d), 6), np.uint32), np.zeros((len(d), 2), np.uint32), np.zeros(len(d), np.int64)
    dp, u32 = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    inv_p = None if inv is None else np.ascontiguousarray(inv, dtype=np.float64).ctypes.data_as(dp)
    d0, t0, r0 = d.ctypes.data, taps.ctypes.data, raw.ctypes.data
    for i in range(len(d)):
        rc[i] = f(w, h, inv_p, C.cast(d0 + 24 * i, dp), C.cast(t0 + 24 * i, u32), C.cast(r0 + 8 * i, u32))
    return taps, raw, rc


@pytest.mark.parametrize("size", F.SELFTEST_SIZES, ids=lambda s: "%dx%d" % s)
def test_host_taps_match_the_definition(size):
    w, h = size
    rng = np.random.default_rng(4242 + h)
    directed = F.directed_directions()
    for orient in (None, F.ORIENT["B"][0]):
        inv = None if orient is None else F.inverse_rotation(*orient)
        dirs = np.concatenate([directed, F.random_directions(rng, F.N_RANDOM if orient is None else 5000)])
        X, Y = F.oracle_virtual_indices(w, h, inv, dirs)
        x0, x1, y0, y1, fx, fy, tx, ty, oob = F.taps(X, Y, w, h)
        want = np.stack([x0, x1, y0, y1, fx, fy], axis=1)
        taps, raw, rc = host_taps(w, h, inv, dirs)
        bad = np.nonzero((taps != want).any(axis=1) | (raw[:, 0] != tx) | (raw[:, 1] != ty) | ((rc != 0) != oob))[0]
        assert len(bad) == 0, (size, orient, len(bad), [(dirs[i].tolist(), taps[i].tolist(), want[i].tolist(), raw[i].tolist(), int(rc[i]))
                                                        for i in bad[:3]])
        assert set(rc.tolist()) <= {0, _abi.E_INVALID} and oob.any()
        # X >> 8, Y >> 8 are the nearest lookup's raw indices, bit for bit
        x, y = C.c_uint32(0), C.c_uint32(0)
        dp = C.POINTER(C.c_double)
        for i in range(0, len(dirs), 97):
            v = np.ascontiguousarray(dirs[i])
            _abi.lib().curvis_sky_texel_index(w, h, None if inv is None else inv.ctypes.data_as(dp), v.ctypes.data_as(dp), C.byref(x), C.byref(y))
            assert (x.value, y.value) == (int(raw[i, 0]), int(raw[i, 1])), (size, dirs[i].tolist())


def test_host_taps_refuse_oversized_skies_with_outputs_set():
    v = np.array([0.3, -0.4, 0.2])
    for w, h in ((F.MAX_SIDE + 1, 1), (1, F.MAX_SIDE + 1), (2 ** 32 - 1, 7)):
        taps, raw, rc = host_taps(w, h, None, v[None, :])
        x, y = C.c_uint32(0), C.c_uint32(0)
        dp = C.POINTER(C.c_double)
        assert _abi.lib().curvis_sky_texel_index(w, h, None, v.ctypes.data_as(dp), C.byref(x), C.byref(y)) == 0
        assert rc[0] == _abi.E_INVALID and raw[0].tolist() == [x.value, y.value] and not taps.any()
    taps, raw, rc = host_taps(F.MAX_SIDE, F.MAX_SIDE, None, v[None, :])
    assert rc[0] == 0 and (taps[0, :4] < F.MAX_SIDE).all()
    sky = curvis_amd.SphericalImage(np.array(F.real_skies()[0]))
    taps, raw, ok = sky.bilinear_taps_from_vector3((-1.0, 0.0, 0.0))         # the seam on the equator
    assert ok and raw == sky.pixel_index_from_vector3((-1.0, 0.0, 0.0)) and taps[:2] == (12, 0) and taps[4] == 128


# ---- the binary's flag ----------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("sub", ["image", "video"])
@pytest.mark.parametrize("value", ["linear", "0", "1", "Bilinear", "nearest ", ""])
def test_binary_refuses_other_values(sub, value, tmp_path):
    # (the backgrounds do not exist: the flag is refused before anything is opened)
    for spelled in (["--sky-filter", value], ["--sky-filter=" + value]):
        r = run(sub, tmp_path / "a.png", tmp_path / "b.png", *spelled)
        assert r.returncode == 2, (spelled, r.returncode, r.stderr)
        assert "--sky-filter must be nearest or bilinear" in r.stderr


def test_binary_accepts_the_values_and_lists_the_flag(tmp_path):
    for sub in ("image", "video"):
        for spelled in (["--sky-filter", "nearest"], ["--sky-filter", "bilinear"], ["--sky-filter=nearest"], ["--sky-filter=bilinear"]):
            r = run(sub, tmp_path / "a.png", tmp_path / "b.png", *spelled)
            assert r.returncode == 1 and "sky-filter" not in r.stderr, (sub, spelled, r.stderr)   # fails later: the files do not exist
    r = run("image", tmp_path / "a.png", tmp_path / "b.png", "--sky-filter")
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "[--sky-filter nearest|bilinear]" in r.stdout


# ---- Python keywords ------------------------------------------------------------------------------------------------------------
class NoContext:
    """stands where a Context would: any use of it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the context was touched (%s) before the value was checked" % name)


BAD = ["linear", "Bilinear", "", 0, 1, True, None, b"bilinear"]


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_python_keywords_refuse_other_values(bad):
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, 8, 8)
    sky = curvis_amd.SphericalImage(np.zeros((4, 8, 4), np.uint8))
    system = curvis_amd.RelativisticSystem(curvis_amd.EllisMetric(1.0), sky, sky, cam, context=NoContext())
    for call in (lambda: system.render_image(100, 10.0, 0.05, sky_filter=bad),
                 lambda: system.render_image_efficient(100, 10.0, 0.05, 100, 100, 1e-5, 1e-5, sky_filter=bad),
                 lambda: system.render_image_direct(100, 10.0, 0.05, sky_filter=bad)):
        with pytest.raises(ValueError, match=MESSAGE):
            call()
    # the rendering systems check the value before they read a file or create a context (the settings name files that do not exist)
    vs = rendering.VideoRenderingSettings(1.0, 8, 8, 43.0, 15.0, "/nonexistent/path.csv", "/nonexistent/a.png", "/nonexistent/b.png",
                                          "/nonexistent/out")
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem.new(curvis_amd.EllisMetric(1.0), vs, context=NoContext(), sky_filter=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 1.0, (8, 8), 43.0, 15.0, 10.0, 100, 0.05,
                                       sky_filter=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.ImageRenderingSystem.new(curvis_amd.EllisMetric(1.0), object(), context=NoContext(), sky_filter=bad)


def test_python_keywords_default_to_nearest():
    import inspect
    from curvis_amd import systems
    for f in (systems.RelativisticSystem.render_image, systems.RelativisticSystem.render_image_efficient,
              systems.RelativisticSystem.render_image_direct, rendering.ImageRenderingSystem.new, rendering.VideoRenderingSystem.new,
              rendering.ImageRenderingSystem.__init__, rendering.VideoRenderingSystem.__init__):
        assert inspect.signature(f).parameters["sky_filter"].default == "nearest", f
    assert systems.check_sky_filter("nearest") == 0 and systems.check_sky_filter("bilinear") == 1


# ---- the per-ray functions' host instantiation under the sanitizers ----------------------------------------------------------------
def test_per_ray_functions_are_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/san_sky_filter.cpp: its own main, cv_device.h compiled for the host with -fsanitize=address,undefined; every tap
    of every directed direction read from a heap image of exactly w x h texels"""
    exe = tmp_path / "san_sky_filter"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_sky_filter.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sky filter ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
