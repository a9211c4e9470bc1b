"""Camera projections (library option "projection"), the parts that need no GPU: the per-pixel compositions of tests/projection_ref.py
pinned against the oracle's own renders; curvis_camera_outward_vector_projected against the definition in numpy, bit for bit; the
binary's --projection flag, checked while the command line is parsed; the Python keywords, which refuse a bad value before they touch
a context; and the host instantiation of the per-ray functions under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import common
import oracle_lib as O
import projection_ref as P
import curvis_amd
from curvis_amd import _abi, rendering, systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
MESSAGE = "projection must be 'perspective', 'equirectangular' or 'fisheye'"
FLAG_MESSAGE = "--projection must be perspective, equirectangular or fisheye"


# ---- 1. the compositions reproduce the oracle's renders with the perspective vector ------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
def test_compositions_reproduce_the_oracle(kind):
    om, oc = P.scene(kind, (13, 9))[:2]
    sp, sn = (O.sky(np.array(t)) for t in P.index_skies())
    dirs = P.oracle_perspective_world(oc)
    # the numpy definition of projection 0, normalised and rotated in numpy, is cvo_camera_outward_world bit for bit
    assert common.bits(P.outward_vectors(oc, P.PERSPECTIVE)[1]).tobytes() == common.bits(dirs).tobytes()
    want, _, st = O.render_image(O.CV, om, oc, sp, sn, P.CAP, P.R, P.DELTA)
    got, cnt, codes = P.compose_brute(om, oc, dirs, sp, sn, P.CAP, P.R, P.DELTA)
    assert got.tobytes() == want.tobytes() and cnt == tuple(int(getattr(st, k)) for k in P.COUNTERS)
    assert min(cnt[2:5]) >= 1 and (codes == O.NOT_ESCAPED).sum() == cnt[4]
    want, smp, st = O.render_image_efficient(O.CV, om, oc, sp, sn, *P.efficient_args())
    got, cnt, _ = P.compose_efficient(om, oc, dirs, sp, sn, *P.efficient_args())
    assert got.tobytes() == want.tobytes() and cnt == tuple(int(getattr(st, k)) for k in P.COUNTERS) and cnt[1] == smp["steps"]
    assert min(cnt[2:4]) >= 1
    want, st = O.render_image_direct(O.CV, om, oc, sp, sn, P.CAP, P.R, P.DELTA)
    got, cnt, _ = P.compose_direct(om, oc, dirs, sp, sn, P.CAP, P.R, P.DELTA)
    assert got.tobytes() == want.tobytes() and cnt == tuple(int(getattr(st, k)) for k in P.COUNTERS)
    assert min(cnt[2:4]) >= 1


# ---- 2. curvis_camera_outward_vector_projected -----------------------------------------------------------------------------------
def host_vectors(pc, projection, px, py):
    """the ABI function over pixel lists: (camera space [n, 3], world space [n, 3])"""
    f = _abi.lib().curvis_camera_outward_vector_projected
    cs, ws = np.zeros((len(px), 3)), np.zeros((len(px), 3))
    dp = C.POINTER(C.c_double)
    for k in range(len(px)):
        assert f(C.byref(pc._c), projection, int(px[k]), int(py[k]), C.cast(cs.ctypes.data + 24 * k, dp), C.cast(ws.ctypes.data + 24 * k, dp)) == 0
    return cs, ws


SIZES = [((1, 1), 1), ((2, 1), 1), ((13, 9), 1), ((21, 15), 1), ((64, 32), 1), ((4096, 2048), 97)]


@pytest.mark.parametrize("size,stride", SIZES, ids=lambda s: "%dx%d" % s if isinstance(s, tuple) else None)
def test_outward_vector_projected_is_the_definition(size, stride):
    _, oc, _, pc = P.scene("ellis", size)                # a tilted camera
    idx = np.arange(0, size[0] * size[1], stride)
    px, py = idx % size[0], idx // size[0]
    for projection in (P.PERSPECTIVE, P.EQUIRECTANGULAR, P.FISHEYE):
        want_cs, want_ws = P.outward_vectors(oc, projection, px, py)
        cs, ws = host_vectors(pc, projection, px, py)
        for got, want, name in ((cs, want_cs, "camera space"), (ws, want_ws, "world space")):
            bad = np.nonzero((common.bits(got) != common.bits(want)).any(axis=1))[0]
            assert len(bad) == 0, (P.NAMES[projection], name, size, len(bad), [(int(px[i]), int(py[i]), got[i].tolist(), want[i].tolist()) for i in bad[:3]])
        if projection == P.PERSPECTIVE:
            old_cs, old_ws = np.zeros(3), np.zeros(3)
            for k in range(0, len(px), 7):
                assert _abi.lib().curvis_camera_outward_vector(C.byref(pc._c), int(px[k]), int(py[k]), O._dp(old_cs), O._dp(old_ws)) == 0
                assert common.bits(old_cs).tobytes() == common.bits(cs[k]).tobytes() and common.bits(old_ws).tobytes() == common.bits(ws[k]).tobytes()
        # the Camera mirror's methods
        k = len(px) // 2
        assert pc.outward_vector_on_camera_space(px[k], py[k], projection=P.NAMES[projection]).tobytes() == cs[k].tobytes()
        assert pc.outward_vector_on_world_space_from_x_y(px[k], py[k], projection=P.NAMES[projection]).tobytes() == ws[k].tobytes()
    if size == (21, 15):
        cs, _ = host_vectors(pc, P.FISHEYE, [10], [7])
        assert cs[0].tolist() == [1.0, 0.0, 0.0]


def test_outward_vector_projected_refuses_other_projections():
    pc = P.scene("ellis", (8, 8))[3]
    out = np.zeros(3)
    for bad in (3, -1, 1 << 20):
        assert _abi.lib().curvis_camera_outward_vector_projected(C.byref(pc._c), bad, 0, 0, O._dp(out), None) == _abi.E_INVALID
    assert _abi.lib().curvis_camera_outward_vector_projected(None, 0, 0, 0, O._dp(out), None) == _abi.E_INVALID
    assert inspect.signature(pc.outward_vector_on_camera_space).parameters["projection"].default == "perspective"
    assert inspect.signature(pc.outward_vector_on_world_space_from_x_y).parameters["projection"].default == "perspective"
    with pytest.raises(ValueError, match=MESSAGE):
        pc.outward_vector_on_camera_space(0, 0, projection="pano")


# ---- 3. the binary's flag --------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("sub", ["image", "video"])
@pytest.mark.parametrize("value", ["pano", "0", "Fisheye", ""])
def test_binary_refuses_other_values(sub, value, tmp_path):
    # (the backgrounds do not exist: the flag is refused before anything is opened)
    for spelled in (["--projection", value], ["--projection=" + value]):
        r = run(sub, tmp_path / "a.png", tmp_path / "b.png", *spelled)
        assert r.returncode == 2, (spelled, r.returncode, r.stderr)
        assert FLAG_MESSAGE in r.stderr


def test_binary_accepts_the_values_and_lists_the_flag(tmp_path):
    for sub in ("image", "video"):
        for value in P.NAMES:
            for spelled in (["--projection", value], ["--projection=" + value]):
                r = run(sub, tmp_path / "a.png", tmp_path / "b.png", *spelled)
                assert r.returncode == 1 and "projection" not in r.stderr, (sub, spelled, r.stderr)   # fails later: the files do not exist
    r = run("image", tmp_path / "a.png", tmp_path / "b.png", "--projection")
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "[--projection perspective|equirectangular|fisheye]" in r.stdout


# ---- 4. Python keywords ------------------------------------------------------------------------------------------------------------
class NoContext:
    """stands where a Context would: any use of it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the context was touched (%s) before the value was checked" % name)


BAD = ["pano", "0", "Fisheye", "", 0, 1, 2, True, None, b"fisheye"]


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_python_keywords_refuse_other_values(bad):
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, 8, 8)
    sky = curvis_amd.SphericalImage(np.zeros((4, 8, 4), np.uint8))
    system = curvis_amd.RelativisticSystem(curvis_amd.EllisMetric(1.0), sky, sky, cam, context=NoContext())
    for call in (lambda: system.render_image(100, 10.0, 0.05, projection=bad),
                 lambda: system.render_image_efficient(100, 10.0, 0.05, 100, 100, 1e-5, 1e-5, projection=bad),
                 lambda: system.render_image_direct(100, 10.0, 0.05, projection=bad)):
        with pytest.raises(ValueError, match=MESSAGE):
            call()
    # the rendering systems check the value before they read a file or create a context (the settings name files that do not exist)
    vs = rendering.VideoRenderingSettings(1.0, 8, 8, 43.0, 15.0, "/nonexistent/path.csv", "/nonexistent/a.png", "/nonexistent/b.png",
                                          "/nonexistent/out")
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem.new(curvis_amd.EllisMetric(1.0), vs, context=NoContext(), projection=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 1.0, (8, 8), 43.0, 15.0, 10.0, 100, 0.05,
                                       projection=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.ImageRenderingSystem.new(curvis_amd.EllisMetric(1.0), object(), context=NoContext(), projection=bad)


def test_python_keywords_default_to_perspective():
    for f in (systems.RelativisticSystem.render_image, systems.RelativisticSystem.render_image_efficient,
              systems.RelativisticSystem.render_image_direct, rendering.ImageRenderingSystem.new, rendering.VideoRenderingSystem.new,
              rendering.ImageRenderingSystem.__init__, rendering.VideoRenderingSystem.__init__):
        assert inspect.signature(f).parameters["projection"].default == "perspective", f
    assert [systems.check_projection(n) for n in P.NAMES] == [0, 1, 2]


# ---- 5. the per-ray functions' host instantiation under the sanitizers -------------------------------------------------------------
def test_per_ray_functions_are_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/san_projection.cpp: its own main, cv_device.h and cv_efficient.h compiled for the host with
    -fsanitize=address,undefined; camera_pixel_vector, ray_init and efficient_pixel_geometry over the pixels of every size above, all
    projections"""
    exe = tmp_path / "san_projection"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_projection.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "projection ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
