"""Supersampling, the parts that need no GPU: the binary's --supersample flag is checked while the command line is parsed, and the
Python keywords refuse a bad factor before they touch a context."""
import os
import subprocess

import numpy as np
import pytest

import curvis_amd
from curvis_amd import rendering

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "curvis_amd", "bin", "curvis")
MESSAGE = "supersample must be 1, 2, 4 or 8"


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("sub", ["image", "video"])
@pytest.mark.parametrize("value", ["3", "0", "x", "16", "-1", "2.0", ""])
def test_binary_refuses_other_factors(sub, value, tmp_path):
    # (the backgrounds do not exist: the flag is refused before anything is opened)
    for spelled in (["--supersample", value], ["--supersample=" + value]):
        r = run(sub, tmp_path / "a.png", tmp_path / "b.png", *spelled)
        assert r.returncode == 2, (spelled, r.returncode, r.stderr)
        assert "--" + MESSAGE in r.stderr


def test_binary_accepts_the_factors_and_lists_the_flag(tmp_path):
    for value in ("1", "2", "4", "8"):
        r = run("image", tmp_path / "a.png", tmp_path / "b.png", "--supersample", value)
        assert r.returncode == 1 and "background image 1" in r.stderr and "supersample" not in r.stderr, (value, r.stderr)
    r = run("image", tmp_path / "a.png", tmp_path / "b.png", "--supersample")
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "[--supersample 1|2|4|8]" in r.stdout


class NoContext:
    """stands where a Context would: any use of it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the context was touched (%s) before the factor was checked" % name)


BAD = [0, 3, 16, -1, 2.0, "2", None, True]


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_python_keywords_refuse_other_factors(bad):
    cam = curvis_amd.Camera((0.0, 5.0, np.pi / 2, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 15.0, 43.0, 8, 8)
    sky = curvis_amd.SphericalImage(np.zeros((4, 8, 4), np.uint8))
    system = curvis_amd.RelativisticSystem(curvis_amd.EllisMetric(1.0), sky, sky, cam, context=NoContext())
    for call in (lambda: system.render_image(100, 10.0, 0.05, supersample=bad),
                 lambda: system.render_image_efficient(100, 10.0, 0.05, 100, 100, 1e-5, 1e-5, supersample=bad),
                 lambda: system.render_image_direct(100, 10.0, 0.05, supersample=bad)):
        with pytest.raises(ValueError, match=MESSAGE):
            call()
    # the rendering systems check the factor before they read a file or create a context (the settings name files that do not exist)
    vs = rendering.VideoRenderingSettings(1.0, 8, 8, 43.0, 15.0, "/nonexistent/path.csv", "/nonexistent/a.png", "/nonexistent/b.png",
                                          "/nonexistent/out")
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem.new(curvis_amd.EllisMetric(1.0), vs, context=NoContext(), supersample=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.VideoRenderingSystem(curvis_amd.EllisMetric(1.0), NoContext(), None, 1.0, (8, 8), 43.0, 15.0, 10.0, 100, 0.05,
                                       supersample=bad)
    with pytest.raises(ValueError, match=MESSAGE):
        rendering.ImageRenderingSystem.new(curvis_amd.EllisMetric(1.0), object(), context=NoContext(), supersample=bad)


def test_python_keywords_default_to_one():
    import inspect
    from curvis_amd import systems
    for f in (systems.RelativisticSystem.render_image, systems.RelativisticSystem.render_image_efficient,
              systems.RelativisticSystem.render_image_direct, rendering.ImageRenderingSystem.new, rendering.VideoRenderingSystem.new):
        assert inspect.signature(f).parameters["supersample"].default == 1, f
    for good in (1, 2, 4, 8, np.int64(4)):
        assert systems.check_supersample(good) == int(good)
