"""The moving camera's two functions, cv_device.h camera_boost_prepare and camera_boost, in their host instantiation under
AddressSanitizer and UBSan: a stand-alone program with its own main (tests/sanitize/san_camera_boost.cpp), compiled and run here.
No GPU, and nothing is loaded into the interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_camera_boost_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "san_camera_boost"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_camera_boost.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "camera boost ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
