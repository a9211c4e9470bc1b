"""The brute renderer's call plan (curvis_amd/csrc/brute_plan.h: refusal, path and kernel family of a call, from the facts of the
call) over the full cross product of its facts, under AddressSanitizer and UBSan: a stand-alone program with its own main
(tests/sanitize/san_brute_plan.cpp), compiled and run here.  No GPU, and nothing is loaded into the interpreter.

The program also checks that no plan that is not a refusal names a kernel family absent for the call's launch shape.  DIGEST and
COUNTS were not produced by brute_plan.h: they are the listing of the decision code the plan replaced -- render_impl's refusal
blocks, render_rays' Schwarzschild / variant = 0 line, choose_render_path's fused / relay expressions and the branches of
launch_integrate_any / launch_integrate / launch_disc with every launch replaced by the family's name -- run over the same
98 304 combinations in the same line format.  `san_brute_plan --dump` prints the listing, for a diff after a mismatch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = 98304
DIGEST = "17c3ad87a875452869dc5d8f31301e91821c7412e5915d9961505bdf42142ba3"
COUNTS = {
    "REFUSE Schwarzschild metric: variant = 0 (the persistent kernel) is not built for this kind (set variant = -1, 1 or 2: the static kernel renders it)": 16,
    "REFUSE a disc is set: fuse_shade = 0 shades from the ray store, which has no slot for a disc colour": 12288,
    "REFUSE a disc is set: the debug dump shades from the ray store, which has no slot for a disc colour (remove the disc: curvis_ctx_set_disc with rgba = NULL)": 32768,
    "REFUSE a disc is set: variant = 0 (the persistent kernel) shades from the ray store, which has no slot for a disc colour": 8192,
    "REFUSE camera velocity: fuse_shade = 0 (the unfused static kernel) has the static camera only": 3072,
    "REFUSE camera velocity: the debug dump replays the static camera (clear the velocities: curvis_ctx_set_camera_velocities with n = 0)": 8192,
    "REFUSE camera velocity: the emission shift of a moving disc takes the camera to be at rest (set the disc's motion to 0, or clear the velocities)": 768,
    "REFUSE camera velocity: variant = 0 (the persistent kernel) has the static camera only": 2048,
    "REFUSE integrator = 1: fuse_shade = 0 (the unfused static kernel) takes the reference's Euler step only outside the debug dump": 48,
    "REFUSE integrator = 1: variant = 0 (the persistent kernel) takes the reference's Euler step only": 64,
    "REFUSE projection != 0: fuse_shade = 0 (the unfused static kernel) has the perspective camera only": 768,
    "REFUSE projection != 0: the debug dump replays the perspective camera (set projection = 0)": 2048,
    "REFUSE projection != 0: variant = 0 (the persistent kernel) has the perspective camera only": 512,
    "REFUSE sky_filter = 1: fuse_shade = 0 shades from the ray store, which has the nearest lookup only": 384,
    "REFUSE sky_filter = 1: the debug dump records the nearest lookup (set sky_filter = 0)": 1024,
    "REFUSE sky_filter = 1: variant = 0 (the persistent kernel) shades from the ray store, which has the nearest lookup only": 256,
    "REFUSE sky_mipmap = 1: fuse_shade = 0 shades from the ray store, which has the nearest lookup only": 1536,
    "REFUSE sky_mipmap = 1: the debug dump records the nearest lookup (set sky_mipmap = 0)": 4096,
    "REFUSE sky_mipmap = 1: variant = 0 (the persistent kernel) shades from the ray store, which has the nearest lookup only": 1024,
    "REFUSE step_scale != 0: fuse_shade = 0 (the unfused static kernel) takes the reference's fixed step only outside the debug dump": 96,
    "REFUSE step_scale != 0: variant = 0 (the persistent kernel) takes the reference's fixed step only": 128,
    "REFUSE supersample > 1: fuse_shade = 0 shades single rays from the ray store and has no tile-local resolve": 192,
    "REFUSE supersample > 1: the debug dump has one record per ray, not per pixel (set supersample = 1)": 512,
    "REFUSE supersample > 1: variant = 0 (the persistent kernel) stages single rays and has no tile-local resolve": 128,
    "REFUSE the disc motion is Keplerian and needs the Schwarzschild metric: in the other kinds g00 = -1, free matter is at rest and nothing orbits (set the motion to 0: curvis_ctx_set_disc_motion)": 4608,
    "disc fused=1 relay=0": 6144,
    "disc_motion fused=1 relay=0": 768,
    "fused fused=1 relay=0": 6048,
    "persistent fused=0 relay=0": 48,
    "relay fused=1 relay=1": 96,
    "staged_adapt fused=0 relay=0": 144,
    "unfused fused=0 relay=0": 288,
}


def test_brute_plan_decides_as_the_code_it_replaced_and_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "san_brute_plan"
    subprocess.run([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "sanitize", "san_brute_plan.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "brute plan ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = r.stdout.splitlines()
    assert lines[:2] == ["rows %d" % ROWS, "outcomes %d" % len(COUNTS)]
    counts = {}
    for line in lines[3:-1]:
        n, outcome = line.strip().split(" ", 1)
        counts[outcome] = int(n)
    assert counts == COUNTS
    assert sum(counts.values()) == ROWS
    assert lines[2] == "sha256 " + DIGEST
