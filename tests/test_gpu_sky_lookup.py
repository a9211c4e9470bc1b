"""The last stage of every pixel -- direction -> texel (cvk::sky_indices, cv_device.h; src/images.rs:115-174, src/algebra.rs:106-134)
-- through every renderer, on skies whose colour IS the texel index (common.index_sky) and whose sizes are deliberately awkward:
not powers of two, not 2:1, and different for the two skies of a scene.  On the checker skies of the rest of the suite a lookup
that is a few texels off, uses the other sky's shape or swaps width and height changes a pixel only where it crosses a 64-texel
cell; here every such error changes the pixel, for the renderers that have no debug dump (fused epilogues, the efficient per-pixel
kernel, the direct kernel) as well.

Three parts: (1) every lookup site against the oracle's own render of the same scene under O.CV -- never one renderer against
another: on an index sky the brute and the efficient renderer differ in nearly every pixel in the oracle itself --; (2)
sky_indices alone on the device (curvis_selftest_sky_indices), on directed inputs bit for bit with cvo_sky_indices, and on random
directions against the exact texel from extended precision, which shares no code with cv_math.h; (3) a sky beyond 4 GiB."""
import collections
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common
import oracle_lib as O
import curvis_amd

pytestmark = pytest.mark.gpu

HP = common.HALF_PI
DELTA = 0.05
EFF = (100, 100, 1e-5, 1e-5)   # alpha_nums, max_iterations_sampling, the two convergence thresholds
SAMPLER_CAP = 1536             # cv_sampler_dev.h kSamplerCap: a larger table sends a device-sampled call to the host-paced sampler
OPTIONS = ("variant", "fuse_shade", "relay_min_blocks", "relay_segment", "device_sampler", "fast_math")
STATS = ("rays", "steps", "n_pos", "n_neg", "n_none", "n_oob")


# ---- sky pairs: (+l sky, -l sky), unequal, not 2:1; the last one with a non-default orientation on each sky ----
class SkyPair(collections.namedtuple("SkyPair", "name shapes salts orient")):
    def image(self, k):
        return _index_sky(self.shapes[k][0], self.shapes[k][1], self.salts[k])

    def inv(self, k):
        if self.orient[k] is None:
            return None
        fwd, up = (np.array(v, dtype=np.float64) for v in self.orient[k])
        rot, inv, upo = np.zeros(9), np.zeros(9), np.zeros(3)
        assert O.lib().cvo_orientation_new(O._dp(fwd), O._dp(up), O._dp(rot), O._dp(inv), O._dp(upo)) == 0
        return inv

    def oracle_skies(self):
        return O.sky(self.image(0), self.inv(0)), O.sky(self.image(1), self.inv(1))

    def product_skies(self):
        return [curvis_amd.SphericalImage(self.image(k), *(self.orient[k] or ())) for k in (0, 1)]

    def bind(self, ctx):
        for k, img in enumerate(self.product_skies()):
            ctx.set_sky(k, img)


@functools.lru_cache(maxsize=None)
def _index_sky(w, h, salt):
    return common.index_sky(w, h, salt)


S0, S1 = 0x3C5A96, 0xC3A569


def _pair(a, b, orient=(None, None)):
    return SkyPair("%dx%d+%dx%d%s" % (a + b + ("-rotated" if orient[0] else "",)), (a, b), (S0, S1), orient)


PAIRS = [_pair((1000, 500), (333, 777)), _pair((4001, 1999), (7, 4096)), _pair((1, 1), (3, 2)), _pair((4095, 2047), (4096, 5)),
         _pair((1, 4096), (4096, 1)),
         _pair((2047, 1025), (129, 3001), (((0.3, -0.8, 0.52), (0.1, 0.2, 1.0)), ((-0.6, 0.1, -0.79), (1.0, -0.4, 0.2))))]
PAIR = {p.name: p for p in PAIRS}

# ---- scenes.  capped: the renderers whose oracle frame must have capped rays (n_none > 0: a cap that binds) ----
Scene = collections.namedtuple("Scene", "name metric res pos fwd cap R capped")
SCENES = [
    Scene("ellis-l5", ("ellis", 1.0), (96, 54), (0.0, 5.0, HP, 0.0), (-1.0, 0.0, 0.0), 4096, 100.0, ()),
    # from the -l side: sky 1 carries most of the frame; 64 x 32: whole waves, whole 8x8 tiles
    Scene("interstellar-from-minus-l", ("interstellar", 0.1, 1e-4, 1.0), (64, 32), (0.0, -2.0, 1.1, 0.7), (1.0, 0.2, -0.1), 8192, 100.0, ()),
    Scene("ellis-l3-cap-binds", ("ellis", 1.0), (61, 35), (0.0, 3.0, HP, 1.0), (-1.0, 0.1, 0.05), 2100, 100.0, ("brute", "efficient", "direct")),
    # inside the long throat (|l| < a), looking along it sideways: half of the rays leave on either side
    Scene("inside-throat", ("interstellar", 0.1, 1.0, 1.0), (45, 27), (0.0, 0.5, 1.0, 0.0), (-0.1, 1.0, 0.2), 4000, 60.0, ("brute", "efficient", "direct")),
    Scene("pole-crossing-rows", ("ellis", 1.0), (64, 9), (0.0, 3.0, HP, 0.0), (-1.0, 0.0, 0.0), 4096, 100.0, ()),   # ADVERSARIAL's
    Scene("flat", ("flat",), (37, 21), (0.0, 5.0, 1.0, 0.5), (1.0, 0.3, 0.2), 4096, 100.0, ()),
]
SCENE = {s.name: s for s in SCENES}
UP = (0.0, 0.0, 1.0)


def metrics(scene):
    m = scene.metric
    if m[0] == "ellis":
        return O.ellis(m[1]), curvis_amd.EllisMetric(m[1])
    if m[0] == "interstellar":
        return O.interstellar(*m[1:]), curvis_amd.InterstellarMetric(*m[1:])
    return O.flat(), curvis_amd.FlatSphericalMetric()


def brute_poses(scene):
    """the scene's camera and two more for the batch of three: turned and tilted a little more each"""
    p, f = scene.pos, scene.fwd
    return [((p[0], p[1], p[2] + 0.07 * k, p[3] + 0.9 * k), (f[0], f[1] + 0.1 * k, f[2] - 0.05 * k)) for k in range(3)]


def efficient_poses(scene):
    """the scene's camera and its mirror image on the other side of the throat (flat space has no other side: further out)"""
    p, f = scene.pos, scene.fwd
    if scene.metric[0] == "flat":
        return [(p, f), ((p[0], p[1] + 2.0, p[2], p[3]), f)]
    return [(p, f), ((p[0], -p[1], p[2], p[3]), (-f[0], f[1], f[2]))]


def cameras(scene, poses):
    W, H = scene.res
    return ([O.camera(p, f, UP, 15.0, 43.0, scene.res) for p, f in poses],
            [curvis_amd.Camera(p, f, UP, 15.0, 43.0, W, H) for p, f in poses])


def tup(st):
    return tuple(int(getattr(st, n)) for n in STATS)


@functools.lru_cache(maxsize=None)
def oracle_results(pair_name, scene_name):
    """what O.CV renders for this scene over this pair of skies: {"brute": [(rgb, dbg, stats)] x 3 cameras, "efficient": [(rgb, table
    size, stats)] x 2 cameras, "direct": (rgb, stats)}; the renders run side by side on the host's threads"""
    pair, scene = PAIR[pair_name], SCENE[scene_name]
    om, _ = metrics(scene)
    sp, sn = pair.oracle_skies()
    ob, _ = cameras(scene, brute_poses(scene))
    oe, _ = cameras(scene, efficient_poses(scene))

    def brute(oc):
        rgb, dbg, st = O.render_image(O.CV, om, oc, sp, sn, scene.cap, scene.R, DELTA, debug=True)
        return rgb, dbg, tup(st)

    def efficient(oc):
        rgb, smp, st = O.render_image_efficient(O.CV, om, oc, sp, sn, scene.cap, scene.R, DELTA, *EFF)
        return rgb, len(smp["a"]), tup(st)

    def direct(oc):
        rgb, st = O.render_image_direct(O.CV, om, oc, sp, sn, scene.cap, scene.R, DELTA)
        return rgb, tup(st)
    jobs = [(brute, c) for c in ob] + [(efficient, c) for c in oe] + [(direct, ob[0])]
    with np.errstate(all="ignore"), ThreadPoolExecutor(min(len(jobs), common.host_threads(16))) as ex:
        res = list(ex.map(lambda j: j[0](j[1]), jobs))
    out = {"brute": res[:3], "efficient": res[3:5], "direct": res[5]}
    # the scene must really use both skies (and a binding cap where it says so): on the oracle's own statistics
    for kind, st in (("brute", out["brute"][0][2]), ("efficient", out["efficient"][0][2]), ("direct", out["direct"][1])):
        d = dict(zip(STATS, st))
        if scene.metric[0] != "flat":
            assert d["n_pos"] > 0 and d["n_neg"] > 0, (scene.name, kind, d)
        if kind in scene.capped:
            assert d["n_none"] > 0, (scene.name, kind, d)
    return out


def assert_pixels(got, want, pair, what):
    """got == want, and if not: where, and which texel of which sky either side shows"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=2))
    if len(bad):
        lines = ["pixel (%d, %d): got %s, oracle %s" % (j, i, common.describe_texel(got[i, j], pair.shapes, pair.salts),
                                                       common.describe_texel(want[i, j], pair.shapes, pair.salts)) for i, j in bad[:6]]
        pytest.fail("%s over %s: %d of %d pixels differ from the oracle\n  %s" % (what, pair.name, len(bad), got.shape[0] * got.shape[1],
                                                                                "\n  ".join(lines)), pytrace=False)


def band_stats(pair, dbg, b, e):
    """the six statistics of rows [b, e) from the oracle's per-ray dump"""
    d = dbg[b:e]
    oob = 0
    for code, (w, h) in ((O.POSITIVE, pair.shapes[0]), (O.NEGATIVE, pair.shapes[1])):
        m = d["code"] == code
        oob += int(((d["tx"][m] >= w) | (d["ty"][m] >= h)).sum())
    return (d.size, int(d["steps"].astype(np.uint64).sum()), int((d["code"] == O.POSITIVE).sum()), int((d["code"] == O.NEGATIVE).sum()),
            int((d["code"] == O.NOT_ESCAPED).sum()), oob)


def check_brute_sites(ctx, pair, scene, want):
    _, pm = metrics(scene)
    _, cams = cameras(scene, brute_poses(scene))
    pc = cams[0]
    w_rgb, w_dbg, w_st = want["brute"][0]
    args = (scene.cap, scene.R, DELTA)
    relayable = scene.cap >= 1000 and scene.metric[0] != "flat"
    for what, opts in (("geodesic_static, fused epilogue", dict(variant=1, fuse_shade=1)),
                       ("geodesic_static + shade_kernel", dict(variant=1, fuse_shade=0)),
                       ("geodesic_persistent", dict(variant=0, fuse_shade=1)),
                       ("geodesic_relay", dict(variant=2, fuse_shade=1, relay_min_blocks=0))):
        for k, v in opts.items():
            ctx.set_option(k, v)
        parks = 0
        for seg in ((16, 100) if opts["variant"] == 2 else (0,)):
            ctx.set_option("relay_segment", seg)
            rgb, st = ctx.render_brute(pm, pc, *args)
            assert_pixels(rgb, w_rgb, pair, "%s (%s)" % (what, scene.name))
            assert tup(st) == w_st, (what, scene.name, pair.name)
            if opts["variant"] == 2:
                assert ctx.get_option("last_relay_launches") >= 1
                parks += ctx.get_option("last_relay_parks")
        if opts["variant"] == 2 and relayable:
            assert parks > 0, "the relay's hand-over path did not run"
        ctx.set_option("relay_min_blocks", -1)
        ctx.set_option("relay_segment", 0)
    ctx.set_option("variant", -1)
    # the debug path: pixels and the texel indices themselves
    rgb, st, dbg = ctx.render_brute(pm, pc, *args, debug=True)
    for f in ("code", "steps", "tx", "ty"):
        bad = np.argwhere(dbg[f] != w_dbg[f])
        assert len(bad) == 0, ("debug dump", f, scene.name, pair.name, len(bad), bad[:4].tolist(),
                               [(int(dbg[f][tuple(b)]), int(w_dbg[f][tuple(b)])) for b in bad[:4]])
    assert_pixels(rgb, w_rgb, pair, "debug path (%s)" % scene.name)
    assert tup(st) == w_st
    # a row band that cuts the 8-row tiles
    H = scene.res[1]
    b, e = H // 3, min(H, H // 3 + max(1, H // 2) + 1)
    rgb, st = ctx.render_brute_rows(pm, pc, b, e - b, *args)
    assert_pixels(rgb, w_rgb[b:e], pair, "rows [%d, %d) (%s)" % (b, e, scene.name))
    assert tup(st) == band_stats(pair, w_dbg, b, e), ("row band", scene.name, pair.name)
    assert band_stats(pair, w_dbg, 0, H) == w_st         # (the dump-derived statistics are the oracle's)
    # three cameras in one launch
    rgb, st = ctx.render_brute(pm, cams, *args)
    per = ctx.frame_stats()
    assert len(per) == 3
    for f in range(3):
        assert_pixels(rgb[f], want["brute"][f][0], pair, "batch frame %d (%s)" % (f, scene.name))
        assert tup(per[f]) == want["brute"][f][2], ("batch frame statistics", f, scene.name, pair.name)
    assert tup(st) == tuple(sum(want["brute"][f][2][k] for f in range(3)) for k in range(6))


def expected_path(device_sampler, table_sizes):
    """"last_sampler_path": the sampler asked for, or 2 where a table outgrows the device sampler's arrays (flat space's does)"""
    return device_sampler if max(table_sizes) <= SAMPLER_CAP else 2 * device_sampler


def check_efficient_frames(ctx, pair, scene, want, device_sampler, n_frames, what):
    _, pm = metrics(scene)
    _, cams = cameras(scene, efficient_poses(scene))
    rgb, st = ctx.render_efficient(pm, cams[:n_frames], scene.cap, scene.R, DELTA, *EFF)
    assert ctx.get_option("last_sampler_path") == expected_path(device_sampler, [want["efficient"][f][1] for f in range(n_frames)]), what
    for f in range(n_frames):
        assert_pixels(rgb[f], want["efficient"][f][0], pair, "%s, frame %d (%s)" % (what, f, scene.name))
        assert tup(ctx.frame_stats(f)) == want["efficient"][f][2], (what, f, scene.name, pair.name)
    assert tup(st) == tuple(sum(want["efficient"][f][2][k] for f in range(n_frames)) for k in range(6)), what


def check_efficient_sites(ctx, pair, scene, want):
    for device_sampler in (0, 1):
        ctx.set_option("device_sampler", device_sampler)
        for fast in (1, 0):
            ctx.set_option("fast_math", fast)
            what = "efficient_pixel_kernel, device_sampler %d, %s step" % (device_sampler, "fast" if fast else "strict")
            check_efficient_frames(ctx, pair, scene, want, device_sampler, 1, what)
            check_efficient_frames(ctx, pair, scene, want, device_sampler, 2, what + ", batch across the throat")


def check_direct_site(ctx, pair, scene, want):
    _, pm = metrics(scene)
    _, cams = cameras(scene, brute_poses(scene)[:1])
    for fast in (1, 0):
        ctx.set_option("fast_math", fast)
        rgb, st = ctx.render_direct(pm, cams[0], scene.cap, scene.R, DELTA)
        assert_pixels(rgb, want["direct"][0], pair, "direct_kernel, %s step (%s)" % ("fast" if fast else "strict", scene.name))
        assert tup(st) == want["direct"][1], ("direct", fast, scene.name, pair.name)


class restored_options:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.saved = {k: self.ctx.get_option(k) for k in OPTIONS}

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.ctx.set_option(k, v)


@pytest.mark.parametrize("scene", [s.name for s in SCENES])
@pytest.mark.parametrize("pair", [p.name for p in PAIRS])
def test_every_lookup_site_on_awkward_skies_vs_oracle(gpu_ctx, pair, scene):
    """all renderers and kernel variants over one pair of index skies; the session's one context takes a new pair of shapes with
    every case (SkyTexture::reset and the per-call parameters must not keep a previous one)"""
    pair, scene = PAIR[pair], SCENE[scene]
    want = oracle_results(pair.name, scene.name)
    with restored_options(gpu_ctx):
        pair.bind(gpu_ctx)
        check_brute_sites(gpu_ctx, pair, scene, want)
        check_efficient_sites(gpu_ctx, pair, scene, want)
        check_direct_site(gpu_ctx, pair, scene, want)


def test_sky_shape_changes_between_prefetch_and_render(gpu_ctx):
    """curvis_ctx_prefetch_efficient samples under one pair of skies; both skies change size before the render that consumes the
    prefetched tables: the per-pixel kernel must look up with the shapes of the render call"""
    before, after = PAIRS[0], PAIRS[1]
    scene = SCENE["ellis-l5"]
    want = oracle_results(after.name, scene.name)
    _, pm = metrics(scene)
    _, cams = cameras(scene, efficient_poses(scene))
    with restored_options(gpu_ctx):
        gpu_ctx.set_option("device_sampler", 1)
        before.bind(gpu_ctx)
        gpu_ctx.prefetch_efficient(pm, cams, scene.cap, scene.R, DELTA, *EFF)
        after.bind(gpu_ctx)
        check_efficient_frames(gpu_ctx, after, scene, want, 1, 2, "prefetched under other sky shapes")
        assert gpu_ctx.get_option("last_sampling_prefetched") == 1


@pytest.mark.parametrize("copy", [1, 0])
def test_skies_handed_over_as_device_pointers(gpu_ctx, copy):
    """curvis_ctx_set_sky_device, copied (the source is overwritten before the first render) and borrowed: a second context's frame
    buffer is the device allocation (no torch in this process)"""
    pair = PAIRS[3]
    imgs = [pair.image(0), pair.image(1)]
    blob = np.concatenate([imgs[0].reshape(-1), imgs[1].reshape(-1)])
    other = curvis_amd.Context(0)
    try:
        with restored_options(gpu_ctx):
            other.upload_frames(blob)
            dev, nbytes = other.framebuffer()
            assert nbytes == blob.size
            off = 0
            for k in (0, 1):
                w, h = pair.shapes[k]
                gpu_ctx.set_sky_device(k, dev + off, w, h, copy=bool(copy))
                off += w * h * 4
            if copy:
                other.upload_frames(np.zeros_like(blob))
                assert other.framebuffer()[0] == dev     # (the same allocation: the copies' source is gone)
            for k in (0, 1):
                w, h = pair.shapes[k]
                at = ((h - 1) * w + w // 3) * 4          # in the last row
                n = min(4096, w * h * 4 - at)
                assert np.array_equal(gpu_ctx.read_sky(k, at, n), imgs[k].reshape(-1)[at:at + n]), k
            for name in ("ellis-l5", "interstellar-from-minus-l"):
                scene = SCENE[name]
                want = oracle_results(pair.name, name)
                _, pm = metrics(scene)
                _, cams = cameras(scene, brute_poses(scene)[:1])
                rgb, st = gpu_ctx.render_brute(pm, cams[0], scene.cap, scene.R, DELTA)
                assert_pixels(rgb, want["brute"][0][0], pair, "brute, set_sky_device copy=%d (%s)" % (copy, name))
                assert tup(st) == want["brute"][0][2]
                for device_sampler in (0, 1):
                    gpu_ctx.set_option("device_sampler", device_sampler)
                    check_efficient_frames(gpu_ctx, pair, scene, want, device_sampler, 2, "set_sky_device copy=%d" % copy)
                check_direct_site(gpu_ctx, pair, scene, want)
    finally:
        pair.bind(gpu_ctx)       # the session's context must not keep a pointer into the other context's memory
        other.close()


# a pair whose +l sky stands on its head and sideways (-z along the world's +x), and a camera that looks past the throat: some rays end
# EXACTLY on the sky's -z axis, where (theta / pi) h == h and the reference's get_pixel would panic
OOB_PAIR = SkyPair("1000x500+333x777-on-its-head", ((1000, 500), (333, 777)), (S0, S1), (((0.0, 0.0, 1.0), (-1.0, 0.0, 0.0)), ((0.0, 0.0, 1.0), (-1.0, 0.0, 0.0))))
OOB_SCENE = Scene("ellis-l5-off-axis", ("ellis", 1.0), (160, 90), (0.0, 5.0, HP, 0.0), (-1.0, 0.3, 0.1), 4096, 100.0, ())
PAIR[OOB_PAIR.name], SCENE[OOB_SCENE.name] = OOB_PAIR, OOB_SCENE


def test_out_of_range_texels_are_clamped_and_counted(gpu_ctx):
    """ty == h in a render: the clamp to the last row and n_oob, compared with the oracle where the count is NOT zero (it is 0 == 0
    in the rest of the suite), at every lookup site.  The brute renderer's frame has such rays; the efficient and the direct renderer's
    frames of this scene have none in the oracle (their clamp sees ty == h through curvis_selftest_sky_indices only)."""
    want = oracle_results(OOB_PAIR.name, OOB_SCENE.name)
    assert want["brute"][0][2][5] > 0, want["brute"][0][2]
    dbg = want["brute"][0][1]
    assert ((dbg["ty"] == 500) & (dbg["code"] == O.POSITIVE)).any()
    with restored_options(gpu_ctx):
        OOB_PAIR.bind(gpu_ctx)
        check_brute_sites(gpu_ctx, OOB_PAIR, OOB_SCENE, want)
        check_efficient_sites(gpu_ctx, OOB_PAIR, OOB_SCENE, want)
        check_direct_site(gpu_ctx, OOB_PAIR, OOB_SCENE, want)


# ---- sky_indices alone on the device ----
EXTRA_SHAPES = [(1, 65535), (2, 2 ** 31), (3, 65537), (65535, 1), (65537, 2), (2 ** 31, 3), (2 ** 32 - 1, 2 ** 32 - 1), (2, 3)]
ORIENTATIONS = [None, ((0.3, -0.8, 0.52), (0.1, 0.2, 1.0)), ((-0.6, 0.1, -0.79), (1.0, -0.4, 0.2))]


def all_shapes():
    seen = []
    for p in PAIRS:
        for s in p.shapes:
            if s not in seen:
                seen.append(s)
    return seen + EXTRA_SHAPES


def _ulps(v):
    """v, and v with each component in turn one ulp up / down"""
    out = [v]
    for k in range(3):
        for to in (np.inf, -np.inf):
            u = v.copy()
            u[:, k] = np.nextafter(u[:, k], to)
            out.append(u)
    return np.concatenate(out)


def directed_directions(w, h):
    """image-space directions on and next to everything sky_indices can trip over (module docstring; the issue's list)"""
    tiny = [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300]
    parts = []
    axes = []
    for k in range(3):
        for s in (1.0, -1.0):      # theta = 0 / pi (+-z), phi = 0 / +-pi: the seam (+-x), phi = +-pi/2 (+-y)
            for a in tiny:
                for b in tiny:
                    v = [a, b]
                    v.insert(k, s)
                    axes.append(v)
    parts.append(_ulps(np.array(axes)))
    mags = np.array([[1.0, 1.0, 1.0], [0.3, 0.7, 0.2], [1e-3, 1.0, 1e3], [1.0, 1e-17, 1e-17], [1e-17, 1e-17, 1.0], [3.0, 4.0, 0.0]])
    signs = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=np.float64)
    octants = (mags[:, None, :] * signs[None, :, :]).reshape(-1, 3)
    parts.append(octants)
    if w <= 4096:                  # the equator at the phi of every texel boundary: frac(1/2 - phi / 2 pi) w = k
        phi = 2.0 * np.pi * (0.5 - np.arange(w + 1) / w)
        eq = np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)], axis=1)
        parts += [_ulps(eq), _ulps(eq * [1.0, 1.0, 0.0] + [0.0, 0.0, 0.25])]
    if h <= 4096:                  # theta at every row boundary: (theta / pi) h = k
        th = np.pi * np.arange(h + 1) / h
        for p0 in (0.0, 2.0, -2.6):
            parts.append(_ulps(np.stack([np.sin(th) * np.cos(p0), np.sin(th) * np.sin(p0), np.cos(th)], axis=1)))
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -0.5]
    parts.append(np.array([[a, b, c] for a in special for b in special for c in special]))
    # norms whose square under- or overflows, and either side of sqrt_plain's guarded range [2^-700, 2^700) of the squared norm
    scales = [1e-200, 1e200, 1e-160, 1e160, 1e-154, 1e154, 1e155, 1e-308, 1e-320, 1e307, 2.0 ** -351, 2.0 ** -350, 2.0 ** -349, 2.0 ** 349,
              2.0 ** 350, 2.0 ** 351, 2.0 ** -300, 2.0 ** 300, 2.0 ** -1074, 2.0 ** 1023]
    with np.errstate(all="ignore"):
        parts.append(np.concatenate([octants[:24] * s for s in scales] + [np.array(axes[::7]) * s for s in scales]))
    return np.concatenate(parts)


def random_directions(rng, n):
    """over the exponent range: unit-scale directions times one power of two per direction, and components with exponents of their own"""
    a = rng.standard_normal((n // 2, 3)) * np.exp2(rng.integers(-1060, 1020, n // 2))[:, None]
    b = rng.standard_normal((n - n // 2, 3)) * np.exp2(rng.integers(-80, 80, (n - n // 2, 3)))
    return np.concatenate([a, b])


def rotation_of(orient):
    fwd, up = (np.array(v, dtype=np.float64) for v in orient)
    rot, inv, upo = np.zeros(9), np.zeros(9), np.zeros(3)
    assert O.lib().cvo_orientation_new(O._dp(fwd), O._dp(up), O._dp(rot), O._dp(inv), O._dp(upo)) == 0
    return rot.reshape(3, 3), inv


def assert_indices_equal_oracle(ctx, w, h, inv, dirs, what):
    want = O.sky_indices_array(O.CV, O.sky_shape(w, h, inv), dirs)
    got = ctx.selftest_sky_indices(w, h, dirs, inv)
    for name, cols in (("sky_indices<false>", got[:, :2]), ("sky_indices<true>", got[:, 2:])):
        bad = np.nonzero((cols != want).any(axis=1))[0]
        assert len(bad) == 0, "%s, %dx%d, %s: %d of %d directions differ from cvo_sky_indices; first: %s" % (
            name, w, h, what, len(bad), len(dirs),
            [(dirs[i].tolist(), [float.hex(float(c)) for c in dirs[i]], "device", cols[i].tolist(), "oracle", want[i].tolist()) for i in bad[:3]])
    return got, want


def test_sky_indices_on_the_device_bit_for_bit_with_the_oracle(gpu_ctx):
    """both instantiations of cvk::sky_indices (IEEE quotients; the efficient pixel kernel's shared reciprocals and sqrt_plain), raw
    indices before the clamp, on directed inputs and 2^17 random directions per shape and orientation (7.5 million in all).  NaN
    payloads cannot show: the outputs are integers."""
    rng = np.random.default_rng(20260)
    n_random = 0
    for (w, h) in all_shapes():
        directed = directed_directions(w, h)
        for orient in ORIENTATIONS:
            rnd = random_directions(rng, 1 << 17)
            n_random += len(rnd)
            if orient is None:
                inv, dirs = None, np.concatenate([directed, rnd])
            else:
                rot, inv = rotation_of(orient)
                with np.errstate(all="ignore"):       # world-space directions that land on (or an ulp or two from) the directed ones
                    dirs = np.concatenate([directed, directed @ rot.T, rnd])
            assert_indices_equal_oracle(gpu_ctx, w, h, inv, dirs, "orientation %s" % (orient,))
    assert n_random >= 3_000_000
    # theta = pi by value: ty == h exactly, from the device and from the oracle (why the clamp and n_oob exist); the seam
    down = np.array([[0.0, 0.0, -1.0], [-0.0, 0.0, -2.5], [0.0, -0.0, -1e-150]])
    for (w, h) in ((1000, 500), (7, 4096), (2 ** 32 - 1, 2 ** 32 - 1)):
        got, want = assert_indices_equal_oracle(gpu_ctx, w, h, None, down, "theta = pi")
        assert (got[:, 1] == h).all() and (got[:, 3] == h).all() and (want[:, 1] == h).all(), (w, h, got, want)
    got, _ = assert_indices_equal_oracle(gpu_ctx, 1000, 500, None, np.array([[-1.0, 0.0, 0.0], [-1.0, -0.0, 0.0], [1.0, 0.0, 0.0]]), "seam")
    assert got[:, 0].tolist() == [0, 0, 500] and got[:, 2].tolist() == [0, 0, 500] and (got[:, 1] == 250).all()   # phi = pi and -pi: one column


# ---- against extended precision: a reference that shares nothing with cv_math.h ----
LD = np.longdouble
TWO_M30 = 2.0 ** -30    # a direction is left out only when an exact coordinate lies this close to an integer (texels)


def _exact_coordinates_longdouble(d, w, h):
    """(cx, cy) = (frac(1/2 - phi / 2 pi) w, (theta / pi) h) in x87 extended precision (64-bit significand); theta from atan2(|xy|, z),
    which is well conditioned at the poles too.  Error: a few 2^-64 relative, i.e. below 2^-50 texel for w, h <= 4096."""
    x, y, z = (d[:, k].astype(LD) for k in range(3))
    pi = 4 * np.arctan(LD(1))
    cy = np.arctan2(np.hypot(x, y), z) / pi * h
    f = LD(0.5) - np.arctan2(y, x) / (2 * pi)
    f = f - np.floor(f)
    return f * w, cy


def _exact_coordinates_mpmath(d, w, h):
    import mpmath
    mp = mpmath.mp
    mp.dps = 60
    out = []
    for x, y, z in d:
        x, y, z = mp.mpf(float(x)), mp.mpf(float(y)), mp.mpf(float(z))
        cy = mp.atan2(mp.sqrt(x * x + y * y), z) / mp.pi * h
        f = mp.mpf(0.5) - mp.atan2(y, x) / (2 * mp.pi)
        f -= mp.floor(f)
        out.append((f * w, cy))
    return out


def exact_texels(d, w, h, n_mp=20000):
    """(directions, tx, ty, kept): the exact texel of every direction, and which directions keep both coordinates 2^-30 texel away
    from an integer.  numpy.longdouble where it carries >= 64 significand bits, cross-checked with mpmath at 60 digits on n_mp of
    the directions; where it is only a double, mpmath alone on the first n_mp directions (those are what comes back)."""
    import mpmath
    if np.finfo(LD).nmant < 63:
        d = d[:n_mp]
        ref = _exact_coordinates_mpmath(d, w, h)
        kept = np.array([min(abs(r[k] - mpmath.nint(r[k])) for k in (0, 1)) > TWO_M30 for r in ref])
        return (d, np.array([int(mpmath.floor(r[0])) for r in ref], dtype=np.int64),
                np.array([int(mpmath.floor(r[1])) for r in ref], dtype=np.int64), kept)
    cx, cy = _exact_coordinates_longdouble(d, w, h)
    idx = np.linspace(0, len(d) - 1, n_mp).astype(np.int64)
    ref = _exact_coordinates_mpmath(d[idx], w, h)
    for c, k in ((cx, 0), (cy, 1)):   # the two references agree to 2^-40 texel: far inside the 2^-30 rule, far above longdouble's 2^-64 relative
        hi = c[idx].astype(np.float64)
        lo = (c[idx] - hi.astype(LD)).astype(np.float64)
        worst = max(abs(ref[i][k] - (mpmath.mpf(float(hi[i])) + mpmath.mpf(float(lo[i])))) for i in range(len(idx)))
        assert worst < 2.0 ** -40, ("longdouble vs mpmath", w, h, k, float(worst))
    kept = (np.abs(cx - np.rint(cx)) > TWO_M30) & (np.abs(cy - np.rint(cy)) > TWO_M30)
    return d, np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64), kept


HP_SHAPES = [(4096, 2048), (1000, 500), (333, 777)]
HP_N = 2_000_000


def check_against_exact(indices_of, w, h, seed):
    """indices_of(dirs) -> [n, 2k] raw indices (k instantiations); every kept direction must land on the exact texel"""
    d = np.random.default_rng(seed).standard_normal((HP_N, 3))
    d, tx, ty, kept = exact_texels(d, w, h)
    dropped = int((~kept).sum())
    assert dropped * 10 ** 6 <= len(d), "%d of %d directions within 2^-30 texel of a boundary: the inputs are wrong" % (dropped, len(d))
    got = indices_of(d).astype(np.int64)
    for c in range(0, got.shape[1], 2):
        bad = np.nonzero(kept & ((got[:, c] != tx) | (got[:, c + 1] != ty)))[0]
        assert len(bad) == 0, "%dx%d, instantiation %d: %d of %d directions miss the exact texel; first: %s" % (
            w, h, c // 2, len(bad), int(kept.sum()), [(d[i].tolist(), "got", got[i, c:c + 2].tolist(), "exact", (int(tx[i]), int(ty[i]))) for i in bad[:3]])
    return int(kept.sum())


@pytest.mark.parametrize("w,h", HP_SHAPES)
def test_sky_indices_on_the_device_vs_exact_texel(gpu_ctx, w, h):
    """2 million random unit-scale directions per shape: the device's texel (both instantiations) is the exact one,
    floor(frac(1/2 - phi / 2 pi) w), floor((theta / pi) h), computed without cv_math.h.  Left out: directions with a coordinate within
    2^-30 texel of an integer (1000 times what double rounding can move a coordinate at w <= 4096; expected 4e-9 per direction), at
    most one in a million -- a condition on the inputs, not a measurement."""
    check_against_exact(lambda d: gpu_ctx.selftest_sky_indices(w, h, d), w, h, 7700 + w)


# ---- a sky beyond 4 GiB ----
BIG_W, BIG_H = 46343, 25013            # 1.159e9 texels, 4.637e9 bytes: the last 1843 rows lie beyond byte 2^32


def _host_bytes_available():
    vals = []
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    vals.append(int(line.split()[1]) * 1024)
    except OSError:
        pass
    try:
        with open("/sys/fs/cgroup/memory.max") as f1, open("/sys/fs/cgroup/memory.current") as f2:
            mx = f1.read().strip()
            if mx != "max":
                vals.append(int(mx) - int(f2.read()))
    except (OSError, ValueError):
        pass
    return min(vals) if vals else None


def _big_sky():
    """texel (x, y) = a 24-bit hash of (x, y), alpha 255; filled in row blocks on the host's threads"""
    tex = np.empty((BIG_H, BIG_W), np.uint32)
    xa = ((np.arange(BIG_W, dtype=np.uint64) * 0x9E3779B1) & 0xFFFFFFFF).astype(np.uint32)

    def fill(b0):
        b1 = min(BIG_H, b0 + 128)
        yb = ((np.arange(b0, b1, dtype=np.uint64) * 0x85EBCA6B) & 0xFFFFFFFF).astype(np.uint32)
        v = tex[b0:b1]
        np.add(xa[None, :], yb[:, None], out=v)
        v ^= v >> np.uint32(15)
        v *= np.uint32(0x2C1B3C6D)
        v ^= v >> np.uint32(12)
        v >>= np.uint32(8)
        v |= np.uint32(0xFF000000)
    with ThreadPoolExecutor(common.host_threads(16)) as ex:
        list(ex.map(fill, range(0, BIG_H, 128)))
    return tex.view(np.uint8).reshape(BIG_H, BIG_W, 4)


def test_sky_beyond_4_gib(gpu_ctx):
    """a +l sky of more than 2^30 texels and 2^32 bytes with a width that is no power of two: upload, read_sky beyond byte 2^32, and
    brute and efficient frames that land on the sky's last rows -- a byte offset or ty * w formed in 32 bits anywhere shows as
    wrong pixels.  Needs the sky once in host memory; a lease that cannot hold it skips with the number it found."""
    nbytes = BIG_W * BIG_H * 4
    assert BIG_W * BIG_H > 2 ** 30 and nbytes > 2 ** 32 and BIG_W & (BIG_W - 1)
    avail = _host_bytes_available()
    if avail is not None and avail < nbytes + (2 << 30):
        pytest.skip("the %.2f GB sky needs %.1f GB of host memory; this lease has %.1f GB available" % (nbytes / 1e9, (nbytes + (2 << 30)) / 1e9, avail / 1e9))
    big = _big_sky()
    small = common.index_sky(333, 777, S1)
    # the big sky stands on its head and sideways (its -z axis along the world's +x): the frame of a camera at l = 5 that looks past
    # the throat lands on the last 40 % of its rows, on both sides of byte 2^32, and a few rays exactly on theta = pi (ty == h: clamped)
    pos, fwd, res, turned = (0.0, 5.0, HP, 0.0), (-1.0, 0.3, 0.1), (160, 90), ((0.0, 0.0, 1.0), (-1.0, 0.0, 0.0))
    om, pm = O.ellis(1.0), curvis_amd.EllisMetric(1.0)
    oc = O.camera(pos, fwd, UP, 15.0, 43.0, res)
    pc = curvis_amd.Camera(pos, fwd, UP, 15.0, 43.0, res[0], res[1])
    sp, sn = O.sky(big, rotation_of(turned)[1]), O.sky(small)
    with ThreadPoolExecutor(2) as ex:
        fb = ex.submit(lambda: O.render_image(O.CV, om, oc, sp, sn, 4096, 100.0, DELTA, debug=True))
        fe = ex.submit(lambda: O.render_image_efficient(O.CV, om, oc, sp, sn, 4096, 100.0, DELTA, *EFF))
        try:
            gpu_ctx.set_sky(0, curvis_amd.SphericalImage(big, *turned))
            gpu_ctx.set_sky(1, curvis_amd.SphericalImage(small))
            flat = big.reshape(-1)
            for at in (2 ** 32 - 2048, 2 ** 32 + 12345 * 4, nbytes - 4096, 0):
                assert np.array_equal(gpu_ctx.read_sky(0, at, 4096), flat[at:at + 4096]), at
            got_b, st_b = gpu_ctx.render_brute(pm, pc, 4096, 100.0, DELTA)
            got_e, st_e = gpu_ctx.render_efficient(pm, pc, 4096, 100.0, DELTA, *EFF)
            want_b, dbg, wst_b = fb.result()
            want_e, _, wst_e = fe.result()
        finally:
            PAIRS[0].bind(gpu_ctx)        # give the 4.6 GB of HBM back
    hit = dbg["code"] == O.POSITIVE
    beyond = int((((dbg["ty"][hit].astype(np.uint64) * BIG_W + dbg["tx"][hit]) * 4) >= 2 ** 32).sum())
    assert beyond >= 1000, "only %d rays read texels beyond byte 2^32: the pose does not test what it is meant to" % beyond
    bad = np.argwhere((got_b != want_b).any(axis=2))
    assert len(bad) == 0, ("brute", len(bad), bad[:4].tolist(), [(dbg["tx"][tuple(b)], dbg["ty"][tuple(b)]) for b in bad[:4]])
    assert tup(st_b) == tup(wst_b) and wst_b.n_oob > 0 and wst_b.n_neg > 0
    bad = np.argwhere((got_e != want_e).any(axis=2))
    assert len(bad) == 0, ("efficient", len(bad), bad[:4].tolist())
    assert tup(st_e) == tup(wst_e)
    assert len(np.unique(want_b.reshape(-1, 3), axis=0)) > 1000      # a picture of hashed texels, not a constant
