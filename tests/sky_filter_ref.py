"""Library option "sky_filter" = 1 (bilinear sky lookup): the definition in numpy integers, written from the text of the option's
paragraph in include/curvis_hip.h, and the inputs the GPU and the host tests share.  Nothing here calls the product.

For a ray that escapes to a sky of w x h RGBA8 texels T[y][x]:
  1. (X, Y) are the raw `as u32` indices the nearest lookup returns for a sky of 256 w x 256 h texels of the same orientation;
  2. out of bounds exactly when X >> 8 >= w or Y >> 8 >= h; Xc = min(X, 256 w - 1), Yc = min(Y, 256 h - 1);
  3. U = Xc - 128 if Xc >= 128 else Xc + 256 w - 128; x0 = U >> 8, fx = U & 255, x1 = x0 + 1, or 0 when that equals w;
  4. V = max(Yc - 128, 0); y0 = V >> 8, fy = V & 255, y1 = min(y0 + 1, h - 1);
  5. per channel ((256-fx)(256-fy) T[y0][x0] + fx (256-fy) T[y0][x1] + (256-fx) fy T[y1][x0] + fx fy T[y1][x1] + 32768) >> 16.
(X, Y) come from the CPU oracle: cvo_sky_indices on the virtual sky, or a frame it renders over an index sky of that size."""
import math

import numpy as np

import common
import oracle_lib as O

MAX_SIDE = 1 << 23


def texture(w, h, salt):
    """an h x w RGBA8 image whose colours come from a hash of (x, y, salt): neighbours differ in every channel, alpha is 255"""
    x = np.arange(w, dtype=np.uint64)[None, :]
    y = np.arange(h, dtype=np.uint64)[:, None]
    v = (x * np.uint64(0x9E3779B1) + y * np.uint64(0x85EBCA77) + np.uint64(salt) * np.uint64(0xC2B2AE3D)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(12)
    v = (v * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    img = np.empty((h, w, 4), np.uint8)
    for c in range(3):
        img[..., c] = (v >> np.uint64(8 * c)) & np.uint64(255)
    img[..., 3] = 255
    return img


def taps(X, Y, w, h):
    """steps 2-4 on raw indices of the 256 w x 256 h sky: (x0, x1, y0, y1, fx, fy, tx, ty, oob), int64 arrays"""
    X, Y = np.asarray(X).astype(np.int64), np.asarray(Y).astype(np.int64)
    tx, ty = X >> 8, Y >> 8
    oob = (tx >= w) | (ty >= h)
    Xc, Yc = np.minimum(X, 256 * w - 1), np.minimum(Y, 256 * h - 1)
    U = np.where(Xc >= 128, Xc - 128, Xc + 256 * w - 128)
    x0, fx = U >> 8, U & 255
    x1 = np.where(x0 + 1 == w, 0, x0 + 1)
    V = np.maximum(Yc - 128, 0)
    y0, fy = V >> 8, V & 255
    y1 = np.minimum(y0 + 1, h - 1)
    return x0, x1, y0, y1, fx, fy, tx, ty, oob


def blend(T, x0, x1, y0, y1, fx, fy):
    """step 5 on the image T (h x w x 4 uint8): [..., 3] uint8"""
    fx, fy = fx[..., None].astype(np.int64), fy[..., None].astype(np.int64)
    c = lambda yy, xx: T[yy, xx, :3].astype(np.int64)   # noqa: E731
    s = (256 - fx) * (256 - fy) * c(y0, x0) + fx * (256 - fy) * c(y0, x1) + (256 - fx) * fy * c(y1, x0) + fx * fy * c(y1, x1) + 32768
    assert s.max(initial=0) < 1 << 32
    return (s >> 16).astype(np.uint8)


def oracle_virtual_indices(w, h, inv, dirs):
    """(X, Y) of step 1 from the oracle: cvo_sky_indices on the sky of 256 w x 256 h texels"""
    xy = O.sky_indices_array(O.CV, O.sky_shape(256 * w, 256 * h, inv), dirs)
    return xy[:, 0], xy[:, 1]


def expected_taps_and_colours(T, inv, dirs):
    h, w = T.shape[:2]
    X, Y = oracle_virtual_indices(w, h, inv, dirs)
    x0, x1, y0, y1, fx, fy, tx, ty, oob = taps(X, Y, w, h)
    return np.stack([x0, x1, y0, y1, fx, fy], axis=1).astype(np.uint32), np.stack([tx, ty], axis=1).astype(np.uint32), oob, \
        blend(T, x0, x1, y0, y1, fx, fy)


# ---- directions ----------------------------------------------------------------------------------------------------------------
def _ulps(v):
    """v and its neighbours one ulp away in every component and direction"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    out = [v]
    for k in range(3):
        for to in (np.inf, -np.inf):
            u = v.copy()
            u[:, k] = np.nextafter(u[:, k], to)
            out.append(u)
    return np.concatenate(out)


DIRECTED_SKY = (13, 7)   # the sky whose texel centres and edges the directed directions sit on


def directed_directions():
    """+-z; the seam +- 1 ulp; every texel-centre and texel-edge longitude and latitude of a 13 x 7 sky +- 1 ulp; zeros, NaN and
    infinities"""
    w, h = DIRECTED_SKY
    parts = [_ulps([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [-0.0, 0.0, -2.5], [1e-300, -1e-300, 1.0]])]
    parts.append(_ulps([[-1.0, 0.0, 0.0], [-1.0, -0.0, 0.0], [-3.0, 5e-324, 0.0], [-3.0, -5e-324, 0.0], [-1.0, 0.0, 0.3], [-1.0, -0.0, -0.3]]))
    k = np.arange(2 * w + 1) / 2.0              # frac(1/2 - phi / 2 pi) w = k: edges at the integers, centres half-way
    phi = 2.0 * np.pi * (0.5 - k / w)
    for z in (0.0, 0.25, -3.0):
        parts.append(_ulps(np.stack([np.cos(phi), np.sin(phi), np.full_like(phi, z)], axis=1)))
    j = np.arange(2 * h + 1) / 2.0              # (theta / pi) h = j
    th = np.pi * j / h
    for p0 in (0.0, 2.0, -2.6, np.pi):
        parts.append(_ulps(np.stack([np.sin(th) * np.cos(p0), np.sin(th) * np.sin(p0), np.cos(th)], axis=1)))
    # the corners: a centre or edge latitude at a centre or edge longitude
    pp, tt = np.meshgrid(phi, th)
    parts.append(np.stack([np.sin(tt) * np.cos(pp), np.sin(tt) * np.sin(pp), np.cos(tt)], axis=2).reshape(-1, 3))
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -0.5]
    parts.append(np.array([[a, b, c] for a in special for b in special for c in special]))
    return np.concatenate(parts)


def random_directions(rng, n):
    """unit-scale directions times one power of two each, and components with exponents of their own"""
    a = rng.standard_normal((n // 2, 3)) * np.exp2(rng.integers(-1000, 1000, n // 2))[:, None]
    b = rng.standard_normal((n - n // 2, 3)) * np.exp2(rng.integers(-60, 60, (n - n // 2, 3)))
    return np.concatenate([a, b])


SELFTEST_SIZES = ((1, 1), (3, 2), (13, 7), (1000, 500), (4095, 2047), (MAX_SIDE, 1))
N_RANDOM = 100_000


def inverse_rotation(forward, up):
    """the oracle's Orientation::new(forward, up).inverse_rotation_matrix, 9 doubles row-major"""
    fwd, upv = np.array(forward, dtype=np.float64), np.array(up, dtype=np.float64)
    rot, inv, upo = np.zeros(9), np.zeros(9), np.zeros(3)
    assert O.lib().cvo_orientation_new(O._dp(fwd), O._dp(upv), O._dp(rot), O._dp(inv), O._dp(upo)) == 0
    return inv


# ---- the frames' scene -------------------------------------------------------------------------------------------------------------
SHAPES = ((13, 7), (16, 5))                 # +l sky, -l sky (w, h); their fine index skies are 3328 x 1792 and 4096 x 1280
TEX_SALTS = (0x51F7, 0xA2C9)
# index-sky salts: byte 2's high nibble is y >> 8 of the texel black decodes to -- 7 (y >= 1792) and 13 (y >= 3328): outside either fine
# sky; and the nibbles' xor, 10, sends every texel of one fine sky (y >> 8 <= 6) outside the other when decoded with the wrong salt
INDEX_SALTS = (0x7A3C1B, 0xDEA5C4)
RES = (24, 16)
R, DELTA, CAP = 10.0, 0.05, 340
ORIENT = {"A": (((0.0, 0.0, 1.0), (1.0, 0.0, 0.0)), ((0.0, 0.0, 1.0), (-1.0, 0.0, 0.0))),
          "B": (((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0)), ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))}
_cache = {}


def real_skies():
    if "real" not in _cache:
        _cache["real"] = tuple(texture(w, h, s) for (w, h), s in zip(SHAPES, TEX_SALTS))
        for t in _cache["real"]:
            t.setflags(write=False)
    return _cache["real"]


def fine_skies():
    if "fine" not in _cache:
        _cache["fine"] = tuple(common.index_sky(256 * w, 256 * h, s) for (w, h), s in zip(SHAPES, INDEX_SALTS))
    return _cache["fine"]


def oracle_fine_skies(orient):
    return tuple(O.sky(img, inverse_rotation(*ORIENT[orient][k])) for k, img in enumerate(fine_skies()))


def assert_salts(shapes=SHAPES, salts=INDEX_SALTS, fine=None):
    """black decodes to no texel of either fine sky, and no colour of one fine sky to a texel of the other"""
    fine = fine or fine_skies()
    for k, ((w, h), salt) in enumerate(zip(shapes, salts)):
        x, y = common.texel_of(np.zeros(3, np.uint8), salt)
        assert not (x < 256 * w and y < 256 * h), (k, int(x), int(y))
    for k in (0, 1):
        w2, h2 = shapes[1 - k]
        x, y = common.texel_of(fine[k][..., :3], salts[1 - k])
        assert not ((x < 256 * w2) & (y < 256 * h2)).any(), k


def decode(fine_rgb, shapes=SHAPES, salts=INDEX_SALTS):
    """a frame the oracle rendered over the fine index skies -> (which: -1 black / capped, 0 +l sky, 1 -l sky; Xc; Yc) per pixel"""
    which = np.full(fine_rgb.shape[:2], -1, np.int64)
    Xc, Yc = np.zeros(fine_rgb.shape[:2], np.int64), np.zeros(fine_rgb.shape[:2], np.int64)
    hits = np.zeros(fine_rgb.shape[:2], np.int64)
    for k, ((w, h), salt) in enumerate(zip(shapes, salts)):
        x, y = common.texel_of(fine_rgb, salt)
        inside = (x < 256 * w) & (y < 256 * h)
        which[inside], Xc[inside], Yc[inside] = k, x[inside], y[inside]
        hits += inside
    black = (fine_rgb == 0).all(axis=-1)
    assert ((hits == 1) | black).all() and (hits[black] == 0).all()
    return which, Xc, Yc


def filtered_frame(fine_rgb, shapes=SHAPES, real=None, salts=INDEX_SALTS):
    """steps 3-5 on the decoded (Xc, Yc) of every pixel (the oracle has clamped them: min(X, 256 w - 1) is step 2's), capped rays black"""
    which, Xc, Yc = decode(fine_rgb, shapes, salts)
    out = np.zeros(fine_rgb.shape, np.uint8)
    for k, ((w, h), T) in enumerate(zip(shapes, real or real_skies())):
        m = which == k
        x0, x1, y0, y1, fx, fy, _, _, _ = taps(Xc[m], Yc[m], w, h)
        out[m] = blend(T, x0, x1, y0, y1, fx, fy)
    return out, which, Xc, Yc


def classes(which, Xc, Yc, k):
    """the rays of sky k by what the filter does with them"""
    w, h = SHAPES[k]
    m = which == k
    x, y = Xc[m], Yc[m]
    left, right = x < 128, x >= 256 * w - 128
    top, bottom = y < 128, y >= 256 * h - 128
    fx, fy = (x - 128) & 255, (y - 128) & 255
    interior = ~(left | right | top | bottom) & (fx != 0) & (fy != 0)
    return dict(n=int(m.sum()), left=int(left.sum()), right=int(right.sum()), top=int(top.sum()), bottom=int(bottom.sum()),
                corner=int(((left | right) & (top | bottom)).sum()), interior=int(interior.sum()),
                fx_values=len(set(fx[interior].tolist())), fy_values=len(set(fy[interior].tolist())))


def assert_classes(cl, what, pole=None):
    """what every oracle-based comparison relies on: both seam wraps, a pole clamp, a seam-and-pole corner, and more than 300 interior
    rays with more than 100 distinct weights each way"""
    assert cl["left"] >= 1 and cl["right"] >= 1, (what, cl)
    assert cl["top"] + cl["bottom"] >= 1 and cl["corner"] >= 1, (what, cl)
    if pole:
        assert cl[pole] >= 1, (what, pole, cl)
    assert cl["interior"] > 300 and cl["fx_values"] > 100 and cl["fy_values"] > 100, (what, cl)


def box_average(a, n):
    h, w = a.shape[0] // n, a.shape[1] // n
    s = a.astype(np.uint32).reshape(h, n, w, n, 3).sum(axis=(1, 3), dtype=np.uint32)
    return ((s + n * n // 2) >> (2 * (n.bit_length() - 1))).astype(np.uint8)


HALF_PI = math.pi / 2


def scene(kind, res=RES, l=5.0):
    return common.scene(kind, res=res, pos=(0.0, l, HALF_PI, 0.0))
