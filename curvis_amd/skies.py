"""Procedural equirectangular sky textures (synthetic inputs for tests and bench.py).

S_smooth: R = floor(255*x/W), G = floor(255*y/H), B = 128 (+l) / 32 (-l): adjacent texels differ by
          <= 1 LSB per channel, so a +-1-texel disagreement is <= 1 per channel.
S_check:  64-px checkerboard cells with a per-cell xorshift32 colour: any texel-index disagreement
          across a cell border is visible, used to measure exact-index agreement.
ring_texture: a texture for an accretion disc (curvis_amd.Disc): bright and hot at the inner edge, fading outwards, with
          azimuthal streaks and a few transparent gaps -- integers only, so the same bytes everywhere.
"""
import numpy as np


def smooth(width, height, blue):
    x = (np.arange(width, dtype=np.uint64) * 255 // width).astype(np.uint8)
    y = (np.arange(height, dtype=np.uint64) * 255 // height).astype(np.uint8)
    img = np.empty((height, width, 4), dtype=np.uint8)
    img[..., 0] = x[None, :]
    img[..., 1] = y[:, None]
    img[..., 2] = blue
    img[..., 3] = 255
    return img


def _xorshift32(v):
    v = v.astype(np.uint32)
    v ^= (v << np.uint32(13)) & np.uint32(0xFFFFFFFF)
    v ^= v >> np.uint32(17)
    v ^= (v << np.uint32(5)) & np.uint32(0xFFFFFFFF)
    return v


def checker(width, height, seed=0xC0FFEE, cell=64):
    cx = np.arange(width, dtype=np.uint32) // cell
    cy = np.arange(height, dtype=np.uint32) // cell
    ncx = (width + cell - 1) // cell
    cid = cy[:, None] * np.uint32(ncx) + cx[None, :]
    h = _xorshift32(np.uint32(seed) ^ (cid + np.uint32(1)))
    h = _xorshift32(h)
    img = np.empty((height, width, 4), dtype=np.uint8)
    img[..., 0] = (h & 0xFF).astype(np.uint8)
    img[..., 1] = ((h >> 8) & 0xFF).astype(np.uint8)
    img[..., 2] = ((h >> 16) & 0xFF).astype(np.uint8)
    img[..., 3] = 255
    return img


def ring_texture(width, height, seed=0xD15C):
    """height x width x 4 uint8 for curvis_amd.Disc(image, l_inner, l_outer): width runs along azimuth, height along l from the inner
    edge (row 0) to the outer.  Radial brightness falls outwards (255 -> 64), the colour goes from near white through orange to
    red, streaks of per-column xorshift32 noise -- smoothed along azimuth over 8 columns, drifting with the row so that they wind -- dim
    it by up to a third, and a few rows (about one in sixteen, chosen by the seed) are transparent gaps.  Pure integer arithmetic."""
    w, h = int(width), int(height)
    if w <= 0 or h <= 0:
        raise ValueError("ring_texture: width and height must be positive")
    y = np.arange(h, dtype=np.int64)[:, None]
    x = np.arange(w, dtype=np.int64)[None, :]
    fall = 255 - (191 * y) // max(h - 1, 1)                                   # 255 at the inner edge, 64 at the outer
    noise = (_xorshift32(_xorshift32(np.uint32(seed) ^ (np.arange(w, dtype=np.uint32) + np.uint32(1)))) & np.uint32(0xFF)).astype(np.int64)
    smooth8 = sum(np.roll(noise, k) for k in range(8)) // 8                  # 0..255, correlated over 8 columns
    streak = smooth8[(x + 3 * y) % w]                                         # wound: the pattern drifts 3 columns per row
    lum = fall * (512 + streak) // 767                                        # dimmed to between 2/3 and 1 of `fall`
    img = np.empty((h, w, 4), dtype=np.uint8)
    img[..., 0] = np.minimum(255, lum + lum // 8)
    img[..., 1] = lum * (255 - (150 * y) // max(h - 1, 1)) // 255
    img[..., 2] = lum * (200 - (190 * y) // max(h - 1, 1)) // 255
    rows = (_xorshift32(np.uint32(seed) ^ np.uint32(0x9E3779B9) ^ (np.arange(h, dtype=np.uint32) + np.uint32(1))) & np.uint32(15)) == 0
    img[..., 3] = np.where(rows[:, None], 0, 255)
    return img
