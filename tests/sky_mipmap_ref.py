"""Library option "sky_mipmap" = 1 (the bilinear sky lookup on a mip pyramid): the definition in numpy integers, written from the
text of the option's paragraph in include/curvis_hip.h.  Nothing here calls the product; decoding, taps and blend are sky_filter_ref's.

  Pyramid.   Level 0 is the sky, w x h.  w_{k+1} = (w_k + 1) >> 1, h_{k+1} = (h_k + 1) >> 1; T_{k+1}[y][x] = (a + b + c + d + 2) >> 2 per
             colour channel over columns 2x, min(2x + 1, w_k - 1) and rows 2y, min(2y + 1, h_k - 1) of level k; alpha 255;
             L = 1 + ceil(log2(max(w, h))) levels.
  Footprint. Partners of ray (px, py): (px ^ 1, py) and (px, py ^ 1), absolute ray coordinates.  A partner inside the frame, not capped
             and on the same sky contributes |wrap(Xc' - Xc)| (wrap: modulo 256 w into [-128 w, 128 w)) and |Yc' - Yc|; rho is the
             largest contribution, 0 without any.
  Level.     rho < 256: k = 0, f = 0; else k = msb(rho) - 8, f = (rho >> k) & 255; then k >= L - 1: k = L - 1, f = 0.
  Colour.    c_k = steps 3-5 of "sky_filter" on T_k with w_k, h_k, Xc >> k, Yc >> k; f = 0: c_k, else per channel
             ((256 - f) c_k + f c_{k+1} + 128) >> 8."""
import numpy as np

import sky_filter_ref as F


def n_levels(w, h):
    m, L = max(w, h), 1
    while m > 1:
        m, L = (m + 1) >> 1, L + 1
    return L


def pyramid(T):
    """the levels of the h x w x 4 uint8 image T, level 0 first (T itself with alpha as given)"""
    levels = [np.asarray(T)]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        S = levels[-1].astype(np.int64)
        hs, ws = S.shape[:2]
        hd, wd = (hs + 1) >> 1, (ws + 1) >> 1
        x0, y0 = 2 * np.arange(wd), 2 * np.arange(hd)
        x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
        D = (S[y0][:, x0] + S[y0][:, x1] + S[y1][:, x0] + S[y1][:, x1] + 2) >> 2
        D[..., 3] = 255
        levels.append(D.astype(np.uint8))
    assert len(levels) == n_levels(T.shape[1], T.shape[0])
    return levels


def wrap_abs(d, w):
    """|wrap(d)| for integer differences d: wrap reduces modulo 256 w into [-128 w, 128 w)"""
    m = 256 * w
    r = np.mod(np.asarray(d, np.int64) + 128 * w, m) - 128 * w
    return np.abs(r)


def footprint(which, Xc, Yc, widths, row0=0, frame_h=None):
    """rho per ray of an H x W array of rays whose first row is absolute row `row0` of a frame of frame_h rows (default: the array is
    the frame).  which: -1 capped, else the sky; widths[k]: w of sky k.  Also returns what the partners were, for the tests' presence
    checks: dict of counts."""
    H, W = which.shape
    frame_h = H if frame_h is None else frame_h
    py, px = np.meshgrid(np.arange(H) + row0, np.arange(W), indexing="ij")
    rho = np.zeros((H, W), np.int64)
    seen = dict(outside=0, capped=0, other_sky=0, wrapped=0, used=0)
    w_of = np.where(which == 1, widths[1], widths[0]).astype(np.int64)
    for qx, qy in ((px ^ 1, py), (px, py ^ 1)):
        inside = (qx < W) & (qy < frame_h)
        assert ((qy - row0 < H) | ~inside).all() and (qy >= row0).all(), "the array must hold whole quads of the frame"
        jx, jy = np.minimum(qx, W - 1), np.minimum(qy - row0, H - 1)
        pw, pX, pY = which[jy, jx], Xc[jy, jx], Yc[jy, jx]
        own = which >= 0
        ok = own & inside & (pw == which)
        seen["outside"] += int((own & ~inside).sum())
        seen["capped"] += int((own & inside & (pw < 0)).sum())
        seen["other_sky"] += int((own & inside & (pw >= 0) & (pw != which)).sum())
        dX = wrap_abs(pX - Xc, w_of)
        seen["wrapped"] += int((ok & (dX != np.abs(pX - Xc))).sum())
        seen["used"] += int(ok.sum())
        dY = np.abs(pY - Yc)
        rho = np.where(ok, np.maximum(rho, np.maximum(dX, dY)), rho)
    return rho, seen


def level(rho, L):
    rho = np.asarray(rho, np.int64)
    msb = np.zeros(rho.shape, np.int64)
    for b in range(1, 33):
        msb = np.where(rho >> b > 0, b, msb)
    big = rho >= 256
    k = np.where(big, msb - 8, 0)
    f = np.where(big, (rho >> np.maximum(k, 0)) & 255, 0)
    top = k >= L - 1
    return np.where(top, L - 1, k), np.where(top, 0, f)


def level_colour(T, Xk, Yk):
    h, w = T.shape[:2]
    assert (Xk < 256 * w).all() and (Yk < 256 * h).all()
    x0, x1, y0, y1, fx, fy, _, _, _ = F.taps(Xk, Yk, w, h)
    return F.blend(T, x0, x1, y0, y1, fx, fy)


def colour(levels, Xc, Yc, rho):
    """[n, 3] uint8 for flat int arrays Xc, Yc, rho over the pyramid `levels`"""
    Xc, Yc = np.asarray(Xc, np.int64), np.asarray(Yc, np.int64)
    k, f = level(rho, len(levels))
    out = np.zeros(Xc.shape + (3,), np.uint8)
    for kk in sorted(set(k.tolist())):
        m = k == kk
        ck = level_colour(levels[kk], Xc[m] >> kk, Yc[m] >> kk).astype(np.int64)
        ff = f[m][:, None]
        if (ff != 0).any():
            ck1 = level_colour(levels[kk + 1], Xc[m] >> (kk + 1), Yc[m] >> (kk + 1)).astype(np.int64)
            mixed = ((256 - ff) * ck + ff * ck1 + 128) >> 8
            ck = np.where(ff != 0, mixed, ck)
        out[m] = ck.astype(np.uint8)
    return out, k, f


def mip_frame(which, Xc, Yc, real, row0=0, frame_h=None):
    """the frame of the definition from decoded rays (sky_filter_ref.decode): (frame, rho, k, f, partner counts); capped rays black"""
    widths = [t.shape[1] for t in real]
    rho, seen = footprint(which, Xc, Yc, widths, row0, frame_h)
    out = np.zeros(which.shape + (3,), np.uint8)
    K, Fr = np.zeros(which.shape, np.int64), np.zeros(which.shape, np.int64)
    for s, T in enumerate(real):
        m = which == s
        if m.any():
            out[m], K[m], Fr[m] = colour(pyramid(T), Xc[m], Yc[m], rho[m])
    return out, rho, K, Fr, seen


def directed_rhos(levels_max=24):
    vals = {0, 255, 256, 257, 511, 512, 2 ** 32 - 1}
    for k in range(0, levels_max + 1):
        for d in (-1, 0, 1):
            v = 256 * 2 ** k + d
            if 0 <= v < 2 ** 32:
                vals.add(v)
    return sorted(vals)
