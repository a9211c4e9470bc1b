"""The index skies of tests/common.py (colour == texel index) and the array form of the oracle's sky lookup -- the two pieces of
test infrastructure tests/test_gpu_sky_lookup.py stands on, checked on the CPU."""
import ctypes as C

import numpy as np
import pytest

import common
import oracle_lib as O


@pytest.mark.parametrize("w,h,salt", [(4096, 4096, 0x5A17E5), (1, 1, 0xFFFFFF), (333, 777, 0), (4001, 1999, 0x0F00F0)])
def test_index_sky_is_injective_and_inverts(w, h, salt):
    img = common.index_sky(w, h, salt)
    assert img.shape == (h, w, 4) and img.dtype == np.uint8 and img.flags.c_contiguous and (img[..., 3] == 255).all()
    packed = img[..., 0].astype(np.uint32) | (img[..., 1].astype(np.uint32) << 8) | (img[..., 2].astype(np.uint32) << 16)
    assert np.unique(packed).size == w * h                       # injective: every texel its own colour
    x, y = common.texel_of(img[..., :3], salt)
    assert np.array_equal(x, np.broadcast_to(np.arange(w)[None, :], (h, w)))
    assert np.array_equal(y, np.broadcast_to(np.arange(h)[:, None], (h, w)))
    assert common.texel_of(img[h - 1, w - 1, :3], salt) == (w - 1, h - 1)


def test_two_salts_never_share_a_colour_at_the_same_texel():
    a, b = common.index_sky(300, 200, 0x123456), common.index_sky(300, 200, 0x123457)
    assert ((a[..., :3] != b[..., :3]).any(axis=2)).all()
    assert common.describe_texel(a[7, 12, :3], [(300, 200), (5, 5)], [0x123456, 0x123457]) == "sky 0 (12, 7)"


def test_oracle_sky_indices_array_equals_the_scalar_call():
    rng = np.random.default_rng(11)
    d = rng.standard_normal((4000, 3))
    d[:9] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [-1, -0.0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0], [np.nan, 1, 1]]
    fwd, up = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    rot, inv, upo = np.zeros(9), np.zeros(9), np.zeros(3)
    assert O.lib().cvo_orientation_new(O._dp(fwd), O._dp(up), O._dp(rot), O._dp(inv), O._dp(upo)) == 0
    for fl in (O.CV, O.LIBM):
        for (w, h), m in (((1000, 500), None), ((7, 4096), inv), ((2 ** 32 - 1, 3), None)):
            s = O.sky_shape(w, h, m)
            got = O.sky_indices_array(fl, s, d)
            x, y = C.c_uint32(0), C.c_uint32(0)
            for i in range(len(d)):
                O.lib().cvo_sky_indices(fl, C.byref(s), O._dp(d[i]), C.byref(x), C.byref(y))
                assert (got[i, 0], got[i, 1]) == (x.value, y.value), (fl, w, h, i, d[i])
            if m is None:
                assert got[1, 1] == h   # theta = pi: ty == h, the reason n_oob exists
