"""mdg_min_image_fused_inv (csrc/traj_small.hip, host only): the multiplier inv' with which the ring kernels' three-instruction
minimum image, o = fma(d, inv', M) - M = rint of the EXACT product d inv', picks the image that the four-instruction form,
rint(fl(d inv)), picks -- for every float d the window form can meet (|d inv| < 1.5; the window test keeps |d inv| below 1.48).

Both forms are monotone in d and odd, so they can differ only where they leave image 0: around +-tau, tau = the smallest d > 0
with fl(d inv) > 0.5.  The test finds tau on its own (numpy float32 products), compares the two forms for every float within
4096 ulps of +-tau and for 1e5 random d, and pins the cells the kernels' records name.  Exact products: a product of two
float32 has 48 significant bits and is exact in float64; numpy's rint rounds halves to even, like the fma's one rounding
(12582912 + x, |x| < 2^22, has one-unit spacing, so that rounding IS rint(x) to nearest-even)."""
import ctypes as C

import numpy as np
import pytest

from mdgrad_amd import _lib

F = np.float32


def _fused(h, inv=None):
    h = F(h)
    inv = F(1.0) / h if inv is None else F(inv)
    out = C.c_float(0.0)
    ok = _lib.load().mdg_min_image_fused_inv(C.c_float(float(h)), C.c_float(float(inv)), C.byref(out))
    return (F(out.value) if ok else None), inv


def _tau(h, inv):
    """smallest float d > 0 with fl(d inv) > 0.5, by stepping floats around h / 2"""
    t = F(0.5) * F(h)
    while F(np.nextafter(t, F(0)) * inv) > F(0.5):
        t = np.nextafter(t, F(0))
    while not F(t * inv) > F(0.5):
        t = np.nextafter(t, F(np.inf))
    return F(t)


def _reference(d, inv):
    return np.rint((d * inv).astype(F))                                   # the product rounded to float32 first


def _exact(d, c):
    return np.rint(d.astype(np.float64) * np.float64(c))                  # exact product, one rounding


def _around(t, n):
    bits = np.array(t, dtype=F).view(np.int32).astype(np.int64) + np.arange(-n, n + 1)
    d = bits.astype(np.int32).view(F)
    return np.concatenate([d, -d])


def test_headline_cell_takes_the_neighbour_below():
    c, inv = _fused(4.8)
    assert inv == F(0.20833333) and c == np.nextafter(inv, F(0)) and abs(float(c) - 0.20833331) < 1e-8
    assert _tau(F(4.8), inv) == F(2.4000003)


@pytest.mark.parametrize("h", [4.0, 4.9, 5.2, 8.0])
def test_inv_itself_is_preferred(h):
    c, inv = _fused(h)
    assert c is not None and c == inv


@pytest.mark.parametrize("h", [6.4, 7.2, 3.2])
def test_cells_without_a_multiplier(h):
    assert _fused(h)[0] is None


def test_degenerate_arguments_have_no_multiplier():
    for h, inv in ((0.0, 1.0), (-4.8, -0.2), (4.8, 0.0), (float("inf"), 0.0), (float("nan"), 0.2), (4.8, float("nan"))):
        assert _fused(h, inv)[0] is None
    assert _lib.load().mdg_min_image_fused_inv(C.c_float(4.8), C.c_float(1.0 / 4.8), None) == 0


def test_fused_form_picks_the_reference_image():
    rng = np.random.default_rng(20240)
    hs = rng.uniform(2.0, 60.0, 200).astype(F)
    found = 0
    for h in hs:
        c, inv = _fused(h)
        if c is None:
            continue
        found += 1
        assert abs(int(c.view(np.int32)) - int(inv.view(np.int32))) <= 4
        t = _tau(h, inv)
        d = _around(t, 4096)
        assert np.array_equal(_reference(d, inv), _exact(d, c)), "h = %r: around tau" % h
        d = (rng.uniform(-1.48, 1.48, 100000) * float(h)).astype(F)
        d = d[np.abs((d * inv).astype(F)) < F(1.48)]
        assert np.array_equal(_reference(d, inv), _exact(d, c)), "h = %r: random d" % h
    assert found >= 100                                                   # (a multiplier exists for roughly four cells in five)
