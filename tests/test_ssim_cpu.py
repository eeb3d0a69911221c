"""CPU: nerf.eval.ssim_reference, the float64 numpy definition of the SSIM
that ngp_frame_ssim computes and the oracle of
tests/test_gpu_ssim.py."""
import numpy as np
import pytest

import ssim_helpers as sh

H, W = 37, 53


def _pair(kind, seed=0):
    """(x, y) float32 [H, W, 3]: flat, a nearly constant 0.999 image against a
    1e-3 perturbation of it; noise; smooth."""
    rng = np.random.default_rng(seed)
    if kind == "flat":
        y = np.full((H, W, 3), 0.999)
        x = y + 1e-3 * (rng.random((H, W, 3)) - 0.5)
    elif kind == "noise":
        x, y = rng.normal(0.3, 0.5, (H, W, 3)), rng.random((H, W, 3))
    else:
        x, y = sh.smooth(H, W, 0.4), sh.smooth(H, W, 0.0)
    return x.astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("kind", sh.KINDS)
def test_separable_against_direct(kind):
    from nerf.eval import ssim_reference
    x, y = _pair(kind)
    m, mean = ssim_reference(x, y)
    d = sh.direct_map(x, y)
    worst = float(np.abs(m - d).max())
    print(f"{kind}: separable vs direct 121-tap, worst {worst:.3e}")
    assert worst <= 1e-11
    assert mean == float(m.mean())
    if kind == "noise":
        assert m.min() < 0  # uncorrelated noise: values of both signs


@pytest.mark.parametrize("kind", sh.KINDS)
def test_identical_images(kind):
    from nerf.eval import ssim_reference
    x, _ = _pair(kind)
    m, mean = ssim_reference(x, x.copy())
    assert np.abs(m - 1).max() <= 1e-12 and abs(mean - 1) <= 1e-12


@pytest.mark.parametrize("a,b", [(0.0, 0.0), (0.25, 0.75), (1.0, 0.5), (0.999, 1.0)])
def test_constant_images(a, b):
    from nerf.eval import ssim_reference
    x, y = np.full((H, W, 3), a, np.float32), np.full((H, W, 3), b, np.float32)
    m, _ = ssim_reference(x, y)
    a, b = float(np.float32(a)), float(np.float32(b))
    # the variances are 0 up to the rounding of the windowed sums, against C2 = 9e-4
    assert np.abs(m - (2 * a * b + sh.C1) / (a * a + b * b + sh.C1)).max() <= 1e-12


@pytest.mark.parametrize("kind", sh.KINDS)
def test_symmetric(kind):
    from nerf.eval import ssim_reference
    x, y = _pair(kind)
    m, mean = ssim_reference(x, y)
    n, mean2 = ssim_reference(y, x)
    assert np.abs(m - n).max() <= 1e-15 and abs(mean - mean2) <= 1e-15


def test_shape_and_smallest_size():
    from nerf.eval import ssim_reference
    x, y = _pair("smooth")
    m, _ = ssim_reference(x, y)
    assert m.shape == (H - 10, W - 10, 3) and m.dtype == np.float64
    m1, mean1 = ssim_reference(x[:11, :11], y[:11, :11])
    assert m1.shape == (1, 1, 3) and abs(mean1 - float(m[0, 0].mean())) <= 1e-15
    assert np.array_equal(m1[0, 0], m[0, 0])  # a position depends on its window alone
    for bad in ((10, 11), (11, 10)):
        with pytest.raises(ValueError, match="11"):
            ssim_reference(x[:bad[0], :bad[1]], y[:bad[0], :bad[1]])
    with pytest.raises(ValueError):
        ssim_reference(x.astype(np.float64), y)
    with pytest.raises(ValueError):
        ssim_reference(x[..., :2], y[..., :2])


def test_weights():
    from nerf.eval import ssim_weights
    g = ssim_weights()
    assert g.shape == (11,) and g.dtype == np.float64
    assert abs(g.sum() - 1) <= 1e-15 and np.array_equal(g, g[::-1])
    assert abs(g[5] - 0.26601172) <= 5e-9
    k = np.arange(11) - 5.0
    e = np.exp(-k * k / 4.5)
    assert np.allclose(g, e / e.sum(), rtol=0, atol=1e-16)
