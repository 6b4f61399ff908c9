"""-m gpu: the reflect-padded blur operator of the deblurring program and its adjoint (csrc/blur.hip: dpir_blur_reflect,
dpir_blur_reflect_adjoint, the fused residual of dpir_grad_and_value_blur) against the float64 statements of tests/blur_f64.py with the
plane-wise checker of tests/ops_f64.py, an exact one-hot case, batch independence bit for bit, and the shape rejections."""
import ctypes as C

import numpy as np
import pytest
import torch

import diffpir_amd
from diffpir_amd import utils_model
from diffpir_amd.utils_deblur import BlurOperator
from tests import blur_f64 as BF
from tests import ops_f64 as OF

pytestmark = pytest.mark.gpu

# (B, H, W, K): plane smaller than a tile with p = H - 1 (an interior pixel reflected from both sides); non-square; halo ~ tile; the
# workloads' PSF at the smallest image that admits it; identity; one workload-sized case
SHAPES = [(1, 7, 9, 13), (2, 24, 40, 5), (3, 32, 32, 31), (1, 64, 64, 61), (1, 16, 16, 1), (2, 256, 256, 61)]


@pytest.fixture(scope="module")
def engine():
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


def _psfs(B, K, rng):
    """Per-image PSFs: image 0 a normalised Gaussian-like bump, image 1 with negative lobes and not normalised, image 2 a random positive one."""
    ax = np.arange(K) - K // 2
    out = []
    for n in range(B):
        if n % 3 == 0:
            s = 0.15 * K + 0.5
            k = np.exp(-(ax[:, None] ** 2 + (0.5 * ax[None, :]) ** 2) / (2 * s * s))
            k /= k.sum()
        elif n % 3 == 1:
            r = np.hypot(ax[:, None] + 0.3, ax[None, :] - 0.2)
            k = np.cos(1.3 * r) * np.exp(-r / (0.2 * K + 1)) * 0.37
        else:
            k = rng.random((K, K)) / (K * K) * 1.1
        out.append(k)
    return np.stack(out)[:, None].astype(np.float32)


_CASES = {}


def _case(shape):
    """Inputs and the float64 / float32 torch statements of one shape, computed once and shared by the tests."""
    if shape not in _CASES:
        B, H, W, K = shape
        rng = np.random.default_rng(1000 + H * 7 + K)
        x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
        g = rng.standard_normal((B, 3, H, W)).astype(np.float32)
        if B > 1:                       # an error in a small image cannot hide under a batch maximum
            x[1] *= np.float32(1e-3)
            g[1] *= np.float32(1e-3)
        k = _psfs(B, K, rng)
        tx, tg, tk = torch.from_numpy(x), torch.from_numpy(g), torch.from_numpy(k)
        with torch.no_grad():
            f64, f32 = BF.blur_reflect(tx, tk).numpy(), BF.blur_reflect(tx, tk, dtype=torch.float32).numpy()
        a64, a32 = BF.blur_reflect_adjoint(tg, tk).numpy(), BF.blur_reflect_adjoint(tg, tk, dtype=torch.float32).numpy()
        _CASES[shape] = dict(x=x, g=g, k=k, f64=f64, f32=f32, a64=a64, a32=a32)
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_adjoint_against_float64(engine, shape):
    """e_p <= max(K o_p, FLOOR) on every (image, channel) plane, K and FLOOR those of tests/ops_f64.py, o_p torch's own float32 evaluation."""
    c = _case(shape)
    op = BlurOperator(c["k"], engine=engine)
    out = op(engine.to_device(c["x"])).numpy()
    gx = op.transpose(engine.to_device(c["g"])).numpy()
    sf = OF.stats(out, c["f64"], c["f32"])
    sa = OF.stats(gx, c["a64"], c["a32"])
    print(f"blur {shape}: forward e_p/o_p {sf['ratio']:.3f} (e {sf['e']:.3e}), adjoint e_p/o_p {sa['ratio']:.3f} (e {sa['e']:.3e})")
    OF.check(out, c["f64"], c["f32"], f"blur_reflect {shape}", K=BF.K_RATIO, F=BF.FLOOR)
    OF.check(gx, c["a64"], c["a32"], f"blur_reflect_adjoint {shape}", K=BF.K_RATIO, F=BF.FLOOR)


def _reflect(t, L):
    t = np.where(t < 0, -t, t)
    return np.where(t > L - 1, 2 * (L - 1) - t, t)


def test_one_hot_psf_is_an_exact_reflected_shift(engine):
    """A one-hot PSF of 1.0 placed off-centre and off the main diagonal: the forward output is float32(x * 0.5 + 0.5) gathered through the
    reflected shift and the adjoint the matching scatter, both exactly -- a flipped PSF, a repeated edge sample or swapped axes all show."""
    B, H, W, K = 2, 9, 12, 7
    p = K // 2
    taps = [(1, 5), (6, 2)]
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    g = rng.integers(-64, 65, (B, 3, H, W)).astype(np.float32)          # integer-valued: the scatter's sums are exact in any order
    k = np.zeros((B, 1, K, K), np.float32)
    for n, (a, b) in enumerate(taps):
        k[n, 0, a, b] = 1.0
    op = BlurOperator(k, engine=engine)
    out = op(engine.to_device(x)).numpy()
    gx = op.transpose(engine.to_device(g)).numpy()
    v = x * np.float32(0.5) + np.float32(0.5)
    want_f, want_a = np.empty_like(x), np.zeros_like(x)
    for n, (a, b) in enumerate(taps):
        ri, rj = _reflect(np.arange(H) + a - p, H), _reflect(np.arange(W) + b - p, W)
        want_f[n] = v[n][:, ri][:, :, rj]
        for i in range(H):
            for j in range(W):
                want_a[n, :, ri[i], rj[j]] += g[n, :, i, j]
    want_a *= np.float32(0.5)
    assert np.array_equal(out, want_f)
    assert np.array_equal(gx, want_a)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] > 1], ids=lambda s: "x".join(map(str, s)))
def test_image_n_of_a_batch_equals_the_image_alone(engine, shape):
    """Forward, adjoint and the fused residual with its per-image norm (dpir_grad_and_value_blur, x is x_hat): bit for bit."""
    c = _case(shape)
    B = shape[0]
    meas = np.random.default_rng(9).random(c["x"].shape).astype(np.float32)
    op = BlurOperator(c["k"], engine=engine)
    xd, gd, md = engine.to_device(c["x"]), engine.to_device(c["g"]), engine.to_device(meas)
    out, gx = op(xd).numpy(), op.transpose(gd).numpy()
    ng, nv = utils_model.grad_and_value(operator=op, x=xd, x_hat=xd, measurement=md)
    ng, nv = ng.numpy(), nv.numpy()
    for n in range(B):
        one = BlurOperator(c["k"][n:n + 1], engine=engine)
        x1, g1, m1 = engine.to_device(c["x"][n:n + 1]), engine.to_device(c["g"][n:n + 1]), engine.to_device(meas[n:n + 1])
        assert np.array_equal(one(x1).numpy()[0], out[n]), ("forward", n)
        assert np.array_equal(one.transpose(g1).numpy()[0], gx[n]), ("adjoint", n)
        ng1, nv1 = utils_model.grad_and_value(operator=one, x=x1, x_hat=x1, measurement=m1)
        assert np.array_equal(ng1.numpy()[0], ng[n]) and nv1.numpy()[0] == nv[n], ("residual", n)
    # and the norm is each image's own: against the float64 statement of the forward operator (shared with the test above)
    n64 = np.sqrt(((meas.astype(np.float64) - c["f64"]) ** 2).reshape(B, -1).sum(axis=1))
    assert np.abs(nv / n64 - 1).max() < 1e-5, (nv, n64)


@pytest.mark.parametrize("B,H,W,kh,kw", [(1, 16, 16, 5, 7), (1, 16, 16, 4, 4), (1, 4, 16, 9, 9), (1, 16, 4, 9, 9), (0, 16, 16, 5, 5)],
                         ids=["kh!=kw", "even_K", "p>=H", "p>=W", "B<=0"])
def test_shape_rejections_launch_nothing(engine, B, H, W, kh, kw):
    """DPIR_ERR_INVALID before anything is allocated or enqueued: the profiler counts no launch.  The buffers would hold a legal call."""
    buf = engine.empty((3 * 16 * 16,))
    k = engine.empty((9 * 9,))
    engine.sync()
    engine.prof_enable(True)
    engine.prof_reset()
    lib, h = engine.lib, engine.h
    try:
        got = [lib.dpir_blur_reflect(h, buf.ptr, k.ptr, kh, kw, 0.5, 0.5, buf.ptr, B, H, W),
               lib.dpir_blur_reflect_adjoint(h, buf.ptr, k.ptr, kh, kw, 0.5, buf.ptr, B, H, W),
               lib.dpir_grad_and_value_blur(h, 0, buf.ptr, buf.ptr, k.ptr, kh, kw, buf.ptr, None, B, H, W)]
        counts = {nm: c for nm, (ms, c) in engine.prof_read().items()}
    finally:
        engine.prof_enable(False)
    assert got == [-1, -1, -1], (got, engine.lib.dpir_last_error(engine.h))
    assert all(c == 0 for c in counts.values()), counts
    engine.sync()
