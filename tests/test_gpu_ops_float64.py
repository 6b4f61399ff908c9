"""-m gpu: the non-FFT data steps and the loop arithmetic (csrc/elem.hip, csrc/degrade.hip, the elementwise / resampling tail of csrc/grad.hip)
through the C ABI, by shape: non-square images, lengths that are no power of two, sf 2 / 3 / 4 / 5 / 8, planes smaller than one workgroup, the
grid-stride branch, even / image-sized PSFs.

  * resampling family (dpir_resize_down, dpir_bicubic_up, dpir_prox_ibp, dpir_grad_and_value(through_network = 0), dpir_degrade for sr): against
    the float64 statements of tests/ops_f64.py through its plane-wise checker, e_p <= max(K o_p, FLOOR);
  * expression-mirroring kernels (dpir_prox_mask, dpir_repaint_mix, dpir_renoise, dpir_eps_from_xstart, dpir_ewise, dpir_finalize, the blur's
    quantised output, u8 -> single, the noise finish): array_equal with the same expression in numpy float32, one rounding per operation;
  * dpir_metrics against a float64 PSNR at the suite's 2e-5 dB;
  * for every entry: image n of a batch equals, bit for bit, the same image run alone; in-place forms equal out-of-place ones;
  * the shape checks of the entries (DPIR_ERR_INVALID before anything is divided, allocated or enqueued), last in the file.

K and the floor of the checker and the figures measured on the MI355X: tests/ops_f64.py.  The 268 M-element cap of grid1d is not reachable at
a sensible test size (> 1 GB per tensor) and is not exercised; launch_ewise's 65 536-workgroup cap is, with 32 x 3 x 512 x 512 elements."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffpir_amd import degrade as dgr, schedule
from diffpir_amd.engine import device_count
from oracle import diffpir_oracle as do
from tests import ops_f64 as F

pytestmark = pytest.mark.gpu

# (H, W, sf, B)
GRID = [(48, 80, 2, 3), (24, 36, 3, 1), (96, 40, 4, 5), (16, 128, 8, 2), (30, 50, 5, 1), (256, 256, 2, 16), (256, 256, 4, 16), (512, 512, 4, 8),
        (6, 9, 3, 1)]
# (B, H, W) of the elementwise cases: non-square and tiny shapes of the grid
ELEM_SHAPES = [(1, 6, 9), (3, 48, 80), (5, 96, 40), (2, 16, 128), (1, 30, 50)]
BIG = (32, 512, 512)            # 25.2 M elements: more than launch_ewise's 65 536 workgroups of 256 cover in one pass
SCHEDULES = [(eta, zeta) for eta in (0.0, 0.7) for zeta in (0.0, 0.3, 1.0)]
_ids = lambda v: "x".join(str(q) for q in v)      # noqa: E731


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


_cache = {}


def cached(key, fn):
    """The float64 reference of one shape is computed once."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def probe(shape, seed, lo=0.0, hi=1.0):
    """float32 [B, 3, H, W] uniform in [lo, hi); image 1 of a batch is scaled by 1e-3, so that an error cannot hide under a batch-wide maximum."""
    x = (lo + (hi - lo) * np.random.default_rng(seed).random(shape)).astype(np.float32)
    if shape[0] > 1:
        x[1] *= np.float32(1e-3)
    return x


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ====================================================================================================================== resampling family
def _resize(engine, x, sf):
    B, _, H, W = x.shape
    xd, out = engine.to_device(x), engine.empty((B, 3, H // sf, W // sf))        # xd stays referenced until the result is read back
    engine._check(engine.lib.dpir_resize_down(engine.h, xd.ptr, out.ptr, sf, B, H, W))
    return out.numpy()


@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_resize_down(engine, case):
    H, W, sf, B = case
    x = probe((B, 3, H, W), 1)
    out = _resize(engine, x, sf)
    f64 = cached(("down", case), lambda: F.resize_down(x, sf))
    F.check(out, f64, do.resizer_apply(t32(x), 1.0 / sf).numpy(), f"resize_down {case}")
    assert np.array_equal(_resize(engine, x[B - 1:], sf), out[B - 1:])


def _degrade_sr(engine, gt, sf):
    y, _ = dgr.degrade(engine, "sr", gt, noise_level_img=0.0, sf=sf, sr_mode="cubic")
    return y.numpy()


@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_degrade_sr(engine, case):
    """dpir_degrade, task sr: u8 -> single and the Resizer at every shape of the grid (sf 2, 3, 4, 5, 8; non-square)."""
    H, W, sf, B = case
    gt = np.random.default_rng(2).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    if B > 1:
        gt[1] //= 64                                              # a dark image next to bright ones
    single = F.u8_to_single(gt)
    out = _degrade_sr(engine, gt, sf)
    # the fp32 oracle is the whole operation: the noise finish runs at level 0 too, and its * 2 - 1, / 2 + .5 round trip in float32
    # (main_ddpir.py:112-114 on the float32 img_L) costs up to 3e-8 absolute -- 3e-6 of the dark image's maximum
    o32 = F.noise_finish_f32(do.resizer_apply(t32(single), 1.0 / sf).numpy(), None, 0.0)
    F.check(out, F.resize_down(single, sf), o32, f"degrade sr {case}")
    assert np.array_equal(_degrade_sr(engine, gt[B - 1:], sf), out[B - 1:])


def _bicubic(engine, y, sf):
    B, _, h, w = y.shape
    yd, out = engine.to_device(y), engine.empty((B, 3, h * sf, w * sf))
    engine._check(engine.lib.dpir_bicubic_up(engine.h, yd.ptr, out.ptr, sf, B, h, w))
    return out.numpy()


@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_bicubic_up(engine, case):
    H, W, sf, B = case
    y = probe((B, 3, H // sf, W // sf), 3)
    out = _bicubic(engine, y, sf)
    o32 = torch.nn.functional.interpolate(t32(y), size=(H, W), mode="bicubic", align_corners=False).numpy()
    F.check(out, F.bicubic_up(y, sf), o32, f"bicubic_up {case}")
    assert np.array_equal(_bicubic(engine, y[B - 1:], sf), out[B - 1:])


def _ibp(engine, x0, y, rho, gamma, in_iter, sf):
    B, _, H, W = x0.shape
    d, yd = engine.to_device(x0), engine.to_device(y)
    engine._check(engine.lib.dpir_prox_ibp(engine.h, d.ptr, yd.ptr, rho, gamma, in_iter, sf, B, H, W))
    return d.numpy()


@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_prox_ibp(engine, case):
    H, W, sf, B = case
    x0 = probe((B, 3, H, W), 4, -1.0, 1.0)
    y = probe((B, 3, H // sf, W // sf), 5)
    for in_iter, gamma, rho in ((1, 0.01, 0.2), (3, 0.5, 0.37), (3, 1.0, 1e-3)):
        rho32 = float(np.float32(rho))
        out = _ibp(engine, x0, y, rho, gamma, in_iter, sf)
        f64 = F.prox_ibp(x0, y, rho32, float(np.float32(gamma)), sf, in_iter)
        o32 = do.prox_ibp(t32(x0), t32(y), torch.tensor(rho32), sf, float(np.float32(gamma)), in_iter).numpy()
        F.check(out, f64, o32, f"prox_ibp {case} in_iter {in_iter} gamma {gamma} rho {rho}")
    assert np.array_equal(_ibp(engine, x0[B - 1:], y[B - 1:], rho, gamma, in_iter, sf), out[B - 1:])


def _grad(engine, x, m, sf):
    g, nv = engine.grad_and_value(False, engine.to_device(x), m if not isinstance(m, np.ndarray) else engine.to_device(m), sf)
    return g.numpy(), float(nv.numpy()[0])


def _check_grad(engine, x, m, sf, label):
    g, nv = _grad(engine, x, m, sf)
    g64, n64 = F.grad_and_value(x, m, sf)
    xr = t32(x).requires_grad_()
    n32 = torch.linalg.norm(t32(m) - do.resizer_apply(xr, 1.0 / sf))
    g32 = torch.autograd.grad(n32, xr)[0].numpy()
    F.check(g, g64, g32, label + " gradient")
    en, on = abs(nv - n64) / n64, abs(float(n32.detach()) - n64) / n64
    print(f"ops_f64 {label} norm: e {en:.3e}, fp32 oracle {on:.3e}")
    assert en <= max(F.K_RATIO * on, F.FLOOR), (label, nv, n64, float(n32.detach()))
    return g, nv


@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_grad_and_value_without_the_network(engine, case):
    """dpir_grad_and_value(through_network = 0): diff_norm, both band_resample_T passes and neg_scale_by_norm.  (i) norm and gradient against
    float64; (ii) the adjoint identity <R x, v> = <x, R^T v> in float64, R^T v obtained from the engine with x_hat = 0 and measurement v (then
    diff = v exactly and the output is -R^T v / ||v||); every element of R^T v is a sum of at most taps_H + taps_W <= 70 fp32 fused
    multiply-adds, so its error is below 70 * 2^-24 * (|R|^T |v|) = 4.2e-6 of the absolute sum, and the two roundings of / norm, * norm add
    1.2e-7: the identity is held to 1e-5 sum |x| (|R|^T |v|); (iii) a DPS_yt-style measurement sa m + s1m n formed by the stepwise plugs
    (dpir_ewise)."""
    H, W, sf, B = case
    h, w = H // sf, W // sf
    x = probe((B, 3, H, W), 6, -1.0, 1.0)
    m = probe((B, 3, h, w), 7, -1.0, 1.0)
    g, nv = _check_grad(engine, x, m, sf, f"grad_and_value {case}")
    if B > 1:         # the norm is batch-wide: image n alone has its own norm, and gradient * norm is the per-image quantity
        g1, n1 = _grad(engine, x[B - 1:], m[B - 1:], sf)
        a, b = g1.astype(np.float64) * n1, g[B - 1:].astype(np.float64) * nv
        assert np.abs(a - b).max() <= 4 * 2.0 ** -24 * np.abs(b).max()
    # (ii)
    rng = np.random.default_rng(8)
    v = rng.standard_normal((B, 3, h, w)).astype(np.float32)
    gz, nz = _grad(engine, np.zeros_like(x), v, sf)
    RTv = -gz.astype(np.float64) * nz
    xp = rng.standard_normal((B, 3, H, W))
    lhs, rhs = float((F.resize_down(xp, sf) * v).sum()), float((xp * RTv).sum())
    th, tw = F.tables(H, sf), F.tables(W, sf)
    absRT = F.scatter_axis(F.scatter_axis(np.abs(v), np.abs(tw[0]), tw[1], W, -1), np.abs(th[0]), th[1], H, -2)
    scale = float((np.abs(xp) * absRT).sum())
    print(f"ops_f64 adjoint {case}: <Rx, v> {lhs:.9e} <x, RTv> {rhs:.9e} |diff| / sum|x||R|T|v| {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 1e-5 * scale
    # the borders of the transposed resampler on their own: R^T v against the float64 scatter, plane by plane
    xr = t32(x).requires_grad_()
    RTv32 = torch.autograd.grad((do.resizer_apply(xr, 1.0 / sf) * t32(v)).sum(), xr)[0].numpy()
    F.check(RTv, F.resize_down_T(v, sf), RTv32, f"band_resample_T {case}")
    # (iii)
    _, steps, _ = schedule.build_steps(iter_num=10, sigma=0.05, lambda_=7.0, zeta=0.3, generate_mode="DPS_yt")
    sa, s1m = np.float32(steps[3]["sa_t"]), np.float32(steps[3]["s1m_t"])
    n = rng.standard_normal((B, 3, h, w)).astype(np.float32)
    yt = sa * engine.to_device(m) + s1m * engine.to_device(n)
    yt_ref = sa * m + s1m * n
    assert np.array_equal(yt.numpy(), yt_ref)
    gd, nd = _grad(engine, x, yt, sf)
    g64, n64 = F.grad_and_value(x, yt_ref, sf)
    xr = t32(x).requires_grad_()
    n32 = torch.linalg.norm(t32(yt_ref) - do.resizer_apply(xr, 1.0 / sf))
    F.check(gd, g64, torch.autograd.grad(n32, xr)[0].numpy(), f"grad_and_value DPS_yt {case}")
    assert abs(nd - n64) / n64 <= max(F.K_RATIO * abs(float(n32.detach()) - n64) / n64, F.FLOOR)


# ====================================================================================================================== expression mirrors
def masks(shape, rng):
    """name -> uint8 [B, 3, H, W]: all 0, all 1, random per pixel (one mask for the three channels), different per channel."""
    B, _, H, W = shape
    per_pixel = np.ascontiguousarray(np.broadcast_to(rng.integers(0, 2, (B, 1, H, W), dtype=np.uint8), shape))
    return {"zeros": np.zeros(shape, np.uint8), "ones": np.ones(shape, np.uint8), "pixel": per_pixel,
            "channel": rng.integers(0, 2, shape, dtype=np.uint8)}


def ulps(a, b):
    """Largest distance in units of the last place between two float32 arrays (0 when they are array_equal)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max())


def same_bits(got, ref, label):
    d = ulps(got, ref)
    if d:
        print(f"ops_f64 {label}: NOT bit-equal, {d} ulp, max |diff| {np.abs(got.astype(np.float64) - ref).max():.3e}")
    assert np.array_equal(got, ref), (label, d)


def _prox_mask(engine, x0, y, m, tau, g):
    B, _, H, W = x0.shape
    d, yd, md = engine.to_device(x0), engine.to_device(y), engine.to_device(m)
    engine._check(engine.lib.dpir_prox_mask(engine.h, d.ptr, yd.ptr, md.ptr, tau, g, B, H, W))
    return d.numpy()


@pytest.mark.parametrize("shape", ELEM_SHAPES, ids=_ids)
def test_prox_mask_bits(engine, shape):
    B, H, W = shape
    rng = np.random.default_rng(10)
    x0, y = probe((B, 3, H, W), 11, -1.0, 1.0), probe((B, 3, H, W), 12)
    for name, m in masks((B, 3, H, W), rng).items():
        for tau, g in ((4e-11, 1.0), (1e-4, 0.7), (0.3, 1.0), (1e3, 0.7)):
            out = _prox_mask(engine, x0, y, m, tau, g)
            same_bits(out, F.prox_mask_f32(x0, y, m, tau, g), f"prox_mask {shape} mask {name} tau {tau}")
            assert np.abs(out - F.prox_mask(x0, y, m, float(np.float32(tau)), float(np.float32(g)))).max() <= 1e-5
    assert np.array_equal(_prox_mask(engine, x0[B - 1:], y[B - 1:], m[B - 1:], tau, g), out[B - 1:])


def _steps(eta, zeta):
    _, steps, arr = schedule.build_steps(iter_num=10, sigma=0.05, lambda_=7.0, zeta=zeta, eta=eta)
    return steps, arr


def _repaint(engine, x, y, m, n, st):
    B, _, H, W = x.shape
    d, yd, md, nd = engine.to_device(x), engine.to_device(y), engine.to_device(m), engine.to_device(n)
    engine._check(engine.lib.dpir_repaint_mix(engine.h, d.ptr, yd.ptr, md.ptr, C.byref(st), nd.ptr, B, H, W))
    return d.numpy()


@pytest.mark.parametrize("shape", ELEM_SHAPES, ids=_ids)
def test_repaint_mix_bits(engine, shape):
    B, H, W = shape
    rng = np.random.default_rng(13)
    x, n = (rng.standard_normal((B, 3, H, W)).astype(np.float32) for _ in range(2))
    y = probe((B, 3, H, W), 14)
    for name, m in masks((B, 3, H, W), rng).items():
        for eta, zeta in SCHEDULES:
            steps, arr = _steps(eta, zeta)
            for i in (0, 4, len(steps) - 1):
                out = _repaint(engine, x, y, m, n, arr[i])
                same_bits(out, F.repaint_mix_f32(x, y, m, n, steps[i]["sa_t"], steps[i]["s1m_t"]), f"repaint_mix {shape} mask {name} eta {eta} zeta {zeta} step {i}")
                assert np.abs(out - F.repaint_mix(x, y, m, n, steps[i]["sa_t"], steps[i]["s1m_t"])).max() <= 1e-5
    assert np.array_equal(_repaint(engine, x[B - 1:], y[B - 1:], m[B - 1:], n[B - 1:], arr[i]), out[B - 1:])


def _renoise(engine, x, x0, st, n1, n2):
    B, _, H, W = x.shape
    d, x0d, n1d, n2d = engine.to_device(x), engine.to_device(x0), engine.to_device(n1), engine.to_device(n2)
    engine._check(engine.lib.dpir_renoise(engine.h, d.ptr, x0d.ptr, C.byref(st), n1d.ptr, n2d.ptr, B, H, W))
    return d.numpy()


@pytest.mark.parametrize("shape", ELEM_SHAPES, ids=_ids)
def test_renoise_bits(engine, shape):
    """With (eta 0.7) and without the eta term, zeta 0 / 0.3 / 1, at three steps of each schedule."""
    B, H, W = shape
    rng = np.random.default_rng(15)
    x, x0, n1, n2 = (rng.standard_normal((B, 3, H, W)).astype(np.float32) for _ in range(4))
    for eta, zeta in SCHEDULES:
        steps, arr = _steps(eta, zeta)
        for i in (0, 4, len(steps) - 2):
            out = _renoise(engine, x, x0, arr[i], n1, n2)
            same_bits(out, F.renoise_f32(x, x0, steps[i], n1, n2), f"renoise {shape} eta {eta} zeta {zeta} step {i}")
            ref = F.renoise(x, x0, steps[i], n1, n2)
            assert np.abs(out - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    assert np.array_equal(_renoise(engine, x[B - 1:], x0[B - 1:], arr[i], n1[B - 1:], n2[B - 1:]), out[B - 1:])


@pytest.mark.parametrize("shape", ELEM_SHAPES, ids=_ids)
def test_eps_from_xstart_bits(engine, shape):
    B, H, W = shape
    rng = np.random.default_rng(16)
    x, x0 = (rng.standard_normal((B, 3, H, W)).astype(np.float32) for _ in range(2))
    steps, _ = _steps(0.0, 0.3)
    for i in (0, 4, len(steps) - 1):
        sa, s1m = steps[i]["sa_t"], steps[i]["s1m_t"]
        for score in (0, 1):
            xd, x0d, out = engine.to_device(x), engine.to_device(x0), engine.empty(x.shape)
            engine._check(engine.lib.dpir_eps_from_xstart(engine.h, xd.ptr, x0d.ptr, sa, s1m, score, out.ptr, x.size))
            same_bits(out.numpy(), F.eps_from_xstart_f32(x, x0, sa, s1m, score), f"eps_from_xstart {shape} step {i} score {score}")
            ref = F.eps_from_xstart(x, x0, float(np.float32(sa)), float(np.float32(s1m)), score)
            assert np.abs(out.numpy() - ref).max() <= 1e-6 * np.abs(ref).max()
            engine._check(engine.lib.dpir_eps_from_xstart(engine.h, xd.ptr, x0d.ptr, sa, s1m, score, xd.ptr, x.size))     # in place
            assert np.array_equal(xd.numpy(), out.numpy())
            xa, x0a, alone = engine.to_device(x[B - 1:]), engine.to_device(x0[B - 1:]), engine.empty(x[B - 1:].shape)
            engine._check(engine.lib.dpir_eps_from_xstart(engine.h, xa.ptr, x0a.ptr, sa, s1m, score, alone.ptr, x[B - 1:].size))
            assert np.array_equal(alone.numpy(), out.numpy()[B - 1:])


def _ewise_all(engine, a, b, label):
    """The six ops with a tensor, a one-element tensor and a scalar on the right, out of place and in place."""
    one = np.array([b.ravel()[3]], np.float32)
    bd, oned = engine.to_device(b), engine.to_device(one)
    for op in range(6):
        for kind, args, rhs in (("tensor", (bd.ptr, b.size, 0.0), b), ("one", (oned.ptr, 1, 0.0), one[0]), ("scalar", (None, 0, float(one[0])), one[0])):
            ad, out = engine.to_device(a), engine.empty(a.shape)
            engine._check(engine.lib.dpir_ewise(engine.h, op, ad.ptr, args[0], args[1], args[2], out.ptr, a.size))
            got = out.numpy()
            same_bits(got, F.ewise_f32(op, a, rhs), f"ewise {label} op {op} rhs {kind}")
            engine._check(engine.lib.dpir_ewise(engine.h, op, ad.ptr, args[0], args[1], args[2], ad.ptr, a.size))                # in place
            assert np.array_equal(ad.numpy(), got), (label, op, kind)
            del ad, out


@pytest.mark.parametrize("shape", ELEM_SHAPES, ids=_ids)
def test_ewise_bits(engine, shape):
    B, H, W = shape
    rng = np.random.default_rng(17)
    a = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    b = ((0.1 + rng.random((B, 3, H, W))) * rng.choice([-1.0, 1.0], (B, 3, H, W))).astype(np.float32)
    _ewise_all(engine, a, b, str(shape))
    for op in range(6):                     # image n of the batch against the same image alone
        ad, bd, out = engine.to_device(a), engine.to_device(b), engine.empty(a.shape)
        engine._check(engine.lib.dpir_ewise(engine.h, op, ad.ptr, bd.ptr, b.size, 0.0, out.ptr, a.size))
        a1, b1, o1 = engine.to_device(a[B - 1:]), engine.to_device(b[B - 1:]), engine.empty(a[B - 1:].shape)
        engine._check(engine.lib.dpir_ewise(engine.h, op, a1.ptr, b1.ptr, b[B - 1:].size, 0.0, o1.ptr, a[B - 1:].size))
        assert np.array_equal(o1.numpy(), out.numpy()[B - 1:]), op


def test_grid_stride_branch_at_32x3x512x512(engine):
    """25.2 M elements: dpir_ewise caps its grid at 65 536 workgroups (16.7 M elements) and strides; dpir_prox_mask and dpir_renoise at the
    same size.  Every element against the numpy expression, and the last image against the same image alone."""
    B, H, W = BIG
    rng = np.random.default_rng(18)
    a = rng.standard_normal((B, 3, H, W), dtype=np.float32)
    b = (np.float32(0.1) + rng.random((B, 3, H, W), dtype=np.float32))
    ad, bd = engine.to_device(a), engine.to_device(b)
    out = engine.empty(a.shape)
    for op in range(6):
        engine._check(engine.lib.dpir_ewise(engine.h, op, ad.ptr, bd.ptr, b.size, 0.0, out.ptr, a.size))
        same_bits(out.numpy(), F.ewise_f32(op, a, b), f"ewise big op {op} tensor")
        engine._check(engine.lib.dpir_ewise(engine.h, op, ad.ptr, None, 0, 0.37, out.ptr, a.size))
        same_bits(out.numpy(), F.ewise_f32(op, a, np.float32(0.37)), f"ewise big op {op} scalar")
    tmp = engine.to_device(a)
    engine._check(engine.lib.dpir_ewise(engine.h, 3, tmp.ptr, bd.ptr, b.size, 0.0, tmp.ptr, a.size))
    same_bits(tmp.numpy(), F.ewise_f32(3, a, b), "ewise big in place")
    del out, tmp
    m = rng.integers(0, 2, (B, 3, H, W), dtype=np.uint8)
    x0 = np.clip(a, -1, 1)
    got = _prox_mask(engine, x0, b, m, 1e-4, 0.7)
    same_bits(got, F.prox_mask_f32(x0, b, m, 1e-4, 0.7), "prox_mask big")
    assert np.array_equal(_prox_mask(engine, x0[B - 1:], b[B - 1:], m[B - 1:], 1e-4, 0.7), got[B - 1:])
    steps, arr = _steps(0.7, 0.3)
    n2 = rng.standard_normal((B, 3, H, W), dtype=np.float32)
    got = _renoise(engine, a, x0, arr[4], b, n2)
    same_bits(got, F.renoise_f32(a, x0, steps[4], b, n2), "renoise big")
    assert np.array_equal(_renoise(engine, a[B - 1:], x0[B - 1:], arr[4], b[B - 1:], n2[B - 1:]), got[B - 1:])


def _finalize(engine, x, want_f=True, want_u=True, in_place=False):
    B, _, H, W = x.shape
    xd = engine.to_device(x)
    of = xd if in_place else (engine.empty(x.shape) if want_f else None)
    ou = engine.empty((B, H, W, 3), np.uint8) if want_u else None
    engine._check(engine.lib.dpir_finalize(engine.h, xd.ptr, None if of is None else of.ptr, None if ou is None else ou.ptr, B, H, W))
    return None if of is None else of.numpy(), None if ou is None else ou.numpy()


@pytest.mark.parametrize("shape", ELEM_SHAPES + [(2, 256, 256)], ids=_ids)
def test_finalize_bits(engine, shape):
    """x / 2 + .5 and the uint8 NHWC quantisation, bit-exact: values whose * 255 lands exactly on k + 0.5 (round half to even), values just
    outside [0, 1], either output null, and out_f32 == x."""
    B, H, W = shape
    rng = np.random.default_rng(19)
    x = (rng.random((B, 3, H, W)).astype(np.float32) * 2.4 - 1.2).astype(np.float32)
    flat = x.reshape(-1)
    k = np.arange(flat.size) % 255
    halves = ((k + 0.5) / 255.0).astype(np.float32) * np.float32(2) - np.float32(1)
    flat[::2] = halves[::2]
    edge = np.array([1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2)), 1.000001, -1.000001, 1.5,
                     -1.5, 0.0, -0.0], np.float32)
    flat[1:2 * edge.size:2] = edge
    vf, vu = F.finalize_f32(x)
    q = np.clip(vf, 0, 1).astype(np.float32) * np.float32(255)
    assert np.count_nonzero(q - np.floor(q) == 0.5) >= 8, "the probe holds no exact k + 0.5"
    assert np.array_equal(vu, do.tensor2uint_batch(torch.from_numpy(vf)))          # the statement is the reference's tensor2uint_batch
    of, ou = _finalize(engine, x)
    same_bits(of, vf, f"finalize {shape} f32")
    assert np.array_equal(ou, vu)
    of2, none = _finalize(engine, x, want_u=False)
    assert none is None and np.array_equal(of2, vf)
    none, ou2 = _finalize(engine, x, want_f=False)
    assert none is None and np.array_equal(ou2, vu)
    of3, ou3 = _finalize(engine, x, in_place=True)
    assert np.array_equal(of3, vf) and np.array_equal(ou3, vu)
    of4, ou4 = _finalize(engine, x[B - 1:])
    assert np.array_equal(of4, vf[B - 1:]) and np.array_equal(ou4, vu[B - 1:])


# ====================================================================================================================== degradation, metrics
def _psf(shape, rng):
    k = rng.random(shape)
    return (k / k.sum()).astype(np.float32)


def _blur_images(B, H, W, rng):
    """uint8 [B, H, W, 3]: random images with one flat patch of 200 (its exact blur is the integer 200: a normalised float32 PSF puts the
    float64 sum either side of it); image 0 is flat altogether, so that every PSF size sees whole-support flat pixels."""
    gt = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    gt[:, : (3 * H) // 4, : (3 * W) // 4] = 200
    gt[0] = 200
    return gt


@pytest.mark.parametrize("H,W,kh,kw", [(12, 16, 1, 1), (40, 56, 4, 6), (40, 56, 7, 3), (40, 56, 25, 25), (12, 16, 12, 16), (12, 16, 4, 6)],
                         ids=lambda v: str(v))
def test_wrap_blur_quantised_output_equals_the_numpy_statement(engine, H, W, kh, kw):
    B = 5
    rng = np.random.default_rng(20 + kh)
    gt = _blur_images(B, H, W, rng)
    k = np.stack([_psf((kh, kw), rng) for _ in range(B)])[:, None]
    y, _ = dgr.degrade(engine, "deblur", gt, k=k, noise_level_img=0.0)
    blurred = F.blur_wrap_u8(gt, k[:, 0])
    ref = F.noise_finish_f32(blurred, None, 0.0)               # the finish kernel runs at level 0 too (F.degrade_deblur)
    got = y.numpy()
    flat = np.rint(blurred[0] * 255).astype(int)
    print(f"ops_f64 blur {H}x{W} PSF {kh}x{kw}: flat image quantises to {sorted(set(flat.ravel().tolist()))}; differing pixels {np.count_nonzero(got != ref)}")
    assert np.array_equal(got, ref)
    alone, _ = dgr.degrade(engine, "deblur", gt[B - 1:], k=k[B - 1:], noise_level_img=0.0)
    assert np.array_equal(alone.numpy(), got[B - 1:])
    # host noise at two levels on the float32 path
    nz = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    for level in (12.75 / 255, 50.0 / 255):
        yn, _ = dgr.degrade(engine, "deblur", gt, k=k, noise_level_img=level, noise=nz)
        same_bits(yn.numpy(), F.noise_finish_f32(blurred, nz, level), f"noise finish f32 {H}x{W} level {level:.3f}")
        y1, _ = dgr.degrade(engine, "deblur", gt[B - 1:], k=k[B - 1:], noise_level_img=level, noise=nz[B - 1:])
        assert np.array_equal(y1.numpy(), yn.numpy()[B - 1:])
    if kh * kw > 1:
        # eight flat images of 200, one normalised float32 PSF each: the float64 sums must fall on BOTH sides of the integer in this probe
        # (else it no longer tests the truncation), and the engine must follow each of them
        flat_gt = np.full((8, H, W, 3), 200, np.uint8)
        kf = np.stack([_psf((kh, kw), rng) for _ in range(8)])[:, None]
        sums = F.blur_wrap_acc(flat_gt, kf[:, 0])
        assert (sums < 200).any() and (sums >= 200).any(), "the flat probe does not straddle 200"
        yf, _ = dgr.degrade(engine, "deblur", flat_gt, k=kf, noise_level_img=0.0)
        ref_f = F.degrade_deblur(flat_gt, kf[:, 0])
        assert {199, 200} <= set(np.rint(F.blur_wrap_u8(flat_gt, kf[:, 0]) * 255).astype(int).ravel().tolist())
        assert np.array_equal(yf.numpy(), ref_f)


@pytest.mark.parametrize("H,W", [(12, 16), (40, 56), (7, 9)], ids=lambda v: str(v))
def test_inpainting_degradation_with_a_per_channel_mask(engine, H, W):
    B = 5
    rng = np.random.default_rng(30)
    gt = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mask = rng.integers(0, 2, (B, 3, H, W), dtype=np.uint8)
    nz = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    for level, noise in ((0.0, None), (12.75 / 255, nz), (50.0 / 255, nz)):
        y, _ = dgr.degrade(engine, "inpaint", gt, mask=mask, noise_level_img=level, noise=noise)
        same_bits(y.numpy(), F.noise_finish_inpaint(gt, mask, noise, level), f"inpaint degrade {H}x{W} level {level:.3f}")
    alone, _ = dgr.degrade(engine, "inpaint", gt[B - 1:], mask=mask[B - 1:], noise_level_img=level, noise=nz[B - 1:])
    assert np.array_equal(alone.numpy(), y.numpy()[B - 1:])


@pytest.mark.parametrize("B,H,W", [(1, 7, 9), (5, 7, 9), (1, 256, 256), (5, 256, 256), (1, 512, 512), (5, 512, 512)], ids=lambda v: str(v))
def test_metrics_against_float64_psnr(engine, B, H, W):
    """PSNR and PSNR-Y at the suite's 2e-5 dB, now against float64: H W = 63 (less than one workgroup), 256^2, 512^2; mean squared errors that
    differ by 10^6 within one batch each keep their own value; an identical image gives +inf, next to images that do not."""
    rng = np.random.default_rng(40 + B)
    gt = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    amp = np.array([0.1, 1e-4, 0.03, 1e-3, 0.3], np.float32)[:B]
    x0 = (F.u8_to_single(gt) + amp[:, None, None, None] * rng.standard_normal((B, 3, H, W)).astype(np.float32)).astype(np.float32)
    gtd = engine.to_device(gt)
    p, py = dgr.metrics(engine, engine.to_device(x0), gtd)
    rp, rpy = F.psnr(x0, gt), F.psnr(x0, gt, y_only=True)
    print(f"ops_f64 metrics B {B} {H}x{W}: psnr {rp}, |d| {np.abs(p - rp).max():.2e} dB, psnr_y |d| {np.abs(py - rpy).max():.2e} dB")
    assert np.abs(p - rp).max() <= 2e-5 and np.abs(py - rpy).max() <= 2e-5
    if B > 1:
        assert rp[1] - rp[0] > 55.0                        # the batch really holds mean squared errors 10^6 apart
    for n in sorted({0, B - 1}):
        p1, py1 = dgr.metrics(engine, engine.to_device(x0[n:n + 1]), engine.to_device(gt[n:n + 1]))
        assert p1[0] == p[n] and py1[0] == py[n]
    same = x0.copy()
    same[B - 1] = F.u8_to_single(gt[B - 1:])[0]
    p, py = dgr.metrics(engine, engine.to_device(same), gtd)
    assert np.isposinf(p[B - 1]) and np.isposinf(py[B - 1])
    assert np.abs(p[:B - 1] - rp[:B - 1]).max(initial=0.0) <= 2e-5 and np.all(np.isfinite(p[:B - 1]))
    assert np.abs(py[:B - 1] - rpy[:B - 1]).max(initial=0.0) <= 2e-5 and np.all(np.isfinite(py[:B - 1]))


# ====================================================================================================================== argument checks
# Read from csrc/api.hip before these were written: every entry below calls check_shape right after its null checks, ahead of hipSetDevice,
# the workspace, the Resizer tables and every launch, so none of the calls below reaches a kernel, an allocation or a division.
BAD_SHAPES = [(-1, 8, 8), (0, 8, 8), (2, 0, 8), (2, 8, -4)]


def _rejected(engine, rc, entry):
    msg = engine.lib.dpir_last_error(engine.h).decode()
    assert rc == -1 and entry in msg, (entry, rc, msg)


def test_bad_shapes_are_rejected_and_the_engine_stays_usable(engine):
    lib, h = engine.lib, engine.h
    buf = engine.to_device(np.zeros((2, 3, 8, 8), np.float32))
    u8 = engine.to_device(np.zeros((2, 3, 8, 8), np.uint8))
    _, arr = _steps(0.0, 0.3)
    host = np.zeros(4, np.float32)
    for B, H, W in BAD_SHAPES:
        _rejected(engine, lib.dpir_prox_mask(h, buf.ptr, buf.ptr, u8.ptr, 0.1, 1.0, B, H, W), "dpir_prox_mask")
        _rejected(engine, lib.dpir_repaint_mix(h, buf.ptr, buf.ptr, u8.ptr, C.byref(arr[0]), buf.ptr, B, H, W), "dpir_repaint_mix")
        _rejected(engine, lib.dpir_renoise(h, buf.ptr, buf.ptr, C.byref(arr[0]), buf.ptr, buf.ptr, B, H, W), "dpir_renoise")
        _rejected(engine, lib.dpir_finalize(h, buf.ptr, buf.ptr, None, B, H, W), "dpir_finalize")
        _rejected(engine, lib.dpir_randn(h, buf.ptr, 1, 0, 0, B, 3, H, W), "dpir_randn")
        _rejected(engine, lib.dpir_bicubic_up(h, buf.ptr, buf.ptr, 2, B, H, W), "dpir_bicubic_up")
        _rejected(engine, lib.dpir_resize_down(h, buf.ptr, buf.ptr, 2, B, H, W), "dpir_resize_down")
        _rejected(engine, lib.dpir_prox_ibp(h, buf.ptr, buf.ptr, 0.1, 0.5, 1, 2, B, H, W), "dpir_prox_ibp")
        _rejected(engine, lib.dpir_metrics(h, buf.ptr, u8.ptr, B, H, W, host.ctypes.data, host.ctypes.data), "dpir_metrics")
        _rejected(engine, lib.dpir_grad_and_value(h, 0, buf.ptr, buf.ptr, 2, buf.ptr, None, B, H, W), "dpir_grad_and_value")
    _rejected(engine, lib.dpir_randn(h, buf.ptr, 1, 0, 0, 2, 0, 8, 8), "dpir_randn")
    for sf in (0, -2, 3, 16):           # sf = 0 used to divide by zero on the host (SIGFPE) in dpir_prox_ibp; 3 and 16 do not divide 8
        _rejected(engine, lib.dpir_prox_ibp(h, buf.ptr, buf.ptr, 0.1, 0.5, 1, sf, 2, 8, 8), "dpir_prox_ibp")
        _rejected(engine, lib.dpir_resize_down(h, buf.ptr, buf.ptr, sf, 2, 8, 8), "dpir_resize_down")
        _rejected(engine, lib.dpir_grad_and_value(h, 0, buf.ptr, buf.ptr, sf, buf.ptr, None, 2, 8, 8), "dpir_grad_and_value")
    for sf in (0, -2):
        _rejected(engine, lib.dpir_bicubic_up(h, buf.ptr, buf.ptr, sf, 2, 4, 4), "dpir_bicubic_up")
    # valid calls on the same engine still give the right answer
    x = probe((2, 3, 24, 36), 50, -1.0, 1.0)
    y = probe((2, 3, 8, 12), 51)
    F.check(_ibp(engine, x, y, 0.37, 0.5, 2, 3), F.prox_ibp(x, y, float(np.float32(0.37)), 0.5, 3, 2),
            do.prox_ibp(t32(x), t32(y), torch.tensor(0.37), 3, 0.5, 2).numpy(), "prox_ibp after the rejected calls")
    m = np.random.default_rng(52).integers(0, 2, x.shape, dtype=np.uint8)
    same_bits(_prox_mask(engine, x, np.abs(x), m, 0.3, 1.0), F.prox_mask_f32(x, np.abs(x), m, 0.3, 1.0), "prox_mask after the rejected calls")


def test_engine_on_device_1_while_device_0_is_current(engine):
    """The entries select their engine's device themselves: an elementwise entry (dpir_prox_mask, which did not) and a resampling entry
    (dpir_bicubic_up, which did not either) on an engine of device 1, each right after a call that leaves device 0 current."""
    n = device_count()
    if n < 2:
        pytest.skip(f"needs two GPUs: dpir_device_count() = {n} on this box")
    import diffpir_amd
    e1 = diffpir_amd.Engine(1)
    try:
        x = probe((2, 3, 24, 36), 60, -1.0, 1.0)
        y = probe((2, 3, 24, 36), 61)
        m = np.random.default_rng(62).integers(0, 2, x.shape, dtype=np.uint8)
        d, yd, md = e1.to_device(x), e1.to_device(y), e1.to_device(m)
        lr = probe((2, 3, 8, 12), 63)
        lrd, up = e1.to_device(lr), e1.empty((2, 3, 24, 36))
        cur = engine.to_device(x)
        torch.cuda.set_device(0)
        engine._check(engine.lib.dpir_ewise(engine.h, 0, cur.ptr, None, 0, 1.0, cur.ptr, x.size))      # selects device 0 in this thread
        e1._check(e1.lib.dpir_prox_mask(e1.h, d.ptr, yd.ptr, md.ptr, 0.3, 1.0, 2, 24, 36))
        engine._check(engine.lib.dpir_ewise(engine.h, 0, cur.ptr, None, 0, 1.0, cur.ptr, x.size))
        e1._check(e1.lib.dpir_bicubic_up(e1.h, lrd.ptr, up.ptr, 3, 2, 8, 12))
        same_bits(d.numpy(), F.prox_mask_f32(x, y, m, 0.3, 1.0), "prox_mask on device 1")
        F.check(up.numpy(), F.bicubic_up(lr, 3), torch.nn.functional.interpolate(t32(lr), scale_factor=3, mode="bicubic", align_corners=False).numpy(),
                "bicubic_up on device 1")
        engine.sync()
    finally:
        e1.close()
