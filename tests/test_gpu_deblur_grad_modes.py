"""-m gpu: the gradient modes of the standalone deblurring program (LoopConfig(driver="main_ddpir_deblur")): grad_and_value on a BlurOperator,
the DPS_y0 / DPS_yt / first-order / analytic loops against the torch-CPU restatement of main_ddpir_deblur.py (tests/blur_f64.py) run on each
image alone, and the stepwise plug loop against the monolithic one, bit for bit.  Tiny topology, 64 x 64, K = 9, B = 2 with two PSFs, 4 NFE."""
import numpy as np
import pytest
import torch

import diffpir_amd
from diffpir_amd import restore, schedule, script_util, utils_model
from diffpir_amd.utils_deblur import BlurOperator
from oracle import unet_oracle as uo, diffpir_oracle as do
from tests import blur_f64 as BF
from tests.gpu_common import make_model, seeded_noise_fn_np, per_image_err, fft_prox_parity

pytestmark = pytest.mark.gpu

TOL_GRAD = 1e-4         # tests/test_gpu_dps.py TOL_GRAD: the bound of the engine's input gradients against autograd (max error over max value)
B, SIZE, K, NFE, SEED = 2, 64, 9, 4, 77

# (engine config, oracle config, check): the tolerances are the ones the corresponding `sr` mode is held to
#   DPS_y0:      tests/test_gpu_dps.py::test_dps_y0_loop_matches_live_reference_fixture            |dPSNR| <= 1e-3 dB and max error < 2e-4
#   DPS_yt:      tests/test_gpu_dps.py::test_dps_yt_and_first_order_loops_match_live_reference_fixture   max error < 1e-4 max(1, output range)
#   first order: the same test                                                                     max error < 1e-4
#   analytic:    tests/test_gpu_loop.py (FFT prox): tests/gpu_common.py::fft_prox_parity against the restatement with an exact prox
MODES = {
    "DPS_y0": dict(generate_mode="DPS_y0", lambda_=6.0, zeta=0.25),
    "DPS_yt": dict(generate_mode="DPS_yt", lambda_=6.0, zeta=0.25),
    "first_order": dict(generate_mode="DiffPIR", lambda_=6.0e5, zeta=0.25, sub_1_analytic=False),
    "analytic": dict(generate_mode="DiffPIR", lambda_=7.0, zeta=0.3),
}


def _cfgs(mode):
    kw = MODES[mode]
    cfg = restore.LoopConfig(driver="main_ddpir_deblur", task="deblur", iter_num=NFE, **kw)
    ocfg = do.LoopConfig("deblur", NFE, 12.75 / 255, kw["lambda_"], kw["zeta"], generate_mode=kw["generate_mode"],
                         sub_1_analytic=kw.get("sub_1_analytic", True))
    return cfg, ocfg


def _gauss(std, stretch):
    ax = np.arange(K) - K // 2
    k = np.exp(-(ax[:, None] ** 2 + (stretch * ax[None, :]) ** 2) / (2 * std * std))
    return (k / k.sum()).astype(np.float32)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:SIZE, 0:SIZE] / SIZE
    gt = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * (f * xx + g * yy) + ph) for f, g, ph in rng.uniform(0.5, 3, (B * 3, 3))]).reshape(B, 3, SIZE, SIZE)
    gt = gt.astype(np.float32)
    k = np.stack([_gauss(1.6, 1.0), _gauss(2.4, 0.5)])[:, None]
    with torch.no_grad():
        y = BF.blur_reflect(torch.from_numpy(gt * 2 - 1), torch.from_numpy(k), dtype=torch.float32).numpy()
    y = (y + (12.75 / 255) * rng.standard_normal(y.shape)).astype(np.float32)
    return dict(gt=gt, k=k, y=y)


@pytest.fixture(scope="module")
def eng():
    e = diffpir_amd.Engine(0)
    e.set_precision("f16x3")
    e.enable_grad()
    model, sd = make_model(e, uo.tiny_hp())
    yield e, model, sd
    e.close()


_REFS = {}


def _ref(mode, sd, case, exact=False):
    """The restatement run on each image alone with its slices of the batch-shaped noise; computed once per mode."""
    key = (mode, exact)
    if key not in _REFS:
        _, ocfg = _cfgs(mode)
        _REFS[key] = BF.restore_deblur_batch(sd, uo.tiny_hp(), ocfg, torch.from_numpy(case["y"]), torch.from_numpy(case["k"]), SEED,
                                             exact_prox=exact).numpy()
    return _REFS[key]


def _check(mode, out, sd, case, label):
    ref = _ref(mode, sd, case)
    errs = [float(np.abs(out[n] - ref[n]).max()) for n in range(B)]
    scale = float(np.abs(ref).max())
    print(f"{label}: per-image max|engine - restatement| {['%.3e' % v for v in errs]} (output range {scale:.2f})")
    if mode == "analytic":
        fft_prox_parity(out, ref, case["gt"], label, exact=_ref(mode, sd, case, exact=True))
        return
    gt2 = case["gt"] * 2 - 1
    if mode == "DPS_y0":
        gap = abs(restore.psnr_batch(out * 2 - 1, gt2) - restore.psnr_batch(ref * 2 - 1, gt2))
        assert gap <= 1e-3 and max(errs) < 2e-4, (errs, gap)
    elif mode == "DPS_yt":
        assert max(errs) < 1e-4 * max(1.0, scale), errs
    else:
        assert max(errs) < 1e-4, errs


_MONO = {}


def _mono(e, case, mode):
    if mode not in _MONO:
        cfg, _ = _cfgs(mode)
        _MONO[mode] = restore.restore_batch(e, cfg, case["y"], k=case["k"], noise_source="host", noise_fn=seeded_noise_fn_np(SEED)).numpy()
    return _MONO[mode]


@pytest.mark.parametrize("mode", list(MODES))
def test_loops_match_the_restatement_per_image(eng, case, mode):
    """Each image of the batch against the restatement run on that image alone with its noise slices (its norm is that image's own)."""
    e, model, sd = eng
    _check(mode, _mono(e, case, mode), sd, case, f"deblur driver {mode}")
    if mode != "analytic":
        cfg, _ = _cfgs(mode)
        assert np.isfinite(restore.restore_batch(e, cfg, case["y"], k=case["k"], noise_source="device", seed=5).numpy()).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_stepwise_plug_loop_gives_the_bits_of_the_monolithic_loop(eng, case, mode):
    """restore_batch_stepwise (model_fn 'pred_x_prev_and_start' / 'pred_xstart', grad_and_value(BlurOperator), the loop's own expressions on
    device arrays; the analytic data step through dpir_prox_fft_apply) against restore_batch, array_equal."""
    e, model, sd = eng
    cfg, _ = _cfgs(mode)
    mono = _mono(e, case, mode)
    diffusion = script_util.create_gaussian_diffusion(steps=1000, learn_sigma=True)
    step = restore.restore_batch_stepwise(model, diffusion, cfg, e.to_device(case["y"]), k=e.to_device(case["k"]),
                                          noise_fn=seeded_noise_fn_np(SEED)).numpy()
    print(f"{mode}: stepwise plugs vs monolithic loop max|diff| {float(np.abs(step - mono).max()):.3e}")
    assert np.array_equal(step, mono)


def test_grad_and_value_on_a_blur_operator(eng, case):
    """x is x_hat (first-order step, DPS_yt) and through the clamp and the network (DPS_y0) against float64 autograd, per image."""
    e, model, sd = eng
    rng = np.random.default_rng(11)
    op = BlurOperator(case["k"], engine=e)
    tk, ty = torch.from_numpy(case["k"]), torch.from_numpy(case["y"])
    xh = (rng.uniform(-1, 1, (B, 3, SIZE, SIZE))).astype(np.float32)
    xh[1] *= np.float32(0.3)
    xd, yd = e.to_device(xh), e.to_device(case["y"])
    g, nv = utils_model.grad_and_value(operator=op, x=xd, x_hat=xd, measurement=yd)
    g64, n64 = BF.grad_and_value(torch.from_numpy(xh), ty, tk)
    err, at = per_image_err(g.numpy(), g64.numpy())
    nerr = float(np.abs(nv.numpy() / n64.numpy() - 1).max())
    print(f"grad_and_value(BlurOperator), x is x_hat: worst per-image error {err:.3e} (image {at}); norm rel err {nerr:.3e}")
    assert err < TOL_GRAD and nerr < TOL_GRAD

    # through the network: x -> p_sample -> x0 = clamp(c1 x - c2 eps) -> || y_n - Tx(x0)_n ||
    t = 417
    dt = schedule.DriverTables.make()
    diffusion = script_util.create_gaussian_diffusion(steps=1000, learn_sigma=True)
    x = rng.standard_normal((B, 3, SIZE, SIZE)).astype(np.float32)
    noise = rng.standard_normal(x.shape).astype(np.float32)
    xdev = e.to_device(x)
    utils_model.set_randn_like(lambda like: e.to_device(noise))
    try:
        xt, x0 = utils_model.model_fn(xdev, noise_level=float(dt.reduced[t]) * 255, model_out_type="pred_x_prev_and_start", model_diffusion=model,
                                      diffusion=diffusion, alphas_cumprod=dt.alphas_cumprod)
    finally:
        utils_model.set_randn_like(None)
    g, nv = utils_model.grad_and_value(operator=op, x=xdev, x_hat=x0, measurement=yd)
    sd64 = {k: v.double() for k, v in sd.items()}
    dtab = do.DiffusionTables(1000)
    xr = torch.from_numpy(x).double().requires_grad_()
    eps = uo.unet_forward(sd64, uo.tiny_hp(), xr, torch.tensor([t] * B), dtype=torch.float64)[:, :3]
    c1, c2 = float(np.float32(dtab.sqrt_recip_ac[t])), float(np.float32(dtab.sqrt_recipm1_ac[t]))
    x0r = (c1 * xr - c2 * eps).clamp(-1, 1)
    p = K // 2
    k4 = [torch.einsum('ab,cd->abcd', torch.eye(3, dtype=torch.float64), tk[n, 0].double()) for n in range(B)]
    norms = torch.stack([torch.linalg.norm(ty[n:n + 1].double() - torch.nn.functional.conv2d(
        torch.nn.ReflectionPad2d(p)(x0r[n:n + 1] / 2 + 0.5), k4[n])) for n in range(B)])
    gref = torch.autograd.grad(norms.sum(), xr)[0].numpy()
    err, at = per_image_err(g.numpy(), gref)
    nerr = float(np.abs(nv.numpy() / norms.detach().numpy() - 1).max())
    print(f"grad_and_value(BlurOperator) through the network: worst per-image error {err:.3e} (image {at}); norm rel err {nerr:.3e}")
    assert err < TOL_GRAD and nerr < TOL_GRAD


def test_default_driver_still_refuses_deblurring_in_gradient_modes():
    with pytest.raises(NotImplementedError):
        restore.LoopConfig(task="deblur", generate_mode="DPS_y0").check_supported()
