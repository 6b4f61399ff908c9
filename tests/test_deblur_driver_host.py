"""Host logic of LoopConfig(driver="main_ddpir_deblur") -- no GPU: what the driver admits and refuses, its t_y start coefficients, its draw
order against the restatement of tests/blur_f64.py, and (where the reference tree is present) that restatement's operator and
grad_and_value against the live reference."""
import numpy as np
import pytest
import torch

from diffpir_amd import restore, schedule
from oracle import unet_oracle as uo, diffpir_oracle as do, ref_import
from tests import blur_f64 as BF

MODES = [dict(generate_mode="DiffPIR"), dict(generate_mode="DPS_y0"), dict(generate_mode="DPS_yt"), dict(generate_mode="DiffPIR", sub_1_analytic=False)]


@pytest.mark.parametrize("kw", MODES, ids=["DiffPIR", "DPS_y0", "DPS_yt", "first_order"])
def test_deblur_driver_admits_its_modes(kw):
    restore.LoopConfig(driver="main_ddpir_deblur", task="deblur", **kw).check_supported()


def test_deblur_driver_refuses_other_tasks_and_unknown_drivers():
    with pytest.raises(ValueError):
        restore.LoopConfig(driver="main_ddpir_deblur", task="sr", sf=4).check_supported()
    with pytest.raises(ValueError):
        restore.LoopConfig(driver="main_ddpir_sr", task="deblur").check_supported()
    with pytest.raises(NotImplementedError):                # the default driver keeps refusing
        restore.LoopConfig(task="deblur", generate_mode="DPS_y0").check_supported()


@pytest.mark.parametrize("level,init", [(12.75, "max"), (2.55, "max"), (25.5, 600)])
def test_start_coefficients_follow_t_y(level, init):
    """main_ddpir_deblur.py:228-231 in numpy float32 on schedule.DriverTables."""
    cfg = restore.LoopConfig(driver="main_ddpir_deblur", task="deblur", noise_level_img=level / 255.0, noise_init_img=init)
    dt = schedule.DriverTables.make()
    t_start = restore.t_start_of(cfg, dt.reduced)
    t_y = schedule.find_nearest(dt.reduced, 2 * cfg.noise_level_img)
    f = np.float32
    eff = f(dt.sqrt_ac[t_start]) / f(dt.sqrt_ac[t_y])
    s1m = np.sqrt(f(dt.sqrt_1m_ac[t_start]) ** 2 - eff ** 2 * f(dt.sqrt_1m_ac[t_y]) ** 2)
    sa_got, s1m_got = restore.start_coefficients(cfg, dt)
    assert eff.dtype == np.float32 and s1m.dtype == np.float32
    assert sa_got == eff and s1m_got == s1m
    assert t_y < t_start and 0 < s1m_got <= dt.sqrt_1m_ac[t_start]
    # the default driver keeps main_ddpir.py:315
    base = restore.start_coefficients(restore.LoopConfig(task="deblur", noise_level_img=level / 255.0, noise_init_img=init), dt)
    assert base == (dt.sqrt_ac[t_start], dt.sqrt_1m_ac[t_start])


@pytest.mark.parametrize("kw", MODES, ids=["DiffPIR", "DPS_y0", "DPS_yt", "first_order"])
def test_draw_order_matches_the_restatement(kw):
    """dps_host_noise_shapes for the driver's modes == the batch shapes of the restatement's randn_like calls, in order."""
    Bn, size, nfe = 2, 64, 4
    hp = uo.tiny_hp()
    sd = uo.synth_state_dict(hp, 0)
    lam = 6.0e5 if kw.get("sub_1_analytic") is False else 6.0
    cfg = restore.LoopConfig(driver="main_ddpir_deblur", task="deblur", iter_num=nfe, lambda_=lam, zeta=0.25, **kw)
    ocfg = do.LoopConfig("deblur", nfe, 12.75 / 255, lam, 0.25, generate_mode=kw["generate_mode"], sub_1_analytic=kw.get("sub_1_analytic", True))
    rng = np.random.default_rng(0)
    y = torch.from_numpy(rng.random((1, 3, size, size)).astype(np.float32))
    k = torch.ones(5, 5) / 25
    shapes = []
    out = BF.restore_deblur(sd, hp, ocfg, y, k, BF.image_noise_fn(1, Bn, 0, shapes))
    assert torch.isfinite(out).all()
    _, steps, _ = restore._steps(cfg)
    assert restore.dps_host_noise_shapes(cfg, steps, Bn, size, size) == shapes
    # the default driver's lists are what they were: init + one draw per step (+ the y_t draw of DPS_yt on non-final steps)
    sr = restore.LoopConfig(task="sr", sf=4, sr_mode="cubic", iter_num=nfe, generate_mode="DPS_yt")
    _, s2, _ = restore._steps(sr)
    n_re = sum(1 for s in s2 if not s["last"])
    assert restore.dps_host_noise_shapes(sr, s2, 2, 64, 64) == [(2, 3, 64, 64)] + sum(
        ([(2, 3, 64, 64)] + ([(2, 3, 16, 16)] if not s["last"] else []) for s in s2), []) and n_re > 0


def _grad_mode_configs():
    for sf in (2, 4):
        for mode in ("DPS_y0", "DPS_yt"):
            yield f"sr_x{sf}_{mode}", dict(task="sr", sf=sf, sr_mode="cubic", generate_mode=mode)
    for eta in (0.0, 0.5):
        for name, kw in (("DPS_y0", dict(generate_mode="DPS_y0")), ("DPS_yt", dict(generate_mode="DPS_yt")),
                         ("first_order", dict(generate_mode="DiffPIR", sub_1_analytic=False))):
            yield f"deblur_{name}_eta{eta}", dict(driver="main_ddpir_deblur", task="deblur", eta=eta, **kw)


@pytest.mark.parametrize("iters", [dict(iter_num=4), dict(iter_num=600, skip_type="quad")], ids=["4", "600quad"])
@pytest.mark.parametrize("name,kw", list(_grad_mode_configs()), ids=[n for n, _ in _grad_mode_configs()])
def test_grad_mode_drawer_follows_dps_host_noise_shapes(name, kw, iters):
    """draw_grad_host_noise asks noise_fn for exactly the shapes of dps_host_noise_shapes, in its order, and returns what the loops are fed:
    one p_sample draw per step, the y_t draws (zeros where a step has none) or the re-noise draws of the non-final steps."""
    Bn, size = 2, 16
    cfg = restore.LoopConfig(**kw, **iters)
    cfg.check_supported()
    _, steps, _ = restore._steps(cfg)
    if iters["iter_num"] == 600:
        assert sum(s["last"] for s in steps) == 2           # the quad schedule repeats its final timestep
    asked, count = [], [0]

    def noise_fn(shape):
        asked.append(tuple(shape))
        count[0] += 1
        return np.full(shape, count[0], np.float32)          # draw number, to see where each draw lands
    got = restore.draw_grad_host_noise(noise_fn, cfg, steps, Bn, size, size)
    assert asked == restore.dps_host_noise_shapes(cfg, steps, Bn, size, size)
    full, n_re = (Bn, 3, size, size), sum(1 for s in steps if not s["last"])
    assert got["init"].shape == full and (got["init"] == 1).all()
    if cfg.generate_mode == "DiffPIR":
        assert set(got) == {"init", "n1", "n2"} and got["n2"].shape == (n_re,) + full
        assert (got["n1"] is None) == (cfg.eta == 0) and (got["n1"] is None or got["n1"].shape == (n_re,) + full)
        assert [float(got["n2"][j, 0, 0, 0, 0]) for j in range(n_re)] == [4.0 + 3 * j for j in range(n_re)]
        return
    assert set(got) == {"init", "ps", "yt"} and got["ps"].shape == (len(steps),) + full
    if cfg.generate_mode == "DPS_y0":
        assert got["yt"] is None
        assert [float(v) for v in got["ps"][:, 0, 0, 0, 0]] == [2.0 + i for i in range(len(steps))]
        return
    assert got["yt"].shape == (len(steps), Bn, 3, size // cfg.sf, size // cfg.sf)
    assert [float(v) for v in got["ps"][:n_re, 0, 0, 0, 0]] == [2.0 + 2 * i for i in range(n_re)]
    assert [float(v) for v in got["yt"][:, 0, 0, 0, 0]] == [3.0 + 2 * i for i in range(n_re)] + [0.0] * (len(steps) - n_re)


@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
def test_statements_against_the_live_reference():
    """The helper's operator == utils_deblur.Blurkernel's depthwise reflect-padded convolution with the same weights, and its (norm_grad, norm)
    == the reference's utils_model.grad_and_value, to float32 round-off (16 x 16, K = 5)."""
    import importlib
    ns = ref_import.load()
    ref_um = ns.utils_model if hasattr(ns, "utils_model") else ns["utils_model"]
    ref_ud = importlib.import_module("utils.utils_deblur")
    rng = np.random.default_rng(2)
    Kk = 5
    k = rng.random((Kk, Kk)).astype(np.float32)
    k /= k.sum()
    x = torch.from_numpy(rng.uniform(-1, 1, (1, 3, 16, 16)).astype(np.float32))
    m = torch.from_numpy(rng.random((1, 3, 16, 16)).astype(np.float32))
    conv = ref_ud.Blurkernel(blur_type="gaussian", kernel_size=Kk, std=1.0)
    conv.update_weights(torch.from_numpy(k))
    with torch.no_grad():
        want = conv(x / 2 + 0.5).numpy()
    tk = torch.from_numpy(k)[None, None]
    got = BF.blur_reflect(x, tk).detach().numpy()
    assert np.abs(got - want).max() < 1e-6, np.abs(got - want).max()

    def Tx(v):
        return conv(v / 2 + 0.5)
    xr = x.clone().requires_grad_()
    ng_ref, n_ref = ref_um.grad_and_value(operator=Tx, x=xr, x_hat=xr, measurement=m)
    ng, nv = BF.grad_and_value(x, m, tk)
    assert abs(float(nv[0]) / float(n_ref) - 1) < 1e-6
    assert np.abs(ng.numpy() - ng_ref.numpy()).max() < 1e-6 * max(1.0, float(ng_ref.abs().max()))
