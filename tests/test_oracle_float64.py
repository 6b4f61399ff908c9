"""The oracle network's float64 mode (unet_forward(..., dtype=torch.float64)), the high-precision checker of the GPU gradient tests
(tests/test_gpu_grad_batches.py).  CPU only, tiny topology."""
import numpy as np
import torch

from oracle import unet_oracle as uo


def _inputs(B=2, size=64, seed=11):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 3, size, size), generator=gen)
    gout = torch.randn((B, 6, size, size), generator=gen)
    return x, gout, torch.tensor([417, 23][:B])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_float64_forward_and_input_gradient_agree_with_fp32_oracle():
    """Same network in both precisions: they agree to fp32 rounding level, and every intermediate of the float64 run is float64."""
    hp = uo.tiny_hp()
    sd = uo.synth_state_dict(hp, 0)
    sd64 = {k: v.double() for k, v in sd.items()}
    x, gout, t = _inputs()
    x32 = x.clone().requires_grad_()
    o32 = uo.unet_forward(sd, hp, x32, t)
    (o32 * gout).sum().backward()
    x64 = x.double().requires_grad_()
    taps = {}
    o64 = uo.unet_forward(sd64, hp, x64, t, taps=taps, dtype=torch.float64)
    (o64 * gout.double()).sum().backward()
    assert o64.dtype == torch.float64 and x64.grad.dtype == torch.float64
    assert taps and all(v.dtype == torch.float64 for v in taps.values())
    fwd = _rel(o32.detach().numpy(), o64.detach().numpy())
    grad = _rel(x32.grad.numpy(), x64.grad.numpy())
    print(f"tiny 64^2: fp32 oracle vs float64 oracle: forward {fwd:.3e}, input gradient {grad:.3e}")
    # fp32 rounding level; non-zero, so the float64 run really is a different evaluation
    assert 0.0 < fwd < 1e-5 and 0.0 < grad < 1e-5


def test_default_precision_is_unchanged(golden):
    """dtype defaults to fp32, the reference's arithmetic: passing it explicitly changes nothing, bit for bit, and the output and input gradient
    stay on the live reference's fixtures (tests/golden/dps.npz, unet_tiny.npz) at the tolerances of test_oracle_golden.py."""
    hp = uo.tiny_hp()
    sd = uo.synth_state_dict(hp, 0)
    g = golden("unet_tiny")
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t"])
    a = uo.unet_forward(sd, hp, x, t)
    b = uo.unet_forward(sd, hp, x, t, dtype=torch.float32)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    np.testing.assert_allclose(a.numpy(), g["out"], rtol=0, atol=1e-5)
    d = golden("dps")
    gen = torch.Generator().manual_seed(int(d["vjp_tiny_seed"]))
    x = torch.randn((2, 3, 64, 64), generator=gen)
    gout = torch.randn((2, 6, 64, 64), generator=gen)
    dxs = []
    for kw in ({}, {"dtype": torch.float32}):
        xr = x.clone().requires_grad_()
        dxs.append(torch.autograd.grad((uo.unet_forward(sd, hp, xr, torch.from_numpy(d["vjp_tiny_t"]), **kw) * gout).sum(), xr)[0])
    assert torch.equal(dxs[0], dxs[1])
    np.testing.assert_allclose(dxs[0].numpy(), d["vjp_tiny_dx"], rtol=0, atol=1e-6)


def _resizer_apply_before(x, sf_inv):
    """oracle.diffpir_oracle.resizer_apply as it stood before it took a dtype (float32 weight tensors, unconditionally)."""
    from oracle import diffpir_oracle as do
    out = x
    for dim in (2, 3):
        n = out.shape[dim]
        w, fov = do.resizer_contributions(n, int(np.ceil(n * sf_inv)), sf_inv)
        w_t = torch.tensor(w.T, dtype=torch.float32)
        fov_t = torch.tensor(fov.T.astype(np.int32), dtype=torch.long)
        xt = torch.transpose(out, dim, 0)
        xt = torch.sum(xt[fov_t] * w_t.reshape(list(w_t.shape) + [1] * 3), dim=0)
        out = torch.transpose(xt, dim, 0)
    return out


def _prox_ibp_before(x0, y, rho, sf, gamma, in_iter):
    """oracle.diffpir_oracle.prox_ibp as it stood before it took a dtype."""
    for _ in range(in_iter):
        x0 = x0 / 2 + 0.5
        x0 = x0 + gamma * torch.nn.functional.interpolate(y - _resizer_apply_before(x0, 1.0 / sf), scale_factor=sf) / (1 + rho)
        x0 = x0 * 2 - 1
    return x0


def _renoise_before(x, x0, dt, t_i, t_im1, eta, zeta, n1, n2):
    """oracle.diffpir_oracle.renoise as it stood before it took a dtype."""
    eps = (x - dt.sqrt_ac[t_i] * x0) / dt.sqrt_1m_ac[t_i]
    eta_sigma = eta * dt.sqrt_1m_ac[t_im1] / dt.sqrt_1m_ac[t_i] * torch.sqrt(dt.betas[t_i])
    return dt.sqrt_ac[t_im1] * x0 + np.sqrt(1 - zeta) * (
        torch.sqrt(dt.sqrt_1m_ac[t_im1] ** 2 - eta_sigma ** 2) * eps + eta_sigma * n1) \
        + np.sqrt(zeta) * dt.sqrt_1m_ac[t_im1] * n2


def test_operator_dtype_is_opt_in_and_float64_agrees_with_the_numpy_statement(golden):
    """resizer_apply / prox_ibp / renoise: (i) the default (fp32) results are array_equal to what they were before the dtype argument existed:
    each against a verbatim copy of its old body (the Resizer also against the live-reference fixture), and an explicit torch.float32 request
    gives the same bits; (ii) their float64 mode agrees with tests/ops_f64.py to 1e-12."""
    from diffpir_amd import schedule
    from oracle import diffpir_oracle as do
    from tests import ops_f64 as F
    g = golden("operators")
    x = torch.from_numpy(g["resizer_in"])
    new = do.resizer_apply(x, 0.25)
    assert new.dtype == torch.float32 and np.array_equal(new.numpy(), _resizer_apply_before(x, 0.25).numpy())
    assert np.array_equal(new.numpy(), do.resizer_apply(x, 0.25, dtype=torch.float32).numpy())
    np.testing.assert_allclose(new.numpy(), g["resizer_out"], rtol=0, atol=2e-6)
    rng = np.random.default_rng(5)
    for (H, W, sf) in ((64, 64, 4), (24, 36, 3), (30, 50, 5), (16, 128, 8), (6, 9, 3)):
        xr = rng.random((2, 3, H, W)).astype(np.float32)
        d64 = do.resizer_apply(torch.from_numpy(xr).double(), 1.0 / sf, dtype=torch.float64).numpy()
        assert d64.dtype == np.float64 and np.abs(d64 - F.resize_down(xr, sf)).max() <= 1e-12
        assert np.array_equal(do.resizer_apply(torch.from_numpy(xr), 1.0 / sf).numpy(), _resizer_apply_before(torch.from_numpy(xr), 1.0 / sf).numpy())
        x0 = (xr * 2 - 1).astype(np.float32)
        y = rng.random((2, 3, H // sf, W // sf)).astype(np.float32)
        rho = torch.tensor(0.37)
        a = do.prox_ibp(torch.from_numpy(x0), torch.from_numpy(y), rho, sf, 0.5, 2)
        assert a.dtype == torch.float32 and torch.equal(a, do.prox_ibp(torch.from_numpy(x0), torch.from_numpy(y), rho, sf, 0.5, 2, dtype=torch.float32))
        assert torch.equal(a, _prox_ibp_before(torch.from_numpy(x0), torch.from_numpy(y), rho, sf, 0.5, 2))
        i64 = do.prox_ibp(torch.from_numpy(x0).double(), torch.from_numpy(y).double(), rho, sf, 0.5, 2, dtype=torch.float64).numpy()
        assert np.abs(i64 - F.prox_ibp(x0, y, float(np.float32(0.37)), 0.5, sf, 2)).max() <= 1e-12
        # the float64 statements of the two other resampling ops against torch's own float64 evaluation
        up64 = torch.nn.functional.interpolate(torch.from_numpy(y).double(), scale_factor=sf, mode="bicubic", align_corners=False).numpy()
        assert np.abs(up64 - F.bicubic_up(y, sf)).max() <= 1e-12
        xg = torch.from_numpy(xr).double().requires_grad_()
        m = torch.from_numpy(y).double() * 2 - 1
        norm = torch.linalg.norm(m - do.resizer_apply(xg, 1.0 / sf, dtype=torch.float64))
        g64, n64 = F.grad_and_value(xr, m.numpy(), sf)
        assert abs(float(norm.detach()) - n64) <= 1e-12 * n64 and np.abs(torch.autograd.grad(norm, xg)[0].numpy() - g64).max() <= 1e-12
    odt = do.DriverTables()
    shape = (2, 3, 12, 20)
    xs, x0s, n1, n2 = (rng.standard_normal(shape).astype(np.float32) for _ in range(4))
    for eta, zeta in ((0.0, 0.3), (0.7, 0.3), (0.7, 0.0), (0.0, 1.0)):
        _, steps, _ = schedule.build_steps(iter_num=10, sigma=0.05, lambda_=7.0, zeta=zeta, eta=eta)
        st = steps[4]
        t = [torch.from_numpy(v) for v in (xs, x0s, n1, n2)]
        a = do.renoise(t[0], t[1], odt, st["t"], st["t_im1"], eta, zeta, t[2], t[3])
        assert a.dtype == torch.float32 and torch.equal(a, _renoise_before(t[0], t[1], odt, st["t"], st["t_im1"], eta, zeta, t[2], t[3]))
        assert torch.equal(a, do.renoise(t[0], t[1], odt, st["t"], st["t_im1"], eta, zeta, t[2], t[3], dtype=torch.float32))
        np.testing.assert_allclose(a.numpy(), F.renoise_f32(xs, x0s, st, n1, n2), rtol=0, atol=2e-6)      # the bound test_gpu_ops.py holds the kernel to
        r64 = do.renoise(t[0].double(), t[1].double(), odt, st["t"], st["t_im1"], eta, zeta, t[2].double(), t[3].double(), dtype=torch.float64)
        assert r64.dtype == torch.float64 and np.abs(r64.numpy() - F.renoise(xs, x0s, st, n1, n2)).max() <= 1e-12
