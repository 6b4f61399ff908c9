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
