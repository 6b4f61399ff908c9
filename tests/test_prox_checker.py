"""CPU: the float64 prox yardstick of tests/prox_f64.py is sharp.  It accepts the fp32 oracle (utils_sisr.py:65-95 on float32 inputs) and rejects
each of a set of float64-computed defects that a prox kernel can plausibly have -- while the batch-wide 2e-4 bound the older prox tests use lets at
least one of them through.  Also pins the analytic delta-PSF solution the GPU tests use as an oracle-free yardstick."""
import numpy as np
import pytest
import torch

from oracle import diffpir_oracle as do
from tests import prox_f64 as pf


def _old_bound_ok(out, ref):
    """The bound of test_gpu_ops.py's full-size prox tests: max |out - ref| < 2e-4 * max(1, max |ref|) over the whole batch."""
    return float(np.abs(out - ref).max()) < 2e-4 * max(1.0, float(np.abs(ref).max()))


def _data_solution64(z, FB, F2B, FBFy, alpha, sf, fx_hook=None, n_alias=None):
    """utils_sisr.py:65-75 in float64 with optional defects: fx_hook edits FX before the inverse transform, n_alias < sf^2 averages over the
    first n_alias aliases only."""
    alpha = pf.alpha32(alpha)
    FR = FBFy + torch.fft.fftn(alpha * torch.from_numpy(np.asarray(z, np.float64)), dim=(-2, -1))
    x1 = FB * FR
    sa, sw = do.splits(x1, sf), do.splits(F2B, sf)
    if n_alias is not None:
        sa, sw = sa[..., :n_alias], sw[..., :n_alias]
    FBR, invW = sa.mean(dim=-1), sw.mean(dim=-1)
    FX = (FR - torch.conj(FB) * (FBR / (invW + alpha)).repeat(1, 1, sf, sf)) / alpha
    if fx_hook is not None:
        FX = fx_hook(FX.clone())
    return torch.real(torch.fft.ifftn(FX, dim=(-2, -1))).numpy()


def _case(B, H, W, sf, psf, seed):
    rng = np.random.default_rng(seed)
    y = pf.probe_batch(B, H // sf, W // sf, rng, offset=0)
    z = pf.probe_batch(B, H, W, rng, offset=3)
    k = pf.psf_batch(psf, B, rng)
    pre64, pre32 = pf.references(y, k, sf)
    return y, z, k, pre64, pre32


def _nyq_col_zero(FX):
    FX[..., FX.shape[-1] // 2] = 0
    return FX


def _nyq_col_conj(FX):
    FX[..., FX.shape[-1] // 2] = torch.conj(FX[..., FX.shape[-1] // 2])
    return FX


def _nyq_row_conj(FX):
    FX[..., FX.shape[-2] // 2, :] = torch.conj(FX[..., FX.shape[-2] // 2, :])
    return FX


def _nyq_row_zero(FX):
    FX[..., FX.shape[-2] // 2, :] = 0
    return FX


@pytest.mark.parametrize("alpha", [1e-4, 1e-2, 1.0])
@pytest.mark.parametrize("H,W,sf", [(32, 32, 1), (64, 32, 2), (32, 64, 4)])
def test_checker_accepts_fp32_oracle(H, W, sf, alpha):
    y, z, k, pre64, pre32 = _case(3, H, W, sf, "rand15", H + W + sf)
    x64, x32 = pf.solve(z, pre64, alpha, sf, torch.float64), pf.solve(z, pre32, alpha, sf, torch.float32)
    s = pf.check_solution(x32, x64, x32, f"fp32 oracle {H}x{W} sf {sf} alpha {alpha:g}")
    assert s["ratio"] == pytest.approx(1.0)
    pf.check_spectra({"FB": pre32[0].numpy(), "F2B": pre32[2].numpy(), "FBFy": pre32[3].numpy()}, pre64, "fp32 oracle spectra")
    # and the float64 reference taken apart here equals the oracle's (the defects below differ from it only by the defect)
    assert np.abs(_data_solution64(z, pre64[0], pre64[2], pre64[3], alpha, sf) - x64).max() < 1e-12


DEFECTS = {
    "nyquist_col_zeroed": dict(fx_hook=_nyq_col_zero),
    "nyquist_col_unconjugated": dict(fx_hook=_nyq_col_conj),
    "nyquist_row_zeroed": dict(fx_hook=_nyq_row_zero),
    "nyquist_row_unconjugated": dict(fx_hook=_nyq_row_conj),
    "alias_mean_sf2_minus_1": dict(n_alias=-1),
    "psf_rolled_one_pixel": dict(),
    "fb_of_next_image": dict(),
}


@pytest.mark.parametrize("K", [pf.K_RATIO, pf.K_SMALL_ALPHA_SF])
@pytest.mark.parametrize("alpha", [1e-4, 1e-2, 1.0])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_checker_rejects_defect(defect, alpha, K):
    """(a) the Nyquist row / column of FX zeroed or left unconjugated, (b) the alias mean over sf^2 - 1 aliases, (c) the PSF rolled one pixel off,
    (d) image n using image n + 1's FB, each computed in float64 and held to the fp32 oracle's own conditioning at alpha in {1e-4, 1e-2, 1}, with
    both K the GPU tests use."""
    H, W, sf, B = 64, 32, 2, 3
    y, z, k, pre64, pre32 = _case(B, H, W, sf, "rand15", 7)
    FB, F2B, FBFy = pre64[0], pre64[2], pre64[3]
    kw = dict(DEFECTS[defect])
    if kw.get("n_alias") == -1:
        kw["n_alias"] = sf * sf - 1
    if defect == "psf_rolled_one_pixel":
        FB = torch.roll(torch.fft.ifftn(FB, dim=(-2, -1)), 1, dims=-1)
        FB = torch.fft.fftn(FB, dim=(-2, -1))
        F2B = torch.abs(FB) ** 2
        STy = torch.zeros(z.shape, dtype=torch.float64)
        STy[..., ::sf, ::sf] = torch.from_numpy(y).double()
        FBFy = torch.conj(FB) * torch.fft.fftn(STy, dim=(-2, -1))
    if defect == "fb_of_next_image":
        FB, F2B = torch.roll(FB, -1, dims=0), torch.roll(F2B, -1, dims=0)
    bad = _data_solution64(z, FB, F2B, FBFy, alpha, sf, **kw)
    x64, x32 = pf.solve(z, pre64, alpha, sf, torch.float64), pf.solve(z, pre32, alpha, sf, torch.float32)
    assert pf.solution_ok(x32, x64, x32, K=K)
    s = pf.solution_stats(bad, x64, x32, K=K)
    print(f"{defect} alpha {alpha:g} K {K:g}: worst plane {s['at']} e_p {s['e']:.2e}, bound used {s['margin']:.1f}x")
    assert s["margin"] > 1.0, (defect, s["e"], s["at"])


def test_checker_rejects_perturbed_scaled_plane_that_the_batch_bound_passes():
    """(e) one plane of the 1e-3-scaled image perturbed by 1e-4 of its own magnitude: the per-plane checker rejects it; the batch-wide
    2e-4 x max bound of the older tests does not see it."""
    H, W, sf, B = 64, 64, 1, 3
    y, z, k, pre64, pre32 = _case(B, H, W, sf, "rand25", 11)
    for alpha in (1e-2, 1.0):
        x64, x32 = pf.solve(z, pre64, alpha, sf, torch.float64), pf.solve(z, pre32, alpha, sf, torch.float32)
        assert pf.solution_ok(x32, x64, x32) and _old_bound_ok(x32, x64)
        bad = x64.copy()
        plane = bad[1, 2]                       # image 1 is the scaled one
        assert np.abs(plane).max() < 2 * pf.SCALED
        rng = np.random.default_rng(0)
        plane += 1e-4 * np.abs(plane).max() * rng.choice([-1.0, 1.0], plane.shape)
        s = pf.solution_stats(bad, x64, x32)
        assert s["margin"] > 1.0 and s["at"] == (1, 2), s["at"]
        assert _old_bound_ok(bad, x64)
    # a defect of a kernel rather than of its output: the scaled image (1) solved with image 2's FB.  Its error is large on its own plane and
    # small next to the batch's largest value
    for alpha in (1e-2, 1.0):
        x64, x32 = pf.solve(z, pre64, alpha, sf, torch.float64), pf.solve(z, pre32, alpha, sf, torch.float32)
        FB, F2B = pre64[0].clone(), pre64[2].clone()
        FB[1], F2B[1] = pre64[0][2], pre64[2][2]
        bad = _data_solution64(z, FB, F2B, pre64[3], alpha, sf)
        s = pf.solution_stats(bad, x64, x32)
        print(f"image 1 with image 2's FB, alpha {alpha:g}: per-plane e_p {s['e']:.2e} at {s['at']}, batch-wide {np.abs(bad - x64).max():.2e}")
        assert s["margin"] > 1.0 and s["at"][0] == 1
        assert _old_bound_ok(bad, x64)


@pytest.mark.parametrize("sf", [1, 2, 4])
def test_checker_rejects_spectrum_defects(sf):
    """FB of the next image and FBFy with the Nyquist column conjugated are rejected by the spectra bound."""
    y, z, k, pre64, pre32 = _case(3, 32, 32, sf, "r7x9", 5 + sf)
    got = {"FB": torch.roll(pre64[0], -1, dims=0).numpy(), "F2B": pre32[2].numpy(), "FBFy": pre32[3].numpy()}
    assert pf.spectrum_err(got["FB"], pre64[0].numpy())[0] > pf.SPEC_TOL
    fy = pre32[3].numpy().copy()
    fy[..., 5, 16] = np.conj(fy[..., 5, 16])
    assert pf.spectrum_err(fy, pre64[3].numpy())[0] > pf.SPEC_TOL


@pytest.mark.parametrize("alpha", [7e-7, 1e-2, 1e3])
@pytest.mark.parametrize("sf", [1, 2, 4, 8])
def test_delta_psf_closed_form_equals_float64_oracle(sf, alpha):
    """With a 1 x 1 delta PSF the prox is separable per pixel: (y + alpha z) / (1 + alpha) at the sampled pixels (sf i, sf j), z elsewhere.
    The float64 oracle agrees with it, so the GPU tests may use it as a yardstick that involves no oracle at all."""
    y, z, k, pre64, pre32 = _case(2, 32, 32, sf, "delta", sf)
    x64 = pf.solve(z, pre64, alpha, sf, torch.float64)
    ref = pf.delta_solution(y, z, alpha, sf)
    assert pf.plane_errs(x64, ref).max() < 1e-9 if alpha > 1e-6 else pf.plane_errs(x64, ref).max() < 1e-6


def test_probe_batch_and_psfs():
    rng = np.random.default_rng(0)
    p = pf.probe_batch(3, 8, 8, rng)
    assert p.dtype == np.float32 and p.shape == (3, 3, 8, 8)
    assert np.abs(p[1]).max() <= pf.SCALED and np.abs(p[0]).max() > 0.5
    assert p[0, 2, 0, 0] == np.float32(0.2) and p[0, 2, 0, 1] == np.float32(0.8)      # plane 2: checkerboard
    assert p[2, 0, 7, 7] == 1.0 and p[2, 0].sum() == 1.0                              # plane 6: impulse at (H-1, W-1)
    for nm in pf.PSFS:
        k = pf.psf(nm, rng)
        assert abs(float(k.sum()) - 1.0) < 1e-6 and (k >= 0).all(), nm
    fb = do.p2o(torch.from_numpy(pf.psf("pair", rng))[None, None].double(), (16, 16))
    assert float(torch.abs(fb[..., 8]).max()) == 0.0                        # [0.5, 0.5]: FB is exactly zero on the Nyquist column
