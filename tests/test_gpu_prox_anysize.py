"""-m gpu: the closed-form FFT prox at sides that are no power of two and at any integer sf (csrc/fft_mixed.hip, ProxLayout::FullDigitrev) against
float64, plane by plane, with the yardstick of tests/prox_f64.py as it stands: spectra read back through dpir_prox_read within SPEC_TOL, data_solution
within e_p <= max(k_ratio(sf, alpha) o_p, FLOOR) at alpha 7e-7 .. 1e3.  The cases are the smallest shapes that reach every code path: radices 2, 4,
3 and 5, the generic odd-prime butterfly (7, 11, 13, 31), composite sf, a guarded last strip, one power-of-two side.  Then the delta-PSF closed form,
the guided apply, bit-equality across batch sizes and repeats, the error codes, and the strict launch modes 0 and 1, which keep refusing these
shapes.  The module prints the worst values at its end (run with -s); profiles/prox_anysize/README.md records them.

Measured on an MI355X (K = 8, or 30 for sf > 1 at alpha <= 1e-4; F = 1e-5; SPEC_TOL = 2e-6), worst over the twelve cases: spectra FB 1.7e-7, F2B 3.7e-7,
FBFy 3.8e-7; data_solution e_p where F binds 2.2e-6 (480 x 640); e_p / o_p where K o_p binds 3.7 outside sf > 1 at small alpha and 11.5 there (30 x 50,
sf 5, the [0.5, 0.5] PSF at alpha 7e-7: 38 % of its bound; the same case at alpha 1e-2 uses 44 % of K = 8, the largest share of any case);
delta-PSF closed form 3.8; guided apply 1.6."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffpir_amd import utils_sisr as sr
from oracle import diffpir_oracle as do
from tests import prox_f64 as pf

pytestmark = pytest.mark.gpu

ALPHAS = (7e-7, 1e-4, 1e-2, 1.0, 1e3)
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
_WORST = {}


def _note(key, **vals):
    w = _WORST.setdefault(key, {})
    for k, v in vals.items():
        w[k] = max(w.get(k, 0.0), v)


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    e.set_prox_launch("wave+anysize")       # the engine's default (mode 3), set explicitly: modes 0 and 1 refuse these shapes
    yield e
    e.close()
    print("\nworst per case (per-plane, against float64):")
    for key in sorted(_WORST):
        print(f"  {key}: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(_WORST[key].items())))


def _inputs(B, H, W, sf, psf_name, seed):
    rng = np.random.default_rng(seed)
    y = pf.probe_batch(B, H // sf, W // sf, rng, offset=seed % 7)
    z = pf.probe_batch(B, H, W, rng, offset=(seed + 3) % 7)
    k = pf.psf_batch(psf_name, B, rng)
    return y, z, k


def _spectra(pre):
    return {"FB": pre[0].numpy(), "F2B": pre[2].numpy(), "FBFy": pre[3].numpy()}


CASES = [
    (24, 36, 1, 3, "r7x9"), (24, 36, 3, 3, "rand15"), (30, 50, 5, 2, "pair"), (36, 60, 6, 2, "delta"), (48, 80, 2, 3, "even8"),
    (44, 52, 4, 1, "motion"), (62, 93, 1, 1, "r9x7"), (64, 96, 2, 2, "rand15"), (96, 96, 3, 3, "motion"), (96, 160, 1, 3, "rand25"),
    (224, 352, 1, 1, "rand15"), (480, 640, 2, 1, "rand25"),
]


@pytest.mark.parametrize("H,W,sf,B,psf_name", CASES)
def test_mixed_radix_kernels_vs_float64(engine, H, W, sf, B, psf_name):
    alphas = ALPHAS if H * W < 480 * 640 else (7e-7, 1e-2, 1e3)
    seed = 7 * H + 3 * W + 5 * sf + B + pf.PSFS.index(psf_name)
    label = f"mixed {H}x{W} sf {sf} B {B} psf {psf_name}"
    y, z, k = _inputs(B, H, W, sf, psf_name, seed)
    pre64, pre32 = pf.references(y, k, sf)
    pre = sr.pre_calculate(engine.to_device(y), engine.to_device(k), sf)
    res = pf.check_spectra(_spectra(pre), pre64, label)
    _note(label, **{f"spectrum {nm}": v[0] for nm, v in res.items()})
    zd = engine.to_device(z)
    for a in alphas:
        out = sr.data_solution(zd, *pre, a, sf).numpy()
        s = pf.check_solution(out, pf.solve(z, pre64, a, sf, torch.float64), pf.solve(z, pre32, a, sf, torch.float32), f"{label} alpha {a:g}",
                              K=pf.k_ratio(sf, a))
        _note(label, e_p=s["e"], **{"e_p/o_p where K o_p > F": s["ratio_cond"], "e_p where F binds": s["e_floor"], "margin": s["margin"]})


@pytest.mark.parametrize("H,W,sf", [(24, 36, 3), (30, 50, 5), (96, 160, 1)])
def test_delta_psf_equals_closed_form(engine, H, W, sf):
    """1 x 1 delta PSF: (y + alpha z) / (1 + alpha) at the sampled pixels and z elsewhere, in float64 with no oracle; the fp32 oracle's distance from
    the same closed form sets the conditioning allowance, K = 8 throughout (tests/test_gpu_prox_float64.py takes it the same way)."""
    y, z, k = _inputs(3, H, W, sf, "delta", H + W + sf)
    pre = sr.pre_calculate(engine.to_device(y), engine.to_device(k), sf)
    pre32 = do.pre_calculate(torch.from_numpy(y), torch.from_numpy(k), sf)
    zd = engine.to_device(z)
    for a in ALPHAS:
        exact = pf.delta_solution(y, z, a, sf)
        out = sr.data_solution(zd, *pre, a, sf).numpy()
        s = pf.check_solution(out, exact, pf.solve(z, pre32, a, sf, torch.float32), f"delta PSF mixed {H}x{W} sf {sf} alpha {a:g}")
        _note("delta PSF, closed form", e_p=s["e"], **{"e_p/o_p where K o_p > F": s["ratio_cond"], "e_p where F binds": s["e_floor"]})


def test_guided_apply_vs_float64(engine):
    """dpir_prox_fft_apply (x0 <- x0 + g (2 data_solution(x0/2 + 1/2, tau) - 1 - x0), in place) with guidance 1 and 0.5 at 48 x 80, sf 2, against
    oracle.prox_fft(..., exact=True) on float64 x0, with prox_fft in fp32 as the conditioning yardstick."""
    H, W, sf = 48, 80, 2
    y, z, k = _inputs(3, H, W, sf, "rand15", 11 * H + sf)
    x0 = (z * 2 - 1).astype(np.float32)
    pre64, pre32 = pf.references(y, k, sf)
    pre = sr.pre_calculate(engine.to_device(y), engine.to_device(k), sf)
    for tau in (7e-7, 1e-2, 1.0):
        for g in (1.0, 0.5):
            t32 = torch.tensor(pf.alpha32(tau)).repeat(1, 1, 1, 1)
            ref = do.prox_fft(torch.from_numpy(x0).double(), pre64, t32.double(), sf, g, exact=True).numpy()
            o32 = do.prox_fft(torch.from_numpy(x0), pre32, t32, sf, g).numpy()
            d = engine.to_device(x0)
            engine._check(engine.lib.dpir_prox_fft_apply(engine.h, pre[0].spectra.handle, d.ptr, tau, g))
            s = pf.check_solution(d.numpy(), ref, o32, f"guided apply mixed {H}x{W} sf {sf} tau {tau:g} g {g}", K=pf.k_ratio(sf, tau))
            _note("guided apply", e_p=s["e"], **{"e_p/o_p where K o_p > F": s["ratio_cond"], "e_p where F binds": s["e_floor"]})


@pytest.mark.parametrize("H,W,sf", [(24, 36, 3), (48, 80, 2), (62, 93, 1)])
def test_same_bits_alone_in_a_batch_and_on_repeat(engine, H, W, sf):
    """Image 1 of a batch of 3 has the bits it has as a batch of 1 (spectra and solution), and a second run of the batch repeats the first's bits."""
    y, z, k = _inputs(3, H, W, sf, "r9x7", H + sf)
    runs = []
    for sel in (slice(0, 3), slice(0, 3), slice(1, 2)):
        pre = sr.pre_calculate(engine.to_device(y[sel]), engine.to_device(k[sel]), sf)
        outs = [sr.data_solution(engine.to_device(z[sel]), *pre, a, sf).numpy() for a in (7e-7, 1e-2)]
        runs.append((_spectra(pre), outs))
    for nm in ("FB", "F2B", "FBFy"):
        assert np.array_equal(runs[0][0][nm], runs[1][0][nm]) and np.array_equal(runs[0][0][nm][1:2], runs[2][0][nm]), nm
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a]) and np.array_equal(runs[0][1][a][1:2], runs[2][1][a])


def test_error_codes_and_the_engine_stays_usable(engine):
    y, k = engine.empty((3 * 74 * 64,)), engine.empty((9,))
    for H, W, sf, rc, word in ((74, 64, 1, ERR_UNSUPPORTED, "37"), (64, 64, 3, ERR_INVALID, "divisible")):
        hnd = C.c_void_p()
        got = engine.lib.dpir_prox_fft_precalc(engine.h, y.ptr, k.ptr, 3, 3, sf, 1, H, W, C.byref(hnd))
        msg = engine.lib.dpir_last_error(engine.h)
        assert got == rc and not hnd.value and word in (msg.decode() if isinstance(msg, bytes) else str(msg)), (got, msg)
    test_mixed_radix_kernels_vs_float64(engine, 24, 36, 3, 3, "rand15")


def test_strict_launch_modes_refuse_and_the_default_serves(engine):
    """dpir_set_prox_launch 0 / 1: only the power-of-two families run, 96 x 96 and sf 3 stay DPIR_ERR_UNSUPPORTED and nothing is allocated; 2 / 3 serve
    them, with the same bits under both (the bit that picks the half-spectrum kernels plays no part at these shapes)."""
    y, z, k = _inputs(1, 48, 96, 3, "r7x9", 5)
    yd, kd = engine.to_device(y), engine.to_device(k)
    outs = []
    try:
        for mode in (0, 1):
            engine.set_prox_launch(mode)
            hnd = C.c_void_p()
            got = engine.lib.dpir_prox_fft_precalc(engine.h, yd.ptr, kd.ptr, 7, 9, 3, 1, 48, 96, C.byref(hnd))
            assert got == ERR_UNSUPPORTED and not hnd.value, (mode, got)
        for mode in ("launches+anysize", "wave+anysize"):
            engine.set_prox_launch(mode)
            pre = sr.pre_calculate(yd, kd, 3)
            outs.append(sr.data_solution(engine.to_device(z), *pre, 1e-2, 3).numpy())
    finally:
        engine.set_prox_launch("wave+anysize")
    assert np.array_equal(outs[0], outs[1]) and np.isfinite(outs[0]).all()
