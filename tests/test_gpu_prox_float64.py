"""-m gpu: the closed-form FFT prox (pre_calculate + data_solution, utils_sisr.py:65-95) of all three kernel families against float64, plane by plane.

Families: fft4 (csrc/fft4*.h*: one wave per transform, 256^2 / 512^2, sf 1/2/4, the default), fft2 (csrc/fft2*.h*: two-pass register kernels, 64^2, and
256^2 / 512^2 after set_prox_launch("launches")), generic (csrc/fft.hip: every other power-of-two shape, H <= 1024, W <= 2048, sf up to 16).

Yardstick (tests/prox_f64.py): per plane (image, channel), normalised by the plane's own max |float64|.  data_solution: e_p <= max(K o_p, F), o_p the
fp32 oracle's own error on that plane (the conditioning at small alpha); spectra FB / F2B / FBFy read back with dpir_prox_read: plane-relative
<= SPEC_TOL.  Inputs are probe batches (random, constant, checkerboard, row / column stripes, impulses at both corners, one image scaled by 1e-3)
blurred by PSFs from 1 x 1 to 25 x 25 (even, non-square, motion-like, [0.5, 0.5] whose FB vanishes on the Nyquist column), alpha 7e-7 .. 1e3.
The module prints the worst values per family at its end (run with -s).

Measured on an MI355X (K = 8, F = 1e-5, SPEC_TOL = 2e-6):
  spectra, worst plane-relative error: fft4 FB 2.1e-7, F2B 4.3e-7, FBFy 4.0e-7; fft2 1.8e-7, 4.1e-7, 3.7e-7; generic 2.8e-7, 5.9e-7, 4.8e-7.
  data_solution, worst e_p where F binds: fft4 4.0e-6, fft2 1.7e-6, generic 5.6e-6.  Worst e_p / o_p where K o_p binds: fft4 7.2, fft2 4.8,
  generic 6.4 outside sf > 1 at alpha 7e-7; delta-PSF closed form 2.7 / 1.8 / 2.0 everywhere; guided apply 2.8 / 7.6 / 2.0.
  The sf^2 alias means are summed pairwise, as torch.mean does (fft_regs.h): summed one after another, a 1 x 1 PSF at sf 8 was 515 x the oracle's
  error at alpha 7e-7 (e_p 1.2), and sf 4 was 17.9 x.  What remains (prox_f64.K_SMALL_ALPHA_SF): sf > 1 at alpha 7e-7 with a blurring PSF, up
  to 14.2 (generic 128 x 32 sf 4) and 9.4 (fft4)."""
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
    yield e
    e.close()
    print("\nworst per family (per-plane, against float64):")
    for key in sorted(_WORST):
        print(f"  {key}: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(_WORST[key].items())))


def _family(mode, H, W, sf):
    if sf in (1, 2, 4) and H == W and H in (256, 512) and mode == 1:
        return "fft4"
    if sf in (1, 2, 4) and H == W and H in (64, 256, 512):
        return "fft2"
    return "generic"


def _inputs(B, H, W, sf, psf_name, seed):
    rng = np.random.default_rng(seed)
    y = pf.probe_batch(B, H // sf, W // sf, rng, offset=seed % 7)
    z = pf.probe_batch(B, H, W, rng, offset=(seed + 3) % 7)
    k = pf.psf_batch(psf_name, B, rng)
    return y, z, k


def _spectra(pre):
    return {"FB": pre[0].numpy(), "F2B": pre[2].numpy(), "FBFy": pre[3].numpy()}


def _run_case(e, mode, B, H, W, sf, psf_name, alphas=ALPHAS):
    seed = 7 * H + 3 * W + 5 * sf + B + pf.PSFS.index(psf_name)
    e.set_prox_launch(mode)
    fam = _family(mode, H, W, sf)
    label = f"{fam} {H}x{W} sf {sf} B {B} psf {psf_name}"
    y, z, k = _inputs(B, H, W, sf, psf_name, seed)
    pre64, pre32 = pf.references(y, k, sf)
    pre = sr.pre_calculate(e.to_device(y), e.to_device(k), sf)
    res = pf.check_spectra(_spectra(pre), pre64, label)
    _note(fam, **{f"spectrum {nm}": v[0] for nm, v in res.items()})
    zd = e.to_device(z)
    for a in alphas:
        out = sr.data_solution(zd, *pre, a, sf).numpy()
        s = pf.check_solution(out, pf.solve(z, pre64, a, sf, torch.float64), pf.solve(z, pre32, a, sf, torch.float32), f"{label} alpha {a:g}",
                              K=pf.k_ratio(sf, a))
        _note(fam, e_p=s["e"], **{"e_p/o_p where K o_p > F": s["ratio_cond"], "e_p where F binds": s["e_floor"], "margin": s["margin"]})


# ---------------------------------------------------------------------------------------------------------------- the three families
_ROT = ("rand25", "rand15", "even8", "r7x9", "r9x7", "motion", "pair", "delta")
FFT4 = [(H, sf, B, _ROT[i % len(_ROT)]) for i, (H, sf, B) in enumerate((H, sf, B) for H in (256, 512) for sf in (1, 2, 4) for B in (1, 3, 8))]


@pytest.mark.parametrize("H,sf,B,psf_name", FFT4)
def test_fft4_wave_kernels_vs_float64(engine, H, sf, B, psf_name):
    _run_case(engine, 1, B, H, H, sf, psf_name)


FFT2 = [(H, sf, _ROT[(i + 3) % len(_ROT)]) for i, (H, sf) in enumerate((H, sf) for H in (64, 256, 512) for sf in (1, 2, 4))]


@pytest.mark.parametrize("H,sf,psf_name", FFT2)
def test_fft2_register_kernels_vs_float64(engine, H, sf, psf_name):
    _run_case(engine, 0, 3, H, H, sf, psf_name)


GENERIC = [
    (16, 16, 1, 3, "full16"), (16, 16, 2, 3, "r7x9"), (16, 16, 4, 3, "pair"), (16, 16, 8, 3, "delta"), (16, 16, 16, 3, "r9x7"),
    (32, 128, 1, 3, "rand15"), (32, 128, 2, 3, "motion"), (128, 32, 2, 3, "even8"), (128, 32, 4, 3, "r9x7"), (64, 64, 8, 3, "pair"),
    (128, 128, 8, 3, "rand25"), (256, 256, 8, 3, "motion"), (256, 256, 16, 3, "rand15"),
    (256, 512, 2, 3, "rand25"), (512, 256, 4, 3, "pair"),
    (1024, 1024, 1, 1, "rand25"), (1024, 2048, 2, 1, "motion"),
]


@pytest.mark.parametrize("H,W,sf,B,psf_name", GENERIC)
def test_generic_kernels_vs_float64(engine, H, W, sf, B, psf_name):
    _run_case(engine, 1, B, H, W, sf, psf_name, ALPHAS if H * W <= 512 * 512 else (7e-7, 1e-2, 1e3))


# ---------------------------------------------------------------------------------------------------------------- analytic, no oracle
DELTA = [(1, 256, 256, 1), (1, 256, 256, 2), (1, 512, 512, 4), (0, 256, 256, 4), (0, 64, 64, 1), (0, 64, 64, 2),
         (1, 16, 16, 8), (1, 16, 16, 16), (1, 32, 128, 2), (1, 128, 32, 1), (1, 256, 256, 8)]


@pytest.mark.parametrize("mode,H,W,sf", DELTA)
def test_delta_psf_equals_closed_form(engine, mode, H, W, sf):
    """1 x 1 delta PSF: the exact solution is (y + alpha z) / (1 + alpha) at the sampled pixels (sf i, sf j) and z everywhere else (every pixel
    for sf = 1), evaluated in float64 with no oracle.  The fp32 oracle's distance from the same closed form sets the conditioning allowance."""
    engine.set_prox_launch(mode)
    fam = _family(mode, H, W, sf)
    y, z, k = _inputs(3, H, W, sf, "delta", H + W + sf)
    pre = sr.pre_calculate(engine.to_device(y), engine.to_device(k), sf)
    pre32 = do.pre_calculate(torch.from_numpy(y), torch.from_numpy(k), sf)
    zd = engine.to_device(z)
    for a in ALPHAS:
        exact = pf.delta_solution(y, z, a, sf)
        out = sr.data_solution(zd, *pre, a, sf).numpy()
        s = pf.check_solution(out, exact, pf.solve(z, pre32, a, sf, torch.float32), f"delta PSF {fam} {H}x{W} sf {sf} alpha {a:g}")       # K = 8 throughout
        _note(f"{fam} (delta PSF, closed form)", e_p=s["e"], **{"e_p/o_p where K o_p > F": s["ratio_cond"], "e_p where F binds": s["e_floor"]})


# ---------------------------------------------------------------------------------------------------------------- guided apply, in place
APPLY = [(1, 256, 256, 2), (1, 512, 512, 1), (0, 256, 256, 4), (0, 64, 64, 1), (1, 128, 32, 2), (1, 16, 16, 16)]


@pytest.mark.parametrize("mode,H,W,sf", APPLY)
def test_guided_apply_vs_float64(engine, mode, H, W, sf):
    """dpir_prox_fft_apply (main_ddpir.py:395-400: x0 <- x0 + g (2 data_solution(x0/2 + 1/2, tau) - 1 - x0), in place) with guidance 1 and 0.6
    against oracle.prox_fft(..., exact=True) on float64 x0, with prox_fft in fp32 as the conditioning yardstick."""
    engine.set_prox_launch(mode)
    fam = _family(mode, H, W, sf)
    y, z, k = _inputs(3, H, W, sf, "rand15" if H >= 16 * 2 else "r7x9", 11 * H + sf)
    x0 = (z * 2 - 1).astype(np.float32)
    pre64, pre32 = pf.references(y, k, sf)
    pre = sr.pre_calculate(engine.to_device(y), engine.to_device(k), sf)
    for tau in (7e-7, 1e-2, 1.0):
        for g in (1.0, 0.6):
            t32 = torch.tensor(pf.alpha32(tau)).repeat(1, 1, 1, 1)
            ref = do.prox_fft(torch.from_numpy(x0).double(), pre64, t32.double(), sf, g, exact=True).numpy()
            o32 = do.prox_fft(torch.from_numpy(x0), pre32, t32, sf, g).numpy()
            d = engine.to_device(x0)
            engine._check(engine.lib.dpir_prox_fft_apply(engine.h, pre[0].spectra.handle, d.ptr, tau, g))
            s = pf.check_solution(d.numpy(), ref, o32, f"guided apply {fam} {H}x{W} sf {sf} tau {tau:g} g {g}",
                                  K=pf.k_ratio(sf, tau))
            _note(f"{fam} (guided apply)", e_p=s["e"], **{"e_p/o_p where K o_p > F": s["ratio_cond"], "e_p where F binds": s["e_floor"]})


@pytest.mark.parametrize("mode,H,W,sf", [(1, 256, 256, 4), (0, 512, 512, 2), (1, 64, 64, 1), (1, 32, 128, 2)])
def test_data_solution_in_place_equals_separate_output(engine, mode, H, W, sf):
    engine.set_prox_launch(mode)
    y, z, k = _inputs(3, H, W, sf, "r9x7", H + sf)
    pre = sr.pre_calculate(engine.to_device(y), engine.to_device(k), sf)
    for a in (1e-4, 1.0):
        sep = sr.data_solution(engine.to_device(z), *pre, a, sf).numpy()
        d = engine.to_device(z)
        assert sr.data_solution(d, *pre, a, sf, out=d) is d
        assert np.array_equal(d.numpy(), sep), (mode, H, W, sf, a)


def test_two_live_spectra_interleaved_equal_solo_runs(engine):
    """Several live dpir_prox objects of different shapes and families, used in turn: every result equals, bit for bit, the same object run with
    no other one alive.  They share the engine's named workspaces (prox#hbuf for fft4 / fft2, prox#buf for the generic path), which grow as the
    shapes come in."""
    engine.set_prox_launch(1)
    cases = [(64, 64, 1, 2), (32, 128, 2, 3), (256, 256, 2, 3), (128, 32, 4, 1), (512, 512, 4, 1)]       # fft2, generic, fft4, generic, fft4
    inputs = [_inputs(B, H, W, sf, "r7x9", 100 + i) for i, (H, W, sf, B) in enumerate(cases)]
    solo = []
    for (H, W, sf, B), (y, z, k) in zip(cases, inputs):
        pre = sr.pre_calculate(engine.to_device(y), engine.to_device(k), sf)
        solo.append([sr.data_solution(engine.to_device(z), *pre, a, sf).numpy() for a in (1e-3, 0.3)])
        del pre
    engine.sync()
    live = [sr.pre_calculate(engine.to_device(y), engine.to_device(k), sf) for (H, W, sf, B), (y, z, k) in zip(cases, inputs)]
    zs = [engine.to_device(z) for (y, z, k) in inputs]
    for ai, a in enumerate((1e-3, 0.3)):
        for i in (0, 2, 1, 4, 3, 0, 4, 2, 1, 3):
            out = sr.data_solution(zs[i], *live[i], a, cases[i][2]).numpy()
            assert np.array_equal(out, solo[i][ai]), (cases[i], a)


# ---------------------------------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("B,H,W,sf,kh,kw,rc", [
    (1, 2048, 16, 1, 3, 3, ERR_UNSUPPORTED),      # generic path: the column pass needs H <= 1024
    (1, 2048, 64, 2, 3, 3, ERR_UNSUPPORTED),
    (1, 16, 4096, 1, 3, 3, ERR_UNSUPPORTED),
    (1, 96, 96, 1, 3, 3, ERR_UNSUPPORTED),        # not a power of two
    (3, 16, 16, 1, 17, 3, ERR_INVALID),           # PSF taller than the image
    (1, 64, 64, 1, 3, 65, ERR_INVALID),           # wider (fft2 path)
    (1, 256, 256, 2, 257, 1, ERR_INVALID),        # fft4 path
    (1, 16, 16, 32, 1, 1, ERR_INVALID),           # sf does not divide the image
    (1, 256, 256, 3, 3, 3, ERR_INVALID),
    (1, 48, 48, 3, 3, 3, ERR_UNSUPPORTED),        # sf = 3
    (1, 96, 96, 3, 3, 3, ERR_UNSUPPORTED),
    (0, 64, 64, 1, 3, 3, ERR_INVALID),
])
def test_precalc_rejects_before_any_launch(engine, B, H, W, sf, kh, kw, rc):
    """dpir_prox_fft_precalc returns the documented error for shapes no kernel serves and launches nothing (the profiler counts no fft-prox or
    elementwise work; the stream stays healthy).  The buffers hold the full image, so a launch would have stayed in bounds."""
    engine.set_prox_launch(1)
    y = engine.empty((max(1, B) * 3 * H * W,))
    k = engine.empty((max(1, B) * kh * kw,))
    hnd = C.c_void_p()
    engine.sync()
    engine.prof_enable(True)
    engine.prof_reset()
    try:
        got = engine.lib.dpir_prox_fft_precalc(engine.h, y.ptr, k.ptr, kh, kw, sf, B, H, W, C.byref(hnd))
        counts = {nm: c for nm, (ms, c) in engine.prof_read().items()}
    finally:
        engine.prof_enable(False)
    assert got == rc, (got, engine.lib.dpir_last_error(engine.h))
    assert not hnd.value
    assert all(c == 0 for c in counts.values()), counts
    engine.sync()
