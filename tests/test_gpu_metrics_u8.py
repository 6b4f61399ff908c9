"""-m gpu: the 8-bit metrics on the engine (dpir_metrics_u8, csrc/metrics8.hip) against the float64 statement of tests/metrics_u8_f64.py, at
the smallest shapes (H, W, B, border) where each part can go wrong:
  11 x 11, B 1            one valid window;
  12 x 27, B 2            ragged, smaller than one 32 x 16 tile;
  40 x 56, B 3, border 4  a cropped border, more than one tile in both directions;
  96 x 160, B 2           many tiles (5 x 6), ragged last row and column.
Pair kinds: ground truth + noise with the float32 estimate leaving [0, 1]; one byte moved by 2; identical; flat 255 against flat 254 (the
cancellation worst case); both images tiled from the 194 Y-tie triplets.

Bounds.  |dSSIM|, |dSSIM-Y| <= 1e-9: two float64 summation orders differ by at most 6.3e-13 on these kinds (measured on the CPU,
test_metrics_u8_host.py prints the spread) and a float32 evaluation is off by 1.5e-9 or more, so the bound passes any correct float64 kernel
and fails a float32 one.  |dPSNR| <= 1e-10 dB: the sum of squared differences is an exact integer, only log10 and sqrt can differ, by a few ulp."""
import logging
import os
import re

import numpy as np
import pytest

import diffpir_amd
from diffpir_amd import degrade as dgr
from diffpir_amd.engine import EngineError, _ptr
from tests import metrics_u8_f64 as M

pytestmark = pytest.mark.gpu

SHAPES = [(11, 11, 1, 0), (12, 27, 2, 0), (40, 56, 3, 4), (96, 160, 2, 0)]
IDS = [f"{h}x{w}-B{b}-border{c}" for h, w, b, c in SHAPES]
BATCHED = [s for s in SHAPES if s[2] > 1]
BATCHED_IDS = [f"{h}x{w}-B{b}-border{c}" for h, w, b, c in BATCHED]
DIFFERENT = [k for k in M.KINDS if k != "same"]
SSIM_BOUND, PSNR_BOUND = 1e-9, 1e-10
DPIR_ERR_INVALID = -1


@pytest.fixture(scope="module")
def engine():
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


_CASES = {}


def case(H, W, B, border, kind):
    """(estimate float32, its bytes, ground-truth bytes, float64 statement [B,4]), computed once per (shape, kind) and never modified."""
    key = (H, W, B, border, kind)
    if key not in _CASES:
        est, gt = M.make_pair(H, W, B, kind)
        eu8 = M.quantise(est)
        ref = M.metrics(eu8, gt, border)
        for a in (est, eu8, gt, ref):
            a.setflags(write=False)
        _CASES[key] = (est, eu8, gt, ref)
    return _CASES[key]


def run(engine, est, gt, border):
    return np.stack(dgr.metrics_u8(engine, est, gt, border), 1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def psnr_err(got, ref):
    with np.errstate(invalid="ignore"):
        return np.where(got == ref, 0.0, np.abs(got - ref))        # +inf against +inf is agreement; +inf against a number is an infinite error


@pytest.mark.parametrize("kind", DIFFERENT)
@pytest.mark.parametrize("H,W,B,border", SHAPES, ids=IDS)
def test_four_numbers_against_float64(engine, H, W, B, border, kind):
    est, eu8, gt, ref = case(H, W, B, border, kind)
    if kind == "noise":
        assert est.min() < 0 and est.max() > 1                     # goes in un-clamped
    for name, arg in (("f32", est), ("u8", eu8)):
        got = run(engine, arg, gt, border)
        assert got.shape == (B, 4) and got.dtype == np.float64
        d_psnr, d_ssim = psnr_err(got[:, :2], ref[:, :2]).max(), np.abs(got[:, 2:] - ref[:, 2:]).max()
        print(f"metrics_u8 {H}x{W} B{B} border {border} {kind} [{name}]: engine {got.tolist()} |dPSNR| {d_psnr:.3e} dB |dSSIM| {d_ssim:.3e}")
        assert d_ssim <= SSIM_BOUND
        assert d_psnr <= PSNR_BOUND


@pytest.mark.parametrize("H,W,B,border", SHAPES, ids=IDS)
def test_identical_pair_is_exactly_one_and_inf(engine, H, W, B, border):
    est, eu8, gt, ref = case(H, W, B, border, "same")
    assert np.array_equal(eu8, gt)
    for arg in (est, eu8):
        got = run(engine, arg, gt, border)
        assert np.all(np.isposinf(got[:, :2])) and np.all(got[:, 2:] == 1.0)


@pytest.mark.parametrize("H,W,B,border", SHAPES, ids=IDS)
def test_f32_estimate_has_the_bits_of_the_call_on_finalize_s_bytes(engine, H, W, B, border):
    for kind in ("noise", "byte", "ties"):
        est, _, gt, _ = case(H, W, B, border, kind)
        x = engine.to_device((est * np.float32(2) - np.float32(1)).astype(np.float32))      # the loop's x in [-1, 1]
        of, ou = engine.empty((B, 3, H, W)), engine.empty((B, H, W, 3), np.uint8)
        engine._check(engine.lib.dpir_finalize(engine.h, x.ptr, of.ptr, ou.ptr, B, H, W))   # x_0 = x / 2 + 0.5 and tensor2uint's bytes
        assert np.array_equal(ou.numpy(), M.quantise(of.numpy()))
        gt_d = engine.to_device(gt)
        a, b = run(engine, of, gt_d, border), run(engine, ou, gt_d, border)
        assert same_bits(a, b), (kind, a, b)


@pytest.mark.parametrize("H,W,B,border", BATCHED, ids=BATCHED_IDS)
def test_every_image_has_the_bits_it_has_alone_and_repeats(engine, H, W, B, border):
    for kind in ("noise", "byte"):
        est, eu8, gt, _ = case(H, W, B, border, kind)
        batch = run(engine, est, gt, border)
        assert same_bits(batch, run(engine, est, gt, border)), kind                       # a second call repeats bit for bit
        alone = np.concatenate([run(engine, est[b:b + 1], gt[b:b + 1], border) for b in range(B)])
        assert same_bits(batch, alone), (kind, batch, alone)
        flipped = run(engine, est[::-1], gt[::-1], border)                                # another position in the batch
        assert same_bits(batch, flipped[::-1]), kind
        assert same_bits(batch, run(engine, est, gt, border)), kind                       # and after the smaller calls


def test_invalid_arguments_are_refused_and_the_engine_stays_usable(engine):
    est, eu8, gt, ref = case(12, 27, 2, 0, "noise")
    e_d, u_d, g_d = engine.to_device(est), engine.to_device(eu8), engine.to_device(gt)
    out = np.full((2, 4), -7.0)
    call = lambda *a: engine.lib.dpir_metrics_u8(*a)                                      # noqa: E731
    h, o = engine.h, out.ctypes.data
    bad = {
        "null engine": (None, _ptr(u_d), None, _ptr(g_d), 2, 12, 27, 0, o),
        "null ground truth": (h, _ptr(u_d), None, None, 2, 12, 27, 0, o),
        "null output": (h, _ptr(u_d), None, _ptr(g_d), 2, 12, 27, 0, None),
        "both estimates": (h, _ptr(u_d), _ptr(e_d), _ptr(g_d), 2, 12, 27, 0, o),
        "neither estimate": (h, None, None, _ptr(g_d), 2, 12, 27, 0, o),
        "B 0": (h, _ptr(u_d), None, _ptr(g_d), 0, 12, 27, 0, o),
        "B -1": (h, _ptr(u_d), None, _ptr(g_d), -1, 12, 27, 0, o),
        "border -1": (h, _ptr(u_d), None, _ptr(g_d), 2, 12, 27, -1, o),
        "H - 2 border 10": (h, _ptr(u_d), None, _ptr(g_d), 2, 12, 27, 1, o),
        "W 10": (h, _ptr(u_d), None, _ptr(g_d), 2, 27, 10, 0, o),
        "W - 2 border 9": (h, _ptr(u_d), None, _ptr(g_d), 1, 27, 12, 9, o),
    }
    for what, args in bad.items():
        assert call(*args) == DPIR_ERR_INVALID, what
        if args[0] is not None:
            assert b"dpir_metrics_u8" in engine.lib.dpir_last_error(engine.h), what
        assert np.all(out == -7.0), what                                                  # nothing was written
    with pytest.raises(EngineError, match="must be >= 11"):
        dgr.metrics_u8(engine, eu8, gt, border=1)
    with pytest.raises(ValueError, match="does not go with"):
        dgr.metrics_u8(engine, est[:, :, :11], gt)
    got = run(engine, u_d, g_d, 0)                                                        # still usable, DeviceArrays accepted
    assert np.abs(got[:, 2:] - ref[:, 2:]).max() <= SSIM_BOUND and psnr_err(got[:, :2], ref[:, :2]).max() <= PSNR_BOUND
    assert engine.lib.dpir_version() == 2


def test_driver_logs_the_four_lines_of_its_own_outputs(tmp_path, monkeypatch, caplog):
    """configs/ssim_example.yaml (x4 super-resolution) on --synthetic 2 at 2 NFE: the border is sf, the four batch lines and the four average lines
    carry the means of degrade.metrics_u8 over the batch's outputs, and those agree with the statement on the very images the driver measured."""
    import yaml
    from diffpir_amd import main_ddpir
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "ssim_example.yaml")))
    assert cfg["calc_SSIM"] is True and cfg["task"] == "sr" and cfg["sf"] == 4
    cfg.update(iter_num=2, batch_size=2, cwd=str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    seen = []
    real = dgr.metrics_u8

    def recording(eng, est, gt, border=0):
        out = real(eng, est, gt, border)
        seen.append((est.numpy(), gt.numpy(), border, np.stack(out, 1)))
        return out
    monkeypatch.setattr(dgr, "metrics_u8", recording)
    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        res = main_ddpir.main(["--opt", str(p), "--synthetic", "2", "--max-sweeps", "1"])
    assert len(res) == 1 and np.isfinite(res[0])
    assert len(seen) == 1 and seen[0][2] == 4 and seen[0][3].shape == (2, 4) and np.all(np.isfinite(seen[0][3]))
    est, gt, border, got = seen[0]
    ref = M.metrics(M.quantise(est), gt, border)
    assert np.abs(got[:, 2:] - ref[:, 2:]).max() <= SSIM_BOUND and psnr_err(got[:, :2], ref[:, :2]).max() <= PSNR_BOUND
    mean = got.mean(0)
    lines = [r.getMessage() for r in caplog.records]
    batch = [m for m in lines if m.startswith("batch")]
    assert len(batch) == 5 and re.fullmatch(r"batch   1--> PSNR: \S+dB", batch[0])
    assert batch[1:] == [f"batch   1--> PSNR(8-bit RGB): {mean[0]:.4f}dB", f"batch   1--> PSNR(8-bit Y): {mean[1]:.4f}dB",
                         f"batch   1--> SSIM(RGB): {mean[2]:.4f}", f"batch   1--> SSIM(Y): {mean[3]:.4f}"]
    tail = " of (demo_test) scale factor: (4), sigma: (0.050): "
    assert lines[-4:] == [f"-----------> Average PSNR(8-bit RGB){tail}{mean[0]:.4f} dB", f"-----------> Average PSNR(8-bit Y){tail}{mean[1]:.4f} dB",
                          f"-----------> Average SSIM(RGB){tail}{mean[2]:.4f}", f"-----------> Average SSIM(Y){tail}{mean[3]:.4f}"]
