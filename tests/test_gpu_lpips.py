"""-m gpu: LPIPS on the engine (dpir_lpips, csrc/lpips.hip) against the float64 statement of tests/lpips_f64.py, with seeded synthetic
weights, at the smallest shapes where each part can go wrong:
  16 x 16, B 2    relu5_3 is 1 x 1;
  32 x 32, B 1;
  40 x 56, B 3    5 -> 2 and 7 -> 3 pool floors (the scalar pool path), widths that are no multiple of a convolution tile;
  96 x 160, B 2   several pixel tiles, ragged against the 8 x 32 patch, 8 co-blocks at 512 channels.
Pairs per shape: ground truth + noise (x0 leaves [0, 1] and goes in un-clamped), ground truth with ONE value moved by 2/255, the identical pair."""
import logging
import re

import numpy as np
import pytest
import torch

import diffpir_amd
from diffpir_amd import degrade as dgr, lpips as lp
from diffpir_amd.engine import EngineError
from tests import lpips_f64 as L

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16, 2), (32, 32, 1), (40, 56, 3), (96, 160, 2)]
IDS = [f"{h}x{w}-B{b}" for h, w, b in SHAPES]
BATCHED = [s for s in SHAPES if s[2] > 1]
BATCHED_IDS = [f"{h}x{w}-B{b}" for h, w, b in BATCHED]
SEED = 3


@pytest.fixture(scope="module")
def sd():
    return lp.synth_weights(SEED)


@pytest.fixture(scope="module")
def engine(sd):
    e = diffpir_amd.Engine(0)
    e.load_lpips(sd)
    e.lpips_keep_taps(True)
    yield e
    e.close()


_CASES = {}


def case(sd, H, W, B, kind):
    """(x0, gt_u8, float64 statement, float32 statement), computed once per (shape, kind) and never modified."""
    key = (H, W, B, kind)
    if key not in _CASES:
        x0, gt_u8 = L.make_pair(H, W, B, kind)
        gt = L.gt_single(gt_u8)
        refs = (L.lpips(sd, x0, gt), L.lpips(sd, x0, gt, torch.float32)) if kind != "same" else (None, None)
        for a in (x0, gt_u8):
            a.setflags(write=False)
        _CASES[key] = (x0, gt_u8) + refs
    return _CASES[key]


def run(engine, x0, gt, taps=False):
    score = dgr.lpips(engine, x0, gt)
    if not taps:
        return score
    B, _, H, W = x0.shape
    out, h, w = [], H, W
    for k, c in enumerate(lp.TAP_CHANNELS):
        out.append(engine.lpips_read_tap(k).reshape(2 * B, c, h, w))
        h, w = h // 2, w // 2
    return score, out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("kind", ["noise", "pixel"])
@pytest.mark.parametrize("H,W,B", SHAPES, ids=IDS)
def test_taps_and_score_against_float64(engine, sd, H, W, B, kind):
    x0, gt_u8, r64, r32 = case(sd, H, W, B, kind)
    if kind == "noise":
        assert x0.min() < 0 and x0.max() > 1                      # goes in un-clamped: the statement sees the same values
    score, taps = run(engine, x0, gt_u8, taps=True)
    assert score.dtype == np.float32 and score.shape == (B,) and np.all(np.isfinite(score))
    print(f"lpips {H}x{W} B{B} {kind}: engine {score.tolist()} float64 {r64[0].tolist()} rel {L.score_rel(score, r64[0]).tolist()} "
          f"float32 statement rel {L.score_rel(r32[0], r64[0]).tolist()}")
    L.check(score, taps, r64, r32, f"{H}x{W} B{B} {kind}")
    assert np.all(L.score_rel(score, r64[0]) <= L.SCORE_CAP)      # 1e-4 relative in every case, whatever the yardstick did


@pytest.mark.parametrize("H,W,B", SHAPES, ids=IDS)
def test_identical_pair_is_exactly_zero(engine, sd, H, W, B):
    x0, gt_u8, _, _ = case(sd, H, W, B, "same")
    score, taps = run(engine, x0, gt_u8, taps=True)
    assert np.all(score == 0.0) and not np.signbit(score).any()
    for t in taps:
        assert same_bits(t[:B], t[B:]) and (t >= 0).all() and t.max() > 0


@pytest.mark.parametrize("H,W,B", SHAPES, ids=IDS)
def test_u8_entry_has_the_bits_of_the_f32_entry(engine, sd, H, W, B):
    for kind in ("noise", "pixel"):
        x0, gt_u8, _, _ = case(sd, H, W, B, kind)
        a = run(engine, x0, gt_u8)
        b = run(engine, x0, L.gt_single(gt_u8))
        assert same_bits(a, b), (kind, a, b)


@pytest.mark.parametrize("H,W,B", BATCHED, ids=BATCHED_IDS)
def test_every_image_has_the_bits_it_has_alone_and_repeats(engine, sd, H, W, B):
    for kind in ("noise", "pixel"):
        x0, gt_u8, _, _ = case(sd, H, W, B, kind)
        batch = run(engine, x0, gt_u8)
        assert same_bits(batch, run(engine, x0, gt_u8)), kind                       # a second call repeats bit for bit
        alone = np.concatenate([run(engine, x0[b:b + 1], gt_u8[b:b + 1]) for b in range(B)])
        assert same_bits(batch, alone), (kind, batch, alone)
        flipped = run(engine, x0[::-1], gt_u8[::-1])                               # another position in the batch
        assert same_bits(batch, flipped[::-1]), kind


@pytest.mark.parametrize("H,W,B", BATCHED, ids=BATCHED_IDS)
def test_a_forced_small_chunk_changes_no_bit(engine, sd, H, W, B, monkeypatch):
    x0, gt_u8, _, _ = case(sd, H, W, B, "noise")
    whole, taps_whole = run(engine, x0, gt_u8, taps=True)
    monkeypatch.setenv("DPIR_LPIPS_CHUNK", "2")                                    # one pair per chunk: below 2B rows
    chunked, taps_chunked = run(engine, x0, gt_u8, taps=True)
    monkeypatch.delenv("DPIR_LPIPS_CHUNK")
    assert same_bits(whole, chunked)
    for a, b in zip(taps_whole, taps_chunked):
        assert same_bits(a, b)


def test_precision_mode_does_not_reach_lpips(engine, sd):
    """LPIPS always runs the exact-fp32 convolution: an engine in f16x3 mode gives the bits of one in fp32 mode."""
    H, W, B = SHAPES[2]
    x0, gt_u8, _, _ = case(sd, H, W, B, "noise")
    ref = run(engine, x0, gt_u8)
    e = diffpir_amd.Engine(0)
    try:
        e.set_precision("f16x3")
        e.load_lpips(sd)
        assert same_bits(ref, run(e, x0, gt_u8))
    finally:
        e.close()


def test_small_images_and_missing_weights_are_errors(engine, sd):
    x0, gt_u8 = L.make_pair(8, 32, 1, "noise")
    with pytest.raises(EngineError, match="must be >= 16"):
        run(engine, x0, gt_u8)
    x0, gt_u8, _, _ = case(sd, 16, 16, 2, "noise")
    e = diffpir_amd.Engine(0)
    try:
        with pytest.raises(EngineError, match="no LPIPS weights loaded"):
            run(e, x0, gt_u8)
        with pytest.raises(EngineError, match=r"features\.2\.bias"):
            bad = {k: v for k, v in sd.items() if k != "features.2.bias"}
            # past the host check: the C loader names the key itself
            arr = (diffpir_amd._lib.Tensor * len(bad))()
            for i, (k, a) in enumerate(bad.items()):
                arr[i].name, arr[i].data, arr[i].ndim = k.encode(), a.ctypes.data, a.ndim
                for d in range(a.ndim):
                    arr[i].shape[d] = a.shape[d]
            e._check(e.lib.dpir_lpips_load(e.h, arr, len(bad)))
    finally:
        e.close()
    assert np.all(np.isfinite(run(engine, x0, gt_u8)))             # the module's engine is still usable after the refusals


def test_driver_logs_the_batch_lpips_of_its_own_outputs(sd, tmp_path, monkeypatch, caplog):
    """--synthetic 2, 2 NFE, calc_LPIPS: true with synthetic weight files under <cwd>/model_zoo: the batch line carries the mean of
    degrade.lpips over the batch's outputs, and a fresh engine reproduces those per-image scores bit for bit."""
    import yaml
    from diffpir_amd import main_ddpir
    zoo = tmp_path / "model_zoo"
    zoo.mkdir()
    torch.save({k: torch.from_numpy(v) for k, v in sd.items() if k.startswith("features.")}, zoo / "vgg16-397923af.pth")
    torch.save({f"lin{k}.model.1.weight": torch.from_numpy(sd[f"lin{k}.weight"]).view(1, -1, 1, 1) for k in range(5)}, zoo / "lpips_vgg.pth")
    cfg = yaml.safe_load(open("configs/engine_example.yaml"))
    cfg.update(iter_num=2, batch_size=2, task="deblur", calc_LPIPS=True, cwd=str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    seen = []
    real = dgr.lpips

    def recording(eng, x0, gt):
        out = real(eng, x0, gt)
        seen.append((x0.numpy(), gt.numpy(), out.copy()))
        return out
    monkeypatch.setattr(dgr, "lpips", recording)
    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        res = main_ddpir.main(["--opt", str(p), "--synthetic", "2", "--max-sweeps", "1"])
    assert len(res) == 1 and np.isfinite(res[0])                   # main() still returns the PSNR averages
    assert len(seen) == 1 and seen[0][2].shape == (2,) and np.all(np.isfinite(seen[0][2])) and np.all(seen[0][2] > 0)
    lines = [r.getMessage() for r in caplog.records]
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and "LPIPS" in r.getMessage()]
    batch = [m for m in lines if m.startswith("batch")]
    assert len(batch) == 1
    m = re.fullmatch(r"batch   1--> PSNR: (\S+)dB; LPIPS: (\S+); ave LPIPS: (\S+)", batch[0])
    assert m, batch[0]
    mean = float(np.mean(seen[0][2].astype(np.float64)))
    assert m.group(2) == f"{mean:.4f}" and m.group(3) == f"{mean:.4f}"
    assert [m_ for m_ in lines if m_.startswith("-----------> Average LPIPS of (demo_test)") and m_.endswith(f": {mean:.4f}")]
    e = diffpir_amd.Engine(0)
    try:
        e.load_lpips(sd)
        assert same_bits(real(e, seen[0][0], seen[0][1]), seen[0][2])
    finally:
        e.close()
