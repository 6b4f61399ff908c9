"""-m gpu: the FID Inception-v3 features on the engine (dpir_fid_features, csrc/fid.hip) against the float64 statement of tests/fid_f64.py,
with seeded synthetic weights.  The network fixes its own internal shapes (pixel counts 1225 / 289 / 64 per image that fit no tile, Cout from
32 to 448, K from 27 to 4032, stride-2 valid convolutions), so the cases vary the entry only:
  256 x 256 u8, B 2      the driver's size;
  48 x 64 f32, B 1       non-square, enlarging resize, the float32 entry;
  299 x 299 u8, B 3      identity resize, odd batch;
  512 x 512 u8, B 1      shrinking resize.

Measured on the MI355X (profiles/fid/README.md has the tables): worst e_p / o_p over the four cases 1.84 (Mixed_7a, 256 x 256), so
K = min(8, 2 x 1.84) = 3.68 (tests/fid_f64.py).  The distance end to end, relative deviation from the float64 FID --
  8 columns    (FID 0.0167): float32 statement 1.88e-7, engine 2.97e-8;
  2048 columns (FID 4.963):  float32 statement 1.25e-7, engine 6.20e-8.
The float32 statement's figures repeated to every printed digit over three runs, so both column counts are asserted.
"""
import logging
import re

import numpy as np
import pytest
import torch

import diffpir_amd
from diffpir_amd import degrade as dgr, fid as fd
from diffpir_amd.engine import EngineError
from tests import fid_f64 as Fd

pytestmark = pytest.mark.gpu

CASES = [(256, 256, 2, "u8"), (48, 64, 1, "f32"), (299, 299, 3, "u8"), (512, 512, 1, "u8")]
IDS = [f"{h}x{w}-B{b}-{k}" for h, w, b, k in CASES]
SEED = 3


@pytest.fixture(scope="module")
def raw():
    return fd.synth_weights(SEED, raw=True)


@pytest.fixture(scope="module")
def engine(raw):
    e = diffpir_amd.Engine(0)
    e.load_fid(raw)                                   # the raw layout: Engine.load_fid folds the BatchNorm
    e.fid_keep_taps(True)
    yield e
    e.close()


_CASES = {}


def case(raw, H, W, B, kind):
    """(image as the engine takes it, float64 statement, float32 statement), computed once per case and never modified."""
    key = (H, W, B, kind)
    if key not in _CASES:
        img = Fd.make_images(H, W, B, seed=1, as_u8=kind == "u8")
        f32 = Fd.u8_single(img) if kind == "u8" else img
        img.setflags(write=False)
        _CASES[key] = (img, Fd.features(raw, f32), Fd.features(raw, f32, torch.float32))
    return _CASES[key]


def run_taps(engine, img):
    feats = dgr.fid_features(engine, img)
    B = img.shape[0]
    taps = [engine.fid_read_tap(k).reshape(B, c, s, s) for k, (c, s) in enumerate(fd.TAP_SHAPES)]
    taps.append(engine.fid_read_tap(13).reshape(B, fd.FEATURES))
    return feats, taps


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("H,W,B,kind", CASES, ids=IDS)
def test_taps_and_features_against_float64(engine, raw, H, W, B, kind):
    img, r64, r32 = case(raw, H, W, B, kind)
    feats, taps = run_taps(engine, img)
    assert feats.dtype == np.float32 and feats.shape == (B, 2048) and np.all(np.isfinite(feats))
    assert same_bits(feats, taps[13])
    assert all(t.max() > 0 for t in taps)
    Fd.check(taps, r64, r32, f"{H}x{W} B{B} {kind}")


def test_one_order_per_image(engine, raw, monkeypatch):
    """An image's 2048 features have the same bits alone, at any position of a batch of 3, on a repeat, and under DPIR_FID_CHUNK=1."""
    img, _, _ = case(raw, 299, 299, 3, "u8")
    batch = dgr.fid_features(engine, img)
    assert same_bits(batch, dgr.fid_features(engine, img))
    alone = np.concatenate([dgr.fid_features(engine, img[b:b + 1]) for b in range(3)])
    assert same_bits(batch, alone)
    for perm in ([2, 0, 1], [1, 2, 0]):
        assert same_bits(batch[perm], dgr.fid_features(engine, np.ascontiguousarray(img[perm]))), perm
    monkeypatch.setenv("DPIR_FID_CHUNK", "1")
    chunked, taps_chunked = run_taps(engine, img)
    monkeypatch.delenv("DPIR_FID_CHUNK")
    whole, taps_whole = run_taps(engine, img)
    assert same_bits(batch, chunked) and same_bits(batch, whole)
    for a, b in zip(taps_whole, taps_chunked):
        assert same_bits(a, b)


@pytest.mark.parametrize("H,W,B", [(256, 256, 2), (512, 512, 1)])
def test_u8_entry_has_the_bits_of_the_f32_entry(engine, raw, H, W, B):
    img, _, _ = case(raw, H, W, B, "u8")
    assert same_bits(dgr.fid_features(engine, img), dgr.fid_features(engine, Fd.u8_single(img)))


def test_precision_mode_does_not_reach_fid(engine, raw):
    img, _, _ = case(raw, 48, 64, 1, "f32")
    ref = dgr.fid_features(engine, img)
    e = diffpir_amd.Engine(0)
    try:
        e.set_precision("f16x3")
        e.load_fid(raw)
        assert same_bits(ref, dgr.fid_features(e, img))
    finally:
        e.close()


def _load_raw_tensors(e, sd):
    arr = (diffpir_amd._lib.Tensor * len(sd))()
    for i, (k, a) in enumerate(sd.items()):
        arr[i].name, arr[i].data, arr[i].ndim = k.encode(), a.ctypes.data, a.ndim
        for d in range(a.ndim):
            arr[i].shape[d] = a.shape[d]
    return e.lib.dpir_fid_load(e.h, arr, len(sd))


def test_errors(engine, raw):
    ERR_INVALID, ERR_STATE = -1, -4                  # include/diffpir_engine.h

    def last(e_):
        return e_.lib.dpir_last_error(e_.h).decode()
    img, _, _ = case(raw, 48, 64, 1, "f32")
    folded = fd.canonical(raw)
    e = diffpir_amd.Engine(0)
    try:
        dev = e.to_device(img)
        out = np.empty((1, 2048), np.float32)
        assert e.lib.dpir_fid_features(e.h, None, dev.ptr, 1, 48, 64, out.ctypes.data) == ERR_STATE       # no load yet
        with pytest.raises(EngineError, match="dpir_fid_load"):
            dgr.fid_features(e, img)
        missing = {k: v for k, v in folded.items() if k != "Mixed_6c.branch7x7dbl_3.bias"}
        assert _load_raw_tensors(e, missing) == ERR_INVALID and "Mixed_6c.branch7x7dbl_3.bias" in last(e)
        bad = dict(folded)
        bad["Mixed_7a.branch7x7x3_2.weight"] = np.ascontiguousarray(folded["Mixed_7a.branch7x7x3_2.weight"].transpose(0, 1, 3, 2))     # (7,1) for (1,7)
        assert _load_raw_tensors(e, bad) == ERR_INVALID and "Mixed_7a.branch7x7x3_2.weight" in last(e)
        assert e.lib.dpir_fid_features(e.h, None, dev.ptr, 1, 48, 64, out.ctypes.data) == ERR_STATE       # a refused load leaves nothing behind
        e.load_fid(folded)                                                                                      # the folded layout loads too
        assert e.lib.dpir_fid_features(e.h, None, dev.ptr, 0, 48, 64, out.ctypes.data) == ERR_INVALID
        assert e.lib.dpir_fid_features(e.h, dev.ptr, dev.ptr, 1, 48, 64, out.ctypes.data) == ERR_INVALID
        assert e.lib.dpir_fid_features(e.h, None, None, 1, 48, 64, out.ctypes.data) == ERR_INVALID
        assert same_bits(dgr.fid_features(e, img), dgr.fid_features(engine, img))                              # usable after the refusals
    finally:
        e.close()


def test_the_distance_end_to_end(engine, raw):
    """12 synthetic images against their degraded versions (Gaussian blur + noise, numpy): FID from the engine's features and from the float64
    statement's, on the first 8 feature columns (full-rank covariances) and on all 2048 (rank-deficient, as the paper's 100-image sets are).
    The engine's relative deviation from the float64 FID is at most 4 x the float32 statement's (two sides and the sqrtm)."""
    from scipy import ndimage
    gt = Fd.make_images(64, 64, 12, seed=7, as_u8=False)
    rng = np.random.default_rng(11)
    deg = np.clip(ndimage.gaussian_filter(gt, sigma=(0, 0, 1.5, 1.5)) + rng.standard_normal(gt.shape) * 0.05, 0, 1).astype(np.float32)
    sets = {}
    for name, imgs in (("gt", gt), ("deg", deg)):
        sets[name] = (dgr.fid_features(engine, imgs), Fd.features(raw, imgs)[13], Fd.features(raw, imgs, torch.float32)[13])
    for cols in (8, 2048):
        f_eng, f_64, f_32 = (fd.fid_from_features(sets["deg"][i][:, :cols], sets["gt"][i][:, :cols]) for i in range(3))
        dev_eng, dev_32 = abs(f_eng - f_64) / abs(f_64), abs(f_32 - f_64) / abs(f_64)
        print(f"fid end to end, {cols} columns: float64 {f_64:.9g} engine {f_eng:.9g} (rel {dev_eng:.3e}) float32 statement {f_32:.9g} (rel {dev_32:.3e})")
        assert np.isfinite(f_eng) and f_64 > 0
        assert dev_eng <= 4 * dev_32, (cols, dev_eng, dev_32)


def test_driver_logs_the_fid_of_its_own_outputs(raw, tmp_path, monkeypatch, caplog):
    """--synthetic 4, 2 NFE, calc_FID: true with synthetic weights in pytorch-fid's key layout under <cwd>/model_zoo: the point's FID line is
    fid_from_features of degrade.fid_features on the run's own outputs and ground truth.  Without the file: one WARNING and no FID line."""
    import yaml
    from diffpir_amd import main_ddpir
    cfg = yaml.safe_load(open("configs/engine_example.yaml"))
    cfg.update(iter_num=2, batch_size=2, task="deblur", calc_FID=True, cwd=str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    args = ["--opt", str(p), "--synthetic", "4", "--max-sweeps", "1"]

    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        res = main_ddpir.main(args)
    assert len(res) == 1 and np.isfinite(res[0])
    warns = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and "FID" in r.getMessage()]
    assert len(warns) == 1 and fd.DEFAULT_FILE in warns[0], warns
    assert not [r for r in caplog.records if "FID of (" in r.getMessage()]
    caplog.clear()

    zoo = tmp_path / "model_zoo"
    zoo.mkdir()
    sd = {k: torch.from_numpy(v) for k, v in raw.items()}
    sd["fc.weight"], sd["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.zeros(1008, 2048), torch.tensor(0)
    torch.save(sd, zoo / fd.DEFAULT_FILE)
    seen = []
    real = dgr.fid_features

    def recording(eng, img):
        out = real(eng, img)
        seen.append((img.numpy(), out.copy()))
        return out
    monkeypatch.setattr(dgr, "fid_features", recording)
    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        res = main_ddpir.main(args)
    assert len(res) == 1 and np.isfinite(res[0])
    lines = [r.getMessage() for r in caplog.records]
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and "FID" in r.getMessage()]
    assert len(seen) == 4 and all(u8.dtype == np.uint8 and u8.shape == (2, 256, 256, 3) for u8, _ in seen)    # per batch: ground truth, then outputs
    gt_f = np.concatenate([seen[0][1], seen[2][1]])
    out_f = np.concatenate([seen[1][1], seen[3][1]])
    want = fd.fid_from_features(out_f, gt_f)
    point = [m for m in lines if m.startswith("-----------> FID of (demo_test)")]
    assert len(point) == 1 and re.search(r"sigma: \(\S+\): (\S+)$", point[0]).group(1) == f"{want:.4f}", (point, want)
    assert [m for m in lines if m.startswith("-----------> Average FID of (demo_test)") and m.endswith(f": {want:.4f}")]
    e = diffpir_amd.Engine(0)
    try:
        e.load_fid(raw)
        assert same_bits(real(e, seen[1][0]), seen[1][1])
    finally:
        e.close()
