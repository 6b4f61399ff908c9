"""CPU: the float64 statement of the 8-bit metrics (tests/metrics_u8_f64.py) against the live reference functions that can run here
(rgb2ycbcr, calculate_psnr; calculate_ssim needs cv2, which is not installed), its two summation orders against each other, proof that it
notices planted defects, and the driver's calc_SSIM plumbing against a stub engine."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

from diffpir_amd import _lib, main_ddpir as drv
from oracle import ref_import
from tests import metrics_u8_f64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(11, 11, 1, 0), (12, 27, 2, 0), (40, 56, 3, 4), (96, 160, 2, 0)]      # the shapes of tests/test_gpu_metrics_u8.py
SSIM_BOUND, PSNR_BOUND = 1e-9, 1e-10                                            # the GPU test's bounds

_PAIRS = {}


def pair(H, W, B, border, kind):
    """(estimate bytes, ground-truth bytes, border, separable statement [B,4]), computed once and never modified"""
    key = (H, W, B, border, kind)
    if key not in _PAIRS:
        est, gt = M.make_pair(H, W, B, kind)
        eu8 = M.quantise(est)
        ref = M.metrics(eu8, gt, border)
        for a in (eu8, gt, ref):
            a.setflags(write=False)
        _PAIRS[key] = (eu8, gt, border, ref)
    return _PAIRS[key]


ALL = [s + (k,) for s in SHAPES for k in M.KINDS]


# ------------------------------------------------------------------------------------------------------------------ Y and PSNR
def test_the_numpy_fma_is_libm_s():
    libm = ctypes.CDLL("libm.so.6")
    libm.fma.restype, libm.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    g, r = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing="ij")
    inner = r * M.COEF[0]
    got = M.fma(g, M.COEF[1], inner)                                                        # every (g, r) of the inner fma
    assert np.array_equal(got, np.array([libm.fma(a, M.COEF[1], c) for a, c in zip(g.ravel(), inner.ravel())]).reshape(got.shape))
    rng = np.random.default_rng(0)
    t = np.concatenate([M.tie_triplets(), rng.integers(0, 256, (20000, 3)).astype(np.uint8)]).astype(np.float64)
    u = M.fma(t[:, 1], M.COEF[1], t[:, 0] * M.COEF[0])
    assert np.array_equal(M.fma(t[:, 2], M.COEF[2], u), np.array([libm.fma(b, M.COEF[2], c) for b, c in zip(t[:, 2], u)]))


def test_there_are_194_tie_triplets_and_the_y_orders_differ_only_there():
    t = M.tie_triplets().astype(np.int64)
    assert t.shape == (194, 3) and np.all((65481 * t[:, 0] + 128553 * t[:, 1] + 24966 * t[:, 2]) % 255000 == 127500)
    v = M.tie_triplets().astype(np.float64)
    plain = np.rint(((v[:, 0] * M.COEF[0] + v[:, 1] * M.COEF[1]) + v[:, 2] * M.COEF[2]) / 255.0 + 16.0).astype(np.uint8)
    assert 0 < int((plain != M.y_byte(M.tie_triplets())).sum()) < 194                       # left to right without fma misses some of them


@pytest.mark.skipif(not ref_import.available(), reason="reference tree absent")
def test_y_statement_equals_the_reference_s_rgb2ycbcr_on_all_triplets():
    rgb2ycbcr = ref_import.load().utils_image.rgb2ycbcr
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    bad = []
    for r in range(256):
        img = np.stack([np.full_like(g, r), g, b], -1)
        ref = rgb2ycbcr(img.copy(), only_y=True)
        assert ref.dtype == np.uint8 and ref.shape == g.shape
        miss = ref != M.y_byte(img)
        bad.extend(map(tuple, img[miss].astype(np.int64)))
    # another numpy / BLAS may sum the dot in another order: it can only disagree on the exact ties
    assert all((65481 * r + 128553 * g_ + 24966 * b_) % 255000 == 127500 for r, g_, b_ in bad), bad
    print(f"rgb2ycbcr disagreements (all on ties): {len(bad)}")


@pytest.mark.skipif(not ref_import.available(), reason="reference tree absent")
@pytest.mark.parametrize("H,W,B,border,kind", ALL)
def test_psnr_statement_equals_the_live_calculate_psnr(H, W, B, border, kind):
    ui = ref_import.load().utils_image
    eu8, gt, border, ref = pair(H, W, B, border, kind)
    for i in range(B):
        want = ui.calculate_psnr(eu8[i], gt[i], border=border)
        want_y = ui.calculate_psnr(M.y_byte(eu8[i]), M.y_byte(gt[i]), border=border)
        for got, w in ((ref[i, 0], want), (ref[i, 1], want_y)):
            assert (np.isinf(w) and got == w) or abs(got - w) <= 1e-12, (got, w)


def test_quantise_is_tensor2uint():
    x = np.array([-0.2, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.4999, 1.0, 1.3], np.float32).reshape(1, 1, 1, -1).repeat(3, 1)
    want = np.uint8((np.clip(x.astype(np.float32), 0, 1) * np.float32(255.0)).round())       # tensor2uint: clamp_(0, 1), np.uint8((img * 255.0).round())
    assert np.array_equal(M.quantise(x), want.transpose(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------------------------ SSIM
@pytest.mark.parametrize("H,W,B,border,kind", ALL)
def test_the_two_float64_orders_agree(H, W, B, border, kind):
    eu8, gt, border, ref = pair(H, W, B, border, kind)
    other = M.metrics(eu8, gt, border, form="window2d")
    spread = np.abs(other[:, 2:] - ref[:, 2:]).max()
    print(f"{H}x{W} B{B} border {border} {kind}: order spread {spread:.3e}")
    assert spread <= 1e-11
    assert np.array_equal(other[:, :2], ref[:, :2])                                          # PSNR does not depend on the filter
    if kind == "same":
        assert np.all(ref[:, 2:] == 1.0) and np.all(np.isposinf(ref[:, :2]))
    else:
        assert np.all(np.isfinite(ref[:, 0])) and np.all(ref[:, 2] < 1.0) and np.all(ref[:, 3] <= 1.0)      # one moved byte may leave Y as it was


def test_statement_sanity():
    eu8, gt, _, ref = pair(40, 56, 3, 4, "noise")
    assert np.array_equal(M.metrics(eu8[1:2], gt[1:2], 4), ref[1:2])                          # per image
    assert not np.array_equal(M.metrics(eu8, gt, 0), ref)                                     # the border counts
    w = M.window()
    assert abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == 5
    # a pair with constant planes: mu = x exactly up to rounding, sigma = 0 -> ssim = (2 x y + C1) / (x^2 + y^2 + C1)
    eu8, gt, _, ref = pair(12, 27, 2, 0, "flat")
    C1 = (0.01 * 255) ** 2
    assert abs(ref[0, 2] - (2 * 255 * 254 + C1) / (255 ** 2 + 254 ** 2 + C1)) < 1e-12
    assert abs(ref[0, 0] - 20 * np.log10(255.0)) < 1e-12                                       # mse 1


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_a_planted_defect_moves_a_number_by_more_than_the_gpu_bound(defect):
    moved = []
    for H, W, B, border, kind in ALL:
        eu8, gt, border, ref = pair(H, W, B, border, kind)
        if defect == "crop_off_by_one" and min(H, W) - 2 * border < 12:
            continue                                                                           # no valid window would be left
        got = M.metrics(eu8, gt, border, defect=defect)
        with np.errstate(invalid="ignore"):
            d_psnr = np.where(got[:, :2] == ref[:, :2], 0.0, np.abs(got[:, :2] - ref[:, :2]))     # inf == inf: not moved
        d_ssim = np.abs(got[:, 2:] - ref[:, 2:])
        if d_psnr.max() > PSNR_BOUND or d_ssim.max() > SSIM_BOUND:
            moved.append((H, W, B, border, kind, float(np.nan_to_num(d_psnr, posinf=np.inf).max()), float(d_ssim.max())))
    print(defect, moved)
    assert moved, defect


# ------------------------------------------------------------------------------------------------------------------ driver and ABI
def test_border_rule_and_the_key():
    cfg = lambda **kw: drv.Config(dict(dict(task="deblur", sf=1), **kw))         # noqa: E731
    assert drv.ssim_border(cfg()) is None and drv.ssim_border(cfg(calc_SSIM=False)) is None
    assert drv.ssim_border(cfg(calc_SSIM=False, metrics_border=3)) is None
    assert drv.ssim_border(cfg(calc_SSIM=True)) == 0
    assert drv.ssim_border(cfg(calc_SSIM=True, task="sr", sf=4)) == 4
    assert drv.ssim_border(cfg(calc_SSIM=True, task="inpaint", sf=4)) == 0
    assert drv.ssim_border(cfg(calc_SSIM=True, task="sr", sf=4, metrics_border=0)) == 0
    assert drv.ssim_border(cfg(calc_SSIM=True, metrics_border=7)) == 7


def test_only_the_example_config_switches_it_on():
    import glob
    on = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml"))) if drv.ssim_border(drv.parse_config(p)) is not None]
    assert on == ["ssim_example.yaml"]
    assert drv.ssim_border(drv.parse_config(os.path.join(ROOT, "configs", "ssim_example.yaml"))) == 4       # task sr, sf 4


class _Out:
    def __init__(self, n):
        self.n = n


class _StubEngine:
    def empty(self, shape, dtype=np.float32):
        return np.zeros(shape, dtype)


class _StubDist:
    @staticmethod
    def shard_range(n, rank, world):
        return 0, n

    @staticmethod
    def all_gather_results(a, n, rank, world, engine=None):
        return a


def _stub_driver(monkeypatch, calls):
    """dgr.metrics / lpips / metrics_u8 return numbers that name the call and the image: PSNR 30 + i, PSNR-Y 40 + i, LPIPS 0.1 + i / 100 and the
    8-bit columns 20 + i, 25 + i, 0.9 - i / 100, 0.95 - i / 100 for the i-th image a batch holds."""
    monkeypatch.setattr(drv, "make_operators", lambda config, n, i0, H, W: (None, None))
    monkeypatch.setattr(drv.dgr, "degrade", lambda eng, task, gt, **kw: (None, {"gt": None}))
    monkeypatch.setattr(drv.restore, "restore_batch", lambda eng, cfg, y, per_image=None, **kw: _Out(len(per_image.lambda_)))
    i = lambda out: np.arange(out.n, dtype=np.float64)            # noqa: E731

    def metrics(eng, out, gt):
        calls.append("metrics")
        return (30 + i(out)).astype(np.float32), (40 + i(out)).astype(np.float32)

    def lpips(eng, out, gt):
        calls.append("lpips")
        return (0.1 + i(out) / 100).astype(np.float32)

    def metrics_u8(eng, out, gt, border=0):
        calls.append(("metrics_u8", border))
        return 20 + i(out), 25 + i(out), 0.9 - i(out) / 100, 0.95 - i(out) / 100
    monkeypatch.setattr(drv.dgr, "metrics", metrics)
    monkeypatch.setattr(drv.dgr, "lpips", lpips)
    monkeypatch.setattr(drv.dgr, "metrics_u8", metrics_u8)


def _run_sweeps(caplog, with_lpips, border):
    config = drv.parse_config(os.path.join(ROOT, "configs", "engine_example.yaml"))
    config.batch_size = 2
    imgs = np.zeros((3, 16, 16, 3), np.uint8)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        extra = () if border is None else (border,)
        res = drv.run_batched_sweeps(_StubEngine(), config, drv.sweeps(config), imgs, _StubDist, 0, 1, False, {}, with_lpips, *extra)
    return res, [re.sub(r"\[[0-9.]+ images/s", "[N images/s", r.getMessage()) for r in caplog.records]


@pytest.mark.parametrize("with_lpips", [False, True])
def test_driver_columns_and_lines_with_the_key_on_and_off(monkeypatch, caplog, with_lpips):
    calls = []
    _stub_driver(monkeypatch, calls)
    rows = drv.metric_rows(None, _Out(2), None, with_lpips)
    assert rows.shape == (2, 3 if with_lpips else 2) and rows.dtype == np.float64
    assert calls == (["metrics", "lpips"] if with_lpips else ["metrics"])                 # off: dpir_metrics_u8 is never called
    del calls[:]
    on = drv.metric_rows(None, _Out(2), None, with_lpips, 4)
    assert on.shape == (2, rows.shape[1] + 4) and np.array_equal(on[:, :-4], rows)
    assert np.array_equal(on[:, -4:], [[20, 25, 0.9, 0.95], [21, 26, 0.89, 0.94]]) and calls[-1] == ("metrics_u8", 4)

    # the flattened sweep path, three images in batches of two: off is what the parent logs, line for line
    del calls[:]
    res_off, off = _run_sweeps(caplog, with_lpips, None)
    assert not [c for c in calls if isinstance(c, tuple)]
    tail = "; LPIPS: {:.4f}; ave LPIPS: {:.4f}"
    want = ["eta:0, zeta:0.30000000000000004, lambda:7, guidance_scale:1.0",
            "batch   1--> PSNR: 30.5000dB" + (tail.format(0.105, 0.07) if with_lpips else ""),
            "batch   2--> PSNR: 30.0000dB" + (tail.format(0.1, 0.07 + 0.1 / 3) if with_lpips else ""),
            "-----------> Average PSNR(RGB) of (demo_test) scale factor: (1), sigma: (0.050): 30.3333 dB  [N images/s on 1 GPU(s)]",
            "-----------> Average PSNR(Y) of (demo_test) scale factor: (1), sigma: (0.050): 40.3333 dB"]
    if with_lpips:
        want.append("-----------> Average LPIPS of (demo_test) scale factor: (1), sigma: (0.050): 0.1033")
    assert off == want
    res_on, on_lines = _run_sweeps(caplog, with_lpips, 0)
    assert res_on == res_off and ("metrics_u8", 0) in calls
    new = [m for m in on_lines if m not in off]
    assert [m for m in on_lines if m in off] == off                                       # the old lines, in their order
    assert new == ["batch   1--> PSNR(8-bit RGB): 20.5000dB", "batch   1--> PSNR(8-bit Y): 25.5000dB",
                   "batch   1--> SSIM(RGB): 0.8950", "batch   1--> SSIM(Y): 0.9450",
                   "batch   2--> PSNR(8-bit RGB): 20.0000dB", "batch   2--> PSNR(8-bit Y): 25.0000dB",
                   "batch   2--> SSIM(RGB): 0.9000", "batch   2--> SSIM(Y): 0.9500",
                   "-----------> Average PSNR(8-bit RGB) of (demo_test) scale factor: (1), sigma: (0.050): 20.3333 dB",
                   "-----------> Average PSNR(8-bit Y) of (demo_test) scale factor: (1), sigma: (0.050): 25.3333 dB",
                   "-----------> Average SSIM(RGB) of (demo_test) scale factor: (1), sigma: (0.050): 0.8967",
                   "-----------> Average SSIM(Y) of (demo_test) scale factor: (1), sigma: (0.050): 0.9467"]
    assert on_lines.index(new[0]) == on_lines.index(off[1]) + 1 and on_lines[-4:] == new[-4:]


def test_abi_has_the_entry_and_is_still_version_2():
    assert "dpir_metrics_u8" in _lib.SIGNATURES and len(_lib.SIGNATURES["dpir_metrics_u8"][1]) == 9
    hdr = open(os.path.join(ROOT, "include", "diffpir_engine.h")).read()
    decl = re.search(r"\bint dpir_metrics_u8\(([^)]*)\)", hdr)
    assert decl and len(decl.group(1).split(",")) == 9
    assert "#define DPIR_ABI_VERSION 2" in hdr and _lib.ABI_VERSION == 2
    for cite in ("main_ddpir_deblur.py:380", "main_ddpir_inpainting.py:325", "main_ddpir_sisr.py:406", "main_ddpir_sisr.py:459", "utils_image.py:616-661"):
        assert cite in hdr, cite
    lib = _lib.load()
    assert lib.dpir_version() == 2 and hasattr(lib, "dpir_metrics_u8")
    mk = open(os.path.join(ROOT, "diffpir_amd", "csrc", "Makefile")).read()
    assert re.search(r"\$\(OBJDIR\)/metrics8\.o: metrics8\.hip \$\(HDRS\)\n\t@mkdir -p \$\(OBJDIR\)\n\t\$\(HIPCC\) \$\(CXXFLAGS\) -ffp-contract=off ", mk)
