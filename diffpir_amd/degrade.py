"""Degradation synthesis and metrics on the device: the steps either side of the restoration loop.

`degrade` mirrors CustomDataset.__getitem__'s arithmetic (main_ddpir.py:84-114) for a batch of uint8 ground-truth images;
`metrics` mirrors main_ddpir.py:482-517 (PSNR and PSNR on the Y channel), `lpips` main_ddpir.py:489-493; `fid_features` gives the Inception features of the FID column (README.md:119-141); `metrics_u8` is the 8-bit protocol of the standalone programs (calculate_psnr / calculate_ssim on tensor2uint bytes, RGB and Y, main_ddpir_sisr.py:406, 459); `result_panels` gives the bytes of the saved measurement and of the L / E / H strip (main_ddpir.py:508-511, main_ddpir_deblur.py:412-424, main_ddpir_inpainting.py:343-347).  All are thin wrappers over
dpir_degrade / dpir_metrics / dpir_lpips / dpir_fid_features / dpir_metrics_u8 / dpir_result_panels; PSF and mask GENERATION (a few hundred scalar operations per image under the numpy RNG) stays on the host so that
kernels and masks remain bit-identical to the reference's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .engine import Engine, _ptr
from .restore import TASKS


def engine_task(task: str, sr_mode: str = "blur") -> int:
    if task == "sr":
        return TASKS["sr_blur"] if sr_mode == "blur" else TASKS["sr_cubic"]
    return TASKS[task]


def degrade(engine: Engine, task: str, gt_u8, k=None, mask=None, *, noise_level_img: float, sf: int = 1, sr_mode: str = "blur",
            seed: int = 0, image_offset: int = 0, noise=None, out=None):
    """gt_u8: uint8 [B,H,W,3] (numpy or device); k: [B,1,kh,kw] float32; mask: uint8 [B,3,H,W]; noise: optional host-fed
    standard-normal [B,3,H/sf,W/sf] (parity runs).  Returns (y DeviceArray [B,3,H/sf,W/sf] in [0,1], device copies of gt/k/mask)."""
    keep = {}

    def dev(a, dt, name):
        if a is None:
            return None
        if isinstance(a, np.ndarray):
            a = engine.to_device(np.ascontiguousarray(a, dtype=dt))
        keep[name] = a
        return a
    gt_d, k_d, m_d, n_d = dev(gt_u8, np.uint8, "gt"), dev(k, np.float32, "k"), dev(mask, np.uint8, "mask"), dev(noise, np.float32, "noise")
    B, H, W, _ = gt_d.shape
    d = _lib.DegradeDesc()
    d.task, d.B, d.H, d.W, d.sf = engine_task(task, sr_mode), B, H, W, sf
    if k_d is not None:
        d.kh, d.kw = k_d.shape[2], k_d.shape[3]
    d.noise_level_img, d.seed, d.image_offset = float(noise_level_img), seed, image_offset
    if out is None:
        out = engine.empty((B, 3, H // sf, W // sf))
    engine._check(engine.lib.dpir_degrade(engine.h, C.byref(d), _ptr(gt_d), _ptr(k_d), _ptr(m_d), _ptr(n_d), _ptr(out)))
    return out, keep


def metrics(engine: Engine, x0, gt_u8_dev):
    """Per-image (PSNR, PSNR-Y) in dB as float32 arrays; x0: DeviceArray [B,3,H,W] in [0,1]."""
    B, _, H, W = x0.shape
    p = np.empty(B, np.float32)
    py = np.empty(B, np.float32)
    engine._check(engine.lib.dpir_metrics(engine.h, _ptr(x0), _ptr(gt_u8_dev), B, H, W, p.ctypes.data, py.ctypes.data))
    return p, py


def lpips(engine: Engine, x0, gt):
    """Per-image LPIPS (v0.1, net='vgg') of x0*2-1 against the ground truth*2-1 as a float32 array [B] (dpir_lpips; needs
    engine.load_lpips).  x0: float32 [B,3,H,W] in [0,1], un-clamped; gt: uint8 [B,H,W,3] (img_H) or float32 [B,3,H,W] in [0,1];
    DeviceArrays or numpy."""
    if isinstance(x0, np.ndarray):
        x0 = engine.to_device(np.ascontiguousarray(x0, dtype=np.float32))
    if isinstance(gt, np.ndarray):
        gt = engine.to_device(np.ascontiguousarray(gt))
    B, _, H, W = x0.shape
    u8 = np.dtype(gt.dtype) == np.uint8
    if tuple(gt.shape) != ((B, H, W, 3) if u8 else (B, 3, H, W)) or not (u8 or np.dtype(gt.dtype) == np.float32):
        raise ValueError(f"lpips: ground truth {gt.dtype} {tuple(gt.shape)} does not go with x0 {tuple(x0.shape)} (uint8 [B,H,W,3] or float32 [B,3,H,W])")
    out = np.empty(B, np.float32)
    engine._check(engine.lib.dpir_lpips(engine.h, _ptr(x0), _ptr(gt) if u8 else None, None if u8 else _ptr(gt), B, H, W, out.ctypes.data))
    return out


def metrics_u8(engine: Engine, est, gt_u8, border: int = 0):
    """Per-image (PSNR, PSNR-Y, SSIM, SSIM-Y) of the 8-bit result as four float64 arrays [B] (dpir_metrics_u8): util.calculate_psnr and
    util.calculate_ssim on tensor2uint bytes and on their rgb2ycbcr Y byte, `border` pixels cropped from every side first.  est: uint8
    [B,H,W,3] (what dpir_finalize writes) or float32 [B,3,H,W] in [0,1], un-clamped (quantised on the device to the same bytes); gt_u8:
    uint8 [B,H,W,3]; DeviceArrays or numpy."""
    if isinstance(est, np.ndarray):
        est = engine.to_device(np.ascontiguousarray(est))
    if isinstance(gt_u8, np.ndarray):
        gt_u8 = engine.to_device(np.ascontiguousarray(gt_u8))
    if np.dtype(gt_u8.dtype) != np.uint8 or len(tuple(gt_u8.shape)) != 4 or gt_u8.shape[3] != 3:
        raise ValueError(f"metrics_u8: ground truth {gt_u8.dtype} {tuple(gt_u8.shape)} is not uint8 [B,H,W,3]")
    B, H, W, _ = gt_u8.shape
    u8 = np.dtype(est.dtype) == np.uint8
    if tuple(est.shape) != ((B, H, W, 3) if u8 else (B, 3, H, W)) or not (u8 or np.dtype(est.dtype) == np.float32):
        raise ValueError(f"metrics_u8: estimate {est.dtype} {tuple(est.shape)} does not go with the ground truth {tuple(gt_u8.shape)} "
                         "(uint8 [B,H,W,3] or float32 [B,3,H,W])")
    out = np.empty((B, 4), np.float64)
    engine._check(engine.lib.dpir_metrics_u8(engine.h, _ptr(est) if u8 else None, None if u8 else _ptr(est), _ptr(gt_u8), B, H, W, int(border),
                                             out.ctypes.data))
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy()


RESULT_MODES = {"kernel": 0, "inpaint": 1}


def kernel_bytes(k):
    """uint8 [B,kh,kw]: util.single2uint(k / np.max(k)) per image (main_ddpir_deblur.py:414-415, before the tile to three channels); k numpy
    [B,1,kh,kw] or [B,kh,kw]."""
    k = np.asarray(k)
    k = k.reshape((k.shape[0],) + k.shape[-2:])
    return np.stack([np.uint8((np.clip(kk / np.max(kk), 0, 1) * 255.).round()) for kk in k])


def result_panels(engine: Engine, y, est_u8, gt_u8, k=None, sf: int = 1, mode: str = "kernel", want_L: bool = True, want_LEH: bool = True):
    """(L_u8 [B,h,w,3], leh_u8 [B,H,3W,3]) as numpy uint8 (dpir_result_panels): the saved measurement single2uint(y) of the engine's float32 y and
    the reference's L / E / H strip (main_ddpir_deblur.py:412-421 for mode "kernel", main_ddpir_inpainting.py:346-347 for mode "inpaint").  y:
    float32 [B,3,H/sf,W/sf] (what `degrade` returns); est_u8, gt_u8: uint8 [B,H,W,3]; k: HOST numpy PSF [B,1,kh,kw] for the inset (None: no
    inset); DeviceArrays or numpy otherwise.  An output that is not wanted is None and is not computed."""
    if mode not in RESULT_MODES:
        raise ValueError(f"result_panels: mode {mode!r} is not one of {sorted(RESULT_MODES)}")
    if isinstance(y, np.ndarray):
        y = engine.to_device(np.ascontiguousarray(y, dtype=np.float32))
    if isinstance(est_u8, np.ndarray):
        est_u8 = engine.to_device(np.ascontiguousarray(est_u8))
    if isinstance(gt_u8, np.ndarray):
        gt_u8 = engine.to_device(np.ascontiguousarray(gt_u8))
    if np.dtype(gt_u8.dtype) != np.uint8 or len(tuple(gt_u8.shape)) != 4 or gt_u8.shape[3] != 3:
        raise ValueError(f"result_panels: ground truth {gt_u8.dtype} {tuple(gt_u8.shape)} is not uint8 [B,H,W,3]")
    B, H, W, _ = gt_u8.shape
    sf = int(sf)
    if sf < 1 or H % sf or W % sf:
        raise ValueError(f"result_panels: sf {sf} does not divide H {H} and W {W}")
    if np.dtype(est_u8.dtype) != np.uint8 or tuple(est_u8.shape) != (B, H, W, 3):
        raise ValueError(f"result_panels: estimate {est_u8.dtype} {tuple(est_u8.shape)} does not go with the ground truth {tuple(gt_u8.shape)}")
    if np.dtype(y.dtype) != np.float32 or tuple(y.shape) != (B, 3, H // sf, W // sf):
        raise ValueError(f"result_panels: y {y.dtype} {tuple(y.shape)} is not float32 [{B},3,{H // sf},{W // sf}]")
    d = _lib.ResultDesc()
    d.B, d.H, d.W, d.sf, d.mode = B, H, W, sf, RESULT_MODES[mode]
    kv_d = None
    if k is not None and mode == "kernel" and want_LEH:          # the inset belongs to the strip: an L-only call needs no kernel and no 3 kh <= H
        kv = kernel_bytes(k)
        if kv.shape[0] != B:
            raise ValueError(f"result_panels: {kv.shape[0]} kernels for {B} images")
        d.kh, d.kw = kv.shape[1], kv.shape[2]
        kv_d = engine.to_device(kv)
    L_d = engine.empty((B, H // sf, W // sf, 3), np.uint8) if want_L else None
    leh_d = engine.empty((B, H, 3 * W, 3), np.uint8) if want_LEH else None
    engine._check(engine.lib.dpir_result_panels(engine.h, C.byref(d), _ptr(y), _ptr(kv_d), _ptr(est_u8), _ptr(gt_u8), _ptr(L_d), _ptr(leh_d)))
    return (None if L_d is None else L_d.numpy()), (None if leh_d is None else leh_d.numpy())


def fid_features(engine: Engine, img):
    """FID Inception-v3 `pool3` features as a float32 array [B, 2048] (dpir_fid_features; needs engine.load_fid).  img: uint8 [B,H,W,3]
    (what dpir_finalize writes; the ground truth) or float32 [B,3,H,W] in [0,1]; a DeviceArray or numpy."""
    if isinstance(img, np.ndarray):
        img = engine.to_device(np.ascontiguousarray(img))
    u8 = np.dtype(img.dtype) == np.uint8
    shape = tuple(img.shape)
    if len(shape) != 4 or shape[3 if u8 else 1] != 3 or not (u8 or np.dtype(img.dtype) == np.float32):
        raise ValueError(f"fid_features: image {img.dtype} {shape} is neither uint8 [B,H,W,3] nor float32 [B,3,H,W]")
    B, H, W = (shape[0], shape[1], shape[2]) if u8 else (shape[0], shape[2], shape[3])
    out = np.empty((B, 2048), np.float32)
    engine._check(engine.lib.dpir_fid_features(engine.h, _ptr(img) if u8 else None, None if u8 else _ptr(img), B, H, W, out.ctypes.data))
    return out
