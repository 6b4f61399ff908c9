"""Plain-numpy statement of the bytes the reference saves beside its metrics, which dpir_result_panels (csrc/results.hip) and the driver's
kernel picture implement; nothing here calls the engine or imports diffpir_amd.  Slicing, np.repeat for the nearest-neighbour zoom and
assignments in the reference's own order:

  single2uint      utils_image.py:195-197   np.uint8((img.clip(0, 1) * 255.).round()), on the float32 measurement the engine holds
  kernel bytes     main_ddpir_deblur.py:414-415   single2uint(k / np.max(k)), tiled to three channels
  LEH, kernel      main_ddpir_deblur.py:416-421 = main_ddpir_sisr.py:443-451
  LEH, inpainting  main_ddpir_inpainting.py:347
  kernel picture   main_ddpir.py:299, main_ddpir_deblur.py:177   cv2.imwrite(k * 255. * 200): saturate to [0, 255], round half to even

cv2 is not installed where this suite runs.  cv2.resize(..., interpolation=cv2.INTER_NEAREST) at an integer factor f reads source pixel
floor(destination / f), which is np.repeat(f) along both axes; cv2.imwrite converts a float array with saturate_cast<uchar>, rint (half to even)
then a clamp to [0, 255].  Both are stated from their definitions, not from an executed comparison.
"""
import numpy as np


def single2uint(img):
    return np.uint8((img.clip(0, 1) * 255.).round())


def l_bytes(y):
    """y float32 [B,3,h,w] -> uint8 [B,h,w,3]: single2uint of the float32 array, image by image in HWC as the reference holds img_L"""
    assert y.dtype == np.float32
    return np.stack([single2uint(np.transpose(v, (1, 2, 0))) for v in y])


def kernel_bytes(k):
    """k float [kh,kw] -> uint8 [kh,kw]: single2uint(k / np.max(k)) (the grey value of all three channels)"""
    return single2uint(k / np.max(k) * 1.0)


def nearest_zoom(img, f):
    """cv2.resize(img, (f w, f h), interpolation=cv2.INTER_NEAREST) for an integer f: destination (Y, X) reads source (Y // f, X // f)"""
    return np.repeat(np.repeat(img, f, axis=0), f, axis=1)


def leh_kernel(img_L, img_E, img_H, k, sf):
    """main_ddpir_deblur.py:412-421 for one image.  img_L uint8 [h,w,3], img_E / img_H uint8 [H,W,3], k float [kh,kw] or None (no inset)."""
    img_I = nearest_zoom(img_L, sf)
    if k is not None:
        k_v = np.tile(kernel_bytes(k)[..., np.newaxis], [1, 1, 3])
        k_v = nearest_zoom(k_v, 3)
        img_I[:k_v.shape[0], -k_v.shape[1]:, :] = k_v          # 3kh > H or 3kw > W: the slice is clipped and numpy raises ValueError
    img_I[:img_L.shape[0], :img_L.shape[1], :] = img_L
    return np.concatenate([img_I, img_E, img_H], axis=1)


def leh_inpaint(img_L, img_E, img_H):
    """main_ddpir_inpainting.py:347 for one image"""
    return np.concatenate([img_L, img_E, img_H], axis=1)


def panels(y, est, gt, k=None, sf=1, mode="kernel"):
    """(L [B,h,w,3], LEH [B,H,3W,3]) for a batch: y float32 [B,3,h,w], est / gt uint8 [B,H,W,3], k float [B,kh,kw] or None"""
    L = l_bytes(y)
    if mode == "inpaint":
        return L, np.stack([leh_inpaint(L[b], est[b], gt[b]) for b in range(len(L))])
    return L, np.stack([leh_kernel(L[b], est[b], gt[b], None if k is None else k[b], sf) for b in range(len(L))])


def kernel_picture(k):
    """uint8 [kh,kw]: cv2.imwrite of the float array k * 255. * 200, evaluated in float64"""
    return np.rint(np.clip(np.asarray(k, np.float64) * 255. * 200, 0, 255)).astype(np.uint8)


def tie_values(ns=(0, 1, 2, 100, 127, 128, 253, 254)):
    """float32 values at, one ulp below and one ulp above (n + 0.5) / 255 for several n: where clamp, x 255 in float32 and half-to-even meet"""
    c = ((np.asarray(ns, np.float64) + 0.5) / 255.0).astype(np.float32)
    return np.concatenate([np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(2))]).astype(np.float32)
