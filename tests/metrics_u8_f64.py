"""Float64 statement of the 8-bit evaluation protocol that dpir_metrics_u8 (csrc/metrics8.hip) implements, in plain numpy; nothing here calls
the engine or diffpir_amd.  tests/test_metrics_u8_host.py holds it against the live reference functions where they can run and proves that it
notices planted defects; tests/test_gpu_metrics_u8.py holds the kernel to it.

cv2 is not installed, so util.calculate_ssim itself cannot be executed: agreement with it rests on the written definitions of the two cv2
calls it makes and on this text, not on a run of the reference function.
  cv2.getGaussianKernel(11, 1.5)   g[i] = exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10, divided by its sum (float64).
  cv2.filter2D(img, -1, window)    the CORRELATION of every channel plane with the window, anchor at its centre; calculate_ssim keeps only
                                   [5:-5, 5:-5], where every tap lies inside the image, so filter2D's border rule never enters.
The four quantities of one image pair (uint8 [H,W,3] each), after `border` pixels are cropped from all four sides:
  psnr    utils_image.calculate_psnr: mse = mean((a - b)^2) over the three channels in float64, 20 log10(255 / sqrt(mse)), +inf at mse == 0;
  Y byte  utils_image.rgb2ycbcr(uint8, only_y=True): round(dot(rgb, [65.481, 128.553, 24.966]) / 255 + 16), half to even, with the dot
          evaluated as fma(b, 24.966, fma(g, 128.553, r * 65.481)) -- the order that equals numpy's on the 194 byte triplets that are exact
          .5 ties (tie_triplets); off the ties every order gives the same byte;
  psnr_y  the same PSNR on the Y bytes;
  ssim    utils_image.ssim on the whole H x W x 3 array: mu = filter(x), sigma = filter(x^2) - mu^2, sigma12 = filter(xy) - mu1 mu2,
          C1 = (0.01 255)^2, C2 = (0.03 255)^2, map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), and the mean over
          all valid positions of all three channels (calculate_ssim's loop over range(3) appends that same number three times);
  ssim_y  the same on the 2-D Y image.
Two evaluation orders of the filter are given: `window2d` (the 121-tap window at once) and `separable` (rows, then columns); they differ
by rounding only (test_metrics_u8_host.py: <= 1e-11)."""
import functools

import numpy as np

TAPS = 11
HALO = TAPS - 1
COEF = (65.481, 128.553, 24.966)
KINDS = ("noise", "byte", "same", "flat", "ties")
DEFECTS = ("window_not_normalised", "sigma_1p4", "crop_off_by_one", "y_truncated", "float32_moments", "c2_from_0p3", "channel0_only")


# ------------------------------------------------------------------------------------------------------------------ exact fma in numpy
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _round_odd_sum(a, b):
    """a + b rounded to odd: the float64 next to the exact sum whose last mantissa bit is 1 when the sum is inexact."""
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    return np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def fma(a, b, c):
    """Correctly rounded a * b + c for float64 arrays where `a` holds integers of at most 26 bits (here: bytes), by error-free transformations
    (Dekker's product, then Boldo and Melquiond's three-term sum through rounding to odd).  numpy has no fma; the host test holds this one to
    libm's."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    t = b * 134217729.0                         # Veltkamp split of b at 26 bits: a * bh and a * bl are exact
    bh = t - (t - b)
    bl = b - bh
    ph = a * b
    pl = (a * bh - ph) + a * bl                 # ph + pl == a * b exactly
    th, tl = _two_sum(c, pl)
    vh, vl = _two_sum(ph, th)
    return vh + _round_odd_sum(np.ascontiguousarray(vl), np.ascontiguousarray(tl))


def y_byte(rgb_u8, truncate=False):
    """uint8 [...,3] -> uint8 [...]: the Y byte of rgb2ycbcr(only_y=True)."""
    v = np.asarray(rgb_u8).astype(np.float64)
    s = fma(v[..., 2], COEF[2], fma(v[..., 1], COEF[1], v[..., 0] * COEF[0])) / 255.0 + 16.0
    return (np.floor(s) if truncate else np.rint(s)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def tie_triplets():
    """uint8 [194, 3]: the byte triplets whose Y value is an exact .5 tie: (65481 r + 128553 g + 24966 b) mod 255000 == 127500."""
    r, g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    hit = (65481 * r + 128553 * g + 24966 * b) % 255000 == 127500
    out = np.stack([r[hit], g[hit], b[hit]], 1).astype(np.uint8)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------ the statement
def window(sigma=1.5, normalise=True):
    g = np.exp(-((np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2) ** 2) / (2.0 * sigma * sigma))
    return g / g.sum() if normalise else g


def quantise(x_f32):
    """float32 [B,3,H,W] -> uint8 [B,H,W,3], as util.tensor2uint and dpir_finalize do: clamp to [0,1], x 255.0 in float32, round half to even."""
    x = np.asarray(x_f32, np.float32)
    q = np.clip(x, np.float32(0), np.float32(1)) * np.float32(255.0)
    return np.rint(q).astype(np.uint8).transpose(0, 2, 3, 1).copy()


def crop(img, border, off_by_one=False):
    h, w = img.shape[:2]
    lo = border + (1 if off_by_one else 0)
    return img[lo:h - border, lo:w - border]


def psnr(a_u8, b_u8):
    d = a_u8.astype(np.float64) - b_u8.astype(np.float64)
    mse = np.mean(d ** 2)
    return np.inf if mse == 0 else 20.0 * np.log10(255.0 / np.sqrt(mse))


def _filter_window2d(x, g):
    """valid correlation of every plane of x [h,w] or [h,w,c] with outer(g, g), the 121 taps at once"""
    w2 = np.outer(g, g).astype(x.dtype)
    v = np.lib.stride_tricks.sliding_window_view(x, (TAPS, TAPS), axis=(0, 1))
    return np.einsum("...ij,ij->...", v, w2, optimize=False)


def _filter_separable(x, g):
    """the same as a row pass followed by a column pass, each an explicit 11-term sum from tap 0 to tap 10"""
    g = g.astype(x.dtype)
    h, w = x.shape[:2]
    rows = np.zeros((h, w - HALO) + x.shape[2:], x.dtype)
    for k in range(TAPS):
        rows += g[k] * x[:, k:k + w - HALO]
    out = np.zeros((h - HALO, w - HALO) + x.shape[2:], x.dtype)
    for k in range(TAPS):
        out += g[k] * rows[k:k + h - HALO]
    return out


def ssim(a_u8, b_u8, form="separable", dtype=np.float64, sigma=1.5, normalise=True, c2_from=0.03, channel0_only=False):
    """utils_image.ssim on uint8 [h,w] or [h,w,3]; h, w >= 11.  Everything after the bytes is carried out in `dtype`."""
    flt = {"separable": _filter_separable, "window2d": _filter_window2d}[form]
    g = window(sigma, normalise)
    a, b = a_u8.astype(dtype), b_u8.astype(dtype)
    C1, C2 = dtype((0.01 * 255) ** 2), dtype((c2_from * 255) ** 2)
    mu1, mu2 = flt(a, g), flt(b, g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = flt(a ** 2, g) - mu1_sq
    s2 = flt(b ** 2, g) - mu2_sq
    s12 = flt(a * b, g) - mu1_mu2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    if channel0_only and m.ndim == 3:
        m = m[..., 0]
    return float(m.astype(np.float64).mean())


def metrics(est_u8, gt_u8, border=0, form="separable", defect=None):
    """uint8 [B,H,W,3] twice -> float64 [B,4]: psnr, psnr_y, ssim, ssim_y per image.  defect (tests only): one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    kw = {}
    if defect == "window_not_normalised":
        kw["normalise"] = False
    elif defect == "sigma_1p4":
        kw["sigma"] = 1.4
    elif defect == "float32_moments":
        kw["dtype"] = np.float32
    elif defect == "c2_from_0p3":
        kw["c2_from"] = 0.3
    out = np.empty((len(est_u8), 4), np.float64)
    for i, (e, t) in enumerate(zip(np.asarray(est_u8), np.asarray(gt_u8))):
        e, t = crop(e, border, defect == "crop_off_by_one"), crop(t, border, defect == "crop_off_by_one")
        ey, ty = y_byte(e, defect == "y_truncated"), y_byte(t, defect == "y_truncated")
        out[i] = (psnr(e, t), psnr(ey, ty), ssim(e, t, form, channel0_only=defect == "channel0_only", **kw), ssim(ey, ty, form, **kw))
    return out


# ------------------------------------------------------------------------------------------------------------------ test pairs
def make_pair(H, W, B, kind, seed=0):
    """(estimate float32 [B,3,H,W], ground truth uint8 [B,H,W,3]) of one test case; quantise(estimate) are the estimate's bytes.
    'noise'  a smooth random ground truth, estimate = gt/255 + N(0, 0.05^2) with one value per image set to -0.2 and one to 1.3: it leaves
             [0, 1] and is NOT clamped;
    'byte'   estimate = gt/255 with ONE byte per image moved by 2;
    'same'   estimate = gt/255;
    'flat'   ground truth 254 everywhere, estimate 255 everywhere: mu^2 cancels against the filtered square to the last bits;
    'ties'   both images tiled from the 194 tie triplets (the estimate one triplet further along), so every Y byte is a rounding tie."""
    assert kind in KINDS, kind
    gt = np.empty((B, H, W, 3), np.uint8)
    if kind == "flat":
        gt[:] = 254
        return np.ones((B, 3, H, W), np.float32), gt
    if kind == "ties":
        t = tie_triplets()
        idx = (np.arange(H * W).reshape(H, W) * 7)[None] + 13 * np.arange(B)[:, None, None]
        gt[:] = t[idx % len(t)]
        est = t[(idx + 1) % len(t)]
        return (est.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).astype(np.float32), gt
    from scipy import ndimage
    for b in range(B):
        rng = np.random.default_rng([seed, H, W, b])
        img = ndimage.gaussian_filter(rng.standard_normal((3, H, W)), sigma=(0.6, max(H / 32.0, 1.0), max(W / 32.0, 1.0)), mode="wrap")
        img = (img - img.min()) / (img.max() - img.min())
        gt[b] = np.rint(img * 255).astype(np.uint8).transpose(1, 2, 0)
    est = (gt.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).astype(np.float32)
    if kind == "noise":
        rng = np.random.default_rng([seed, H, W, 1000])
        est = (est + rng.standard_normal(est.shape).astype(np.float32) * np.float32(0.05)).astype(np.float32)
        est[:, 0, 0, 0], est[:, 2, H - 1, W - 1] = np.float32(-0.2), np.float32(1.3)      # at every size two values per image lie outside [0, 1]
    elif kind == "byte":
        for b in range(B):
            c, r, q = (1 + b) % 3, H // 2 + b, W // 3
            est[b, c, r, q] += np.float32(2 / 255) if gt[b, r, q, c] <= 253 else -np.float32(2 / 255)
    return est, gt
