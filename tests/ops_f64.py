"""Float64 statements of the non-FFT data steps and the loop arithmetic (csrc/elem.hip, csrc/degrade.hip and the elementwise / resampling
tail of csrc/grad.hip), and the one checker the -m gpu tests of tests/test_gpu_ops_float64.py hold the kernels to.  Plain vectorised numpy;
nothing here calls the engine or its Python mirrors.  tests/test_ops_checker.py proves on the CPU that the checker rejects planted defects.

Two kinds of statement:
  * resampling family (Resizer down, its transpose, torch bicubic up, the IBP update, || m - R(x) || and its gradient, sr degradation): float64,
    compared through `check` below;
  * expression mirrors (`*_f32`: masked prox, repaint mix, re-noise, eps / score from x0, ewise, finalize, u8 -> single, the noise finish): the
    kernel's expression evaluated in numpy float32 (float64 where the kernel says double), one rounding per operation -- the kernels are built
    with contraction off, so the expectation is bit equality.  Their float64 counterparts (same name without the suffix) are what
    the oracle's float64 mode is compared with.

The checker follows tests/prox_f64.py, plane by plane: e_p = max |out - f64| / max |f64| over plane p, o_p the same for the fp32 oracle
(oracle/diffpir_oracle.py on float32 tensors), and a kernel passes when e_p <= max(K_RATIO o_p, FLOOR) on every plane.

K_RATIO and FLOOR, measured on the MI355X at the first green run (82 checks of tests/test_gpu_ops_float64.py, every plane):
  worst e_p / o_p per entry: resize_down 4.29 (16 x 128, sf 8, B 2; 2.24 at 256^2 sf 4, <= 1.9 elsewhere), bicubic_up 2.44 (24 x 36, sf 3),
  degrade-sr 1.95, band_resample_T 1.83, prox_ibp 1.76, grad_and_value 1.44 (1.35 with a DPS_yt measurement); the bound was used to 54 % at most.
  K = min(8, 2 * 4.29) = 8, the cap (the factor of prox_f64.py).
  No plane of any check had o_p = 0, so the worst zero-oracle-error e_p is 0 and FLOOR = 2 * 0 = 0: the bound is K o_p alone
  (a plane with e_p = 0 passes whatever its bound; e_p > 0 where o_p = 0 fails: tests/test_ops_checker.py).
  (A numpy float32 emulation of the kernels' tap order had predicted 4.29 / 2.44 / 1.76 for Resizer / bicubic / IBP.)
Every expression-mirroring entry (prox_mask, repaint_mix, renoise, eps_from_xstart eps and score, ewise, finalize, the quantised blur, both
noise-finish paths) was bit-equal to its numpy float32 statement on the device at every shape, the 25.2 M-element tensors included.
dpir_metrics was NOT within 2e-5 dB of float64 at first: 1.7e-4 dB on PSNR-Y (B 5, 7 x 9, 87.5 dB) from the float32 roundings of * 2 - 1;
csrc/degrade.hip now forms the differences in float64 (worst 3.8e-6 dB after).  See DESIGN.md section 4.
The 268 M-element cap of elem.hip's grid1d (65535 * 16 workgroups of 256) is not reachable at a sensible test size (> 1 GB per tensor); the
grid-stride branch is exercised through launch_ewise's own 65 536-workgroup cap instead (32 x 3 x 512 x 512 elements)."""
import numpy as np

from oracle.diffpir_oracle import resizer_contributions
from tests.prox_f64 import plane_errs, worst

K_RATIO = 8.0
FLOOR = 0.0


# ------------------------------------------------------------------------------------------------------------------ checker
def stats(out, f64, o32, K=None, F=None):
    """Per-plane statistics of `out` against the float64 statement with the fp32 oracle as yardstick ([B, C, H, W] arrays).  ratio: worst
    e_p / o_p over the planes with o_p > 0; e_zero: worst e_p over the planes with o_p == 0; margin: worst e_p / bound_p (<= 1 passes)."""
    K = K_RATIO if K is None else K
    F = FLOOR if F is None else F
    e, o = plane_errs(out, f64), plane_errs(o32, f64)
    pos = o > 0
    ratio = float((e[pos] / o[pos]).max()) if pos.any() else 0.0
    e_zero = float(e[~pos].max()) if (~pos).any() else 0.0
    em, at = worst(e)
    bound = np.maximum(K * o, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(e == 0, 0.0, e / bound)          # an exact plane passes whatever its bound; e_p > 0 over a zero bound is inf
    return dict(e=em, at=at, o=float(o[at]), o_max=float(o.max()), ratio=ratio, e_zero=e_zero, margin=worst(margin)[0])


def ok(out, f64, o32, K=None, F=None):
    return stats(out, f64, o32, K, F)["margin"] <= 1.0


def check(out, f64, o32, label, K=None, F=None):
    """Asserts e_p <= max(K o_p, F) on every plane; prints and returns the statistics."""
    s = stats(out, f64, o32, K, F)
    msg = (f"ops_f64 {label}: worst plane {s['at']} e_p {s['e']:.3e} (fp32 oracle there {s['o']:.3e}, its worst {s['o_max']:.3e}); worst e_p/o_p "
           f"{s['ratio']:.3f}; worst e_p where o_p = 0: {s['e_zero']:.3e}; bound used to {100 * s['margin']:.0f}%")
    print(msg)
    assert s["margin"] <= 1.0, msg
    return s


def as4(a):
    """[...] -> [B, C, H, W] view for the plane-wise checker (a [B, H, W] or [H, W] array gets unit axes in front)."""
    a = np.asarray(a)
    return a.reshape((1,) * (4 - a.ndim) + a.shape) if a.ndim < 4 else a


# ------------------------------------------------------------------------------------------------------------------ Resizer
def tables(in_len, sf):
    """(weights [out, taps] float64, indices [out, taps]) of the cubic antialiased Resizer at scale 1 / sf (utils_resizer.py:104-167)."""
    w, idx = resizer_contributions(in_len, in_len // sf, 1.0 / sf)
    return np.asarray(w, np.float64), np.asarray(idx, np.int64)


def gather_axis(x, w, idx, axis):
    """out[.., o, ..] = sum_t w[o, t] x[.., idx[o, t], ..] along `axis`."""
    x = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    out = np.zeros(x.shape[:-1] + (w.shape[0],))
    for t in range(w.shape[1]):
        out += x[..., idx[:, t]] * w[:, t]
    return np.moveaxis(out, -1, axis)


def scatter_axis(g, w, idx, in_len, axis):
    """The transpose of gather_axis as an explicit scatter: gin[.., idx[o, t], ..] += w[o, t] g[.., o, ..]."""
    g = np.moveaxis(np.asarray(g, np.float64), axis, -1)
    out = np.zeros(g.shape[:-1] + (in_len,))
    for o in range(w.shape[0]):
        for t in range(w.shape[1]):
            out[..., idx[o, t]] += w[o, t] * g[..., o]
    return np.moveaxis(out, -1, axis)


def resize_down(x, sf):
    """Resizer(1 / sf) of [..., H, W]: dim -2 (H) is resampled before dim -1 (W)."""
    H, W = x.shape[-2:]
    return gather_axis(gather_axis(x, *tables(H, sf), axis=-2), *tables(W, sf), axis=-1)


def resize_down_T(g, sf):
    """Resizer(1 / sf)^T of [..., h, w] -> [..., h sf, w sf]."""
    h, w = g.shape[-2:]
    return scatter_axis(scatter_axis(g, *tables(w * sf, sf), in_len=w * sf, axis=-1), *tables(h * sf, sf), in_len=h * sf, axis=-2)


def grad_and_value(x, m, sf):
    """(d || m - R(x) ||_2 / dx, the norm) with the norm over the whole batch (utils_model.py:390-394)."""
    diff = np.asarray(m, np.float64) - resize_down(x, sf)
    norm = np.sqrt((diff ** 2).sum())
    return -resize_down_T(diff, sf) / norm, norm


# ------------------------------------------------------------------------------------------------------------------ bicubic up, IBP
def cubic_weights(t, A=-0.75):
    """The four cubic-convolution weights at fractional offset t (taps at -1, 0, 1, 2)."""
    def near(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def far(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], axis=-1)


def bicubic_axis(y, sf, axis, A=-0.75, half_pixel=True, clamp_to=None):
    y = np.moveaxis(np.asarray(y, np.float64), axis, -1)
    n = y.shape[-1]
    o = np.arange(n * sf, dtype=np.float64)
    src = (o + 0.5) / sf - 0.5 if half_pixel else o / sf
    i0 = np.floor(src)
    cw = cubic_weights(src - i0, A)
    hi = n - 1 if clamp_to is None else clamp_to
    out = np.zeros(y.shape[:-1] + (n * sf,))
    for a in range(4):
        ii = np.clip(i0.astype(np.int64) - 1 + a, 0, hi)
        out += np.take(y, np.minimum(ii, n - 1), axis=-1) * cw[:, a] * (ii <= n - 1)
    return np.moveaxis(out, -1, axis)


def bicubic_up(y, sf):
    """F.interpolate(mode='bicubic', align_corners=False) by an integer factor: A = -0.75, half-pixel centres, indices clamped to the border."""
    return bicubic_axis(bicubic_axis(y, sf, -1), sf, -2)


def nearest_up(d, sf):
    return np.repeat(np.repeat(d, sf, axis=-2), sf, axis=-1)


def prox_ibp(x0, y, rho, gamma, sf, in_iter):
    """main_ddpir.py:401-406 with F.interpolate's default (nearest) up-sampler."""
    x0 = np.asarray(x0, np.float64)
    for _ in range(in_iter):
        z = x0 / 2 + 0.5
        z = z + gamma * nearest_up(np.asarray(y, np.float64) - resize_down(z, sf), sf) / (1 + rho)
        x0 = z * 2 - 1
    return x0


# ------------------------------------------------------------------------------------------------------------------ elementwise (float64)
def prox_mask(x0, y, m, tau, g):
    x0, y, m = (np.asarray(v, np.float64) for v in (x0, y, m))
    return x0 + g * ((m * (2 * y - 1) + tau * x0) / (m + tau) - x0)


def repaint_mix(x, y, m, n, sa, s1m):
    x, y, m, n = (np.asarray(v, np.float64) for v in (x, y, m, n))
    return (sa * (2 * y - 1) + s1m * n) * m + (1 - m) * x


def renoise(x, x0, st, n1, n2):
    """x = sa_p x0 + k1 (q eps + es n1) + k2 n2, eps = (x - sa_t x0) / s1m_t, with the float32 coefficients of a schedule.build_steps dict."""
    x, x0, n2 = (np.asarray(v, np.float64) for v in (x, x0, n2))
    c = {k: float(np.float32(st[k])) for k in ("sa_t", "s1m_t", "sa_p", "k1", "q", "es", "k2")}
    inner = c["q"] * ((x - c["sa_t"] * x0) / c["s1m_t"])
    if c["es"] != 0.0:
        inner = inner + c["es"] * np.asarray(n1, np.float64)
    return c["sa_p"] * x0 + c["k1"] * inner + c["k2"] * n2


def eps_from_xstart(x, x0, sa, s1m, score):
    v = (np.asarray(x, np.float64) - sa * np.asarray(x0, np.float64)) / s1m
    return -v / s1m if score else v


# ------------------------------------------------------------------------------------------------------------------ expression mirrors (float32)
f32 = np.float32


def prox_mask_f32(x0, y, m, tau, g):
    m, tau, g = m.astype(f32), f32(tau), f32(g)
    num = m * (f32(2) * y - f32(1)) + tau * x0
    return x0 + g * (num / (m + tau) - x0)


def repaint_mix_f32(x, y, m, n, sa, s1m):
    m = m.astype(f32)
    known = f32(sa) * (f32(2) * y - f32(1)) + f32(s1m) * n
    return known * m + (f32(1) - m) * x


def renoise_f32(x, x0, st, n1, n2):
    c = {k: f32(st[k]) for k in ("sa_t", "s1m_t", "sa_p", "k1", "q", "es", "k2")}
    inner = c["q"] * ((x - c["sa_t"] * x0) / c["s1m_t"])
    if c["es"] != 0:
        inner = inner + c["es"] * n1
    return (c["sa_p"] * x0 + c["k1"] * inner) + c["k2"] * n2


def eps_from_xstart_f32(x, x0, sa, s1m, score):
    v = (x - f32(sa) * x0) / f32(s1m)
    return -v / f32(s1m) if score else v


def ewise_f32(op, a, b):
    b = f32(b) if np.ndim(b) == 0 else b
    with np.errstate(all="ignore"):
        return [lambda: a + b, lambda: a - b, lambda: a * b, lambda: a / b, lambda: b - a, lambda: b / a][op]().astype(f32)


def finalize_f32(x):
    """(x / 2 + .5 [B, 3, H, W] float32, uint8 [B, H, W, 3]): clamp to [0, 1], * 255, round half to even (utils_image.py:238-242)."""
    v = x / f32(2) + f32(0.5)
    q = np.rint(np.clip(v, f32(0), f32(1)) * f32(255))
    return v, q.astype(np.uint8).transpose(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------------------ degradation, metrics
def blur_wrap_acc(gt, k):
    """Float64 sum of scipy.ndimage.convolve(gt, k[..., None], mode='wrap') before its cast: gt uint8 [B, H, W, 3], k [B, kh, kw].
    out[y, x] = sum_{i, j} k[i, j] gt[(y + kh // 2 - i) mod H, (x + kw // 2 - j) mod W], accumulated with i outer and j inner."""
    B, (kh, kw) = gt.shape[0], k.shape[-2:]
    acc = np.zeros(gt.shape, np.float64)
    g = gt.astype(np.float64)
    for b in range(B):
        for i in range(kh):
            for j in range(kw):
                acc[b] += np.float64(k[b, i, j]) * np.roll(g[b], (i - kh // 2, j - kw // 2), axis=(0, 1))
    return acc


def blur_wrap_u8(gt, k):
    """The blurred image as the float32 NCHW tensor y: C truncation of the float64 sum to uint8, then util.uint2single."""
    q = np.clip(np.trunc(blur_wrap_acc(gt, k)), 0, 255)
    return (q / 255.0).astype(f32).transpose(0, 3, 1, 2)


def u8_to_single(gt, mask=None):
    v = gt.astype(np.float64).transpose(0, 3, 1, 2)
    if mask is not None:
        v = v * mask.astype(np.float64)
    return (v / 255.0).astype(f32)


def noise_finish_f32(y, noise, level):
    """img_L = img_L * 2 - 1; img_L += normal (float64, in place on the float32 array); img_L / 2 + 0.5   (main_ddpir.py:112-114).  level: the
    float32 noise_level_img the engine receives."""
    v = y * f32(2) - f32(1)
    if noise is not None and level != 0:
        v = (v.astype(np.float64) + noise.astype(np.float64) * (np.float64(f32(level)) * 2.0)).astype(f32)
    return v / f32(2) + f32(0.5)


def degrade_deblur(gt, k, noise=None, level=0.0):
    """dpir_degrade for deblurring: the quantised blur, then the noise finish -- which runs at level 0 too, and whose * 2 - 1, / 2 + .5 round
    trip in float32 moves values below 0.25 by one ulp (the reference's img_L * 2 - 1 ... / 2 + 0.5 does the same)."""
    return noise_finish_f32(blur_wrap_u8(gt, k), noise, level)


def noise_finish_inpaint(gt, mask, noise, level):
    """The inpainting image: float64 gt * mask / 255, noise added in float64, rounded once, then times the mask in float32 (main_ddpir.py:108-114, 311-313)."""
    v = gt.astype(np.float64).transpose(0, 3, 1, 2) * mask.astype(np.float64) / 255.0
    v = v * 2.0 - 1.0
    if noise is not None and level != 0:
        v = v + noise.astype(np.float64) * (np.float64(f32(level)) * 2.0)
    return (v / 2.0 + 0.5).astype(f32) * mask.astype(f32)


def psnr(x0, gt, y_only=False, mean_over=None, order=(0, 1, 2)):
    """Per-image PSNR (max_pixel 2, eps 1e-10) of the float32 image x0 [B, 3, H, W] against uint2single(gt) (float32, as the reference holds
    it), all arithmetic in float64; y_only: on the Y channel of rgb2ycbcr_batch, whose two zero channels stay part of the mean (3 H W)."""
    a = np.asarray(x0, f32).astype(np.float64) * 2 - 1
    b = (gt.transpose(0, 3, 1, 2).astype(f32) / f32(255)).astype(np.float64) * 2 - 1
    n = a[0].size if mean_over is None else mean_over
    if y_only:
        cw = (0.299, 0.587, 0.114)
        a = sum(cw[i] * a[:, order[i]] for i in range(3))
        b = sum(cw[i] * b[:, order[i]] for i in range(3))
    mse = ((a - b) ** 2).reshape(a.shape[0], -1).sum(axis=1) / n
    with np.errstate(divide="ignore"):
        return np.where(mse == 0, np.inf, 20 * np.log10(2.0 / np.sqrt(mse + 1e-10)))
