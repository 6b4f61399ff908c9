"""Float64 statement of the FID Inception-v3 `pool3` features as pytorch-fid defines them, the same statement in float32 as the yardstick,
and the checker the -m gpu tests of tests/test_gpu_fid.py hold csrc/fid.hip to.  Plain torch on the CPU; nothing here calls the engine or reads
`diffpir_amd.fid.inception_spec`: the network below is written out block by block on its own, so that the table in diffpir_amd/fid.py and
the one in csrc/fid.hip are both checked against a second statement.

The definition (neither `pytorch-fid` nor `torchvision` is installed, so this text is the specification):
  entry     v = u8 / 255 (float32 division) or a float32 image in [0,1]; bilinear resize to 299 x 299 (align_corners=False, no antialias);
            then 2 v - 1.
  BasicConv convolution without bias -> BatchNorm in eval mode, eps = 1e-3 -> ReLU.  The statement applies the BatchNorm explicitly on the
            UNFOLDED weights ((x - mean) / sqrt(var + eps) * gamma + beta), so the host's fold is under test too.
  network   stem, Mixed_5b/5c/5d (A), Mixed_6a (B), Mixed_6b..6e (C), Mixed_7a (D), Mixed_7b/7c (E); avg-pools 3x3 s1 p1 with
            count_include_pad=False; Mixed_7c's pool branch is a MAX-pool 3x3 s1 p1; the features are the mean over the 8 x 8 positions.
It returns 14 taps: the stem after each of its two max-pools, the 11 Mixed outputs, and the [B, 2048] features.

Checker, per tap plane as tests/lpips_f64.py: e_p = max |engine - f64| / max |f64| is held to K_RATIO * o_p, o_p the float32 statement's own
error raised to the tap's typical one (plane_yardstick, restated here).  K_RATIO is measured, not chosen: K = min(8, 2 x the worst e_p / o_p seen
on the MI355X over the four entry cases of tests/test_gpu_fid.py); profiles/fid/README.md has the table.
"""
import numpy as np
import torch
import torch.nn.functional as F

K_RATIO = 3.68       # min(8, 2 x 1.84), 1.84 the worst e_p / o_p measured (Mixed_7a, 256 x 256 B 2); see profiles/fid/README.md
BN_EPS = 1e-3
TAP_NAMES = ("pool1", "pool2", "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b",
             "Mixed_7c", "features")


def make_images(H, W, B, seed=0, as_u8=True):
    """Smooth random images (Gaussian-filtered noise stretched to [0,1]) plus N(0, 0.03^2) noise, clipped: uint8 [B,H,W,3] or float32 [B,3,H,W]."""
    from scipy import ndimage
    out = np.empty((B, 3, H, W), np.float32)
    for b in range(B):
        rng = np.random.default_rng([seed, H, W, b])
        img = ndimage.gaussian_filter(rng.standard_normal((3, H, W)), sigma=(0.6, H / 24.0, W / 24.0), mode="wrap")
        img = (img - img.min()) / (img.max() - img.min())
        out[b] = np.clip(img + rng.standard_normal((3, H, W)) * 0.03, 0, 1)
    if as_u8:
        return np.ascontiguousarray(np.rint(out * 255).astype(np.uint8).transpose(0, 2, 3, 1))
    return out


def u8_single(u8):
    """uint8 [B,H,W,3] -> float32 [B,3,H,W] = u8 / 255 (one float32 division)."""
    return np.ascontiguousarray((np.asarray(u8).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).astype(np.float32))


def features(raw, img, dtype=torch.float64):
    """The 14 taps (numpy arrays of `dtype`) for img float32 [B,3,H,W] in [0,1].  raw: pytorch-fid's key layout (<layer>.conv.weight, <layer>.bn.*).
    The input is the float32 image; every operation after it is carried out in `dtype`."""
    def T(key):
        return torch.from_numpy(np.asarray(raw[key])).to(dtype)

    def bc(x, name, stride=1, padding=0):
        x = F.conv2d(x, T(f"{name}.conv.weight"), None, stride=stride, padding=padding)
        g, b, m, v = (T(f"{name}.bn.{leaf}").view(1, -1, 1, 1) for leaf in ("weight", "bias", "running_mean", "running_var"))
        return torch.relu((x - m) / torch.sqrt(v + BN_EPS) * g + b)

    def avg(x):
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)

    def block_a(x, n):
        b1 = bc(x, f"{n}.branch1x1")
        b5 = bc(bc(x, f"{n}.branch5x5_1"), f"{n}.branch5x5_2", padding=2)
        b3 = bc(bc(bc(x, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1), f"{n}.branch3x3dbl_3", padding=1)
        return torch.cat([b1, b5, b3, bc(avg(x), f"{n}.branch_pool")], 1)

    def block_b(x, n):
        b3 = bc(x, f"{n}.branch3x3", stride=2)
        bd = bc(bc(bc(x, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1), f"{n}.branch3x3dbl_3", stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def block_c(x, n):
        b1 = bc(x, f"{n}.branch1x1")
        b7 = bc(bc(bc(x, f"{n}.branch7x7_1"), f"{n}.branch7x7_2", padding=(0, 3)), f"{n}.branch7x7_3", padding=(3, 0))
        bd = bc(x, f"{n}.branch7x7dbl_1")
        for i, p in ((2, (3, 0)), (3, (0, 3)), (4, (3, 0)), (5, (0, 3))):
            bd = bc(bd, f"{n}.branch7x7dbl_{i}", padding=p)
        return torch.cat([b1, b7, bd, bc(avg(x), f"{n}.branch_pool")], 1)

    def block_d(x, n):
        b3 = bc(bc(x, f"{n}.branch3x3_1"), f"{n}.branch3x3_2", stride=2)
        b7 = bc(bc(bc(x, f"{n}.branch7x7x3_1"), f"{n}.branch7x7x3_2", padding=(0, 3)), f"{n}.branch7x7x3_3", padding=(3, 0))
        b7 = bc(b7, f"{n}.branch7x7x3_4", stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def block_e(x, n, pool):
        b1 = bc(x, f"{n}.branch1x1")
        b3 = bc(x, f"{n}.branch3x3_1")
        b3 = torch.cat([bc(b3, f"{n}.branch3x3_2a", padding=(0, 1)), bc(b3, f"{n}.branch3x3_2b", padding=(1, 0))], 1)
        bd = bc(bc(x, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1)
        bd = torch.cat([bc(bd, f"{n}.branch3x3dbl_3a", padding=(0, 1)), bc(bd, f"{n}.branch3x3dbl_3b", padding=(1, 0))], 1)
        return torch.cat([b1, b3, bd, bc(pool(x), f"{n}.branch_pool")], 1)

    x = torch.from_numpy(np.array(img, np.float32)).to(dtype)           # a copy: the callers' arrays are read-only
    x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    x = 2 * x - 1
    taps = []
    x = bc(x, "Conv2d_1a_3x3", stride=2)
    x = bc(x, "Conv2d_2a_3x3")
    x = bc(x, "Conv2d_2b_3x3", padding=1)
    x = F.max_pool2d(x, 3, 2); taps.append(x)
    x = bc(x, "Conv2d_3b_1x1")
    x = bc(x, "Conv2d_4a_3x3")
    x = F.max_pool2d(x, 3, 2); taps.append(x)
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = block_a(x, n); taps.append(x)
    x = block_b(x, "Mixed_6a"); taps.append(x)
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = block_c(x, n); taps.append(x)
    x = block_d(x, "Mixed_7a"); taps.append(x)
    x = block_e(x, "Mixed_7b", avg); taps.append(x)
    x = block_e(x, "Mixed_7c", lambda t: F.max_pool2d(t, 3, 1, 1)); taps.append(x)
    taps.append(x.mean(dim=(2, 3)))
    return [t.numpy() for t in taps]


# ------------------------------------------------------------------------------------------------------------------ checker
def plane_errs(out, ref):
    """[B, C]: max |out - ref| over a plane / max |ref| over it; 0 where both are all zero, inf where only ref is.  A 2-D tap [B, C] (the
    features) is B planes of C values."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    if ref.ndim == 2:
        out, ref = out[:, None, :], ref[:, None, :]
    n, c = ref.shape[:2]
    d = np.abs(out - ref).reshape(n, c, -1).max(axis=2)
    m = np.abs(ref).reshape(n, c, -1).max(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / m)


def plane_yardstick(o32, f64):
    """o_p of the float32 statement, [B, C], with the luck of small planes taken out (as tests/lpips_f64.py states it): every plane of a tap has
    been through the same arithmetic on terms of the same magnitude, so float32 costs every plane of an image about the same ABSOLUTE error, and
    o_p is one sample of it over the plane's own maximum.  Planes of 64 values now and then land within 1e-12 of float64 by luck; no
    implementation can follow such a sample.  So o_p is raised to (median over the image's live planes of the float32 statement's absolute
    plane error) / (the plane's maximum).  A plane whose own o_p is larger keeps it; planes dead in float64 keep o_p = 0 (only an exact 0 passes)."""
    o32, f64 = np.asarray(o32, np.float64), np.asarray(f64, np.float64)
    if f64.ndim == 2:
        o32, f64 = o32[:, None, :], f64[:, None, :]
    o = plane_errs(o32, f64)
    n_img, n_ch = o.shape
    pmax = np.abs(f64).reshape(n_img, n_ch, -1).max(axis=2)
    a32 = np.abs(o32 - f64).reshape(n_img, n_ch, -1).max(axis=2)
    live = pmax > 0
    med = np.array([np.median(a32[n][live[n]]) if live[n].any() else 0.0 for n in range(n_img)])
    with np.errstate(divide="ignore", invalid="ignore"):
        floor = np.where(live, med[:, None] / pmax, 0.0)
    return np.maximum(o, floor)


def tap_stats(out, f64, o32, K=None):
    """ratio = worst e_p / o_p over planes with o_p > 0; e_zero = worst e_p where o_p == 0; margin = worst e_p / (K o_p) (<= 1 passes; an exact
    plane passes whatever its bound)."""
    K = K_RATIO if K is None else K
    if np.shape(out) != np.shape(f64):
        inf = float("inf")
        return dict(e=inf, ratio=inf, e_zero=inf, margin=inf)
    e, o = plane_errs(out, f64), plane_yardstick(o32, f64)
    pos = o > 0
    ratio = float((e[pos] / o[pos]).max()) if pos.any() else 0.0
    e_zero = float(e[~pos].max()) if (~pos).any() else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(e == 0, 0.0, e / (K * o))
    return dict(e=float(e.max()), ratio=ratio, e_zero=e_zero, margin=float(margin.max()))


def check(taps, ref64, ref32, label, K=None):
    """Prints every tap's figures, then asserts e_p <= K o_p on every plane of the 14 taps; returns the per-tap statistics."""
    st = [tap_stats(t, a, b, K) for t, a, b in zip(taps, ref64, ref32)]
    msg = f"fid_f64 {label}: worst e_p/o_p per tap " + " ".join(f"{n}={s['ratio']:.2f}" for n, s in zip(TAP_NAMES, st)) + \
          f"; worst {max(s['ratio'] for s in st):.3f}; worst e_p where o_p = 0: {max(s['e_zero'] for s in st):.3e}; bound used to " \
          f"{100 * max(s['margin'] for s in st):.0f}%"
    print(msg)
    assert len(taps) == len(ref64) == 14 and all(s["margin"] <= 1.0 for s in st), msg
    return st
