"""Float64 statement of LPIPS v0.1, net='vgg' (eval, normalize=False, spatial=False), the same statement in float32 as the yardstick, and the
checker the -m gpu tests of tests/test_gpu_lpips.py hold csrc/lpips.hip to.  Plain torch on the CPU; nothing here calls the engine or
diffpir_amd.  tests/test_lpips_host.py proves on the CPU that the checker rejects planted defects.

The definition (neither `lpips` nor `torchvision` is installed, so this text is the specification):
  in0 = x0*2-1 (x0 un-clamped), in1 = gt*2-1 with gt = img_H/255 (float32 division, util.uint2single);
  scaling layer (v - shift_c) / scale_c, shift (-.030, -.088, -.188), scale (.458, .448, .450), BEFORE the first convolution's zero padding;
  trunk 64,64,M,128,128,M,256,256,256,M,512,512,512,M,512,512,512: conv 3x3 pad 1 + bias + ReLU, M = max-pool 2x2 stride 2 (floor);
  taps behind the ReLU of convolutions 2, 4, 7, 10, 13; per tap n = f / (sqrt(sum_c f^2) + 1e-10), d = sum_c w_c (n0 - n1)^2, spatial mean;
  the score is the sum of the five means.

The checker follows tests/ops_f64.py, plane by plane of every tap: e_p = max |out - f64| / max |f64| over plane p, o_p the same for the
float32 statement (raised to the tap's typical float32 error where it fell below it by luck: plane_yardstick), and the engine passes when
e_p <= max(K_RATIO o_p, FLOOR) on every plane.  The score: its relative error against float64
is at most max(K_RATIO x the float32 statement's, SCORE_FLOOR), and at most SCORE_CAP = 1e-4 in every case (the log prints four decimals of
a value below ~1).

K_RATIO, FLOOR and SCORE_FLOOR, measured on the MI355X at the first green run (the eight pair x shape cases of tests/test_gpu_lpips.py, every plane of
every tap; profiles/lpips/README.md has the table):
  worst e_p / o_p per tap (o_p from plane_yardstick): relu1_2 1.86, relu2_2 2.02, relu3_3 2.34, relu4_3 2.72, relu5_3 4.41 (16 x 16, one value per
  plane; <= 2.91 at every larger size).  K = min(8, 2 x 4.41) = 8, the cap; the bound was used to 55 % at most.
  No live plane had o_p = 0 and every plane that is dead in float64 was exactly 0 on the device: FLOOR = 2 x 0 = 0.
  Score, relative to float64: noisy pairs <= 1.45e-7 (the float32 statement 1.4e-9 ... 6.2e-8), one-pixel pairs 2.9e-6 ... 3.47e-5 (the float32
  statement 2.2e-6 ... 3.94e-5).  SCORE_FLOOR = 2 x 3.47e-5 = 6.94e-5, under the 1e-4 cap.
  Before the trunk ran its convolutions in 16-channel slabs (csrc/lpips.hip) the same cases gave e_p / o_p up to 72 at relu5_3 and one-pixel
  scores up to 1.26e-4 from float64: the fp32 MFMA kernel's one-accumulator sum over Cin x 9 products, which the slabs cut to 144.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.prox_f64 import plane_errs, worst

K_RATIO = 8.0
FLOOR = 0.0
SCORE_FLOOR = 6.94e-5
SCORE_CAP = 1e-4

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
PLAN = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
TAPS = (2, 4, 7, 10, 13)


def gt_single(gt_u8):
    """uint8 [B,H,W,3] -> float32 [B,3,H,W] = img_H / 255 (util.uint2single: one float32 division)."""
    return (np.asarray(gt_u8).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).astype(np.float32)


def make_pair(H, W, B, kind, seed=0):
    """(x0 float32 [B,3,H,W], gt uint8 [B,H,W,3]) of one test case.  The ground truth is a smooth random image (Gaussian-filtered noise, stretched
    to [0, 255]); kind 'noise': x0 = gt/255 + N(0, 0.05^2), which leaves [0, 1] and is NOT clamped; 'pixel': gt/255 with ONE value per image moved
    by 2/255; 'same': gt/255 itself."""
    from scipy import ndimage
    gt_u8 = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        rng = np.random.default_rng([seed, H, W, b])
        img = ndimage.gaussian_filter(rng.standard_normal((3, H, W)), sigma=(0.6, H / 32.0, W / 32.0), mode="wrap")
        img = (img - img.min()) / (img.max() - img.min())
        gt_u8[b] = np.rint(img * 255).astype(np.uint8).transpose(1, 2, 0)
    x0 = gt_single(gt_u8)
    if kind == "noise":
        rng = np.random.default_rng([seed, H, W, 1000])
        x0 = (x0 + rng.standard_normal(x0.shape).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    elif kind == "pixel":
        for b in range(B):
            x0[b, (1 + b) % 3, H // 2 + b, W // 3] += np.float32(2 / 255)
    else:
        assert kind == "same", kind
    return x0, gt_u8


def lpips(sd, x0, gt, dtype=torch.float64, defect=None):
    """(score [B], [five taps, each [2B,C,h,w]: estimate rows then ground-truth rows]) as numpy arrays of `dtype`.
    sd: canonical keys (features.N.weight / .bias, lin{k}.weight [C]); x0, gt: float32 [B,3,H,W] in [0,1]-ish.  The inputs are the float32
    images; every operation after them is carried out in `dtype`.
    defect (tests only): 'pool_ceil', 'tap_before_relu', 'eps_inside_sqrt', 'shift_sign', 'expanded_head'."""
    B = x0.shape[0]
    v = torch.cat([torch.from_numpy(np.ascontiguousarray(x0, np.float32)), torch.from_numpy(np.ascontiguousarray(gt, np.float32))], 0).to(dtype)
    v = v * 2 - 1
    sign = -1.0 if defect == "shift_sign" else 1.0
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(dtype).view(1, 3, 1, 1) * sign
    scale = torch.tensor(SCALE, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    v = (v - shift) / scale
    taps, conv_no, convs = [], 0, iter(FEATURE_INDEX)
    for c in PLAN:
        if c == "M":
            v = F.max_pool2d(v, 2, 2, ceil_mode=(defect == "pool_ceil"))
            continue
        i = next(convs)
        conv_no += 1
        pre = F.conv2d(v, torch.from_numpy(sd[f"features.{i}.weight"]).to(dtype), torch.from_numpy(sd[f"features.{i}.bias"]).to(dtype), padding=1)
        v = torch.relu(pre)
        if conv_no in TAPS:
            taps.append(pre if defect == "tap_before_relu" else v)
    score = torch.zeros(B, dtype=dtype)
    for k, f in enumerate(taps):
        w = torch.from_numpy(sd[f"lin{k}.weight"]).to(dtype).view(1, -1, 1, 1)
        f0, f1 = f[:B], f[B:]
        if defect == "expanded_head":
            # sum w a^2 - 2 sum w a b + sum w b^2 on the normalised values: three large sums whose difference is the score
            n0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
            n1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
            d = (w * n0 * n0).sum(1) - 2 * (w * n0 * n1).sum(1) + (w * n1 * n1).sum(1)
        else:
            if defect == "eps_inside_sqrt":
                n0 = f0 / torch.sqrt((f0 * f0).sum(1, keepdim=True) + 1e-10)
                n1 = f1 / torch.sqrt((f1 * f1).sum(1, keepdim=True) + 1e-10)
            else:
                n0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
                n1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
            d = (w * (n0 - n1) ** 2).sum(1)
        score = score + d.reshape(B, -1).mean(1)
    return score.numpy(), [t.numpy() for t in taps]


# ------------------------------------------------------------------------------------------------------------------ checker
def plane_yardstick(o32, f64):
    """o_p of the float32 statement, [2B, C], with the luck of small planes taken out.  Every plane of a tap has been through the same
    arithmetic on terms of the same magnitude, so float32 costs every plane of an image about the same ABSOLUTE error; o_p, that error over
    the plane's own maximum, is one sample of it.  Deep taps have few pixels per plane (at 16 x 16 relu5_3 is ONE value per plane and
    relu3_3 sixteen), and there a float32 value now and then rounds to within 1e-12 of the float64 one (measured: o_p 2e-11 beside a median
    of 5e-7), also on a plane whose maximum barely clears its ReLU, where any other summation order is 1e-2 away in relative terms.  No
    implementation can follow such a sample.  So o_p is raised to (median over the image's live planes of the float32 statement's absolute
    plane error) / (the plane's maximum): the tap's typical float32 error, at this plane's conditioning.  A plane whose own o_p is larger
    keeps it.  Planes that are dead in float64 keep o_p = 0: there only an exact 0 passes."""
    o32, f64 = np.asarray(o32), np.asarray(f64)
    o = plane_errs(o32, f64)
    n_img, n_ch = o.shape
    pmax = np.abs(f64).reshape(n_img, n_ch, -1).max(axis=2)
    a32 = np.abs(o32.astype(np.float64) - f64).reshape(n_img, n_ch, -1).max(axis=2)
    live = pmax > 0
    med = np.array([np.median(a32[n][live[n]]) if live[n].any() else 0.0 for n in range(n_img)])
    with np.errstate(divide="ignore", invalid="ignore"):
        floor = np.where(live, med[:, None] / pmax, 0.0)
    return np.maximum(o, floor)


def tap_stats(out, f64, o32, K=None, F_=None):
    """Per-plane statistics of one tap [2B,C,h,w] (tests/ops_f64.py stats) with o_p from plane_yardstick: ratio = worst e_p / o_p over the planes
    with o_p > 0, e_zero = worst e_p where o_p == 0, margin = worst e_p / max(K o_p, F) (<= 1 passes; an exact plane passes whatever its bound)."""
    K = K_RATIO if K is None else K
    F_ = FLOOR if F_ is None else F_
    if np.shape(out) != np.shape(f64):               # e.g. a ceil-mode pool: a tap of another size fails outright
        inf = float("inf")
        return dict(e=inf, at=(0, 0), o=0.0, o_max=0.0, ratio=inf, e_zero=inf, margin=inf)
    e, o = plane_errs(out, f64), plane_yardstick(o32, f64)
    pos = o > 0
    ratio = float((e[pos] / o[pos]).max()) if pos.any() else 0.0
    e_zero = float(e[~pos].max()) if (~pos).any() else 0.0
    em, at = worst(e)
    bound = np.maximum(K * o, F_)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(e == 0, 0.0, e / bound)
    return dict(e=em, at=at, o=float(o[at]), o_max=float(o.max()), ratio=ratio, e_zero=e_zero, margin=worst(margin)[0])


def score_rel(score, s64):
    """Per-image relative error of a score against float64; 0 where both are exactly 0, inf where only the float64 one is."""
    score, s64 = np.asarray(score, np.float64), np.asarray(s64, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(score == s64, 0.0, np.abs(score - s64) / np.abs(s64))


def score_bound(s32, s64, K=None, F_=None):
    K = K_RATIO if K is None else K
    F_ = SCORE_FLOOR if F_ is None else F_
    return np.minimum(np.maximum(K * score_rel(s32, s64), F_), SCORE_CAP)


def stats(score, taps, ref64, ref32, K=None, F_=None, SF=None):
    """ref64 / ref32: (score, taps) of the float64 / float32 statement.  margin <= 1 and score_margin <= 1 pass."""
    per_tap = [tap_stats(t, t64, t32, K, F_) for t, t64, t32 in zip(taps, ref64[1], ref32[1])]
    rel, bound = score_rel(score, ref64[0]), score_bound(ref32[0], ref64[0], K, SF)
    with np.errstate(divide="ignore", invalid="ignore"):
        sm = np.where(rel == 0, 0.0, rel / bound)
    return dict(taps=per_tap, margin=max(s["margin"] for s in per_tap), ratio=max(s["ratio"] for s in per_tap),
                e_zero=max(s["e_zero"] for s in per_tap), score_rel=float(rel.max()), score_rel32=float(score_rel(ref32[0], ref64[0]).max()),
                score_margin=float(sm.max()))


def ok(score, taps, ref64, ref32, K=None, F_=None, SF=None):
    s = stats(score, taps, ref64, ref32, K, F_, SF)
    return s["margin"] <= 1.0 and s["score_margin"] <= 1.0


def check(score, taps, ref64, ref32, label, K=None, F_=None, SF=None):
    """Asserts e_p <= max(K o_p, F) on every plane of every tap and the score bound; prints and returns the statistics."""
    s = stats(score, taps, ref64, ref32, K, F_, SF)
    msg = (f"lpips_f64 {label}: taps worst e_p/o_p {s['ratio']:.3f} (per tap " + " ".join(f"{t['ratio']:.2f}" for t in s["taps"]) +
           f"), worst e_p where o_p = 0: {s['e_zero']:.3e}, bound used to {100 * s['margin']:.0f}%; score rel err {s['score_rel']:.3e} "
           f"(float32 statement {s['score_rel32']:.3e}), bound used to {100 * s['score_margin']:.0f}%")
    print(msg)
    assert s["margin"] <= 1.0 and s["score_margin"] <= 1.0, msg
    return s
