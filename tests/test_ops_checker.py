"""The checker of tests/ops_f64.py can fail (CPU): every defect below is planted in a copy of the float64 statement, evaluated at the shapes of
tests/test_gpu_ops_float64.py, rounded to float32 as a kernel would deliver it, and must be rejected -- by ops_f64.check for the resampling
family and the metrics bound, by array_equal for the bit-exact entries.  The same defect is also run at the single shape the suite tested
before (with that test's tolerance against the fp32 oracle / its fixture), and the table printed by test_planted_defects says which defects the
old shape would have let through.  Four planted changes are no defects of the value at all and are reported as such instead of asserted (the
test asserts that the checker sees NO difference, so the claim itself is checked): the np.int16 wrap of the Resizer's field of view (no effect
below 32 768), the order of the two separable Resizer passes (R_H and R_W commute; only the fp32 rounding differs), the renormalisation of the
Resizer weights (at an integer sf the antialiased cubic already sums to 1 to 2e-16), and a clamp to [0, 255] after the * 255 instead of
[0, 1] before it (the same float32 value for every input).  Consequence: these tests do NOT pin the order of the two Resizer passes -- a kernel
that resampled W before H would be held to the K o_p rounding bound like any other, not to the reference's order."""
import numpy as np
import torch

from oracle import diffpir_oracle as do
from tests import ops_f64 as F

f32 = np.float32
NEW_RESAMPLE = [(48, 80, 2, 3), (24, 36, 3, 1), (96, 40, 4, 5), (16, 128, 8, 2), (30, 50, 5, 1), (6, 9, 3, 1)]      # (H, W, sf, B)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32))


# ------------------------------------------------------------------------------------------------------------------ defective Resizer tables
def contrib(in_len, out_len, scale, boundary="mirror", renorm=True, int16=True, centre_len=None):
    """utils_resizer.py:104-167 restated with switches: returns (w [out, taps], mirrored / clamped idx, raw field of view)."""
    cl = in_len if centre_len is None else centre_len
    kw = 4.0 / scale
    outc = np.arange(1, out_len + 1)
    match = (outc - (out_len - cl * scale) / 2) / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(match - kw / 2)
    fov = left[:, None] + np.arange(int(np.ceil(kw)) + 2) - 1
    fov = np.int16(fov).astype(np.int64) if int16 else fov.astype(np.int64)
    w = scale * do._cubic(scale * (match[:, None] - fov - 1))
    if renorm:
        sw = w.sum(axis=1)
        sw[sw == 0] = 1.0
        w = w / sw[:, None]
    if boundary == "mirror":
        m = np.mod(fov, 2 * cl)
        idx = np.where(m < cl, m, 2 * cl - 1 - m)
    else:
        idx = fov
    return w, np.clip(idx, 0, in_len - 1), fov


def down_with(x, sf, **kw):
    H, W = x.shape[-2:]
    swap = kw.pop("swap_passes", False)
    same_table = kw.pop("h_table_for_both", False)
    th = contrib(H, H // sf, 1.0 / sf, **kw)[:2]
    tw = contrib(W, W // sf, 1.0 / sf, centre_len=H if same_table else None, **kw)[:2]
    if swap:
        return F.gather_axis(F.gather_axis(x, *tw, axis=-1), *th, axis=-2)
    return F.gather_axis(F.gather_axis(x, *th, axis=-2), *tw, axis=-1)


def dense(in_len, sf, drop_mirrored=False, narrow=False):
    """R [out, in] of one axis by scattering the tables; drop_mirrored: contributions whose un-mirrored position lies outside the signal are
    lost; narrow: every input loses the first output of its window."""
    w, idx, fov = contrib(in_len, in_len // sf, 1.0 / sf)
    R = np.zeros((in_len // sf, in_len))
    keep = ((fov >= 0) & (fov < in_len)) if drop_mirrored else np.ones(w.shape, bool)
    np.add.at(R, (np.repeat(np.arange(w.shape[0]), w.shape[1]), idx.ravel()), (w * keep).ravel())
    if narrow:
        for i in range(in_len):
            nz = np.nonzero(R[:, i])[0]
            if nz.size:
                R[nz[0], i] = 0.0
    return R


def down_T_with(g, sf, **kw):
    h, w = g.shape[-2:]
    return np.einsum("oi,...op,pj->...ij", dense(h * sf, sf, **kw), np.asarray(g, np.float64), dense(w * sf, sf, **kw))


def ibp_with(x0, y, rho, gamma, sf, in_iter, mode):
    x0 = np.asarray(x0, np.float64)
    H, W = x0.shape[-2:]
    h, w = H // sf, W // sf
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    li = ((yy // sf) * h + xx // sf) % (h * w) if mode == "h_for_w" else (yy % h) * w + xx % w
    for _ in range(in_iter):
        z = x0 / 2 + 0.5
        d = (np.asarray(y, np.float64) - F.resize_down(z, sf)).reshape(x0.shape[:-2] + (h * w,))
        x0 = (z + gamma * d[..., li] / (1 + rho)) * 2 - 1
    return x0


# ------------------------------------------------------------------------------------------------------------------ the families
def resample_inputs(case, seed=0):
    H, W, sf, B = case
    rng = np.random.default_rng(seed)
    return rng.random((B, 3, H, W)).astype(f32), rng.random((B, 3, H // sf, W // sf)).astype(f32)


def resizer_family():
    def run(defect, case):
        x, _ = resample_inputs(case)
        sf = case[2]
        return defect(x, sf).astype(f32), F.resize_down(x, sf), do.resizer_apply(t32(x), 1.0 / sf).numpy()
    defects = {
        "Resizer: boundary clamped instead of mirrored": lambda x, sf: down_with(x, sf, boundary="clamp"),
        "Resizer: W pass before H pass [no defect of the value: the passes commute]": lambda x, sf: down_with(x, sf, swap_passes=True),
        "Resizer: H table for both axes": lambda x, sf: down_with(x, sf, h_table_for_both=True),
        "Resizer: weights not renormalised [no effect at integer sf: the antialiased cubic sums to 1 at spacing 1 / sf to 2e-16]": lambda x, sf: down_with(x, sf, renorm=False),
        "Resizer: np.int16 wrap ignored [no effect below 32 768]": lambda x, sf: down_with(x, sf, int16=False),
    }
    return defects, run, F.resize_down, [(64, 64, 4, 2), (256, 256, 4, 1)], 2e-6          # test_resizer_down_and_bicubic_up


def transpose_family():
    def run(defect, case):
        _, v = resample_inputs(case)
        sf = case[2]
        xr = torch.zeros((case[3], 3, case[0], case[1]), requires_grad=True)
        o32 = torch.autograd.grad((do.resizer_apply(xr, 1.0 / sf) * t32(v)).sum(), xr)[0].numpy()
        return defect(v, sf).astype(f32), F.resize_down_T(v, sf), o32
    defects = {
        "Resizer^T: mirrored contributions dropped at the borders": lambda v, sf: down_T_with(v, sf, drop_mirrored=True),
        "Resizer^T: output window narrowed by one": lambda v, sf: down_T_with(v, sf, narrow=True),
    }
    return defects, run, F.resize_down_T, [], None          # no direct test before: reached only through whole DPS loops


def ibp_family():
    def run(defect, case):
        x, y = resample_inputs(case)
        x0, sf = (x * 2 - 1).astype(f32), case[2]
        o32 = do.prox_ibp(t32(x0), t32(y), torch.tensor(0.37), sf, 0.5, 2).numpy()
        return defect(x0, y, sf).astype(f32), F.prox_ibp(x0, y, float(f32(0.37)), 0.5, sf, 2), o32
    defects = {
        "IBP: xx / sf indexed with h instead of w": lambda x0, y, sf: ibp_with(x0, y, float(f32(0.37)), 0.5, sf, 2, "h_for_w"),
        "IBP: nearest-up taken as yy % h": lambda x0, y, sf: ibp_with(x0, y, float(f32(0.37)), 0.5, sf, 2, "modulo"),
    }
    return defects, run, lambda x0, y, sf: F.prox_ibp(x0, y, float(f32(0.37)), 0.5, sf, 2), [(64, 64, 4, 2)], 3e-6          # test_ibp_prox


def bicubic_family():
    def run(defect, case):
        _, y = resample_inputs(case)
        sf = case[2]
        o32 = torch.nn.functional.interpolate(t32(y), scale_factor=sf, mode="bicubic", align_corners=False).numpy()
        return defect(y, sf).astype(f32), F.bicubic_up(y, sf), o32

    def both(y, sf, **kw):
        return F.bicubic_axis(F.bicubic_axis(y, sf, -1, **kw), sf, -2, **kw)
    defects = {
        "bicubic up: half-pixel offset omitted": lambda y, sf: both(y, sf, half_pixel=False),
        "bicubic up: border clamp to h instead of h - 1": lambda y, sf: both(y, sf, clamp_to=y.shape[-1]) if y.shape[-1] == y.shape[-2] else
        F.bicubic_axis(F.bicubic_axis(y, sf, -1, clamp_to=y.shape[-1]), sf, -2, clamp_to=y.shape[-2]),
        "bicubic up: A = -0.5": lambda y, sf: both(y, sf, A=-0.5),
    }
    return defects, run, F.bicubic_up, [(64, 64, 4, 2)], 2e-6          # test_resizer_down_and_bicubic_up (16^2 -> 64^2)


def test_float64_blur_statement_equals_scipy():
    """ops_f64.blur_wrap_acc against scipy.ndimage.convolve(mode='wrap') for odd, even, 1 x 1 and image-sized PSFs (scipy is imported by the CPU
    suite only): the float64 sums agree to 1e-10 and the quantised images are identical."""
    from scipy import ndimage
    rng = np.random.default_rng(3)
    for H, W, kh, kw in ((12, 16, 1, 1), (40, 56, 4, 6), (40, 56, 7, 3), (40, 56, 25, 25), (12, 16, 12, 16), (9, 7, 4, 6)):
        gt = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
        k = rng.random((kh, kw))
        k = (k / k.sum()).astype(f32)
        acc = F.blur_wrap_acc(gt, k[None])[0]
        assert np.abs(acc - ndimage.convolve(gt[0].astype(np.float64), k.astype(np.float64)[..., None], mode="wrap")).max() <= 1e-10
        assert np.array_equal(F.blur_wrap_u8(gt, k[None])[0], (ndimage.convolve(gt[0], k[..., None], mode="wrap") / 255.0).astype(f32).transpose(2, 0, 1))


def test_planted_defects(golden):
    rows = []

    def record(name, rejected_new, where, old_passes, null=False):
        rows.append((name, rejected_new, where, old_passes, null))

    # ---- resampling families through ops_f64.check
    for family in (resizer_family, transpose_family, ibp_family, bicubic_family):
        defects, run, statement, old_cases, old_atol = family()          # statement: the clean float64 statement, same arguments as a defect
        for name, defect in defects.items():
            rejected = [c for c in NEW_RESAMPLE if not F.ok(*run(defect, c))]
            old = None
            if old_cases:
                old = True
                for c in old_cases:
                    out, _, o32 = run(defect, c)
                    old = old and bool(np.abs(out - o32).max() <= old_atol)
            record(name, bool(rejected), rejected, old, "[no " in name)
        # the statement itself passes its own checker at every new shape
        for c in NEW_RESAMPLE:
            out, f64, o32 = run(statement, c)
            assert F.ok(out, f64, o32), (family.__name__, c)

    # ---- finalize: bit equality with ops_f64.finalize_f32
    rng = np.random.default_rng(1)

    def fin_probe(shape):
        x = (rng.random(shape).astype(f32) * f32(2.4) - f32(1.2)).astype(f32)
        k = np.arange(x.size // 2) % 255
        x.reshape(-1)[::2] = ((k + 0.5) / 255.0).astype(f32) * f32(2) - f32(1)
        return x

    def fin(x, mode):
        v = x / f32(2) + f32(0.5)
        if mode == "strides":
            return np.rint(np.clip(v, 0, 1) * f32(255)).astype(np.uint8).reshape(x.shape[0], x.shape[2], x.shape[3], 3)
        if mode == "trunc":
            return (np.clip(v, 0, 1) * f32(255)).astype(np.uint8).transpose(0, 2, 3, 1)
        return np.rint(np.clip(v * f32(255), f32(0), f32(255))).astype(np.uint8).transpose(0, 2, 3, 1)
    g = golden("operators")
    old_x = (g["u8_in"] * 2 - 1).astype(f32)
    for name, mode in (("finalize: NCHW / NHWC strides swapped", "strides"), ("finalize: truncation instead of round-half-even", "trunc"),
                       ("finalize: clamp applied after the * 255 [no defect of the value: same float32 for every input]", "late")):
        rejected = [s for s in ((1, 3, 6, 9), (3, 3, 48, 80), (2, 3, 16, 128)) if not np.array_equal(fin(x := fin_probe(s), mode), F.finalize_f32(x)[1])]
        record(name, bool(rejected), rejected, bool(np.array_equal(fin(old_x, mode), F.finalize_f32(old_x)[1])), "[no " in name)

    # ---- blur: the quantised image must equal ops_f64.blur_wrap_u8
    def blur(gt, k, mode):
        B, (kh, kw) = gt.shape[0], k.shape[-2:]
        acc = np.zeros(gt.shape)
        cy, cx = ((kh - 1) // 2, (kw - 1) // 2) if mode == "centre" else (kh // 2, kw // 2)
        for b in range(B):
            for i in range(kh):
                for j in range(kw):
                    kv = k[b, kh - 1 - i, kw - 1 - j] if mode == "noflip" else k[b, i, j]
                    acc[b] += np.float64(kv) * np.roll(gt[b].astype(np.float64), (i - cy, j - cx), axis=(0, 1))
        q = np.rint(acc) if mode == "round" else np.trunc(acc)
        return F.noise_finish_f32((np.clip(q, 0, 255) / 255.0).astype(f32).transpose(0, 3, 1, 2), None, 0.0)
    d = golden("degrade")
    for name, mode in (("blur: kernel not flipped", "noflip"), ("blur: centre (kh - 1) / 2 instead of kh / 2", "centre"),
                       ("blur: rounding instead of truncation", "round")):
        rejected = []
        for H, W, kh, kw in ((12, 16, 1, 1), (40, 56, 4, 6), (40, 56, 7, 3), (12, 16, 12, 16)):
            gt = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
            gt[0] = 200
            k = rng.random((2, kh, kw))
            k = (k / k.sum(axis=(1, 2), keepdims=True)).astype(f32)
            if not np.array_equal(blur(gt, k, mode), F.degrade_deblur(gt, k)):
                rejected.append((H, W, kh, kw))
        old = bool(np.array_equal(blur(d["gt"], d["k"][:, 0], mode), d["deblur_y_sigma0"]))
        record(name, bool(rejected), rejected, old)
    assert np.array_equal(F.degrade_deblur(d["gt"], d["k"][:, 0]), d["deblur_y_sigma0"])          # the statement reproduces the reference's fixture

    # ---- metrics: 2e-5 dB against ops_f64.psnr
    for name, kw in (("metrics: Y mean over H W instead of 3 H W", dict(mean_over="hw")), ("metrics: Y from channels in BGR order", dict(order=(2, 1, 0)))):
        rejected = []
        for B, H, W in ((1, 7, 9), (5, 7, 9), (5, 64, 64)):
            gt = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
            x0 = (F.u8_to_single(gt) + f32(0.05) * rng.standard_normal((B, 3, H, W)).astype(f32)).astype(f32)
            bad = F.psnr(x0, gt, y_only=True, **{k2: (H * W if v == "hw" else v) for k2, v in kw.items()})
            if np.abs(bad - F.psnr(x0, gt, y_only=True)).max() > 2e-5:
                rejected.append((B, H, W))
        H, W = d["gt"].shape[1:3]
        bad = F.psnr(d["x0"], d["gt"], y_only=True, **{k2: (H * W if v == "hw" else v) for k2, v in kw.items()})
        record(name, bool(rejected), rejected, bool(np.abs(bad - d["psnr_y"]).max() <= 2e-5))
    assert np.abs(F.psnr(d["x0"], d["gt"]) - d["psnr"]).max() <= 2e-5 and np.abs(F.psnr(d["x0"], d["gt"], y_only=True) - d["psnr_y"]).max() <= 2e-5

    print("\nplanted defect | rejected at the new shapes | passes at the shape the suite used before")
    for name, rej, where, old, null in rows:
        print(f"{name} | {'yes' if rej else 'NO'} {where if rej else ''} | {'no direct test before' if old is None else ('PASSES (unseen before)' if old else 'fails')}")
    for name, rej, where, old, null in rows:
        if null:
            assert not rej, f"{name}: documented as having no effect on the value, but the checker saw one"
        else:
            assert rej, f"{name}: not rejected at any new shape"


def test_checker_on_planes_where_the_fp32_oracle_is_exact():
    """o_p = 0 (flat, zero or exactly representable planes) with the floor at 0: an exact kernel passes (no 0 / 0), one float32 rounding fails."""
    f64 = np.zeros((1, 3, 4, 4))
    f64[0, 1] = 0.5
    f64[0, 2] = np.arange(16).reshape(4, 4)
    o32 = f64.astype(f32)
    assert F.ok(f64.astype(f32), f64, o32, K=8.0, F=0.0)
    bad = f64.astype(f32)
    bad[0, 1, 2, 2] = np.nextafter(f32(0.5), f32(1))
    assert not F.ok(bad, f64, o32, K=8.0, F=0.0) and F.stats(bad, f64, o32, K=8.0, F=0.0)["e_zero"] > 0
