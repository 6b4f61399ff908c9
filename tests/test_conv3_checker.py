"""CPU: the per-element yardstick of tests/conv3_f64.py is sharp.  The float32 CPU convolution plays the kernel: unmodified it passes at the
adopted R (ratio 1 by construction), and each of a set of defects a 3x3 layer kernel can plausibly have -- a transposed tap index, a wrapped
border row, a stale ragged tile column, swapped 64-channel halves, the wrong resampling of the residual or of the source, a dropped low
operand plane, statistics taken at the wrong point -- is rejected at that R, while the whole-tensor max / max metric at 2e-5 that the
forward tests use lets some of them through."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv3_f64 as cf

R_MAX = max(cf.R["f32"], cf.R["f16x3"])


def _op(shape, seed, mode=0, res_mode=-1, quiet_border=False):
    B, c, cout, H, W = shape
    r = np.random.default_rng(seed)
    Hs, Ws = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
    f = lambda *s: r.standard_normal(s).astype(np.float32)
    op = dict(xa=f(B, c, Hs, Ws), xb=None, w=(0.05 * r.standard_normal((cout, c, 3, 3))).astype(np.float32), bias=f(cout),
              mode=mode, res_mode=res_mode, prologue=0, res=None, scaled=False)
    if res_mode >= 0:
        Hr, Wr = (H // 2, W // 2) if res_mode == 1 else ((2 * H, 2 * W) if res_mode == 2 else (H, W))
        op["res"] = f(B, cout, Hr, Wr)
    return op


def _accepts(ref, got):
    e, _ = cf.E(got, ref.ref, ref.S)
    return e <= R_MAX * max(ref.e32, cf.FLOOR)


def _max_over_max(got, ref):
    return float(np.abs(got - ref.ref.numpy()).max() / np.abs(ref.ref.numpy()).max())


def _conv32(x, w, bias):
    return (F.conv2d(x, w, padding=1) + bias[None, :, None, None])


BASE = (2, 32, 128, 20, 36)       # the ragged 8 x 32 case: tiles end at column 32, row 16


def test_float32_conv_is_accepted_with_ratio_one():
    for mode, res_mode in ((0, -1), (1, 0), (2, 1), (0, 2)):
        op = _op(BASE, 3, mode, res_mode)
        ref = cf.Reference(op)
        m = ref.check(ref.base32, min(cf.R.values()), f"float32 conv mode {mode} res_mode {res_mode}")
        assert m["ratio"] == pytest.approx(1.0) or m["E32"] < cf.FLOOR
        assert 2.0 ** -26 < ref.e32 < 2.0 ** -20        # the baseline itself is an fp32 rounding-level number
    ref16 = cf.Reference(_op(BASE, 3), f16_operands=True)
    ref16.check(ref16.base32, cf.R["f16x1"], "float32 conv of the f16-rounded statement")
    # ... and the rounded statement is another function: the unrounded float32 conv does not pass for it
    assert not _accepts(ref16, cf.Reference(_op(BASE, 3)).base32)


def _faults(op, ref):
    """name -> the float32 'kernel' output with one planted defect"""
    x, w, b = cf.prologued(op, torch.float32), torch.from_numpy(op["w"]), torch.from_numpy(op["bias"])
    good = torch.from_numpy(ref.base32.copy())
    out = {}
    out["taps_transposed"] = _conv32(x, w.transpose(2, 3).contiguous(), b)
    wrap = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="circular"), w) + b[None, :, None, None]
    t = good.clone(); t[:, :, 0, :] = wrap[:, :, 0, :]
    out["top_row_wraps"] = t
    t = good.clone(); t[:, :, :, 32:] = 0.0
    out["ragged_tile_column_stale_zero"] = t
    t = good.clone(); t[:, :, 16:, 32:] = float("nan")
    out["ragged_corner_tile_left_poisoned"] = t
    t = good.clone(); t[:, :64], t[:, 64:] = good[:, 64:], good[:, :64]
    out["co_halves_swapped"] = t
    x16 = x.to(torch.float16).to(torch.float32)
    out["activations_rounded_to_f16"] = _conv32(x16, w, b)
    # a single quiet channel with a wrong border row: what max / max over the tensor excuses
    t = good.clone(); t[0, 5, -1, :] = t[0, 5, -2, :]
    out["one_channel_last_row_repeated"] = t
    return {k: v.numpy() for k, v in out.items()}


def test_planted_faults_are_rejected():
    op = _op(BASE, 5)
    ref = cf.Reference(op)
    faults = _faults(op, ref)
    for name, got in faults.items():
        e, at = cf.E(got, ref.ref, ref.S)
        print(f"{name}: E {e:.3e} at {at}, E(float32) {ref.e32:.3e}, max/max {_max_over_max(np.nan_to_num(got), ref):.3e}")
        assert not _accepts(ref, got), name
    # the dropped low plane must not be a marginal rejection: it sits two orders above the bound (the one fault that max / max at 2e-5 lets
    # through is the quiet-channel one of the next test)
    e, _ = cf.E(faults["activations_rounded_to_f16"], ref.ref, ref.S)
    assert e > 20 * R_MAX * ref.e32


def test_quiet_channel_fault_passes_max_over_max_but_not_the_per_element_metric():
    op = _op(BASE, 7)
    op["w"][5] *= 1e-5
    op["bias"][5] = 0.0
    ref = cf.Reference(op)
    got = ref.base32.copy()
    got[0, 5, 0, :] = 0.0           # a dropped border row in a channel a hundred thousand times quieter than the rest
    assert _max_over_max(got, ref) < 2e-5
    assert not _accepts(ref, got)


def test_wrong_residual_and_source_resampling_are_rejected():
    # nearest-up residual replaced by the top-left quarter of a same-shape read
    op = _op(BASE, 9, 0, 1)
    ref = cf.Reference(op)
    B, _, cout, H, W = BASE
    conv = ref.base32 - cf.residual(op, torch.float32).numpy()
    flat = op["res"].reshape(B, cout, -1)
    wrong = np.zeros((B, cout, H * W), np.float32)
    wrong[:, :, :flat.shape[2]] = flat          # the half-resolution planes read with the output's strides
    assert not _accepts(ref, conv + wrong.reshape(B, cout, H, W))
    assert not _accepts(ref, conv + np.pad(op["res"], ((0, 0), (0, 0), (0, H // 2), (0, W // 2))))
    # 2x2 mean replaced by the top-left pick, for the residual and for the source
    op = _op(BASE, 10, 0, 2)
    ref = cf.Reference(op)
    conv = ref.base32 - cf.residual(op, torch.float32).numpy()
    assert not _accepts(ref, conv + op["res"][:, :, ::2, ::2])
    op = _op(BASE, 11, 2)
    ref = cf.Reference(op)
    picked = dict(op, mode=0, xa=np.ascontiguousarray(op["xa"][:, :, ::2, ::2]))
    assert not _accepts(ref, cf.layer(picked, torch.float32).numpy())
    # the prologue belongs before the 2x2 mean: pooling first and activating afterwards is another function
    t = np.empty((2, 32, 4), np.float32)
    t[..., 0], t[..., 1], t[..., 2], t[..., 3] = 0.1, 1.0, 0.2, 1.0
    op = dict(_op(BASE, 12, 2), prologue=1, prm=t)
    ref = cf.Reference(op)
    pooled_first = dict(op, mode=0, xa=F.avg_pool2d(torch.from_numpy(op["xa"]), 2).numpy())
    assert not _accepts(ref, cf.layer(pooled_first, torch.float32).numpy())
    assert ref.measure(ref.base32)["ratio"] == pytest.approx(1.0)


def test_group_norm_statement_matches_torch():
    r = np.random.default_rng(13)
    x = torch.from_numpy(r.standard_normal((2, 96, 8, 8)))
    g, b = torch.from_numpy(0.5 + r.random(96)), torch.from_numpy(0.2 * r.standard_normal(96))
    film = torch.from_numpy(0.2 * r.standard_normal((2, 192)))
    want = F.silu(F.group_norm(x, 32, g, b, eps=1e-5) * (1 + film[:, :96, None, None]) + film[:, 96:, None, None])
    assert (cf.group_norm_film_silu(x, g, b, film) - want).abs().max() < 1e-13
    assert cf.weight_scale(np.array([0.2], np.float32)) == 4096.0 and cf.weight_scale(np.array([0.25], np.float32)) == 2048.0


def test_statistics_check():
    op = _op(BASE, 14, 0, 0)
    ref = cf.Reference(op)
    out = ref.base32
    v = out.astype(np.float64)
    stat = np.stack([v.sum(axis=(2, 3)), (v * v).sum(axis=(2, 3))], axis=-1)
    cf.check_stats(stat, out, "exact")
    # fp32 partial sums of 256 values folded in fp64: inside the contract
    p = out.reshape(2, 128, -1)[:, :, :512].reshape(2, 128, 2, 256)
    rest = out.reshape(2, 128, -1)[:, :, 512:]
    s1 = p.sum(axis=3, dtype=np.float32).astype(np.float64).sum(axis=2) + rest.astype(np.float64).sum(axis=2)
    cf.check_stats(np.stack([s1, stat[..., 1]], axis=-1), out, "fp32 slots")
    # the sum of squares taken before the residual was added
    before = (v - op["res"].astype(np.float64))
    bad = np.stack([stat[..., 0], (before * before).sum(axis=(2, 3))], axis=-1)
    with pytest.raises(AssertionError):
        cf.check_stats(bad, out, "squares before the residual")
    bad = stat.copy(); bad[1, 77, 0] = np.nan
    with pytest.raises(AssertionError):
        cf.check_stats(bad, out, "poison left in a slot")
