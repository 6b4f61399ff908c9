"""-m gpu: the UNet input gradient (generate_mode 'DPS_y0': csrc/unet_bwd.hip, csrc/grad.hip, the dgrads on conv7 / conv6 / conv5 and, in f32
mode, conv2 / conv) at the batches bench.py --full times it at (FFHQ topology, 256^2, B = 8 and 16), at partial tiles (B = 3, 5), under a
magnitude spread across the batch, and in all three precisions -- against torch.autograd through the oracle network in FLOAT64 (an fp32
checker's own error is of the order of the 1e-4 bound).

The network is independent per image (GroupNorm statistics and gout are per image), so the engine runs the whole batch while the float64
checker runs a few probe images one at a time: every image comes from one stream keyed by its index (_image), its probe is evaluated once
per session and shared by every case it appears in (gpu_common._ORACLE_CACHE).  Errors are per image, max|a_n - b_n| / max|b_n|
(gpu_common.per_image_err): the batch-wide rel_err cannot see an image whose gradient is much smaller than another's."""
import numpy as np
import pytest
import torch

import diffpir_amd
from diffpir_amd import restore, synth
from oracle import unet_oracle as uo, diffpir_oracle as do
from tests import gpu_common
from tests.gpu_common import make_model, seeded_noise_fn_np, per_image_err

pytestmark = pytest.mark.gpu
TOL_FWD = 2e-5          # the forward output of the unet_vjp call (tests/test_gpu_dps.py)
TOL_GRAD = 1e-4         # the input gradient and every block's gradient (tests/test_gpu_dps.py TOL_GRAD)
HP = uo.ffhq_hp()
SIZE = 256
TAP_IMAGE = 0           # the probe that also records the gradient reaching every block output (case b)


def _image(i):
    """Image i of the stream: (x [1, 3, 256, 256], gout [1, 6, 256, 256], t)."""
    g = torch.Generator().manual_seed(7000 + i)
    x = torch.randn((1, 3, SIZE, SIZE), generator=g)
    gout = torch.randn((1, 6, SIZE, SIZE), generator=g)
    return x, gout, int(torch.randint(0, 1000, (1,), generator=g))


def _t(images):
    return [_image(i)[2] for i in images]


def _probe(i, t):
    """(forward output, J(x)^T gout, {block: gradient reaching its output} or None) of image i at timestep t: torch.autograd through the
    oracle network in float64."""
    key = f"grad_f64_{i}_{t}"
    if key not in gpu_common._ORACLE_CACHE:
        torch.set_num_threads(16)
        sk = "grad_f64_state_dict"
        if sk not in gpu_common._ORACLE_CACHE:
            gpu_common._ORACLE_CACHE[sk] = {k: v.double() for k, v in uo.synth_state_dict(HP).items()}
        x, gout, t_own = _image(i)
        taps = {} if (i == TAP_IMAGE and t == t_own) else None
        xr = x.double().requires_grad_()
        o = uo.unet_forward(gpu_common._ORACLE_CACHE[sk], HP, xr, torch.tensor([t]), taps=taps, dtype=torch.float64)
        for v in (taps or {}).values():
            if v.requires_grad:
                v.retain_grad()
        (o * gout.double()).sum().backward()
        tg = None if taps is None else {k: v.grad.numpy() for k, v in taps.items() if k != "emb" and v.grad is not None}
        gpu_common._ORACLE_CACHE[key] = (o.detach().numpy(), xr.grad.numpy(), tg)
    return gpu_common._ORACLE_CACHE[key]


@pytest.fixture(scope="module")
def engine():
    """engine(precision): one gradient-mode FFHQ engine per precision for the whole module."""
    made = {}

    def get(precision):
        if precision not in made:
            e = diffpir_amd.Engine(0)
            e.set_precision(precision)
            e.enable_grad()
            make_model(e, HP)
            made[precision] = e
        return made[precision]
    yield get
    for e in made.values():
        e.close()


def _vjp(e, images, ts, scales=None):
    x = torch.cat([_image(i)[0] for i in images])
    gout = torch.cat([_image(i)[1] for i in images])
    if scales is not None:
        gout = gout * torch.tensor(scales, dtype=torch.float32)[:, None, None, None]
    out, dx = e.unet_vjp(e.to_device(x.numpy()), np.asarray(ts, np.int64), e.to_device(gout.numpy()))
    return out.numpy(), dx.numpy()


def _against_f64(label, out, dx, images, ts, positions, scales=None):
    """Per-image errors of the batch positions `positions` against their float64 probes; gout scaled by s_n scales the exact gradient by
    s_n (the VJP is linear in gout).  Returns (worst forward error, worst gradient error, gradient error of every position)."""
    ref_o, ref_d = [], []
    for p in positions:
        o, d, _ = _probe(images[p], ts[p])
        ref_o.append(o[0])
        ref_d.append(d[0] * (1.0 if scales is None else scales[p]))
    pos = list(positions)
    fe, fn = per_image_err(out[pos], np.stack(ref_o))
    ge, gn = per_image_err(dx[pos], np.stack(ref_d))
    each = [per_image_err(dx[p:p + 1], ref_d[k][None])[0] for k, p in enumerate(pos)]
    print(f"{label}: worst per-image error vs float64 autograd over batch positions {pos}: forward {fe:.3e} (position {pos[fn]}), "
          f"input gradient {ge:.3e} (position {pos[gn]})")
    return fe, ge, each


# ---------------------------------------------------------------------------------------------------------------- a. benched DPS batches
@pytest.mark.parametrize("B", [8, 16])
def test_a_benched_batch_t_per_image(engine, B):
    """bench.py --full's DPS_y0 batches, a different t per image: the 3x3 dispatch, split-K factors, 4-image tiles of the 8^2 level, gn_bwd and
    absmax grids all at B = 8 / 16.  Probes: the first, a middle and the last image."""
    images = list(range(B))
    ts = _t(images)
    out, dx = _vjp(engine("f16x3"), images, ts)
    fe, ge, _ = _against_f64(f"a. FFHQ 256^2 B={B} [f16x3], t per image", out, dx, images, ts, (0, B // 2, B - 1))
    assert fe < TOL_FWD and ge < TOL_GRAD


def test_a_benched_batch_uniform_t(engine):
    """The uniform t that model_fn passes (one timestep for the whole batch), B = 8."""
    images = list(range(8))
    ts = [_image(0)[2]] * 8
    out, dx = _vjp(engine("f16x3"), images, ts)
    fe, ge, _ = _against_f64("a. FFHQ 256^2 B=8 [f16x3], uniform t", out, dx, images, ts, (0, 4, 7))
    assert fe < TOL_FWD and ge < TOL_GRAD


# ---------------------------------------------------------------------------------------------------------------- b. layer by layer
def test_b_block_gradients_at_b8(engine):
    """The gradient reaching every block output (engine taps 'grad:<block>') of one image of the B = 8 batch against float64 autograd taps,
    as test_unet_input_gradient_tiny_layer_by_layer does at 64^2: a failure of a or c is localised to one block."""
    e = engine("f16x3")
    images = list(range(8))
    ts = _t(images)
    _vjp(e, images, ts)
    _, _, taps = _probe(TAP_IMAGE, ts[TAP_IMAGE])
    worst, seen = ("", 0.0), 0
    for name, ref in taps.items():
        try:
            got = e.read_tap("grad:" + name).reshape((8,) + ref.shape[1:])[TAP_IMAGE:TAP_IMAGE + 1]
        except diffpir_amd.EngineError:
            continue
        err, _ = per_image_err(got, ref)
        seen += 1
        print(f"  grad {name:28s} per-image err {err:.3e}")
        if err > worst[1]:
            worst = (name, err)
    print(f"b. FFHQ 256^2 B=8 [f16x3], image {TAP_IMAGE}: {seen} of {len(taps)} block gradients compared, worst {worst[0]} {worst[1]:.3e}")
    assert seen == len(taps) and worst[1] < TOL_GRAD


# ---------------------------------------------------------------------------------------------------------------- c. magnitude spread
SPREAD = (1.0, 1e-2, 1e-4, 1e-6)


def test_c_magnitude_spread_across_the_batch(engine):
    """B = 8 with gout scaled per image by 1, 1e-2, 1e-4, 1e-6 (each twice): the small images' gradients sit 20 binades below the large ones'.
    With one dY scale for the whole batch their f16 operands fell toward the subnormals (4.3e-4 here); the dgrad scales each image on its
    own (grad.hip launch_grad_scale).  Built from the three B = 8 probe images, so every position has a float64 reference (the probe's
    gradient times s_n) and the bound is asserted on all eight."""
    base = (0, 4, 7)
    images = [base[k % 3] for k in range(8)]
    scales = [SPREAD[k % 4] for k in range(8)]
    ts = _t(images)
    out, dx = _vjp(engine("f16x3"), images, ts, scales)
    fe, ge, each = _against_f64("c. FFHQ 256^2 B=8 [f16x3], gout spread 1 .. 1e-6", out, dx, images, ts, range(8), scales)
    for s in SPREAD:
        print(f"  gout x {s:.0e}: per-image gradient err {max(v for v, sc in zip(each, scales) if sc == s):.3e}")
    assert fe < TOL_FWD and ge < TOL_GRAD


# ---------------------------------------------------------------------------------------------------------------- d. partial tiles, odd batches
@pytest.mark.parametrize("B", [3, 5])
def test_d_partial_tiles_and_odd_batches(engine, B):
    """B = 3 / 5 at 256^2: the 8^2 level runs 4-image tiles with empty slots, odd split-K and gn_bwd grids."""
    images = list(range(B))
    ts = _t(images)
    out, dx = _vjp(engine("f16x3"), images, ts)
    fe, ge, _ = _against_f64(f"d. FFHQ 256^2 B={B} [f16x3]", out, dx, images, ts, (0, B // 2, B - 1))
    assert fe < TOL_FWD and ge < TOL_GRAD


def test_d_batch_invariance_b8_against_each_image_alone(engine):
    """Image n's gradient from the B = 8 run against the same image run alone, every n.  Not bitwise: the dY scale is batch-wide and the
    split-K factors depend on B."""
    e = engine("f16x3")
    images = list(range(8))
    ts = _t(images)
    _, dx8 = _vjp(e, images, ts)
    worst = (0.0, -1)
    for n in images:
        _, dx1 = _vjp(e, [n], [ts[n]])
        err, _ = per_image_err(dx8[n:n + 1], dx1)
        worst = max(worst, (err, n))
    print(f"d. FFHQ 256^2 [f16x3]: B=8 vs each image alone, worst per-image gradient difference {worst[0]:.3e} (image {worst[1]})")
    assert worst[0] < TOL_GRAD


# ---------------------------------------------------------------------------------------------------------------- e. f32 mode
def test_e_f32_mode_at_b8(engine):
    """Case a at B = 8 with the exact-fp32 convolutions: dgrad on conv2 / conv at 256^2."""
    images = list(range(8))
    ts = _t(images)
    out, dx = _vjp(engine("f32"), images, ts)
    fe, ge, _ = _against_f64("e. FFHQ 256^2 B=8 [f32], t per image", out, dx, images, ts, (0, 4, 7))
    assert fe < TOL_FWD and ge < TOL_GRAD


# ---------------------------------------------------------------------------------------------------------------- f. f16x1 in gradient mode
def test_f_f16x1_gradient_is_supported_reduced_precision(engine):
    """f16x1 (f16 operands, fp32 accumulation) is supported in gradient mode: forward and dgrad run single-product kernels.  Same contract
    as test_f16x1_mode_quality_contract for the forward: within 5e-3 of float64 autograd per image, and above 1e-5 -- so it is the reduced-
    precision path and not the f16x3 one."""
    images = list(range(8))
    ts = _t(images)
    out, dx = _vjp(engine("f16x1"), images, ts)
    fe, ge, each = _against_f64("f. FFHQ 256^2 B=8 [f16x1], t per image", out, dx, images, ts, (0, 4, 7))
    assert fe < 5e-3 and all(1e-5 < v < 5e-3 for v in each), each


# ---------------------------------------------------------------------------------------------------------------- g. DPS_y0 loop
def test_g_dps_y0_loop_at_the_benched_batch_b8(engine):
    """generate_mode 'DPS_y0' as bench.py --full runs it: B = 8, x4 SISR 64^2 -> 256^2, 3 NFE, host noise, against oracle.restore_dps_y0 on the
    WHOLE batch (the residual norm is batch-wide) with the bounds of test_dps_y0_loop_full_size_ffhq_vs_oracle."""
    B = 8
    case = synth.make_case("sr", B, 256, 256, seed=400, sf=4)
    cfg = restore.LoopConfig(task="sr", iter_num=3, lambda_=6.0, zeta=0.25, sf=4, sr_mode="cubic", generate_mode="DPS_y0")
    out = restore.restore_batch(engine("f16x3"), cfg, case["y"], noise_source="host", noise_fn=seeded_noise_fn_np(83)).numpy()
    key = "grad_dps_y0_b8_3nfe"
    if key not in gpu_common._ORACLE_CACHE:
        torch.set_num_threads(16)
        gen = torch.Generator().manual_seed(83)
        ocfg = do.LoopConfig("sr", 3, 12.75 / 255, 6.0, 0.25, sf=4, sr_mode="cubic", generate_mode="DPS_y0")
        gpu_common._ORACLE_CACHE[key] = do.restore_dps_y0(uo.synth_state_dict(HP), HP, ocfg, torch.from_numpy(case["y"]),
                                                          noise_fn=lambda like: torch.randn(like.shape, generator=gen, dtype=torch.float32)).numpy()
    ref = gpu_common._ORACLE_CACHE[key]
    err = float(np.abs(out - ref).max())
    gt = case["gt"] * 2 - 1
    gap = abs(restore.psnr_batch(out * 2 - 1, gt) - restore.psnr_batch(ref * 2 - 1, gt))
    print(f"g. DPS_y0 FFHQ 256^2 B=8 3-NFE [f16x3] vs oracle autograd: max|diff| {err:.3e} (output range {np.abs(ref).max():.2f}), |dPSNR| {gap:.2e} dB")
    assert gap <= 1e-3 and err < 2e-4 * max(1.0, float(np.abs(ref).max()))
