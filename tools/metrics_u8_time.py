"""Cost and accuracy of dpir_metrics_u8 (csrc/metrics8.hip).  GPU box only.

Time: HIP events on the engine stream around one call (every call here synchronises itself: it returns host numbers), B = 16 at 256 x 256,
WARM warm-up calls, the median of REPS; dpir_metrics_u8 (float32 estimate and uint8 estimate) beside dpir_metrics and dpir_lpips (seeded
synthetic weights) in the same run.
Accuracy (--accuracy): per shape and pair kind of tests/test_gpu_metrics_u8.py the worst |dSSIM| (RGB and Y) and |dPSNR| of the engine against
the float64 statement of tests/metrics_u8_f64.py, beside the spread of the statement's two float64 summation orders and the gap of its float32
evaluation, both on the CPU.
usage: python tools/metrics_u8_time.py [--batch 16] [--size 256] [--reps 21] [--accuracy]
"""
import argparse, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import degrade as dgr, lpips as lp, synth
from tests import metrics_u8_f64 as M

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--accuracy", action="store_true")
a = ap.parse_args()
assert a.reps >= 20

e = diffpir_amd.Engine(0)
e.load_lpips(lp.synth_weights(0))
stream = torch.cuda.ExternalStream(e.lib.dpir_stream(e.h))
B, S = a.batch, a.size
gt = synth.smooth_images(B, S, S, 42)
gt_u8 = e.to_device(np.ascontiguousarray((gt * 255.0).round().astype(np.uint8).transpose(0, 2, 3, 1)))
x0_host = (gt + np.random.default_rng(0).standard_normal(gt.shape).astype(np.float32) * np.float32(0.05)).astype(np.float32)
x0 = e.to_device(x0_host)
x0_u8 = e.to_device(M.quantise(x0_host))


def timed(fn):
    ms = []
    for r in range(a.warm + a.reps):
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record(stream)
        out = fn()
        s1.record(stream)
        s1.synchronize()
        if r >= a.warm:
            ms.append(s0.elapsed_time(s1))
    return float(np.median(ms)), min(ms), max(ms), out


rows = [("dpir_metrics_u8, float32 estimate", lambda: dgr.metrics_u8(e, x0, gt_u8, 0)),
        ("dpir_metrics_u8, uint8 estimate", lambda: dgr.metrics_u8(e, x0_u8, gt_u8, 0)),
        ("dpir_metrics_u8, uint8 estimate, border 4", lambda: dgr.metrics_u8(e, x0_u8, gt_u8, 4)),
        ("dpir_metrics", lambda: dgr.metrics(e, x0, gt_u8)),
        ("dpir_lpips", lambda: dgr.lpips(e, x0, gt_u8))]
print(f"B={B} {S}x{S}, median of {a.reps} after {a.warm} warm-up calls (HIP events around the whole synchronising call)")
for name, fn in rows:
    med, lo, hi, out = timed(fn)
    print(f"  {name}: median {med:.3f} ms ({lo:.3f}..{hi:.3f}); first image {[float(np.asarray(c)[0]) for c in (out if isinstance(out, tuple) else (out,))]}")

if a.accuracy:
    print("shape kind | engine |dSSIM| |dSSIM-Y| |dPSNR| dB (worst of the f32 and the u8 entry) | CPU order spread | float32 gap")
    for H, W, Bc, border in [(11, 11, 1, 0), (12, 27, 2, 0), (40, 56, 3, 4), (96, 160, 2, 0)]:
        for kind in M.KINDS:
            est, g = M.make_pair(H, W, Bc, kind)
            eu8 = M.quantise(est)
            ref = M.metrics(eu8, g, border)
            spread = np.abs(M.metrics(eu8, g, border, form="window2d")[:, 2:] - ref[:, 2:]).max()
            gap = np.abs(M.metrics(eu8, g, border, defect="float32_moments")[:, 2:] - ref[:, 2:]).max()
            d = np.zeros(3)
            for arg in (est, eu8):
                got = np.stack(dgr.metrics_u8(e, arg, g, border), 1)
                with np.errstate(invalid="ignore"):
                    dp = np.where(got[:, :2] == ref[:, :2], 0.0, np.abs(got[:, :2] - ref[:, :2])).max()
                d = np.maximum(d, [np.abs(got[:, 2] - ref[:, 2]).max(), np.abs(got[:, 3] - ref[:, 3]).max(), dp])
            print(f"  {H}x{W} B{Bc} border {border} {kind} | {d[0]:.2e} {d[1]:.2e} {d[2]:.2e} | {spread:.2e} | {gap:.2e}")
e.close()
