"""Cost of dpir_lpips (csrc/lpips.hip) at the benched batch.  GPU box only.

HIP events on the engine stream around one dpir_lpips call (the call synchronises itself: it returns host floats), B = 16 pairs at 256 x 256,
seeded synthetic weights, WARM warm-up calls, the median of REPS; beside it the trunk's FLOPs computed from the shapes (2 * MAC of the 13
convolutions, both images of every pair) and the achieved fraction of the fp32 MFMA peak.  With `--loop-ms X` (bench.py's ms_per_step of the
same run: one 100-NFE restoration of the batch) it also prints LPIPS's share of the restoration loop.
usage: python tools/lpips_time.py [--batch 16] [--size 256] [--reps 21] [--loop-ms X]
"""
import argparse, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import degrade as dgr, lpips as lp, synth

PEAK = 157.3e12          # fp32 MFMA (v_mfma_f32_32x32x2_f32), MI355X
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--loop-ms", type=float, default=0.0)
a = ap.parse_args()
assert a.reps >= 20

e = diffpir_amd.Engine(0)
e.load_lpips(lp.synth_weights(0))
stream = torch.cuda.ExternalStream(e.lib.dpir_stream(e.h))
B, S = a.batch, a.size
gt = synth.smooth_images(B, S, S, 42)
gt_u8 = e.to_device(np.ascontiguousarray((gt * 255.0).round().astype(np.uint8).transpose(0, 2, 3, 1)))
x0 = e.to_device((gt + np.random.default_rng(0).standard_normal(gt.shape).astype(np.float32) * np.float32(0.05)).astype(np.float32))
ms = []
for r in range(a.warm + a.reps):
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record(stream)
    score = dgr.lpips(e, x0, gt_u8)
    s1.record(stream)
    s1.synchronize()
    if r >= a.warm:
        ms.append(s0.elapsed_time(s1))
flops = 2 * B * lp.trunk_flops(S, S)
med = float(np.median(ms))
print(f"dpir_lpips B={B} {S}x{S}: median {med:.2f} ms of {len(ms)} ({min(ms):.2f}..{max(ms):.2f}); trunk {flops / 1e9:.1f} GFLOP (2*MAC, {2 * B} rows) -> "
      f"{flops / (med * 1e-3) / 1e12:.1f} TFLOP/s, {100 * flops / (med * 1e-3) / PEAK:.0f}% of the fp32 MFMA peak; scores {score.min():.4f}..{score.max():.4f}")
if a.loop_ms > 0:
    print(f"share of the restoration loop ({a.loop_ms:.0f} ms per batch, bench.py ms_per_step): {100 * med / a.loop_ms:.2f}%")
e.close()
