"""Cost of dpir_fid_features (csrc/fid.hip) at the benched batch.  GPU box only.

HIP events on the engine stream around one dpir_fid_features call (the call synchronises itself: it returns host floats), B = 16 uint8 images at
256 x 256, seeded synthetic weights, WARM warm-up calls, the median of REPS; beside it the FLOPs of the 94 convolutions (fid.flops(), 2 * MAC)
and the achieved fraction of the fp32 MFMA peak.  With `--loop-ms X` (bench.py's ms_per_step of the same session: one 100-NFE restoration of
the batch) it also prints FID's share of the restoration loop, counting BOTH sets (the restored images and the ground truth).
usage: python tools/fid_time.py [--batch 16] [--size 256] [--reps 21] [--loop-ms X]
"""
import argparse, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import degrade as dgr, fid as fd, synth

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
e.load_fid(fd.synth_weights(0))
stream = torch.cuda.ExternalStream(e.lib.dpir_stream(e.h))
B, S = a.batch, a.size
gt = synth.smooth_images(B, S, S, 42)
u8 = e.to_device(np.ascontiguousarray((gt * 255.0).round().astype(np.uint8).transpose(0, 2, 3, 1)))
ms = []
for r in range(a.warm + a.reps):
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record(stream)
    feats = dgr.fid_features(e, u8)
    s1.record(stream)
    s1.synchronize()
    if r >= a.warm:
        ms.append(s0.elapsed_time(s1))
flops = B * fd.flops()
med = float(np.median(ms))
print(f"dpir_fid_features B={B} {S}x{S}: median {med:.2f} ms of {len(ms)} ({min(ms):.2f}..{max(ms):.2f}); {flops / 1e9:.1f} GFLOP (2*MAC, 94 convolutions) -> "
      f"{flops / (med * 1e-3) / 1e12:.1f} TFLOP/s, {100 * flops / (med * 1e-3) / PEAK:.0f}% of the fp32 MFMA peak; features {feats.min():.4f}..{feats.max():.4f}")
if a.loop_ms > 0:
    print(f"share of the restoration loop ({a.loop_ms:.0f} ms per batch, bench.py ms_per_step), both sets (2 calls): {100 * 2 * med / a.loop_ms:.2f}%")
e.close()
