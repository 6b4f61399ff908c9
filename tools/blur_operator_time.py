"""Cost of the deblurring program's blur operator (csrc/blur.hip) and of DPS_y0 deblurring beside DPS_y0 super-resolution.  GPU box only.

  * us per dpir_blur_reflect and per dpir_blur_reflect_adjoint at (8, 256, 256, 61) and (16, 256, 256, 61): HIP events on the engine stream
    around REPS back-to-back launches after a warm-up, SETS sets; median and min..max over the sets, and the achieved fraction of the fp32
    vector peak (2 * K * K flops per output, 157.3 TFLOP/s; the adjoint is charged its (H + K - 1) x (W + K - 1) padded grid).
  * ms per NFE of DPS_y0, B = 8, FFHQ topology at 256 x 256: driver main_ddpir_deblur (the operator pair of this file) beside the x4 SISR
    loop of main_ddpir (the Resizer pair) in the same run: the difference is what the blur operator costs in a step.
usage: python tools/blur_operator_time.py [nfe]
"""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import restore, synth, script_util, weights
from diffpir_amd.utils_deblur import BlurOperator

PEAK = 157.3e12
REPS, SETS, K = 20, 7, 61
nfe = int(sys.argv[1]) if len(sys.argv) > 1 else 6
e = diffpir_amd.Engine(0); e.set_precision(os.environ.get("DIFFPIR_PRECISION", "f16x3")); e.enable_grad()
stream = torch.cuda.ExternalStream(e.lib.dpir_stream(e.h))


def timed(fn):
    """us per call: SETS event pairs around REPS calls each, after one warm-up set."""
    out = []
    for s in range(SETS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(REPS):
            fn()
        b.record(stream)
        b.synchronize()
        if s:
            out.append(a.elapsed_time(b) * 1e3 / REPS)
    return float(np.median(out)), min(out), max(out)


rng = np.random.default_rng(0)
ax = np.arange(K) - K // 2
for B in (8, 16):
    k = np.stack([np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2 * (2.0 + n) ** 2)) for n in range(B)])[:, None]
    op = BlurOperator((k / k.sum(axis=(2, 3), keepdims=True)).astype(np.float32), engine=e)
    x = e.to_device(rng.standard_normal((B, 3, 256, 256)).astype(np.float32))
    out = e.empty(x.shape)
    kd = op.psf(B)
    fwd = timed(lambda: e._check(e.lib.dpir_blur_reflect(e.h, x.ptr, kd.ptr, K, K, 0.5, 0.5, out.ptr, B, 256, 256)))
    adj = timed(lambda: e._check(e.lib.dpir_blur_reflect_adjoint(e.h, x.ptr, kd.ptr, K, K, 0.5, out.ptr, B, 256, 256)))
    ff, fa = 2.0 * K * K * B * 3 * 256 * 256, 2.0 * K * K * B * 3 * (256 + K - 1) ** 2
    print(f"blur operator ({B}, 256, 256, {K}): forward {fwd[0]:.1f} us ({fwd[1]:.1f}..{fwd[2]:.1f}), {100 * ff / (fwd[0] * 1e-6) / PEAK:.1f}% of fp32 vector peak | "
          f"adjoint {adj[0]:.1f} us ({adj[1]:.1f}..{adj[2]:.1f}), {100 * fa / (adj[0] * 1e-6) / PEAK:.1f}%")

hp = weights.model_hp("ffhq")
m = script_util.create_model(**weights.create_model_kwargs(hp), engine=e); m.load_state_dict(weights.synth_state_dict(hp, 0))
B = 8
sr = synth.make_case("sr", B, 256, 256, seed=400, sf=4)
k = np.stack([np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2 * (2.0 + n) ** 2)) for n in range(B)])[:, None]
k = (k / k.sum(axis=(2, 3), keepdims=True)).astype(np.float32)
runs = {"DPS_y0 sr x4 (main_ddpir, Resizer pair)": (restore.LoopConfig(task="sr", iter_num=nfe, lambda_=6.0, zeta=0.25, sf=4, sr_mode="cubic",
                                                                          generate_mode="DPS_y0"), e.to_device(sr["y"]), None),
        "DPS_y0 deblur (main_ddpir_deblur, blur pair)": (restore.LoopConfig(driver="main_ddpir_deblur", task="deblur", iter_num=nfe, lambda_=6.0, zeta=0.25,
                                                                            generate_mode="DPS_y0"), e.to_device(sr["gt"]), e.to_device(k))}
for name, (cfg, y, kd) in runs.items():
    ts = []
    for r in range(4):
        t0 = time.perf_counter(); o = restore.restore_batch(e, cfg, y, k=kd, noise_source="device", seed=1); e.sync()
        if r:
            ts.append((time.perf_counter() - t0) / (nfe - 1) * 1e3)
    print(f"{name}: B={B} {np.median(ts):.2f} ms per NFE ({min(ts):.2f}..{max(ts):.2f}), finite={bool(np.isfinite(o.numpy()).all())}")
