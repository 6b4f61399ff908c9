"""Cost of the inpainting data step: the chain of separate elementwise launches beside the one fused pass (csrc/inpaint.hip).  GPU box only.

  * us per data step at (16, 256, 256) and (32, 256, 256), device noise: the chain xstart + dpir_prox_mask + 2 dpir_randn + dpir_renoise (with back = 1:
    + dpir_randn + the three dpir_ewise launches of the set-back) against one dpir_inpaint_step (asynchronous, the row in the kernel arguments: one launch).  The ABI has no stand-alone eps -> x0 entry; the chain's
    first link is timed with dpir_eps_from_xstart, which moves the same bytes (two reads, one write per element).  HIP events on the engine stream
    around REPS back-to-back data steps after a warm-up, SETS sets, the host kept ahead of the GPU (see timed); median and min..max, and the fused pass's bytes per us.
  * ms per NFE of the inpainting loop, B = 16, FFHQ topology at 256 x 256, iter_num_U = 1: the default driver (dpir_run_loop, the chain inside a graph)
    and driver main_ddpir_inpainting (dpir_run_inpaint_loop), interleaved in one process.
usage: python tools/inpaint_step_time.py [iter_num]
"""
import ctypes as C
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import restore, synth, script_util, weights, _lib, schedule

REPS, SETS, LEAD = 20, 7, 16
iter_num = int(sys.argv[1]) if len(sys.argv) > 1 else 20
e = diffpir_amd.Engine(0); e.set_precision(os.environ.get("DIFFPIR_PRECISION", "f16x3"))
stream = torch.cuda.ExternalStream(e.lib.dpir_stream(e.h))
lib, h = e.lib, e.h


def timed(fn, lead):
    """us per call: SETS event pairs around REPS calls each, after one warm-up set.  A single launch is shorter than the host takes to issue it, so
    LEAD calls of `lead` (about a millisecond of GPU work) are queued ahead of the first event: the timed launches are all in the queue before the
    GPU reaches them, and the events see GPU time, not the host's issue rate."""
    out = []
    for s in range(SETS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(LEAD):
            lead()
        a.record(stream)
        for _ in range(REPS):
            fn()
        b.record(stream)
        b.synchronize()
        if s:
            out.append(a.elapsed_time(b) * 1e3 / REPS)
    return float(np.median(out)), min(out), max(out)


# eta != 0: the eta draw is made, as in the chain's two dpir_randn (fused: two philox_normal4 per group, three with back)
_, rows, arr = schedule.build_inpaint_rows(iter_num=20, iter_num_U=2, sigma=0.05, lambda_=1.0, zeta=0.5, eta=0.5)
rng = np.random.default_rng(0)
for B in (16, 32):
    H = W = 256
    sh, numel = (B, 3, H, W), B * 3 * H * W
    x = e.to_device(rng.standard_normal(sh).astype(np.float32)); eps = e.to_device(rng.standard_normal((B, 6, H, W)).astype(np.float32))
    y = e.to_device(rng.random(sh).astype(np.float32)); m = e.to_device((rng.random(sh) < 0.5).astype(np.uint8), np.uint8)
    x0, n1, n2 = e.empty(sh), e.empty(sh), e.empty(sh)
    for back in (0, 1):
        row = arr[0 if back else 1]
        assert row.back == back and not row.last and row.es != 0
        st = _lib.Step()
        for f, _ in _lib.Step._fields_:
            setattr(st, f, getattr(row, f))

        def chain():
            e._check(lib.dpir_eps_from_xstart(h, x.ptr, eps.ptr, 1.0, 1.0, 0, x0.ptr, numel))       # stands in for eps -> x0: same traffic
            e._check(lib.dpir_prox_mask(h, x0.ptr, y.ptr, m.ptr, row.tau, 1.0, B, H, W))
            e._check(lib.dpir_randn(h, n1.ptr, 1, 1, 0, B, 3, H, W))
            e._check(lib.dpir_randn(h, n2.ptr, 1, 2, 0, B, 3, H, W))
            e._check(lib.dpir_renoise(h, x.ptr, x0.ptr, C.byref(st), n1.ptr, n2.ptr, B, H, W))
            if back:
                e._check(lib.dpir_randn(h, n1.ptr, 1, 2 ** 32, 0, B, 3, H, W))
                e._check(lib.dpir_ewise(h, 2, x.ptr, None, 0, row.sae, x.ptr, numel))
                e._check(lib.dpir_ewise(h, 2, n1.ptr, None, 0, row.sb, n1.ptr, numel))
                e._check(lib.dpir_ewise(h, 0, x.ptr, n1.ptr, numel, 0.0, x.ptr, numel))

        def fused():
            e._check(lib.dpir_inpaint_step(h, x.ptr, eps.ptr, 6, y.ptr, m.ptr, C.byref(row), 0, 1.0, None, None, None, None, 1, 0, 0, None, B, H, W))
        c, f = timed(chain, chain), timed(fused, chain)
        moved = numel * (4 + 4 + 4 + 1 + 4)          # x, eps, y read, mask read, x written
        print(f"inpaint data step ({B}, 256, 256) back={back}: chain {c[0]:.1f} us ({c[1]:.1f}..{c[2]:.1f}) | fused {f[0]:.1f} us ({f[1]:.1f}..{f[2]:.1f}), "
              f"{moved / f[0] / 1e6:.2f} TB/s moved")

hp = weights.model_hp("ffhq")
mdl = script_util.create_model(**weights.create_model_kwargs(hp), engine=e); mdl.load_state_dict(weights.synth_state_dict(hp, 0))
B = 16
case = synth.make_case("inpaint", B=B, H=256, W=256, seed=42)
yd, md = e.to_device(case["y"]), e.to_device(case["mask"], np.uint8)
kw = dict(task="inpaint", iter_num=iter_num, noise_level_img=0.0, lambda_=1.0, zeta=1.0)
cfgs = {"main_ddpir (chain)": restore.LoopConfig(**kw), "main_ddpir_inpainting (fused)": restore.LoopConfig(driver="main_ddpir_inpainting", **kw)}
ts = {k: [] for k in cfgs}
for r in range(6):
    for name, cfg in cfgs.items():
        t0 = time.perf_counter(); o = restore.restore_batch(e, cfg, yd, mask=md, noise_source="device", seed=1, use_graph=True); e.sync()
        if r:
            ts[name].append((time.perf_counter() - t0) / iter_num * 1e3)
for name, v in ts.items():
    print(f"inpainting loop B={B} FFHQ 256x256 U=1, {name}: {np.median(v):.3f} ms per NFE ({min(v):.3f}..{max(v):.3f})")
