"""GPU box: what arming the progressive strip costs on the bench workload (ffhq topology, deblur, B = 16, 256 x 256, 100 NFE, 11 panels,
f32 + uint8 strips), armed against unarmed in ONE process and interleaved, and the snapshot kernel's own time and achieved bandwidth.
The strips are armed through dpir_set_progress directly and stay on the device: restore.Progress would add their download to the loop time.

    python tools/progress_time.py [--reps 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/progress_time.py --kernel-only     # the kernel's own time, no model, no loop
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--nfe", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="200 snapshots of a random image and nothing else (for a kernel trace)")
    a = ap.parse_args()
    import diffpir_amd
    from diffpir_amd import _lib, restore, synth, script_util, weights
    B, H, W = a.batch, a.size, a.size
    e = diffpir_amd.Engine(0)
    if a.kernel_only:
        P = 11
        x = e.to_device(np.random.default_rng(0).standard_normal((B, 3, H, W)).astype(np.float32))
        strip_f32, strip_u8, mm = e.empty((B, 3, H, P * W)), e.empty((B, H, P * W, 3), np.uint8), e.empty((P, B, 2))
        for i in range(200):
            e.progress_snapshot(x, i % P, P, strip_f32=strip_f32, strip_u8=strip_u8, minmax=mm)
        e.sync()
        e.close()
        return
    e.set_precision("f16x3")
    hp = weights.model_hp("ffhq")
    m = script_util.create_model(**weights.create_model_kwargs(hp), engine=e)
    m.load_state_dict(weights.synth_state_dict(hp, 0))
    cfg = restore.LoopConfig(task="deblur", iter_num=a.nfe, lambda_=7.0, zeta=0.3)
    case = synth.make_case("deblur", B, H, W, seed=100, ksize=61, blur="gaussian")
    y, k = e.to_device(case["y"]), e.to_device(case["k"])
    out_f32, out_u8 = e.empty((B, 3, H, W)), e.empty((B, H, W, 3), np.uint8)
    _, steps, _ = restore._steps(cfg)
    table, panels = restore.progress_table(cfg, steps)
    P = len(panels)
    strip_f32, strip_u8, mm = e.empty((B, 3, H, P * W)), e.empty((B, H, P * W, 3), np.uint8), e.empty((P, B, 2))
    tab = (C.c_int32 * len(table))(*table)

    def arm():
        d = _lib.ProgressDesc()
        d.panel_of_step_host, d.n_entries, d.n_panels = tab, len(table), P
        d.strip_f32, d.strip_u8, d.minmax_dev = strip_f32.ptr, strip_u8.ptr, mm.ptr
        e._check(e.lib.dpir_set_progress(e.h, C.byref(d)))

    keep = {}

    def loop(armed):
        if armed:
            arm()
        e.sync()
        t0 = time.perf_counter()
        restore.restore_batch(e, cfg, y, k=k, noise_source="device", seed=1234, use_graph=True, out_f32=out_f32, out_u8=out_u8, _cache=keep)
        e.sync()
        return (time.perf_counter() - t0) * 1e3

    loop(False)
    loop(True)                                     # warm-up of both
    plain, armed = [], []
    for _ in range(a.reps):
        plain.append(loop(False))
        armed.append(loop(True))
    ref = out_f32.numpy()
    assert strip_f32.numpy()[..., -W:].tobytes() == ref.tobytes()
    # the kernel alone: back-to-back snapshots of the final x (out_f32 holds x/2+.5; any float image does for timing)
    n = 200
    for with_mm in (True, False):
        e.progress_snapshot(out_f32, 0, P, strip_f32=strip_f32, strip_u8=strip_u8, minmax=mm if with_mm else None)
    e.sync()
    t0 = time.perf_counter()
    for i in range(n):
        e.progress_snapshot(out_f32, i % P, P, strip_f32=strip_f32, strip_u8=strip_u8, minmax=mm)
    e.sync()
    us = (time.perf_counter() - t0) / n * 1e6
    moved = B * 3 * H * W * (4 + 4 + 1)
    res = dict(workload=f"ffhq deblur B={B} {H}x{W} {a.nfe} NFE, {P} panels, f32 + u8 strips + minmax, hipGraph on", reps=a.reps,
               unarmed_ms=plain, armed_ms=armed, unarmed_ms_median=float(np.median(plain)), armed_ms_median=float(np.median(armed)),
               armed_minus_unarmed_ms=float(np.median(armed) - np.median(plain)), snapshot_us=us, snapshot_bytes=moved,
               snapshot_GBps=moved / us * 1e-3, note="snapshot_us: 200 back-to-back launches (each with its min/max initialisation launch), host-timed")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
