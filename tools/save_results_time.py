"""GPU box: what saving one batch's results costs, part by part, at the example workload's shape (B = 16, 256 x 256, deblur, 61 x 61 kernel).

  kernel   dpir_result_panels (L + LEH), bracketed by HIP events on the engine stream (dpir_prof_enable, class `elementwise`), median of REPS
  D2H      the synchronous copies of L [B,h,w,3], LEH [B,H,3W,3] and E [B,H,W,3] to the host, host-timed around a call that ends in a sync
  encode   PNG encoding and writing of the batch's files (E, L, LEH, kernel picture per image) into a temporary directory: wall time on ONE
           thread, and wall time through main_ddpir.ResultWriter (4 workers) from the first submit to the end of drain()

    python tools/save_results_time.py [--batch 16] [--size 256] [--sf 1] [--reps 11] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sf", type=int, default=1)
    ap.add_argument("--ksize", type=int, default=61)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import diffpir_amd
    from diffpir_amd import degrade as dgr, main_ddpir, synth
    B, H, W, sf = a.batch, a.size, a.size, a.sf
    e = diffpir_amd.Engine(0)
    rng = np.random.default_rng(0)
    # smooth images, as a restored batch is: PNG's cost depends on the content
    gt = np.ascontiguousarray((synth.smooth_images(B, H, W, 42) * 255.0).round().astype(np.uint8).transpose(0, 2, 3, 1))
    est = np.clip(gt.astype(np.int16) + rng.integers(-3, 4, gt.shape), 0, 255).astype(np.uint8)
    k = np.stack([synth.gaussian_psf(a.ksize, 3.0 + b / B) for b in range(B)])[:, None].astype(np.float32)
    y = np.ascontiguousarray(gt[:, ::sf, ::sf].transpose(0, 3, 1, 2).astype(np.float32) / 255.0) + rng.standard_normal((B, 3, H // sf, W // sf)).astype(np.float32) * 0.05
    yd, ed, gd = e.to_device(y.astype(np.float32)), e.to_device(est), e.to_device(gt)

    def call():
        return dgr.result_panels(e, yd, ed, gd, k=k, sf=sf)

    call()
    e.prof_enable(True)
    kernel_ms, total_ms = [], []
    for _ in range(a.reps):
        e.sync()
        e.prof_reset()
        t0 = time.perf_counter()
        L, leh = call()
        E = ed.numpy()
        total_ms.append((time.perf_counter() - t0) * 1e3)
        ms, cnt = e.prof_read()["elementwise"]
        assert cnt == 1, cnt
        kernel_ms.append(ms)
    e.prof_enable(False)
    moved = L.nbytes + leh.nbytes + y.nbytes + est.nbytes + gt.nbytes
    d2h_bytes = L.nbytes + leh.nbytes + E.nbytes

    names = [f"synth_{i:04d}.png" for i in range(B)]
    cfg = main_ddpir.Config(dict(task="deblur", sf=sf, model_name="diffusion_ffhq_10m", testset_name="demo_test", generate_mode="DiffPIR",
                                 noise_level_img=0.05, iter_num=100, eta=0, zeta=0.1, lambda_=1, blur_mode="Gaussian", sr_mode="blur", batch_size=B,
                                 engine_save_results=True, save_E=True, save_L=True, save_LEH=True))
    serial_ms, pool_ms, n_files, n_bytes = [], [], 0, 0
    for _ in range(max(3, a.reps // 3)):
        with tempfile.TemporaryDirectory() as tmp:
            cfg.cwd = tmp
            t0 = time.perf_counter()
            paths = main_ddpir.emit_results(cfg, names, 7.0, 0.3, est_u8=E, L_u8=L, leh_u8=leh, k=k)
            serial_ms.append((time.perf_counter() - t0) * 1e3)
            n_files, n_bytes = len(paths), sum(os.path.getsize(p) for p in paths)
        with tempfile.TemporaryDirectory() as tmp:
            cfg.cwd = tmp
            rw = main_ddpir.ResultWriter(n_files, workers=4)
            t0 = time.perf_counter()
            main_ddpir.emit_results(cfg, names, 7.0, 0.3, est_u8=E, L_u8=L, leh_u8=leh, k=k, submit=rw.submit)
            rw.drain()
            pool_ms.append((time.perf_counter() - t0) * 1e3)
            rw.close()
    med = lambda v: float(np.median(v))      # noqa: E731
    res = dict(shape=f"B={B} {H}x{W} sf={sf} kernel {a.ksize}x{a.ksize}", reps=a.reps,
               kernel_ms=kernel_ms, kernel_ms_median=med(kernel_ms), kernel_bytes_moved=moved, kernel_GBps=moved / med(kernel_ms) * 1e-6,
               call_plus_d2h_ms=total_ms, call_plus_d2h_ms_median=med(total_ms), d2h_bytes=d2h_bytes,
               files_per_batch=n_files, file_bytes_per_batch=n_bytes, encode_serial_ms=serial_ms, encode_serial_ms_median=med(serial_ms),
               encode_pool4_ms=pool_ms, encode_pool4_ms_median=med(pool_ms),
               note="kernel_ms: HIP events around the launch; call_plus_d2h_ms: host-timed degrade.result_panels (kernel-byte upload, two output "
                    "allocations, launch, two synchronous D2H) plus the D2H of E; encode: wall time of PIL's PNG encoder into a temporary directory")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
