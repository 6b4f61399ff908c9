"""Microseconds per FFT-prox apply (dpir_prox_fft_apply_timed, as one captured graph and eagerly) at two sizes that are no power of two -- the
mixed-radix kernels of csrc/fft_mixed.hip -- next to the generic power-of-two kernels (csrc/fft.hip) at the nearest larger sizes, interleaved in
one run.  `python tools/prox_anysize_time.py [B] [rounds]`; profiles/prox_anysize/README.md records a run."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import utils_sisr as sr

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
SHAPES = [("mixed", 96, 160), ("generic", 128, 256), ("mixed", 224, 352), ("generic", 256, 512)]

eng = diffpir_amd.Engine(0)
rng = np.random.default_rng(0)
k = rng.random((B, 1, 15, 15)).astype(np.float32)
k /= k.sum(axis=(2, 3), keepdims=True)
state = []
for fam, H, W in SHAPES:
    pre = sr.pre_calculate(eng.to_device(rng.random((B, 3, H, W)).astype(np.float32)), eng.to_device(k), 1)
    state.append((pre, eng.to_device((rng.random((B, 3, H, W)) * 2 - 1).astype(np.float32))))
for r in range(ROUNDS):
    for (fam, H, W), (pre, x0) in zip(SHAPES, state):
        us_g, us_e = C.c_float(), C.c_float()
        eng._check(eng.lib.dpir_prox_fft_apply_timed(eng.h, pre[0].spectra.handle, x0.ptr, 0.05, 1.0, 40, 1, C.byref(us_g)))
        eng._check(eng.lib.dpir_prox_fft_apply_timed(eng.h, pre[0].spectra.handle, x0.ptr, 0.05, 1.0, 40, 0, C.byref(us_e)))
        print(f"round {r} {fam:7s} {H:3d} x {W:3d} B {B}: graph {us_g.value:7.1f} us/apply, eager {us_e.value:7.1f} us/apply, "
              f"{us_g.value * 1e3 / (B * 3 * H * W):6.3f} ns/pixel (graph)", flush=True)
eng.close()
