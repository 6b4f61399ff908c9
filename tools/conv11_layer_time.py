"""Back-to-back time of the 3x3 convolution launch alone on the geometry-0 shapes of the FFHQ forward: conv7 (route 7, through launch_conv6)
vs conv11 (route 0), same random operand planes, three repeats, the two arms alternating.  BATCH=16 ITERS=50  (GPU box only)"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import _lib
e = diffpir_amd.Engine(0); e.set_precision("f16x3")
dbg = _lib.load_debug()
r = np.random.default_rng(0)
shapes = [(128, 128, 256), (256, 128, 256), (256, 256, 128), (128, 128, 128), (256, 256, 64)]      # (Cin, Cout, size)
B = int(os.environ.get("BATCH", "16"))
reps, iters = 3, int(os.environ.get("ITERS", "50"))
p = lambda a: a.ctypes.data_as(C.c_void_p).value
tot = {7: np.zeros(reps), 0: np.zeros(reps)}
for cin, cout, hw in shapes:
    w = (0.05 * r.standard_normal((cout, cin, 3, 3))).astype(np.float32)
    bias = r.standard_normal(cout).astype(np.float32)
    x = r.standard_normal((B, cin, hw, hw), dtype=np.float32)
    out = np.empty((B, cout, hw, hw), np.float32)
    t = {7: [], 0: []}
    for k in range(reps):
        for route in (7, 0):
            d = _lib.Conv11Desc(B=B, Cin=cin, Cout=cout, H=hw, W=hw, res_mode=-1, route=route, ksplit=1, iters=iters)
            d.x, d.w, d.bias, d.out = p(x), p(w), p(bias), p(out)
            rc = dbg.dpir_debug_conv11_layer(e.h, C.byref(d))
            if rc != 0:
                print("  refused:", e.lib.dpir_last_error(e.h), flush=True)
                t[route].append(float("nan"))
            else:
                t[route].append(d.ms_out * 1e3)
            tot[route][k] += t[route][-1]
    tf = 2.0 * 3 * B * cout * cin * 9 * hw * hw / 1e12
    print(f"LAYER11 {cin}->{cout} @{hw}^2 B={B}: conv7 {' '.join(f'{v:7.1f}' for v in t[7])} us | conv11 {' '.join(f'{v:7.1f}' for v in t[0])} us"
          f" | ratio {np.mean(t[0]) / np.mean(t[7]):.3f} | conv7 {tf / (np.mean(t[7]) * 1e-6):.0f} conv11 {tf / (np.mean(t[0]) * 1e-6):.0f} TF/s-equivalent", flush=True)
print(f"LAYER11 sum: conv7 {' '.join(f'{v:7.1f}' for v in tot[7])} us (spread {tot[7].max() - tot[7].min():.1f}) | conv11 {' '.join(f'{v:7.1f}' for v in tot[0])} us"
      f" | conv7 - conv11 {tot[7].mean() - tot[0].mean():.1f} us", flush=True)
