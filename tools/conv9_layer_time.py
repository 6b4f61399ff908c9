"""Back-to-back launch time of the 8 x 8 layers of the FFHQ forward: launch_conv6's route (split-K + combine) vs conv9."""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import _lib
prec = os.environ.get("DIFFPIR_PRECISION", "f16x3")
e = diffpir_amd.Engine(0); e.set_precision(prec)
dbg = _lib.load_debug()
r = np.random.default_rng(0)
shapes = [(512, 512), (1024, 512)]
batches = [int(b) for b in os.environ.get("BATCHES", "1,2,4,8,16,32").split(",")]
reps = 3
p = lambda a: a.ctypes.data_as(C.c_void_p).value
for cin, cout in shapes:
    w = (0.05 * r.standard_normal((cout, cin, 3, 3))).astype(np.float32)
    bias = r.standard_normal(cout).astype(np.float32)
    for B in batches:
        x = r.standard_normal((B, cin, 8, 8)).astype(np.float32)
        out = np.empty((B, cout, 8, 8), np.float32)
        old, new = [], []
        for _ in range(reps):
            ms = C.c_double()
            rc = dbg.dpir_debug_conv_bench(e.h, B, cin, cout, 8, 8, 3, 0, 0, 2, 200, C.byref(ms))
            assert rc == 0, e.lib.dpir_last_error(e.h)
            old.append(ms.value * 1e3)
            d = _lib.Conv9Desc(B=B, Cin=cin, Cout=cout, H=8, W=8, res_mode=-1, hop=0, iters=200)
            d.x, d.w, d.bias, d.out = p(x), p(w), p(bias), p(out)
            rc = dbg.dpir_debug_conv9_layer(e.h, C.byref(d))
            assert rc == 0, e.lib.dpir_last_error(e.h)
            new.append(d.ms_out * 1e3)
        print(f"LAYER9 [{prec}] {cin}->{cout} @8x8 B={B:2d} wg={B * cout // 32:4d}: conv6 route {' '.join(f'{v:6.1f}' for v in old)} us | conv9 {' '.join(f'{v:6.1f}' for v in new)} us", flush=True)
