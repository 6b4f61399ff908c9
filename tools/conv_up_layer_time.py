"""Back-to-back time of conv1 of the up-sampling ResBlocks of the FFHQ forward, prologue included: the up-sampled planes + launch_conv6 (route 1)
vs the source planes + conv_up (route 0), as a plain layer and as the fused hop with conv2 behind it.  BATCHES=8,16,32  (GPU box only)"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import _lib
prec = os.environ.get("DIFFPIR_PRECISION", "f16x3")
e = diffpir_amd.Engine(0); e.set_precision(prec)
dbg = _lib.load_debug()
r = np.random.default_rng(0)
shapes = [(128, 128), (256, 64), (256, 32)]        # (channels, source size): 128 -> 128 @256^2, 256 -> 256 @128^2, 256 -> 256 @64^2
batches = [int(b) for b in os.environ.get("BATCHES", "16,8,32").split(",")]
reps, iters = 3, int(os.environ.get("ITERS", "20"))
p = lambda a: a.ctypes.data_as(C.c_void_p).value
for c, hs in shapes:
    w = (0.05 * r.standard_normal((c, c, 3, 3))).astype(np.float32)
    w2 = (0.05 * r.standard_normal((c, c, 3, 3))).astype(np.float32)
    bias = r.standard_normal(c).astype(np.float32)
    gamma = np.ones(c, np.float32); beta = np.zeros(c, np.float32)
    for B in batches:
        x = r.standard_normal((B, c, hs, hs)).astype(np.float32)
        out = np.empty((B, c, 2 * hs, 2 * hs), np.float32)
        for hop in (0, 1):
            t = {0: [], 1: []}
            for _ in range(reps):
                for route in (1, 0):
                    d = _lib.ConvUpDesc(B=B, Cin=c, Cout=c, Hs=hs, Ws=hs, hop=hop, force_hop=0, Cout2=c, route=route, iters=iters)
                    d.x, d.w, d.bias, d.out = p(x), p(w), p(bias), p(out)
                    d.gamma2, d.beta2, d.w2, d.bias2, d.out2 = p(gamma), p(beta), p(w2), p(bias), p(out)
                    rc = dbg.dpir_debug_conv_up_layer(e.h, C.byref(d))
                    if rc != 0:
                        t[route].append(float("nan"))
                        print("  refused:", e.lib.dpir_last_error(e.h), flush=True)
                    else:
                        t[route].append(d.ms_out * 1e3)
            what = "act_split + conv1 (hop) + conv2" if hop else "act_split + conv1"
            print(f"LAYERUP [{prec}] {c}->{c} src {hs}^2 B={B:2d} {what}: old route {' '.join(f'{v:7.1f}' for v in t[1])} us | conv_up {' '.join(f'{v:7.1f}' for v in t[0])} us", flush=True)
