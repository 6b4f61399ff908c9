"""Cost of the ancestral data step (csrc/ancestral.hip) beside the inpainting data step (csrc/inpaint.hip).  GPU box only.

  * us per dpir_ancestral_step at (16, 256, 256), repaint, device noise (two philox_normal4 per group: the sampler's draw and the next step's mix), and per
    dpir_inpaint_step at the same shape, repaint, device noise, in the same run, the two alternated.  HIP events on the engine stream around REPS
    back-to-back calls after a warm-up set, SETS sets, LEAD calls queued ahead of the first event so that the events see GPU time and not the host's
    issue rate; median and min..max.
  * the algorithmic bytes of each pass, from the shapes: ancestral -- x read and written, two of the six planes of the network output (eps and v),
    y, mask (uint8): 4 + 4 + 8 + 4 + 1 = 21 bytes per element; inpaint (repaint) -- x read and written, eps, y, mask: 17 bytes per element.
  * bytes over time, and that over the 8.0 TB/s HBM3E peak of the MI355X.  Both passes are bound by memory, not by arithmetic, if they are near the
    ~6.3 TB/s a float4 copy reaches; the Philox draws and expf are what can push them off it.
usage: python tools/ancestral_time.py
"""
import ctypes as C
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffpir_amd
from diffpir_amd import schedule

REPS, SETS, LEAD = 20, 7, 16
HBM_PEAK = 8.0e12
e = diffpir_amd.Engine(0)
stream = torch.cuda.ExternalStream(e.lib.dpir_stream(e.h))
lib, h = e.lib, e.h


def timed(fn, lead):
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


_, _, arows = schedule.build_ancestral_rows(iter_num=20)
_, _, irows = schedule.build_inpaint_rows(iter_num=20, iter_num_U=1, sigma=0.05, lambda_=1.0, zeta=0.5, eta=0.0)
arow, irow = arows[5], irows[5]
assert arow.nonzero and arow.mix_next and irow.mix_next and not irow.last
rng = np.random.default_rng(0)
B = 16
H = W = 256
sh, numel = (B, 3, H, W), B * 3 * H * W
x = e.to_device(rng.standard_normal(sh).astype(np.float32))
out6 = e.to_device(np.concatenate([rng.standard_normal(sh), rng.uniform(-1, 1, sh)], axis=1).astype(np.float32))
y = e.to_device(rng.random(sh).astype(np.float32)); m = e.to_device((rng.random(sh) < 0.5).astype(np.uint8), np.uint8)


def ancestral():
    e._check(lib.dpir_ancestral_step(h, x.ptr, out6.ptr, 6, y.ptr, m.ptr, C.byref(arow), 1, 0, None, None, 1, 0, 0, None, B, H, W))


def inpaint():
    e._check(lib.dpir_inpaint_step(h, x.ptr, out6.ptr, 6, y.ptr, m.ptr, C.byref(irow), 1, 1.0, None, None, None, None, 1, 0, 0, None, B, H, W))


res = {"ancestral": [], "inpaint": []}
for _ in range(3):                      # alternated: the two passes see the same machine
    res["ancestral"].append(timed(ancestral, ancestral))
    res["inpaint"].append(timed(inpaint, inpaint))
for name, per_elem in (("ancestral", 21), ("inpaint", 17)):
    med = float(np.median([r[0] for r in res[name]])); lo = min(r[1] for r in res[name]); hi = max(r[2] for r in res[name])
    moved = numel * per_elem
    print(f"dpir_{name}_step ({B}, 256, 256) repaint, device noise: {med:.1f} us ({lo:.1f}..{hi:.1f}) | {moved / 1e6:.1f} MB algorithmic "
          f"({per_elem} B/element) | {moved / med / 1e6:.2f} TB/s | {100 * moved / (med * 1e-6) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak")
