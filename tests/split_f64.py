"""The f16 operand split of the f16x3 / f16x1 convolution routes, stated in numpy exactly as the kernels do it, and the error model that
follows from the number formats alone (tests/test_split_model_host.py shows that the model is sharp; tests/test_gpu_operand_range.py
holds the kernels to it at every operand magnitude).

The step (csrc/act.hip, csrc/conv_epilogue.h norm_split, conv5 / conv8's own copies), all in fp32:
    bad = !(|v| <= 65000)                     -- true for NaN as well; counted in the engine's guard word
    v   = fminf(fmaxf(v, -65000), 65000)      -- fmaxf / fminf return the other operand for a NaN: a NaN becomes -65000
    hi  = f16(v)                              -- round to nearest even, subnormals kept
    lo  = f16(v - f32(hi))                    -- absent in the one-product mode (f16x1)
The weights are multiplied by the pack's power of two (conv3_f64.weight_scale: max|w| s in [512, 1024)) and split the same way; the
convolution is hi_x hi_w + lo_x hi_w + hi_x lo_w accumulated in fp32 (lo_x lo_w, <= 2^-22 |x||w|, is dropped), un-scaled by 1 / s.

delta(v) = max(2^-22 |v|, 2^-25) bounds |v - hi - lo| for |v| <= 65000.  f16 has 11 significant bits, normal numbers from 2^-14, and
subnormals that are the multiples of 2^-24.
  * hi normal (|v| >= 2^-14): |v - hi| <= half an ulp of hi <= 2^-11 |v|, and r = v - f32(hi) is exact in fp32 (both are multiples of
    ulp24(v) and |r| is below 2^13 of them).
      - lo normal (|r| >= 2^-14): |r - lo| <= 2^-11 |r| <= 2^-22 |v|.
      - lo subnormal (|r| < 2^-14, which every |v| < 2^-3 gives): lo is r rounded to a multiple of 2^-24, |r - lo| <= 2^-25.
  * hi subnormal (|v| < 2^-14): hi is v rounded to a multiple of 2^-24, |r| <= 2^-25, and lo is 0 or +-2^-24 (a tie at 2^-25 rounds to the
    even 0): |v - hi - lo| <= 2^-25.
The error is therefore ABSOLUTE below |v| = 2^-3: the split is not scale free, and a layer whose raw operand is small loses the fp32
equivalence of the three products.  Q(op) is that loss per output element in units of the element's budget S (conv3_f64.budget):
    Q = conv2d(delta(x_prologued), |w|) (times 0.25 where the launch has the device scale) / S.
A kernel of the three-product mode is held to E <= R max(E32, 2^-24) + Q element by element; Q is at most 2^-22 where every operand value
is above 2^-3 and grows like 2^-25 / |x| below."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import conv3_f64 as cf

LIMIT = np.float32(65000.0)
SUB = 2.0 ** -14                  # smallest normal f16
SWEEP_K = (13, 10, 0, -3, -6, -10, -14, -20, -24)


def split(v, x1=False, defect=None):
    """(hi, lo, bad) of fp32 values: hi / lo float16 arrays (lo None for x1), bad the guard's flag per element.
    defect "clamp_65504": a clamp at the largest finite f16 and no flag (what a kernel without the guard would do)."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if defect == "clamp_65504":
            bad = np.zeros(v.shape, bool)
            c = np.fmin(np.fmax(v, np.float32(-65504.0)), np.float32(65504.0))
        else:
            bad = ~(np.abs(v) <= LIMIT)
            c = np.fmin(np.fmax(v, -LIMIT), LIMIT)
        hi = c.astype(np.float16)
        lo = None if x1 else (c - hi.astype(np.float32)).astype(np.float16)
    return hi, lo, bad


def delta(v):
    """The representation error bound of the three-product split, float64 (module docstring)."""
    v = v.abs().to(torch.float64) if isinstance(v, torch.Tensor) else np.abs(np.asarray(v, np.float64))
    return (v * 2.0 ** -22).clamp_min(2.0 ** -25) if isinstance(v, torch.Tensor) else np.maximum(v * 2.0 ** -22, 2.0 ** -25)


def _pad(w):
    return (w.shape[-1] - 1) // 2


def _w4(op):
    """The weight as a conv2d kernel, float64: [Cout][Cin][3][3], or [Cout][Cin] of a 1x1 layer."""
    w = torch.from_numpy(np.ascontiguousarray(op["w"])).to(torch.float64)
    return w if w.dim() == 4 else w[:, :, None, None]


def Q(op, x64=None, S=None):
    """The per-element extra budget of the three-product mode, float64 tensor of the output's shape."""
    if x64 is None:
        x64 = cf.prologued(op, torch.float64)
    w = _w4(op)
    if S is None:
        S = cf.budget(op, x=x64)
    q = F.conv2d(delta(x64), w.abs(), padding=_pad(w))
    if op.get("scaled"):
        q = q * 0.25
    return torch.where(S > 0, q / S, torch.zeros_like(q))


def _flush(h):
    """f16 subnormals to zero"""
    return np.where(np.abs(h.astype(np.float64)) < SUB, np.float16(0), h)


DEFECTS = ("lo_flushed_when_subnormal", "hi_flushed_when_subnormal", "lo_x_hi_w_dropped", "hi_x_lo_w_dropped", "clamp_65504")


def emulate(op, x1=False, defect=None, x64=None):
    """The layer with the operands split as the kernels split them and every sum in float64: what remains against conv3_f64.layer(float64) is
    the format's error alone.  The activation operand is the float64 prologue rounded to fp32 (the kernels hold it in fp32).
    defect: one of DEFECTS -- a flush applies to the stored planes (hi is rounded first, lo taken from the unflushed hi: what a flushing
    reader of correct planes, a matrix instruction for example, would see)."""
    assert defect is None or defect in DEFECTS, defect
    if x64 is None:
        x64 = cf.prologued(op, torch.float64)
    x = x64.to(torch.float32).numpy()
    hx, lx, _ = split(x, x1, defect if defect == "clamp_65504" else None)
    s = cf.weight_scale(op["w"])
    w4 = _w4(op).to(torch.float32).numpy()
    hw, lw, _ = split(w4 * s, x1)
    if defect == "lo_flushed_when_subnormal" and not x1:
        lx, lw = _flush(lx), _flush(lw)
    if defect == "hi_flushed_when_subnormal":
        hx, hw = _flush(hx), _flush(hw)
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    pad = _pad(w4)
    y = F.conv2d(t(hx), t(hw), padding=pad)
    if not x1:
        if defect != "lo_x_hi_w_dropped":
            y = y + F.conv2d(t(lx), t(hw), padding=pad)
        if defect != "hi_x_lo_w_dropped":
            y = y + F.conv2d(t(hx), t(lw), padding=pad)
    y = y / float(s)
    if op.get("scaled"):
        y = y * 0.25
    y = y + torch.from_numpy(op["bias"]).to(torch.float64)[None, :, None, None]
    r = cf.residual(op, torch.float64)
    return y if r is None else y + r


def scaled_op(op, k, wk=0):
    """The operands with xa, xb, bias and res times 2^k (and w times 2^wk): exact in fp32 for the sweep's k.  Bias and residual scale
    with x, otherwise an O(1) bias dominates the budget S and hides the operand's error."""
    out = dict(op)
    for key in ("xa", "xb", "bias", "res"):
        if op.get(key) is not None:
            out[key] = (op[key] * np.float32(2.0 ** k)).astype(np.float32)
    if wk:
        out["w"] = (op["w"] * np.float32(2.0 ** wk)).astype(np.float32)
    return out


def table_scaled_op(op, k):
    """Prologue 1 under the sweep: x times 2^k, the table's mean times 2^k and its scale times 2^-k -- the split operand is unchanged."""
    out = scaled_op(op, k)
    out["bias"], out["res"] = op["bias"], op.get("res")
    t = op["prm"].copy()
    t[..., 0] *= np.float32(2.0 ** k)
    t[..., 1] *= np.float32(2.0 ** -k)
    out["prm"] = t
    return out


def encoded(t):
    """|t| as the matrix instruction's adder sees an f16 operand: a non-zero subnormal counts as 2^-14 (RoundedReference)."""
    a = t.abs()
    return torch.where(a > 0, a.clamp_min(SUB), a)


class RoundedReference:
    """The one-product mode (f16x1) without a prologue: conv3_f64.Reference(op, f16_operands=True) -- the float64 statement on the operands
    rounded to float16 once, subnormals kept -- with the budget the MI355X matrix instruction can be held to at every magnitude.

    What was measured on the MI355X (profiles/operand_range/README.md):
      * v_mfma_f32_*_f16 does NOT flush f16 subnormals and forms their products exactly: operands whose partial sums are all fp32
        numbers (up to 2^20 units) come back bit-exact down to x = m 2^-24 (test_gpu_operand_range.py pins that);
      * with random operands, E against the rounded statement is 7e-8 for operand scales down to 2^-16 and then doubles with every
        halving -- 2.6e-7 at 2^-19, 5.1e-7 at 2^-20, 2.1e-6 at 2^-22, 6.6e-6 at 2^-24 -- on conv5, conv6, conv7, conv9 and conv_up alike:
        an ABSOLUTE rounding step of about 2^-28 in the units of x_16 (w s)_16, where fp32 accumulation alone would round at 2^-33.
    Reading (an inference: no ISA text on the adder's internals is available to this repository): the instruction adds its products
    after aligning them to their ENCODED exponents and keeps 24 bits below the largest; a subnormal is encoded with the exponent of
    2^-14 whatever its leading zeros, so the rounding of the accumulation is relative to max(|x|, 2^-14) |w|, not to |x| |w|.
    So R and E32 stay and the budget changes: |got - ref| <= R max(E32, 2^-24) S_enc, S_enc = conv2d(encoded(x16), encoded(w16)) + |bias|
    + |res|.  S_enc = S wherever no operand is subnormal, and a kernel that flushed subnormals (an error of the order of S itself) is still
    rejected wherever the operand has one (tests/test_split_model_host.py)."""

    def __init__(self, op):
        dt = torch.float64
        s = float(cf.weight_scale(op["w"]))
        x = cf._f16(cf.prologued(op, dt))
        ws = cf._f16(cf._t(op["w"], dt) * s)
        self.ref = cf.layer(op, dt, True)
        self.S = cf.budget(op, True)
        S = F.conv2d(encoded(x), encoded(ws) / s, padding=1)
        if op.get("scaled"):
            S = S * 0.25
        S = S + cf._t(op["bias"], dt).abs()[None, :, None, None]
        r = cf.residual(op, dt)
        self.S_enc = S if r is None else S + r.abs()
        self.base32 = cf.layer(op, torch.float32, True).numpy()
        self.e32, _ = cf.E(self.base32, self.ref, self.S)

    def check(self, got, r, what):
        e, at = cf.E(got, self.ref, self.S)
        e_enc, at_enc = cf.E(got, self.ref, self.S_enc)
        print(f"RANGE {what}: E {e:.3e} at {at}, against the encoded budget {e_enc:.3e} at {at_enc}, E32 {self.e32:.3e} (R {r:g})")
        assert e_enc <= r * max(self.e32, cf.FLOOR), (f"{what}: |got - ref| / S_enc = {e_enc:.3e} at {at_enc} (E = {e:.3e}) > {r:g} x max(E(float32) = "
                                                      f"{self.e32:.3e}, 2^-24)")
        return dict(E=e, E_enc=e_enc, E32=self.e32)


class RangeReference:
    """Float64 statement, budget, fp32 baseline and Q of one layer, computed once (cf.Reference with the model's term)."""

    def __init__(self, op):
        self.op = op
        self.x64 = cf.prologued(op, torch.float64)
        self.ref = cf.layer(op, torch.float64, x=self.x64)
        self.S = cf.budget(op, x=self.x64)
        self.base32 = cf.layer(op, torch.float32).numpy()
        self.e32, _ = cf.E(self.base32, self.ref, self.S)
        self.Q = Q(op, self.x64, self.S)
        self.qmax = float(self.Q.max())

    def measure(self, got, r, with_q=True):
        """E, where, and the worst element's bound; margin = max over elements of err / (r max(E32, floor) + Q), <= 1 passes.
        with_q False: the plain bound r max(E32, floor) -- what a scale-free kernel (fp32) is held to."""
        got = np.asarray(got, np.float64)
        S, ref = self.S.numpy(), self.ref.numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.abs(got - ref) / S
        q = np.where(np.isfinite(got), q, np.inf)
        q = np.where((S == 0) & (got == ref), 0.0, q)
        bound = r * max(self.e32, cf.FLOOR) + (self.Q.numpy() if with_q else np.zeros(q.shape))
        m = q / bound
        i = np.unravel_index(int(np.argmax(m)), m.shape)
        return dict(E=float(q.max()), E32=self.e32, Q=self.qmax, margin=float(m[i]), at=tuple(int(v) for v in i), bound=float(bound[i]))

    def check(self, got, r, what, with_q=True):
        m = self.measure(got, r, with_q)
        print(f"RANGE {what}: E {m['E']:.3e} E32 {m['E32']:.3e} Qmax {m['Q'] if with_q else 0.0:.3e} worst err/bound {m['margin']:.3f} at {m['at']} (R {r:g})")
        assert m["margin"] <= 1.0, (f"{what}: error / (R max(E32, 2^-24){' + Q' if with_q else ''}) = {m['margin']:.3f} at (n, c, h, w) = {m['at']}: E = {m['E']:.3e}, "
                                    f"E32 = {m['E32']:.3e}, bound there {m['bound']:.3e}")
        return m
