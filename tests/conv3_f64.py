"""The float64 statement of one 3x3 convolution layer of the UNet and the per-element yardstick the layer kernels are held to
(tests/test_gpu_conv3_layer.py through dpir_debug_conv3_layer; tests/test_conv3_checker.py shows that the yardstick is sharp).

The layer, as the forward runs it (oracle/unet_oracle.py: in_layers / out_layers of a ResBlock, `out`):
  1. concatenate the two sources along the channels;
  2. apply the prologue AT THE SOURCE RESOLUTION: the table form `(x - mean) * a + b`, then SiLU if flagged, or GroupNorm32 (32 groups, biased
     variance, eps 1e-5, affine), FiLM `y * (1 + scale) + shift`, SiLU;
  3. resample: nearest x2 up-sampling (mode 1) or the 2x2 mean (mode 2).  The oracle's ResBlock normalises and activates before `h_upd`, so
     the 2x2 mean is taken of ACTIVATED values; for the nearest mode and for a table without SiLU the two orders are the same function;
  4. conv2d with zero padding 1, plus the bias;
  5. plus the residual: same shape, nearest-up of a half-resolution tensor, or the 2x2 mean of a double-resolution one;
  6. where the launch carries a device output scale (0.25), it multiplies the convolution sum of step 4, not the bias or the residual:
     Conv6Args::out_scale_dev is folded into the un-scaling of the weight pack, which the epilogue applies to the accumulators before it
     adds bias and residual.  Its one user, the dgrad route (unet_bwd.hip), passes a zero bias and no residual, where this is the same
     function as scaling the whole output; the layer tests run it with a bias and a residual so that the order is pinned as well.

Yardstick: E(got) = max over elements of |got - ref64| / S, S = conv2d(|x_prologued|, |w|) + |bias| + |res_resampled| (the convolution term
times 0.25 where the output's is), i.e. every element is measured against the magnitude of the terms that were summed into it: a border pixel or a quiet channel is
not excused by a loud one.  A kernel passes when E(kernel) <= R * max(E(the same statement in float32 on the CPU), 2^-24)."""
import numpy as np
import torch
import torch.nn.functional as F

GN_EPS = 1e-5
FLOOR = 2.0 ** -24
# R per precision mode: twice the largest E(kernel) / E(float32) measured on the MI355X over every case of tests/test_gpu_conv3_layer.py,
# rounded up to a power of two, at most 4 (f32) / 16 (f16x3) -- profiles/conv3_layer/README.md has the table.  f16x3: largest ratio 3.12 -> 8.
# f32: largest ratio 3.79, which the rule would turn into 8; that is above the ceiling, so 4 stays and the ratio is explained instead: the fp32
# kernel adds the Cin * 9 products of an output into one accumulator in sequence, the CPU convolution in blocked partial sums, so the ratio
# grows like sqrt(Cin) (0.8 at Cin 16, 1.9 at 32, 3.4 - 3.8 at 64) and falls to 0.65 where the kernel splits K (Cin 512).
R = {"f32": 4.0, "f16x3": 8.0}
R["f16x1"] = R["f32"]           # against the f16-rounded statement (rounded_operands): what remains is fp32 accumulation order


def _t(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def _pool(x):
    return F.avg_pool2d(x, 2)


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def _silu(x):
    return x * torch.sigmoid(x)


def group_norm_film_silu(x, gamma, beta, film):
    """GroupNorm32 (biased variance, eps 1e-5) + affine, FiLM rows [B][2C] = {scale, shift}, SiLU -- in x's dtype."""
    B, C = x.shape[:2]
    g = x.reshape(B, 32, -1)
    mean = g.mean(dim=2, keepdim=True)
    var = ((g - mean) ** 2).mean(dim=2, keepdim=True)
    y = ((g - mean) / torch.sqrt(var + GN_EPS)).reshape(x.shape)
    y = y * gamma[None, :, None, None] + beta[None, :, None, None]
    if film is not None:
        y = y * (1 + film[:, :C, None, None]) + film[:, C:, None, None]
    return _silu(y)


def prologued(op, dt=torch.float64):
    """Steps 1-3: the convolution's input operand at the output resolution."""
    x = _t(op["xa"], dt)
    if op.get("xb") is not None:
        x = torch.cat([x, _t(op["xb"], dt)], dim=1)
    pro = op.get("prologue", 0)
    if pro == 1:
        t = _t(op["prm"], dt)
        x = (x - t[:, :, 0, None, None]) * t[:, :, 1, None, None] + t[:, :, 2, None, None]
        if float(op["prm"][0, 0, 3]) != 0.0:
            x = _silu(x)
    elif pro == 2:
        x = group_norm_film_silu(x, _t(op["gamma"], dt), _t(op["beta"], dt), _t(op.get("film"), dt))
    mode = op.get("mode", 0)
    return _up(x) if mode == 1 else (_pool(x) if mode == 2 else x)


def residual(op, dt=torch.float64):
    rm = op.get("res_mode", -1)
    if rm < 0:
        return None
    r = _t(op["res"], dt)
    return _up(r) if rm == 1 else (_pool(r) if rm == 2 else r)


def weight_scale(w):
    """pack_weights_conv6 / pack_weights_conv8: the power of two that puts max|w| * scale into [512, 1024) (fp32 arithmetic)."""
    mx = np.float32(np.abs(w).max())
    if mx == 0:
        return np.float32(1.0)
    s = np.float32(2.0) ** np.floor(np.log2(np.float32(1024.0) / mx, dtype=np.float32))
    while mx * s >= np.float32(1024.0):
        s = s * np.float32(0.5)
    return np.float32(s)


def _f16(t):
    return t.to(torch.float32).to(torch.float16).to(t.dtype)


def layer(op, dt=torch.float64, f16_operands=False, x=None):
    """Steps 1-6 in dtype dt.  f16_operands: the single-product statement -- the activation operand (after the prologue, float32 as the kernels
    hold it) and the weights (after the pack's power-of-two scale) rounded to float16 before the convolution."""
    if x is None:
        x = prologued(op, dt)
    w = _t(op["w"], dt)
    if f16_operands:
        s = float(weight_scale(op["w"]))
        x, w = _f16(x), _f16(w * s) / s
    y = F.conv2d(x, w, padding=1)
    if op.get("scaled"):
        y = y * 0.25
    y = y + _t(op["bias"], dt)[None, :, None, None]
    r = residual(op, dt)
    return y if r is None else y + r


def budget(op, f16_operands=False, x=None):
    """S: the magnitude of the terms summed into each output element, float64."""
    dt = torch.float64
    if x is None:
        x = prologued(op, dt)
    w = _t(op["w"], dt)
    if f16_operands:
        s = float(weight_scale(op["w"]))
        x, w = _f16(x), _f16(w * s) / s
    S = F.conv2d(x.abs(), w.abs(), padding=1)
    if op.get("scaled"):
        S = S * 0.25
    S = S + _t(op["bias"], dt).abs()[None, :, None, None]
    r = residual(op, dt)
    return S if r is None else S + r.abs()


def E(got, ref, S):
    """(max over elements of |got - ref| / S, its index (n, c, h, w)); a non-finite element counts as infinite error."""
    got = np.asarray(got, np.float64)
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    S = S.numpy() if isinstance(S, torch.Tensor) else np.asarray(S, np.float64)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(got - ref) / S
    q = np.where(np.isfinite(got), q, np.inf)
    q = np.where((S == 0) & (got == ref), 0.0, q)
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[i]), tuple(int(v) for v in i)


class Reference:
    """The float64 statement of one layer with its budget and the float32 baseline, computed once and shared between the precisions."""

    def __init__(self, op, f16_operands=False):
        self.op, self.f16 = op, f16_operands
        x64 = prologued(op, torch.float64)
        self.ref = layer(op, torch.float64, f16_operands, x=x64)
        self.S = budget(op, f16_operands, x=x64)
        self.base32 = layer(op, torch.float32, f16_operands).numpy()
        self.e32, self.at32 = E(self.base32, self.ref, self.S)

    def measure(self, got):
        e, at = E(got, self.ref, self.S)
        return dict(E=e, at=at, E32=self.e32, ratio=e / max(self.e32, FLOOR))

    def check(self, got, r, what):
        m = self.measure(got)
        print(f"CONV3 {what}: E {m['E']:.3e} at {m['at']}, E(float32) {m['E32']:.3e}, ratio {m['ratio']:.3f} (R {r:g})")
        n, c, h, w = m["at"]
        assert m["E"] <= r * max(self.e32, FLOOR), (
            f"{what}: E = {m['E']:.3e} at (n, c, h, w) = {m['at']} (got {float(np.asarray(got)[n, c, h, w])!r}, float64 {float(self.ref[n, c, h, w])!r}, "
            f"budget {float(self.S[n, c, h, w]):.3e}) > {r:g} x max(E(float32) = {self.e32:.3e}, 2^-24)")
        return m


def second_stage_op(op, first):
    """The layer that follows a deferred split-K layer (Fwd::gn_conv after a split-K conv1): GroupNorm32(gamma2, beta2) + SiLU of the first
    layer's output, then w2 / bias2."""
    return dict(xa=first, xb=None, w=op["w2"], bias=op["bias2"], prologue=2, gamma=op["gamma2"], beta=op["beta2"], film=None, mode=0, res_mode=-1)


class PairReference:
    """Float64 statement of two layers in sequence (the first in float64 all the way), the second layer's budget, and the pair in float32."""

    def __init__(self, op):
        first64 = layer(op, torch.float64)
        op2 = second_stage_op(op, first64.numpy())
        x64 = prologued(op2, torch.float64)
        self.ref = layer(op2, torch.float64, x=x64)
        self.S = budget(op2, x=x64)
        first32 = layer(op, torch.float32).numpy()
        self.base32 = layer(second_stage_op(op, first32), torch.float32).numpy()
        self.e32, self.at32 = E(self.base32, self.ref, self.S)

    measure = Reference.measure
    check = Reference.check


def check_stats(stat, out, what):
    """stat [B][Cout][2] {sum, sum of squares} against the float64 sums of the kernel's OWN fp32 output: fp32 partial sums of at most 256 values
    folded in fp64 (the contract gn_prm relies on) -- 1e-6 of sum |v| and of sum v^2."""
    v = np.asarray(out, np.float64)
    s1, s2, sa = v.sum(axis=(2, 3)), (v * v).sum(axis=(2, 3)), np.abs(v).sum(axis=(2, 3))
    stat = np.asarray(stat, np.float64)
    assert stat.shape == s1.shape + (2,), (stat.shape, s1.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        d1, d2 = np.abs(stat[..., 0] - s1) / sa, np.abs(stat[..., 1] - s2) / s2
    d1, d2 = np.where(np.isfinite(stat[..., 0]), d1, np.inf), np.where(np.isfinite(stat[..., 1]), d2, np.inf)
    i1, i2 = np.unravel_index(int(np.argmax(d1)), d1.shape), np.unravel_index(int(np.argmax(d2)), d2.shape)
    print(f"CONV3STAT {what}: sum {d1[i1]:.2e} of sum|v| at {i1}, sum of squares {d2[i2]:.2e} at {i2}")
    assert d1[i1] <= 1e-6 and d2[i2] <= 1e-6, f"{what}: statistics off by {d1[i1]:.3e} (sum, plane {i1}) / {d2[i2]:.3e} (squares, plane {i2})"
