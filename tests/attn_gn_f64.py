"""The float64 statements of the attention core and of one GroupNorm + FiLM + SiLU site, forward and backward, and the per-element yardstick
their kernels are held to (tests/test_gpu_attn_gn_layer.py through dpir_debug_attention / dpir_debug_groupnorm; tests/test_attn_gn_checker.py
shows that the yardstick is sharp).  Every statement takes the arithmetic `dt`: the same text in float32 on the CPU is the comparison.

Attention forward (oracle/unet_oracle.py::_attention's core, QKVAttentionLegacy): qkv [B][3C][T] -> (B heads, 192, T), split q | k | v,
  P = softmax_s((q s)^T (k s)), s = 64^-1/4;  out[c][t] = sum_s P[t][s] v[c][s].
Attention backward, the five formulas of launch_attention_bwd (csrc/grad.hip), sc = 1/8:
  P = softmax_s(sc q^T k);  dv[c][s] = sum_t dA[c][t] P[t][s];  dP[t][s] = sum_c dA[c][t] v[c][s];  dS = P (dP - sum_s P dP);
  dq[c][t] = sc sum_s k[c][s] dS[t][s];  dk[c][s] = sc sum_t q[c][t] dS[t][s].
GroupNorm forward, the function value (32 groups, biased variance, eps 1e-5): y = ((x - mean) / sqrt(var + eps) gamma + beta) (1 + scale) + shift;
  the device table {mean, a, b} is applied in float64, (x - mean) a + b, and compared with y.
GroupNorm backward: float64 autograd of resample_mode(act(y(concat(xa, xb)))) with cotangent dA, split back into the two sources;
  ga = (ga_init if acc_a else 0) + extra + dx_a, likewise gb.

Yardstick (the project's, tests/conv3_f64.py): E(got) = max over elements of |got - ref64| / max(S, 2^-102), S the same statement with every
summand replaced by its absolute value, so that a quiet row is not excused by a loud one.  The floor 2^-102 = FLT_MIN 2^24 follows from the
format: a value below float32's normal range that flushes to zero then costs at most 2^-24.  A kernel passes when
E(kernel) <= R max(E(the float32 CPU statement), FLOOR); FLOOR = 2^-24, and 2^-21 for the GroupNorm forward, whose table carries up to five
float32 roundings (mean, rstd, rstd gamma, 1 + scale, the product)."""
import numpy as np
import torch
import torch.nn.functional as F

GN_EPS = 1e-5
HC = 64                                 # head channels
S_FLOOR = 2.0 ** -102
FLOOR = {"attn_fwd": 2.0 ** -24, "attn_bwd": 2.0 ** -24, "gn_fwd": 2.0 ** -21, "gn_bwd": 2.0 ** -24}
# R: conv3_f64.R["f32"], the project's figure for an fp32 kernel that differs from the CPU statement in summation order only.  Not fitted to
# the measurements (profiles/attn_gn/README.md has them); a ratio above it is a finding, and no R goes beyond 8.
R = {"attn_fwd": 4.0, "attn_bwd": 4.0, "gn_fwd": 4.0, "gn_bwd": 4.0}


def _t(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def E(got, ref, S):
    """(max over elements of |got - ref| / max(S, 2^-102), its index); a non-finite element counts as infinite error."""
    got = np.asarray(got, np.float64)
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    S = S.numpy() if isinstance(S, torch.Tensor) else np.asarray(S, np.float64)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.abs(got - ref) / np.maximum(S, S_FLOOR)
    q = np.where(np.isfinite(got), q, np.inf)
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[i]), tuple(int(v) for v in i)


class Held:
    """One output against its float64 statement: ref, S and the float32 baseline, computed once."""

    def __init__(self, group, ref, S, base32):
        self.group, self.ref, self.S = group, ref, S
        self.base32 = base32.numpy() if isinstance(base32, torch.Tensor) else base32
        self.e32, self.at32 = E(self.base32, ref, S)

    def bound(self):
        return R[self.group] * max(self.e32, FLOOR[self.group])

    def measure(self, got):
        e, at = E(got, self.ref, self.S)
        return dict(E=e, at=at, E32=self.e32, ratio=e / max(self.e32, FLOOR[self.group]))

    def accepts(self, got):
        return E(got, self.ref, self.S)[0] <= self.bound()

    def check(self, got, what):
        m = self.measure(got)
        print(f"ATTN_GN {what}: E {m['E']:.3e} at {m['at']}, E(float32) {m['E32']:.3e}, ratio {m['ratio']:.3f} (R {R[self.group]:g})")
        at = m["at"]
        assert m["E"] <= self.bound(), (
            f"{what}: E = {m['E']:.3e} at {at} (got {float(np.asarray(got)[at])!r}, float64 {float(self.ref[at])!r}, budget {float(self.S[at]):.3e}) "
            f"> {R[self.group]:g} x max(E(float32) = {self.e32:.3e}, floor {FLOOR[self.group]:.3e})")
        return m


# ------------------------------------------------------------------------------------------------ attention: inputs
ATTN_FAMILIES = ("mild", "peaked", "offset200", "ascending", "descending", "late_winner", "neg_last_tile")


def attn_inputs(family, B, C, T, seed):
    """(qkv [B][3C][T] in the legacy order, dAtt [B][C][T]), float32.  q, k, v ~ N(0, 1) plus what the family adds to every head:
    peaked: q, k x 4;  offset200: channel 0 of q = 40, of k = 40 + 0.01 s (logits near +200);  ascending / descending: q0 = 8, k0 = linspace(-/+30, +/-30)
    (the running maximum rises in every tile / is found in the first);  late_winner: q0 = 10, k0 = 0 except the last key = 100 (alpha ~ 0 in the last
    tile);  neg_last_tile: q0 = -10, k0 = 0 except the last four keys = 100 (probabilities that underflow in the last tile)."""
    assert family in ATTN_FAMILIES and C % HC == 0
    r = np.random.default_rng(seed)
    nh = C // HC
    x = r.standard_normal((B, nh, 3, HC, T)).astype(np.float32)
    q, k = x[:, :, 0], x[:, :, 1]
    s = np.arange(T, dtype=np.float32)
    if family == "peaked":
        q *= 4; k *= 4
    elif family == "offset200":
        q[:, :, 0, :] = 40.0; k[:, :, 0, :] = 40.0 + 0.01 * s
    elif family in ("ascending", "descending"):
        sign = 1.0 if family == "ascending" else -1.0
        q[:, :, 0, :] = 8.0; k[:, :, 0, :] = np.linspace(-30.0 * sign, 30.0 * sign, T, dtype=np.float32)
    elif family == "late_winner":
        q[:, :, 0, :] = 10.0; k[:, :, 0, :] = 0.0; k[:, :, 0, -1] = 100.0
    elif family == "neg_last_tile":
        q[:, :, 0, :] = -10.0; k[:, :, 0, :] = 0.0; k[:, :, 0, -4:] = 100.0
    return np.ascontiguousarray(x.reshape(B, 3 * C, T)), r.standard_normal((B, C, T)).astype(np.float32)


def _heads(qkv, dt):
    t = _t(qkv, dt) if isinstance(qkv, np.ndarray) else qkv
    B, C3, T = t.shape
    return t.reshape(B * (C3 // (3 * HC)), 3 * HC, T).split(HC, dim=1)


# ------------------------------------------------------------------------------------------------ attention: statements
def attn_forward(qkv, dt=torch.float64):
    """out [B][C][T]."""
    q, k, v = _heads(qkv, dt)
    s = 1.0 / np.sqrt(np.sqrt(float(HC)))
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
    B, C3, T = qkv.shape
    return torch.einsum("bts,bcs->bct", w, v).reshape(B, C3 // 3, T)


def attn_forward_budget(qkv):
    q, k, v = _heads(qkv, torch.float64)
    s = 1.0 / np.sqrt(np.sqrt(float(HC)))
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
    B, C3, T = qkv.shape
    return torch.einsum("bts,bcs->bct", w, v.abs()).reshape(B, C3 // 3, T)


def attn_backward(qkv, dAtt, dt=torch.float64, budget=False):
    """(dq, dk, dv), each [B heads][64][T]; budget: the same formulas with every summand replaced by its absolute value (P is positive)."""
    q, k, v = _heads(qkv, dt)
    dA = _t(dAtt, dt).reshape(q.shape)
    sc = 0.125
    P = torch.softmax(sc * torch.einsum("bct,bcs->bts", q, k), dim=-1)
    if budget:
        q, k, v, dA = q.abs(), k.abs(), v.abs(), dA.abs()
    dv = torch.einsum("bct,bts->bcs", dA, P)
    dP = torch.einsum("bct,bcs->bts", dA, v)
    d = (P * dP).sum(dim=-1, keepdim=True)
    dS = P * (dP + d) if budget else P * (dP - d)
    dq = sc * torch.einsum("bcs,bts->bct", k, dS)
    dk = sc * torch.einsum("bct,bts->bcs", q, dS)
    return dq, dk, dv


def split_dqkv(dqkv):
    """dqkv [B][3C][T] (legacy order) -> (dq, dk, dv), each [B heads][64][T]."""
    B, C3, T = dqkv.shape
    x = np.asarray(dqkv).reshape(B * (C3 // (3 * HC)), 3, HC, T)
    return x[:, 0], x[:, 1], x[:, 2]


def attn_autograd(qkv, dAtt):
    """float64 autograd of the forward statement: the cross-check of the explicit backward formulas."""
    t = _t(qkv, torch.float64).requires_grad_(True)
    out = attn_forward(t, torch.float64)
    g, = torch.autograd.grad(out, t, _t(dAtt, torch.float64))
    return split_dqkv(g.numpy())


class AttnReference:
    """Held statements of one attention case: out, dq, dk, dv."""

    def __init__(self, qkv, dAtt):
        self.out = Held("attn_fwd", attn_forward(qkv), attn_forward_budget(qkv), attn_forward(qkv, torch.float32))
        ref, S, b32 = attn_backward(qkv, dAtt), attn_backward(qkv, dAtt, budget=True), attn_backward(qkv, dAtt, torch.float32)
        self.dq, self.dk, self.dv = (Held("attn_bwd", ref[i], S[i], b32[i]) for i in range(3))


# ------------------------------------------------------------------------------------------------ attention: emulation of csrc/attn.hip
def attn_emulation(qkv, no_key_mask=False, l_not_rescaled=False, o_not_rescaled=False):
    """float32 numpy emulation of attention_kernel's algorithm: keys in tiles of 32 with a zero-filled tail, scores masked to -inf beyond T,
    running maximum with the alpha rescale of the running sum and of the output accumulator, one division at the end.  (All queries of a
    head at once: a wave's 32 queries do not interact.)  The three switches plant the defects the online softmax can have."""
    f = np.float32
    x = np.asarray(qkv, f)
    B, C3, T = x.shape
    x = x.reshape(-1, 3, HC, T)
    scale = f(1.0 / np.sqrt(np.sqrt(float(HC))))
    q, k, v = x[:, 0] * scale, x[:, 1] * scale, x[:, 2]
    n = x.shape[0]
    o = np.zeros((n, HC, T), f)
    m_run = np.full((n, T), -np.inf, f)
    l_run = np.zeros((n, T), f)
    with np.errstate(over="ignore", invalid="ignore"):
        for s0 in range(0, T, 32):
            live = min(32, T - s0)
            kt = np.zeros((n, HC, 32), f); vt = np.zeros((n, HC, 32), f)
            kt[:, :, :live], vt[:, :, :live] = k[:, :, s0:s0 + live], v[:, :, s0:s0 + live]
            st = np.zeros((n, 32, T), f)                                    # S^T[s][t], channels added in ascending order
            for c in range(HC):
                st += kt[:, c, :, None] * q[:, c, None, :]
            if not no_key_mask:
                st[:, live:, :] = -np.inf
            m_new = np.maximum(m_run, st.max(axis=1))
            alpha = np.exp(m_run - m_new).astype(f)
            p = np.exp(st - m_new[:, None, :]).astype(f)
            ps = p.sum(axis=1, dtype=f)
            l_run = (l_run if l_not_rescaled else l_run * alpha) + ps
            m_run = m_new
            if not o_not_rescaled:
                o *= alpha[:, None, :]
            for s in range(32):
                o += vt[:, :, s, None] * p[:, None, s, :]
        o = o * (f(1.0) / l_run)[:, None, :]
    return o.reshape(B, C3 // 3, T)


# ------------------------------------------------------------------------------------------------ GroupNorm: inputs
GN_KINDS = ("mild", "offset", "const", "tinyvar", "outlier")


def gn_inputs(kind, B, ca, cb, Hs, Ws, seed, mode=0, film=True):
    """float32 operands of one site.  x (the concat) ~ N(0, 1), and per kind: offset 30 + 0.5 N (a group mean far from zero); const: group 0
    constant 3.25 (variance exactly zero: rstd = 1 / sqrt(eps)); tinyvar 1e-4 N; outlier: one entry of 1e4.  gamma = 1 + 0.2 N, beta = 0.1 N,
    FiLM rows 0.3 N, dA ~ N(0, 1) at the resolution `mode` implies."""
    assert kind in GN_KINDS
    r = np.random.default_rng(seed)
    C = ca + cb
    x = r.standard_normal((B, C, Hs, Ws))
    if kind == "offset":
        x = 30.0 + 0.5 * x
    elif kind == "const":
        x[:, :C // 32] = 3.25
    elif kind == "tinyvar":
        x = 1e-4 * x
    elif kind == "outlier":
        x[0, C // 2, Hs // 2, Ws // 3] = 1e4
    x = x.astype(np.float32)
    Ho, Wo = (2 * Hs, 2 * Ws) if mode == 1 else ((Hs // 2, Ws // 2) if mode == 2 else (Hs, Ws))
    return dict(B=B, ca=ca, cb=cb, Hs=Hs, Ws=Ws, mode=mode, silu=1, acc_a=0, acc_b=0,
                xa=np.ascontiguousarray(x[:, :ca]), xb=np.ascontiguousarray(x[:, ca:]) if cb else None,
                gamma=(1 + 0.2 * r.standard_normal(C)).astype(np.float32), beta=(0.1 * r.standard_normal(C)).astype(np.float32),
                film=(0.3 * r.standard_normal((B, 2 * C))).astype(np.float32) if film else None,
                dA=r.standard_normal((B, C, Ho, Wo)).astype(np.float32), ga_init=None, gb_init=None, extra=None)


def _concat(op, dt):
    x = _t(op["xa"], dt)
    return x if op.get("xb") is None else torch.cat([x, _t(op["xb"], dt)], dim=1)


# ------------------------------------------------------------------------------------------------ GroupNorm: statements
def _normalise(x):
    B = x.shape[0]
    g = x.reshape(B, 32, -1)
    mean = g.mean(dim=2, keepdim=True)
    var = ((g - mean) ** 2).mean(dim=2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    return ((g - mean) * rstd).reshape(x.shape), mean[:, :, 0], rstd[:, :, 0]


def _affine(op, dt):
    """(multiplier, offset) per (image, channel) behind x_hat: gamma (1 + scale), beta (1 + scale) + shift; and |beta (1 + scale)| + |shift|."""
    g, b = _t(op["gamma"], dt)[None, :], _t(op["beta"], dt)[None, :]
    C = g.shape[1]
    if op.get("film") is None:
        return g, b, b.abs()
    f = _t(op["film"], dt)
    sc, sh = 1 + f[:, :C], f[:, C:]
    return g * sc, b * sc + sh, (b * sc).abs() + sh.abs()


def gn_forward(op, dt=torch.float64, x=None):
    """y [B][C][Hs][Ws] (before SiLU), in dt."""
    x = _concat(op, dt) if x is None else x
    xh, _, _ = _normalise(x)
    B, C = x.shape[:2]
    g, b = _t(op["gamma"], dt)[None, :, None, None], _t(op["beta"], dt)[None, :, None, None]
    y = xh * g + b
    if op.get("film") is not None:
        f = _t(op["film"], dt)
        y = y * (1 + f[:, :C, None, None]) + f[:, C:, None, None]
    return y


def gn_forward_budget(op):
    x = _concat(op, torch.float64)
    xh, _, _ = _normalise(x)
    m, _, babs = _affine(op, torch.float64)
    return (xh * m[:, :, None, None]).abs() + babs[:, :, None, None].expand(x.shape)


def gn_stats(op):
    """float64 (mean, rstd) [B][32]."""
    _, mean, rstd = _normalise(_concat(op, torch.float64))
    return mean.numpy(), rstd.numpy()


def apply_table(op, prm):
    """The table {mean, a, b, flag} [B][C][4] applied in float64: (x - mean) a + b."""
    x = _concat(op, torch.float64)
    t = _t(np.asarray(prm, np.float32), torch.float64)
    return ((x - t[:, :, 0, None, None]) * t[:, :, 1, None, None] + t[:, :, 2, None, None]).numpy()


def table_emulation(op, clamp=True, drop_shift=False, moments32=False):
    """float32 emulation of gn_prm_kernel's table [B][C][4]: float64 sums, var = E[x^2] - mean^2 clamped at zero, then float32 mean, rstd,
    a = rstd gamma (1 + scale), b = beta (1 + scale) + shift.  moments32: the two moments are rounded to float32 before the variance is formed
    (the situation the clamp exists for); clamp / drop_shift plant the two defects."""
    f = np.float32
    x = _concat(op, torch.float64).numpy()
    B, C = x.shape[:2]
    g = x.reshape(B, 32, -1)
    mean, m2 = g.mean(axis=2), (g * g).mean(axis=2)
    if moments32:
        mean, m2 = mean.astype(f).astype(np.float64), m2.astype(f).astype(np.float64)
    var = m2 - mean * mean
    if clamp:
        var = np.maximum(var, 0.0)
    with np.errstate(invalid="ignore"):
        rstd = (1.0 / np.sqrt(var + GN_EPS)).astype(f)
    mean = mean.astype(f)
    cg = C // 32
    a = np.repeat(rstd, cg, axis=1) * op["gamma"][None, :].astype(f)
    b = np.broadcast_to(op["beta"][None, :].astype(f), (B, C)).copy()
    if op.get("film") is not None:
        sc = f(1.0) + op["film"][:, :C].astype(f)
        a = a * sc
        b = b * sc + (f(0.0) if drop_shift else op["film"][:, C:].astype(f))
    prm = np.empty((B, C, 4), f)
    prm[..., 0], prm[..., 1], prm[..., 2], prm[..., 3] = np.repeat(mean, cg, axis=1), a, b, f(op.get("silu", 1))
    return prm


def _resample(y, mode):
    return F.interpolate(y, scale_factor=2, mode="nearest") if mode == 1 else (F.avg_pool2d(y, 2) if mode == 2 else y)


def gn_backward(op, dt=torch.float64):
    """(ga, gb): autograd of resample(act(y(x))) in dt with cotangent dA, plus the prior contents where the site accumulates and `extra`."""
    x = _concat(op, dt).requires_grad_(True)
    y = gn_forward(op, dt, x=x)
    if op.get("silu", 1):
        y = y * torch.sigmoid(y)
    dx, = torch.autograd.grad(_resample(y, op.get("mode", 0)), x, _t(op["dA"], dt))
    ca = op["ca"]
    ga, gb = dx[:, :ca], dx[:, ca:]
    if op.get("extra") is not None:
        ga = _t(op["extra"], dt) + ga
    if op.get("acc_a"):
        ga = _t(op["ga_init"], dt) + ga
    if op.get("acc_b") and op.get("xb") is not None:
        gb = _t(op["gb_init"], dt) + gb
    return ga.detach(), (gb.detach() if op.get("xb") is not None else None)


def gn_backward_budget(op):
    """|G| + mean|G| + |x_hat| mean|G x_hat| + |ga_init| + |extra|, G = adj(dA) act'(u) a per element, means over the group."""
    dt = torch.float64
    x = _concat(op, dt)
    B, C = x.shape[:2]
    xh, _, rstd = _normalise(x)
    m, off, _ = _affine(op, dt)
    u = xh * m[:, :, None, None] + off[:, :, None, None]
    a = (m.expand(B, C) * rstd.repeat_interleave(C // 32, dim=1))[:, :, None, None]
    dA, mode = _t(op["dA"], dt).abs(), op.get("mode", 0)
    dAs = 4 * F.avg_pool2d(dA, 2) if mode == 1 else (0.25 * F.interpolate(dA, scale_factor=2, mode="nearest") if mode == 2 else dA)
    act = torch.ones_like(u)
    if op.get("silu", 1):
        sg = torch.sigmoid(u)
        act = (sg * (1 + u * (1 - sg))).abs()
    G = dAs * act * a.abs()
    grp = lambda t: t.reshape(B, 32, -1).mean(dim=2).repeat_interleave(C // 32, dim=1)[:, :, None, None]
    S = G + grp(G) + xh.abs() * grp(G * xh.abs())
    ca = op["ca"]
    Sa, Sb = S[:, :ca].clone(), S[:, ca:].clone()
    if op.get("extra") is not None:
        Sa += _t(op["extra"], dt).abs()
    if op.get("acc_a"):
        Sa += _t(op["ga_init"], dt).abs()
    if op.get("acc_b") and op.get("xb") is not None:
        Sb += _t(op["gb_init"], dt).abs()
    return Sa, (Sb if op.get("xb") is not None else None)


class GnReference:
    """Held statements of one GroupNorm case: the forward value, ga, gb (None without a second source), and the float64 statistics."""

    def __init__(self, op):
        self.y = Held("gn_fwd", gn_forward(op), gn_forward_budget(op), gn_forward(op, torch.float32))
        self.mean, self.rstd = gn_stats(op)
        ref, S, b32 = gn_backward(op), gn_backward_budget(op), gn_backward(op, torch.float32)
        self.ga = Held("gn_bwd", ref[0], S[0], b32[0])
        self.gb = None if ref[1] is None else Held("gn_bwd", ref[1], S[1], b32[1])

    def check_stats(self, stats, op, what):
        """stats_out [B][32][2] = {mean, rstd}: float64 sums rounded to float32 once.  rstd: the variance is formed as E[x^2] - mean^2 in float64, whose
        cancellation error 2^-52 E[x^2] is relative to var + eps; then one float32 rounding, 2^-24 -- a factor of two on top.  mean: one rounding."""
        stats = np.asarray(stats, np.float64)
        x = _concat(op, torch.float64).numpy()
        m2 = (x * x).reshape(x.shape[0], 32, -1).mean(axis=2)
        rb = 2.0 ** -23 + 2.0 ** -51 * m2 * self.rstd ** 2
        er = np.abs(stats[..., 1] - self.rstd) / self.rstd
        em = np.abs(stats[..., 0] - self.mean)
        mb = 2.0 ** -23 * np.abs(self.mean) + 2.0 ** -50 * np.sqrt(m2)
        print(f"ATTN_GN {what}: rstd off by {er.max():.3e} (relative), mean by {em.max():.3e}")
        assert np.isfinite(stats).all() and (er <= rb).all() and (em <= mb).all(), f"{what}: rstd {er.max():.3e}, mean {em.max():.3e}"
