"""CPU: the yardstick of tests/attn_gn_f64.py is sharp.  For the attention core a float32 numpy emulation of csrc/attn.hip's algorithm plays the
kernel: clean it passes on every input family, and each of three defects the online softmax can have -- no key mask, the running sum not
rescaled, the output accumulator not rescaled -- is rejected on at least one.  The missing key mask is rejected on every ragged T of the mild family and passes at
T = 64 and T = 256: the sizes the whole-network tests run cannot see it, which is why tests/test_gpu_attn_gn_layer.py runs ragged T.  For
GroupNorm a float32 emulation of the table plays the kernel; an unclamped variance and a dropped FiLM shift are rejected.  The explicit
backward formulas of the attention are tied to float64 autograd of the forward statement."""
import numpy as np
import pytest
import torch

from tests import attn_gn_f64 as ag

# (family, T): every family, ragged and whole tiles
ATTN_CASES = [("mild", 8), ("mild", 36), ("mild", 64), ("mild", 100), ("mild", 160), ("mild", 256), ("peaked", 36), ("peaked", 100),
              ("offset200", 100), ("ascending", 100), ("descending", 100), ("late_winner", 100), ("neg_last_tile", 100)]
_cache = {}


def _case(family, T):
    if (family, T) not in _cache:
        qkv, dA = ag.attn_inputs(family, 2, 64, T, seed=1000 + T + 7 * ag.ATTN_FAMILIES.index(family))
        _cache[(family, T)] = (qkv, dA, ag.AttnReference(qkv, dA))
    return _cache[(family, T)]


@pytest.mark.parametrize("family,T", ATTN_CASES)
def test_float32_statement_and_clean_emulation_pass(family, T):
    qkv, dA, ref = _case(family, T)
    m = ref.out.check(ref.out.base32, f"float32 statement {family} T {T}")
    assert m["ratio"] <= 1.0
    m = ref.out.check(ag.attn_emulation(qkv), f"clean emulation {family} T {T}")
    for h, name in ((ref.dq, "dq"), (ref.dk, "dk"), (ref.dv, "dv")):
        h.check(h.base32, f"float32 backward {name} {family} T {T}")
    # the baseline is a float32 rounding-level number wherever the softmax is not sharp; a sharp softmax amplifies the logits' rounding
    assert ref.out.e32 < (2.0 ** -18 if family == "mild" else 1e-3)


def test_backward_formulas_equal_float64_autograd():
    worst = 0.0
    for family, T in ATTN_CASES:
        qkv, dA, ref = _case(family, T)
        for h, g in zip((ref.dq, ref.dk, ref.dv), ag.attn_autograd(qkv, dA)):
            worst = max(worst, float(np.abs(h.ref.numpy() - g).max()))
    print(f"explicit formulas vs float64 autograd: largest absolute difference {worst:.3e}")
    assert worst < 1e-11
    # two heads, legacy order: heads first, then q | k | v
    qkv, dA = ag.attn_inputs("mild", 3, 128, 36, seed=5)
    ref = ag.attn_backward(qkv, dA)
    for a, g in zip(ref, ag.attn_autograd(qkv, dA)):
        assert float(np.abs(a.numpy() - g).max()) < 1e-12


def test_forward_statement_is_the_oracles_attention_core():
    """oracle/unet_oracle.py::_attention with an identity qkv projection and a zero proj_out returns its input, so the core cannot be reached
    through it; the block is run with an identity proj_out instead: out - x = core(qkv_conv(GroupNorm(x)))."""
    from oracle import unet_oracle as uo
    import torch.nn.functional as F
    r = np.random.default_rng(6)
    c, T = 128, 36
    x = torch.from_numpy(r.standard_normal((3, c, 6, 6)))
    sd = {"a.norm.weight": torch.ones(c, dtype=torch.float64), "a.norm.bias": torch.zeros(c, dtype=torch.float64),
          "a.qkv.weight": torch.from_numpy(0.3 * r.standard_normal((3 * c, c, 1))), "a.qkv.bias": torch.from_numpy(r.standard_normal(3 * c)),
          "a.proj_out.weight": torch.eye(c, dtype=torch.float64)[:, :, None], "a.proj_out.bias": torch.zeros(c, dtype=torch.float64)}
    out = uo._attention(sd, "a", x, 64, torch.float64)
    qkv = F.conv1d(F.group_norm(x.reshape(3, c, T), 32, sd["a.norm.weight"], sd["a.norm.bias"], eps=1e-5), sd["a.qkv.weight"], sd["a.qkv.bias"])
    want = (out - x).reshape(3, c, T)
    assert float((ag.attn_forward(qkv.numpy()) - want).abs().max()) < 1e-13


MUTATIONS = ("no_key_mask", "l_not_rescaled", "o_not_rescaled")


def test_each_mutation_is_rejected_somewhere_and_the_key_mask_only_on_ragged_T():
    rejected = {m: [] for m in MUTATIONS}
    for family, T in ATTN_CASES:
        qkv, _, ref = _case(family, T)
        for mut in MUTATIONS:
            got = ag.attn_emulation(qkv, **{mut: True})
            e, at = ag.E(got, ref.out.ref, ref.out.S)
            print(f"{mut} {family} T {T}: E {e:.3e} (bound {ref.out.bound():.3e})")
            if not ref.out.accepts(got):
                rejected[mut].append((family, T))
    for mut in MUTATIONS:
        assert rejected[mut], mut
    # an unmasked tail key has logit 0: it weighs exp(-max) and vanishes under a sharp softmax -- the mild ragged sizes are the ones that see it
    ragged = [(f, T) for f, T in ATTN_CASES if T % 32 and f == "mild"]
    assert all(c in rejected["no_key_mask"] for c in ragged), rejected["no_key_mask"]
    assert not [c for c in rejected["no_key_mask"] if c[1] % 32 == 0]
    assert ("mild", 64) not in rejected["no_key_mask"] and ("mild", 256) not in rejected["no_key_mask"]
    # the rescale defects need a maximum that rises after the first tile
    assert ("peaked", 100) in rejected["o_not_rescaled"] and ("late_winner", 100) in rejected["l_not_rescaled"]


def test_underflow_floor():
    """late_winner backward: budgets far below float32's range.  The floor keeps the float32 statement's flushed values at 2^-24 instead of an E of order one."""
    qkv, dA, ref = _case("late_winner", 100)
    assert float(ref.dk.S.min()) < 1e-45             # the losers' columns: every P in them is about exp(-125)
    worst = 0.0
    for h in (ref.dk,):
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.abs(h.base32.astype(np.float64) - h.ref.numpy()) / h.S.numpy()
        worst = max(worst, float(np.nanmax(q)))
        assert h.e32 <= 2.0 ** -24
    print(f"late_winner backward, float32 statement without the floor: {worst:.3e}")
    assert worst > 0.1


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_SHAPE = (2, 64, 0, 5, 7)


@pytest.mark.parametrize("kind", ag.GN_KINDS)
@pytest.mark.parametrize("film", (True, False))
def test_groupnorm_float32_statement_and_table_emulation_pass(kind, film):
    op = ag.gn_inputs(kind, *GN_SHAPE, seed=20 + ag.GN_KINDS.index(kind), film=film)
    ref = ag.GnReference(op)
    ref.y.check(ref.y.base32, f"float32 GroupNorm {kind} film {film}")
    prm = ag.table_emulation(op)
    ref.y.check(ag.apply_table(op, prm), f"table emulation {kind} film {film}")
    ref.ga.check(ref.ga.base32, f"float32 GroupNorm backward {kind} film {film}")
    # the emulated table's own statistics pass the statistics check (mean in column 0; rstd recovered from two-channel groups is not needed:
    # the check is fed the float32-rounded float64 values, which is what the kernel stores)
    ref.check_stats(np.stack([ref.mean.astype(np.float32), ref.rstd.astype(np.float32)], axis=-1), op, f"rounded statistics {kind}")
    if film:
        assert not ref.y.accepts(ag.apply_table(op, ag.table_emulation(op, drop_shift=True)))


def test_groupnorm_statement_matches_torch():
    import torch.nn.functional as F
    op = ag.gn_inputs("offset", 3, 40, 56, 8, 8, seed=31)
    x = torch.cat([torch.from_numpy(op["xa"]), torch.from_numpy(op["xb"])], dim=1).double()
    f = torch.from_numpy(op["film"]).double()
    want = F.group_norm(x, 32, torch.from_numpy(op["gamma"]).double(), torch.from_numpy(op["beta"]).double(), eps=1e-5)
    want = want * (1 + f[:, :96, None, None]) + f[:, 96:, None, None]
    assert float((ag.gn_forward(op) - want).abs().max()) < 1e-11
    mean, rstd = ag.gn_stats(op)
    g = x.reshape(3, 32, -1)
    assert np.allclose(mean, g.mean(dim=2).numpy(), rtol=0, atol=1e-13) and np.allclose(rstd, 1 / np.sqrt(g.var(dim=2, unbiased=False).numpy() + 1e-5), rtol=1e-13)


def test_unclamped_variance_is_rejected():
    """A group that is constant at a value whose square rounds DOWN in float32: with the moments carried in float32 the variance E[x^2] - mean^2 comes out
    below -eps.  Clamped at zero the table is right (the true variance is zero); unclamped it is NaN and the yardstick rejects it."""
    f = np.float32
    v = next(c for c in (f(30.1) + f(0.1) * f(i) for i in range(64))
             if float(f(float(c) ** 2)) - float(c) ** 2 < -2e-5)
    op = ag.gn_inputs("mild", *GN_SHAPE, seed=40)
    op["xa"][:, :2] = v
    ref = ag.GnReference(op)
    ok = ag.apply_table(op, ag.table_emulation(op, moments32=True))
    held = ag.Held("gn_fwd", ref.y.ref[:, :2], ref.y.S[:, :2], ref.y.base32[:, :2])
    held.check(ok[:, :2], "constant group, float32 moments, clamped")
    bad = ag.apply_table(op, ag.table_emulation(op, moments32=True, clamp=False))
    assert not np.isfinite(bad[:, :2]).all() and not held.accepts(bad[:, :2])


def test_groupnorm_backward_statement_resampling_and_accumulation():
    """The backward statement: mode 1 sums the 2 x 2 children, mode 2 spreads a quarter of the parent; prior contents and `extra` are added."""
    for mode, (Hs, Ws) in ((1, (4, 4)), (2, (8, 8))):
        op = ag.gn_inputs("mild", 1, 32, 0, Hs, Ws, seed=50 + mode, mode=mode)
        ga, _ = ag.gn_backward(op)
        dA = torch.from_numpy(op["dA"]).double()
        adj = 4 * torch.nn.functional.avg_pool2d(dA, 2) if mode == 1 else 0.25 * torch.nn.functional.interpolate(dA, scale_factor=2, mode="nearest")
        ga0, _ = ag.gn_backward(dict(op, mode=0, dA=adj.numpy()))
        assert float((ga - ga0).abs().max()) < 1e-12
    op = ag.gn_inputs("mild", 2, 40, 56, 8, 8, seed=53)
    r = np.random.default_rng(54)
    base_a, base_b = ag.gn_backward(op)
    op2 = dict(op, acc_a=1, acc_b=1, ga_init=r.standard_normal(op["xa"].shape).astype(np.float32), gb_init=r.standard_normal(op["xb"].shape).astype(np.float32))
    ga, gb = ag.gn_backward(op2)
    assert float((ga - base_a - torch.from_numpy(op2["ga_init"]).double()).abs().max()) < 1e-14
    assert float((gb - base_b - torch.from_numpy(op2["gb_init"]).double()).abs().max()) < 1e-14
    Sa, Sb = ag.gn_backward_budget(op2)
    Sa0, Sb0 = ag.gn_backward_budget(op)
    assert float((Sa - Sa0 - torch.from_numpy(op2["ga_init"]).double().abs()).abs().max()) < 1e-12 and bool((Sb >= Sb0).all())
    # a gradient routed to the wrong source of the concat, or a missing group-mean term, does not pass
    ref = ag.GnReference(op)
    assert not ref.ga.accepts(ref.gb.base32[:, :40]) and not ref.gb.accepts(np.concatenate([ref.ga.base32, ref.gb.base32[:, :16]], axis=1))
    G_only = ref.ga.base32 + 0.01 * np.float32(np.abs(ref.ga.base32).mean())
    assert not ref.ga.accepts(G_only)
