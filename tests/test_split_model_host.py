"""CPU: the f16 operand split as stated in tests/split_f64.py -- the representation bound delta over the whole magnitude range with the
guard's flag, the three-product convolution built on it inside the bound the kernels are held to (tests/test_gpu_operand_range.py), and
that bound sharp: planted defects of the split break it at some magnitude of the sweep.

One defect cannot show inside the sweep: a clamp at 65504 without the flag computes the same values as the statement wherever
max|x| <= 65000, which the sweep's own precondition guarantees.  It is shown on the magnitude grid (flag and values beyond 65000) and one
step above the sweep's top (k = 14), where the statement flags and the defect silently saturates."""
import numpy as np
import pytest
import torch

from tests import conv3_f64 as cf
from tests import split_f64 as sf
from tests.test_gpu_conv3_layer import LAYERS, _op

SWEEP_CASES = ("g0_one_tile_one_chunk", "g0_cin_6", "g1_one_tile", "g2_five_images_ragged_group", "g0_ragged_scaled_dgrad_form")
R3 = cf.R["f16x3"]


def _grid():
    mags = 2.0 ** np.arange(-30.0, np.log2(65000.0), 1.0 / 64)
    r = np.random.default_rng(1)
    mags = np.concatenate([mags, mags * (1 + r.random(mags.size))])
    mags = mags[mags <= 65000.0]
    return np.concatenate([mags, -mags]).astype(np.float32)


def test_split_is_within_delta_over_the_magnitude_grid():
    v = _grid()
    hi, lo, bad = sf.split(v)
    assert not bad.any()
    err = np.abs(v.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
    d = sf.delta(v.astype(np.float64))
    worst = float((err / d).max())
    print(f"grid of {v.size} values in [2^-30, 65000]: worst |v - hi - lo| / delta = {worst:.4f}")
    assert (err <= d).all()
    assert worst > 0.9          # ... and delta is not slack: some value comes close to it
    # the one-product mode keeps hi alone: half an ulp of f16
    h1, l1, _ = sf.split(v, x1=True)
    assert l1 is None and np.array_equal(h1.view(np.uint16), hi.view(np.uint16))
    e1 = np.abs(v.astype(np.float64) - h1.astype(np.float64))
    assert (e1 <= np.maximum(np.abs(v.astype(np.float64)) * 2.0 ** -11, 2.0 ** -25)).all()


def test_split_edges_and_the_flag():
    f32 = np.float32
    above = np.nextafter(f32(65000.0), f32(np.inf))
    edges = np.array([0.0, -0.0, 2.0 ** -24, 2.0 ** -14, 2.0 ** -3, 65000.0, above, 65504.0, 1e6, np.inf, -np.inf, np.nan,
                      -65000.0, -above, -1e6, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14 - 2.0 ** -30], f32)
    want_bad = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0], bool)
    hi, lo, bad = sf.split(edges)
    assert np.array_equal(bad, want_bad), bad
    assert np.isfinite(hi.astype(np.float64)).all() and np.isfinite(lo.astype(np.float64)).all()      # the clamp keeps hi finite, a NaN included
    ok = ~want_bad
    err = np.abs(edges[ok].astype(np.float64) - hi[ok].astype(np.float64) - lo[ok].astype(np.float64))
    assert (err <= sf.delta(edges[ok].astype(np.float64))).all(), err
    # what was clamped sits at +-65000 (a NaN at -65000: fmaxf returns the other operand)
    c = hi[want_bad].astype(np.float64) + lo[want_bad].astype(np.float64)
    assert np.array_equal(c, np.array([65000, 65000, 65000, 65000, -65000, -65000, -65000, -65000], np.float64)), c
    # exact values: 2^-24 is the smallest subnormal, 2^-25 ties to the even 0 in hi and again in lo (the model's worst case)
    assert float(hi[2]) == 2.0 ** -24 and float(lo[2]) == 0.0
    assert float(hi[15]) == 0.0 and float(lo[15]) == 0.0 and sf.delta(2.0 ** -25) == 2.0 ** -25
    # the defect of the last part: no flag, and a value beyond 65504 breaks delta
    h2, l2, b2 = sf.split(edges, defect="clamp_65504")
    assert not b2.any()
    assert abs(1e6 - float(h2[8]) - float(l2[8])) > sf.delta(1e6)


_cache = {}


def _case(name, k):
    if (name, k) not in _cache:
        op = sf.scaled_op(_op(LAYERS, name), k)
        _cache[(name, k)] = (op, sf.RangeReference(op))
    return _cache[(name, k)]


@pytest.mark.parametrize("name", SWEEP_CASES)
def test_three_product_model_is_inside_the_bound_at_every_magnitude(name):
    for k in sf.SWEEP_K:
        op, ref = _case(name, k)
        assert float(max(np.abs(op["xa"]).max(), 0 if op["xb"] is None else np.abs(op["xb"]).max())) <= 65000.0, "pick another seed"
        m = ref.check(sf.emulate(op, x64=ref.x64).numpy(), R3, f"{name} k {k} emulated f16x3")
        assert m["E32"] < 2.0 ** -20
    # the one-product emulation IS the f16-rounded statement (torch's float16 keeps subnormals), at the bottom of the sweep as well
    for k in (0, -14, -24):
        op, ref = _case(name, k)
        r16 = cf.Reference(op, f16_operands=True)
        e, _ = cf.E(sf.emulate(op, x1=True, x64=ref.x64).numpy(), r16.ref, r16.S)
        assert e <= 2.0 ** -40, (k, e)


@pytest.mark.parametrize("name", SWEEP_CASES)
def test_one_product_bound_with_the_encoded_budget_still_rejects_a_flush(name):
    """split_f64.RoundedReference counts subnormal operands at their encoded exponent: the emulation passes it at every k, and an
    emulation that flushes f16 subnormals breaks it wherever the operand is mostly subnormal."""
    r1 = cf.R["f16x1"]
    for k in sf.SWEEP_K:
        op, ref = _case(name, k)
        rr = sf.RoundedReference(op)
        rr.check(sf.emulate(op, x1=True, x64=ref.x64).numpy(), r1, f"{name} k {k} emulated f16x1")
        flushed = sf.emulate(op, x1=True, defect="hi_flushed_when_subnormal", x64=ref.x64).numpy()
        e_enc, _ = cf.E(flushed, rr.ref, rr.S_enc)
        over = e_enc / (r1 * max(rr.e32, cf.FLOOR))
        print(f"{name} k {k}: subnormals flushed -> {over:.3g} x the bound")
        if k <= -14:
            assert over > 100.0, (k, over)
        if k == 13:         # no subnormal operand at this scale: the encoded budget is the budget
            assert torch.equal(rr.S_enc, rr.S)


def test_model_numbers_of_the_one_tile_case():
    """The loss of fp32 equivalence by operand scale, as measured on the emulation (format only): printed for the documents."""
    e = {}
    for k in (0, -3, -6, -10, -14, -20):
        op, ref = _case("g0_one_tile_one_chunk", k)
        e[k], _ = cf.E(sf.emulate(op, x64=ref.x64).numpy(), ref.ref, ref.S)
        print(f"x scale 2^{k}: E(model) {e[k]:.2e}, E / E32 {e[k] / ref.e32:.2f}, Qmax {ref.qmax:.2e}")
        assert e[k] <= ref.qmax + 2.0 ** -21
    assert e[0] < 2.4e-7 and e[-14] > 2e-5      # fp32-equivalent at unit scale, worse than the 2e-5 per-layer contract at 2^-14


@pytest.mark.parametrize("defect", [d for d in sf.DEFECTS if d != "clamp_65504"])
def test_planted_defects_break_the_bound_somewhere_in_the_sweep(defect):
    broke = []
    for name in SWEEP_CASES:
        for k in sf.SWEEP_K:
            op, ref = _case(name, k)
            m = ref.measure(sf.emulate(op, defect=defect, x64=ref.x64).numpy(), R3)
            if m["margin"] > 1.0:
                broke.append((name, k, m["margin"]))
    print(f"{defect}: breaks the bound at " + ", ".join(f"{n} k {k} (x{m:.1f})" for n, k, m in broke))
    assert broke, f"{defect} passes the bound at every k: the bound is not sharp"
    assert {n for n, _, _ in broke} == set(SWEEP_CASES), "every sweep case must catch it at some k"


def test_clamp_without_flag_shows_one_step_above_the_sweep():
    op = sf.scaled_op(_op(LAYERS, "g0_one_tile_one_chunk"), 14)
    x = op["xa"]
    assert np.abs(x).max() > 65504.0            # the sweep's precondition fails here: that is the point
    _, _, bad = sf.split(x)
    _, _, bad_defect = sf.split(x, defect="clamp_65504")
    assert bad.any() and not bad_defect.any()
    ref = sf.RangeReference(op)
    m = ref.measure(sf.emulate(op, defect="clamp_65504", x64=ref.x64).numpy(), R3)
    print(f"clamp_65504 at k 14: {int(bad.sum())} values beyond 65000 unflagged, err / bound {m['margin']:.3g}")
    assert m["margin"] > 1.0                    # a wrong layer, and nothing said so
    # inside the sweep it computes what the statement computes
    op13, ref13 = _case("g0_one_tile_one_chunk", 13)
    assert torch.equal(sf.emulate(op13, defect="clamp_65504", x64=ref13.x64), sf.emulate(op13, x64=ref13.x64))
