"""-m gpu: every route of the 3x3 convolution layers, one layer at a time on host operands (dpir_debug_conv3_layer), against the float64
statement of the layer in tests/conv3_f64.py, per element.

What is asserted for each case: the probe succeeds, the launchers report the kernel (0 fp32 kernel, 6 conv6, 7 conv7, 8 conv8) and the
split-K factor that launch_conv6's documented rule gives for the shape (so a dispatch change cannot silently move the coverage), and the
output is within R x the error of the same statement evaluated in float32 on the CPU, every element against its own magnitude budget.
f16x1 (one f16 product) is held to the statement with f16-rounded operands where there is no prologue; with a prologue it is held to the
bound that follows from the format alone (each operand is rounded once: |product error| <= (2^-11 + 2^-11 + 2^-22) |x||w|, so E <= 2^-10 plus
the fp32 accumulation term) and to bit-equality between conv6 and conv7 where both exist.  Statistics are tied to the kernel's own output.

The shapes are the smallest that reach each index path: one tile / ragged tiles in each of the three geometries, a ragged image group in the
four-images-per-tile geometry, Cin below and off the 16-channel chunk, partial / idle / narrow output-channel blocks, uneven split-K slices."""
import ctypes as C

import numpy as np
import pytest

from tests import conv3_f64 as cf
from tests import conv_route_rules as rr

pytestmark = pytest.mark.gpu

F16 = ("f16x3", "f16x1")
ALL = ("f32",) + F16
X1_FORMAT_BOUND = 2.0 ** -10


@pytest.fixture(scope="module")
def engines():
    import diffpir_amd
    made = {}

    def get(prec):
        if prec not in made:
            e = diffpir_amd.Engine(0)
            e.set_precision(prec)
            made[prec] = e
        return made[prec]
    yield get
    for e in made.values():
        e.close()


# ------------------------------------------------------------------------------------------------ operands
def _operands(shape, seed, mode=0, res_mode=-1, scaled=False, prologue=0, silu=True, film=False, second=0, zero_bias=False):
    B, ca, cb, cout, H, W = shape
    r = np.random.default_rng(seed)
    c = ca + cb
    Hs, Ws = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
    f = lambda *s: r.standard_normal(s).astype(np.float32)
    op = dict(shape=shape, mode=mode, res_mode=res_mode, scaled=scaled, prologue=prologue,
              xa=f(B, ca, Hs, Ws), xb=f(B, cb, Hs, Ws) if cb else None, w=(0.05 * r.standard_normal((cout, c, 3, 3))).astype(np.float32),
              bias=f(cout), res=None, prm=None, gamma=None, beta=None, film=None)
    if zero_bias:
        op["bias"][:] = 0
    if res_mode >= 0:
        Hr, Wr = (H // 2, W // 2) if res_mode == 1 else ((2 * H, 2 * W) if res_mode == 2 else (H, W))
        op["res"] = f(B, cout, Hr, Wr)
    if prologue == 1:     # {mean, scale, shift, SiLU flag} per (image, channel), as tests/test_gpu_conv5_small.py::_operands
        t = np.empty((B, c, 4), np.float32)
        t[..., 0] = r.standard_normal((B, c)) * 0.1
        t[..., 1] = 0.5 + r.random((B, c))
        t[..., 2] = r.standard_normal((B, c)) * 0.2
        t[..., 3] = 1.0 if silu else 0.0
        op["prm"] = t
    if prologue == 2:
        op["gamma"] = (0.5 + r.random(c)).astype(np.float32)
        op["beta"] = (0.2 * r.standard_normal(c)).astype(np.float32)
        if film:
            op["film"] = (0.2 * r.standard_normal((B, 2 * c))).astype(np.float32)
    if second:
        op["gamma2"] = (0.5 + r.random(cout)).astype(np.float32)
        op["beta2"] = (0.2 * r.standard_normal(cout)).astype(np.float32)
        op["w2"] = (0.05 * r.standard_normal((second, cout, 3, 3))).astype(np.float32)
        op["bias2"] = f(second)
    return op


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def _run(e, op, route=0, split=0, defer=0):
    """-> dict(rc, out, stat, kind, path, ksplit[, out2])"""
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, ca, cb, cout, H, W = op["shape"]
    out = np.empty((B, cout, H, W), np.float32)
    stat = np.full((B, cout, 2), np.nan, np.float64)
    d = _lib.Conv3Desc(B=B, ca=ca, cb=cb, Cout=cout, H=H, W=W, mode=op["mode"], res_mode=op["res_mode"], scaled=int(bool(op["scaled"])),
                       prologue=op["prologue"], route=route, split=split, defer=defer)
    for k in ("xa", "xb", "w", "bias", "res", "prm", "gamma", "beta", "film"):
        setattr(d, k, _ptr(op[k]))
    d.out, d.stat_out = _ptr(out), _ptr(stat)
    out2 = None
    if defer:
        d.Cout2 = op["w2"].shape[0]
        out2 = np.empty((B, d.Cout2, H, W), np.float32)
        for k in ("gamma2", "beta2", "w2", "bias2"):
            setattr(d, k, _ptr(op[k]))
        d.out2 = _ptr(out2)
    rc = dbg.dpir_debug_conv3_layer(e.h, C.byref(d))
    return dict(rc=rc, out=out, stat=stat, kind=d.stat_kind_out, path=d.path_out, ksplit=d.ksplit_out, out2=out2,
                err=e.lib.dpir_last_error(e.h) if rc else b"")


# launch_conv6's documented rule: tests/conv_route_rules.py (shared with the planner's host tests)
_geo, _expected = rr.geo, rr.expected


_refs = {}


def _reference(name, op, f16_operands=False):
    key = (name, f16_operands)
    if key not in _refs:
        _refs[key] = cf.Reference(op, f16_operands)
    return _refs[key]


def _hold(prec, name, op, got, what, path=None):
    """The numeric bound of the module docstring for one output (the fp32 kernel is held to the f32 bound whatever the engine's precision)."""
    if path == 0:
        prec = "f32"
    assert np.isfinite(got).all(), f"{what}: non-finite output (poison left in place?)"
    if prec != "f16x1":
        return _reference(name, op).check(got, cf.R[prec], what)
    if op["prologue"] == 0:
        return _reference(name, op, True).check(got, cf.R["f16x1"], what + " vs the f16-rounded statement")
    ref = _reference(name, op)
    m = ref.measure(got)
    print(f"CONV3X1 {what}: E {m['E']:.3e} at {m['at']} (format bound 2^-10)")
    assert m["E"] <= X1_FORMAT_BOUND + cf.R["f32"] * max(ref.e32, cf.FLOOR), f"{what}: E = {m['E']:.3e} at {m['at']}"
    return m


def _check_case(engines, prec, name, op, split=0):
    e = engines(prec)
    r = _run(e, op, 0, split)
    assert r["rc"] == 0, (r["rc"], r["err"])
    assert (r["path"], r["ksplit"]) == _expected(prec, op["shape"], 0, split), (r["path"], r["ksplit"])
    what = f"{name} [{prec}] path {r['path']} ksplit {r['ksplit']}"
    _hold(prec, name, op, r["out"], what, r["path"])
    cout = op["shape"][3]
    if r["path"] in (6, 7):
        want = 0 if cout % 32 else (2 if r["ksplit"] > 1 else 1)
        assert r["kind"] == want, (r["kind"], want)
        if want:
            cf.check_stats(r["stat"], r["out"], what)
    if prec == "f16x1" and op["prologue"] != 0 and _geo(*op["shape"][4:]) == 0:
        r6, r7 = _run(e, op, 6, split), _run(e, op, 7, split)
        assert r6["rc"] == 0 and r7["rc"] == 0 and (r6["path"], r7["path"]) == (6, 7), (r6["rc"], r7["rc"], r6["err"], r7["err"])
        assert np.array_equal(r6["out"].view(np.uint32), r7["out"].view(np.uint32)), f"{what}: conv6 and conv7 differ"
    return r


# ------------------------------------------------------------------------------------------------ geometry, residual forms, scale
RAGGED0, RAGGED1, RAGGED2 = (3, 40, 8, 128, 20, 36), (3, 48, 0, 160, 24, 20), (6, 64, 0, 256, 12, 12)
LAYERS = {
    # geometry 0: 8 x 32 tiles
    "g0_one_tile_one_chunk": dict(shape=(2, 16, 0, 128, 8, 32)),
    "g0_ragged_concat_cin48_odd_batch": dict(shape=RAGGED0),
    "g0_cin_6": dict(shape=(1, 6, 0, 128, 16, 32)),
    "g0_cout_200_partial_block": dict(shape=(2, 32, 0, 200, 16, 32)),
    "g0_cout_192_idle_half": dict(shape=(2, 32, 0, 192, 16, 32)),
    "g0_cout_24_narrow": dict(shape=(2, 32, 0, 24, 16, 32)),
    "g0_cout_3_narrow": dict(shape=(2, 64, 0, 3, 16, 64)),
    "g0_ragged_res_same": dict(shape=RAGGED0, res_mode=0),
    "g0_ragged_res_half": dict(shape=RAGGED0, res_mode=1),
    "g0_ragged_res_double": dict(shape=RAGGED0, res_mode=2),
    # the device output scale multiplies the convolution sum; bias and residual are added behind it (tests/conv3_f64.py, step 6)
    "g0_ragged_scaled": dict(shape=RAGGED0, res_mode=0, scaled=True),
    # as the dgrad route launches it: zero bias, no residual -- there it is the whole output times 0.25
    "g0_ragged_scaled_dgrad_form": dict(shape=RAGGED0, scaled=True, zero_bias=True),
    # geometry 1: 16 x 16 tiles
    "g1_one_tile": dict(shape=(2, 32, 0, 128, 16, 16)),
    "g1_ragged": dict(shape=RAGGED1),
    "g1_ragged_res_same": dict(shape=RAGGED1, res_mode=0),
    "g1_ragged_res_half": dict(shape=RAGGED1, res_mode=1),
    "g1_ragged_res_double": dict(shape=RAGGED1, res_mode=2),
    # geometry 2: four images x 8 x 8 per tile
    "g2_four_images": dict(shape=(4, 32, 0, 128, 8, 8)),
    "g2_five_images_ragged_group": dict(shape=(5, 32, 0, 128, 8, 8)),
    "g2_one_image": dict(shape=(1, 32, 0, 128, 8, 8)),
    "g2_ragged_two_co_blocks": dict(shape=RAGGED2),
    "g2_ragged_res_same": dict(shape=RAGGED2, res_mode=0),
    "g2_ragged_res_half": dict(shape=RAGGED2, res_mode=1),
    "g2_ragged_res_double": dict(shape=RAGGED2, res_mode=2),
    # shapes the f16 path refuses: the fp32 kernel in every precision
    "fp32_only_6x6": dict(shape=(2, 16, 0, 32, 6, 6)),
    "fp32_only_w_10": dict(shape=(2, 16, 0, 32, 8, 10)),
    "fp32_only_4x4": dict(shape=(1, 8, 0, 8, 4, 4)),
}
for _silu in (True, False):
    for _mode in (0, 1, 2):
        LAYERS[f"table_g0_mode{_mode}_{'silu' if _silu else 'affine'}"] = dict(shape=(2, 32, 0, 128, 16, 32), mode=_mode, prologue=1, silu=_silu)
        LAYERS[f"table_g1_concat_mode{_mode}_{'silu' if _silu else 'affine'}"] = dict(shape=(2, 48, 16, 128, 16, 16), mode=_mode, prologue=1, silu=_silu)


def _op(table, name):
    kw = dict(table[name])
    return _operands(kw.pop("shape"), seed=sorted(table).index(name) + 1, **kw)


@pytest.mark.parametrize("prec", ALL)
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_layer_against_the_float64_statement(engines, name, prec):
    op = _op(LAYERS, name)
    if op["scaled"] and prec == "f32":      # the device output scale belongs to the dgrad route of the f16 kernels; the fp32 kernel has none
        r = _run(engines(prec), op)
        assert r["rc"] != 0 and b"no device output scale" in r["err"], (r["rc"], r["err"])
        return
    _check_case(engines, prec, name, op)


@pytest.mark.parametrize("prec", F16)
def test_idle_half_conv7_forced_equals_conv6_bit_for_bit(engines, prec):
    op = _op(LAYERS, "g0_cout_192_idle_half")
    e = engines(prec)
    r0, r6, r7 = _run(e, op, 0), _run(e, op, 6), _run(e, op, 7)
    assert (r0["rc"], r6["rc"], r7["rc"]) == (0, 0, 0) and (r0["path"], r6["path"], r7["path"]) == (6, 6, 7)
    assert np.array_equal(r6["out"].view(np.uint32), r7["out"].view(np.uint32))
    assert np.array_equal(r0["out"].view(np.uint32), r6["out"].view(np.uint32))
    assert np.array_equal(r6["stat"], r7["stat"])
    _hold(prec, "g0_cout_192_idle_half", op, r7["out"], f"idle half, conv7 forced [{prec}]")
    # conv6 exists in the 8 x 32 geometry only: forcing it elsewhere is an error, not another kernel
    r = _run(e, _op(LAYERS, "g1_one_tile"), 6)
    assert r["rc"] != 0 and b"8 x 32 geometry only" in r["err"], (r["rc"], r["err"])


@pytest.mark.parametrize("prec", F16)
def test_images_of_one_tile_are_independent(engines, prec):
    """Four images share a tile in the 8 x 8 geometry: image n of the B = 5 launch equals a B = 1 launch on that image bit for bit."""
    op = _op(LAYERS, "g2_five_images_ragged_group")
    e = engines(prec)
    whole = _run(e, op)
    assert whole["rc"] == 0 and whole["path"] == 7
    for n in range(5):
        one = dict(op, shape=(1,) + op["shape"][1:], xa=np.ascontiguousarray(op["xa"][n:n + 1]))
        r = _run(e, one)
        assert r["rc"] == 0 and r["path"] == 7
        assert np.array_equal(r["out"].view(np.uint32), whole["out"][n:n + 1].view(np.uint32)), f"image {n}"
        assert np.array_equal(r["stat"], whole["stat"][n:n + 1]), f"statistics of image {n}"


# ------------------------------------------------------------------------------------------------ split-K
SPLIT = {
    "split_g1_two_slabs": dict(shape=(2, 64, 0, 128, 16, 16), ksplit=2),
    "split_g1_seven_chunks_3_3_1": dict(shape=(2, 112, 0, 128, 16, 16), ksplit=3),
    "split_g0_sixteen_slabs": dict(shape=(2, 512, 0, 256, 32, 32), ksplit=16),
    "split_g0_cout_32_res_half": dict(shape=(2, 512, 0, 32, 32, 32), ksplit=16, res_mode=1),
}


def _split_op(name):
    kw = dict(SPLIT[name])
    kw.pop("ksplit")
    return _operands(kw.pop("shape"), seed=100 + sorted(SPLIT).index(name), second=64, **kw)


@pytest.mark.parametrize("prec", ALL)
@pytest.mark.parametrize("name", sorted(SPLIT))
def test_split_k_resolved(engines, name, prec):
    op = _split_op(name)
    if prec != "f32":     # the case list was written for these factors: a mismatch means the rule changed and the cases must be revisited
        assert _expected(prec, op["shape"], 0, 1)[1] == SPLIT[name]["ksplit"]
    r = _check_case(engines, prec, name, op, split=1)
    if prec != "f32":
        assert r["kind"] == 2 and r["path"] == (6 if _geo(*op["shape"][4:]) == 0 else 7)


@pytest.mark.parametrize("prec", F16)
@pytest.mark.parametrize("name", sorted(SPLIT))
def test_split_k_deferred_into_the_next_prologue(engines, name, prec):
    """gn_act_small finishes the pending convolution: what it stores is the resolved launch bit for bit, and the layer behind it is the
    float64 statement of the pair; the same second layer fed with the stored tensor through the plain prologue gives the same bits."""
    op = _split_op(name)
    e = engines(prec)
    res = _run(e, op, 0, 1)
    dfr = _run(e, op, 0, 1, defer=1)
    assert res["rc"] == 0 and dfr["rc"] == 0, (res["err"], dfr["err"])
    assert dfr["kind"] == 3 and (dfr["path"], dfr["ksplit"]) == _expected(prec, op["shape"], 0, 1) == (res["path"], res["ksplit"])
    assert np.array_equal(dfr["out"].view(np.uint32), res["out"].view(np.uint32)), "the deferred combine differs from conv6_reduce_kernel"
    assert np.isfinite(dfr["out2"]).all()
    B, _, _, cout, H, W = op["shape"]
    op2 = dict(cf.second_stage_op(op, dfr["out"]), shape=(B, cout, 0, 64, H, W), scaled=False, res=None, prm=None)
    again = _run(e, op2)
    assert again["rc"] == 0, again["err"]
    assert np.array_equal(again["out"].view(np.uint32), dfr["out2"].view(np.uint32)), "second layer: pending and plain prologue differ"
    key = (name, "pair")
    if key not in _refs:
        _refs[key] = cf.PairReference(op)
    what = f"{name} deferred, second layer [{prec}]"
    if prec == "f16x3":
        _refs[key].check(dfr["out2"], cf.R[prec], what)
    else:
        # one f16 product: the second layer against the statement on the kernel's own first layer (format bound, module docstring)
        _hold(prec, name + "#second_on_stored", op2, dfr["out2"], what)


# ------------------------------------------------------------------------------------------------ gn_act_small
GN = {}
for _c in ((32, 0), (64, 32)):
    for _src in (8, 16, 32):
        for _mode in (0, 1, 2):
            for _film in (False, True):
                _o = _src * 2 if _mode == 1 else (_src // 2 if _mode == 2 else _src)
                GN[f"gn_c{_c[0] + _c[1]}_src{_src}_mode{_mode}_{'film' if _film else 'plain'}"] = dict(
                    shape=(2, _c[0], _c[1], 64 if _c[1] == 0 else 128, _o, _o), mode=_mode, prologue=2, film=_film)


@pytest.mark.parametrize("prec", F16)
@pytest.mark.parametrize("name", sorted(GN))
def test_gn_act_small_prologue(engines, name, prec):
    op = _op(GN, name)
    if _geo(*op["shape"][4:]) < 0:      # 8 x 8 pooled to 4 x 4: not an f16 layer, so the forward never pairs it with gn_act_small
        r = _run(engines(prec), op)
        assert r["rc"] != 0 and b"gn_act_small only feeds the f16 path" in r["err"], (r["rc"], r["err"])
        return
    _check_case(engines, prec, name, op)


def test_gn_act_small_refuses_more_than_1024_source_pixels(engines):
    op = _operands((1, 32, 0, 64, 16, 68), seed=7, prologue=2)         # HWs = 1088 on an f16 layer; 32 x 32 = 1024 runs above
    r = _run(engines("f16x3"), op)
    assert r["rc"] != 0 and b"gn_act_small refuses" in r["err"], (r["rc"], r["err"])
    assert _run(engines("f16x3"), dict(op, prologue=0))["rc"] == 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_both_prologues_agree_to_the_bound(engines, mode):
    """The same GroupNorm layer through gn_act_small and, with the table folded on the host in float64, through act_split: both are the
    layer (no bit-equality is claimed: the table is rounded to fp32, the fused prologue folds it from its own statistics)."""
    name = f"gn_c96_src16_mode{mode}_film"
    op = _op(GN, name)
    B, ca, cb = op["shape"][:3]
    c = ca + cb
    x = np.concatenate([op["xa"], op["xb"]], axis=1).astype(np.float64).reshape(B, 32, -1)
    mean, var = x.mean(axis=2), x.var(axis=2)
    rstd = np.repeat(1.0 / np.sqrt(var + cf.GN_EPS), c // 32, axis=1)
    sc, sh = 1.0 + op["film"][:, :c].astype(np.float64), op["film"][:, c:].astype(np.float64)
    t = np.empty((B, c, 4), np.float32)
    t[..., 0] = np.repeat(mean, c // 32, axis=1)
    t[..., 1] = rstd * op["gamma"] * sc
    t[..., 2] = op["beta"] * sc + sh
    t[..., 3] = 1.0
    e = engines("f16x3")
    fused = _run(e, op)
    table = _run(e, dict(op, prologue=1, prm=t))
    assert fused["rc"] == 0 and table["rc"] == 0 and fused["path"] == table["path"]
    _hold("f16x3", name, op, fused["out"], f"{name} fused prologue")
    _hold("f16x3", name, op, table["out"], f"{name} table prologue against the GroupNorm statement")


# ------------------------------------------------------------------------------------------------ conv8
CONV8 = {
    "conv8_c32_cout6_one_tile": dict(shape=(1, 32, 0, 6, 8, 32), prologue=1),
    "conv8_c64_cout6_odd_batch": dict(shape=(3, 64, 0, 6, 16, 64), prologue=1),
    "conv8_c128_cout16": dict(shape=(2, 128, 0, 16, 8, 32), prologue=1),
    "conv8_c256_cout1_max_channels": dict(shape=(2, 256, 0, 1, 8, 32), prologue=1),
}
CONV8_REFUSED = {
    "conv8_refused_c48": dict(shape=(1, 48, 0, 6, 8, 32), prologue=1),
    "conv8_refused_h12": dict(shape=(1, 32, 0, 6, 12, 32), prologue=1),
    "conv8_refused_cout17": dict(shape=(1, 32, 0, 17, 8, 32), prologue=1),
    "conv8_refused_no_silu": dict(shape=(1, 32, 0, 6, 8, 32), prologue=1, silu=False),
}


@pytest.mark.parametrize("prec", F16)
@pytest.mark.parametrize("name", sorted(CONV8))
def test_conv8_output_layer(engines, name, prec):
    op = _op(CONV8, name)
    r = _run(engines(prec), op, route=8)
    assert r["rc"] == 0 and r["path"] == 8, (r["rc"], r["path"], r["err"])
    _hold(prec, name, op, r["out"], f"{name} [{prec}] path 8")


@pytest.mark.parametrize("prec", F16)
@pytest.mark.parametrize("name", sorted(CONV8_REFUSED))
def test_conv8_refusals_leave_the_planes_route(engines, name, prec):
    op = _op(CONV8_REFUSED, name)
    r = _run(engines(prec), op, route=8)
    assert r["rc"] != 0 and b"conv8" in r["err"], (r["rc"], r["err"])
    _check_case(engines, prec, name, op)
