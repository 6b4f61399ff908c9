"""-m gpu: conv9 (csrc/conv9.hip), the whole-image 3x3 kernel of the 8 x 8 layers -- one workgroup per (image, 32 output channels), whole
K, no split-K slabs -- one layer at a time on host operands (dpir_debug_conv9_layer) against the float64 statement and the per-element
budget of tests/conv3_f64.py (R = 8 for f16x3; f16x1 against the f16-rounded statement with R["f16x1"], as tests/test_gpu_conv3_layer.py),
the fused hop conv1 -> GroupNorm32 + FiLM + SiLU -> conv2 against the float64 statement of the pair with the existing unfused route
(split-K conv7 + gn_act_small, dpir_debug_conv3_layer) as the yardstick, and the forward with the route on against the route off.

Shapes are the smallest that reach each path of the kernel: Cin 16 / 48 / 80 = one, three and five 16-channel chunks for four waves (three
waves / one wave / three waves with an empty or a shorter K share), Cout 32 / 64 / 96 / 512 = one tile, two, a partial 128-channel block,
four blocks (the XCD-aware workgroup numbering, taken when the tile count is a multiple of 8), every residual form, one and three images.

Largest E(kernel) / E(float32) measured on MI355X: 1.315 (f16x3, R = 8), 0.872 (f16x1 against the f16-rounded statement, R = 4); the hop's
fused / unfused error ratios 0.38 - 1.00 (bound 2): profiles/conv9/README.md."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import conv3_f64 as cf

pytestmark = pytest.mark.gpu

F16 = ("f16x3", "f16x1")
TOL_LAYER = 2e-5        # tests/test_gpu_unet.py: max-abs / max-abs per block output
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engines():
    import diffpir_amd
    made = {}

    def get(prec, grad=False):
        key = (prec, grad)
        if key not in made:
            e = diffpir_amd.Engine(0)
            e.set_precision(prec)
            if grad:
                e.enable_grad(True)
            made[key] = e
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def _operands(B, cin, cout, H, W, seed, res_mode=-1, second=0, film=False):
    r = np.random.default_rng(seed)
    f = lambda *s: r.standard_normal(s).astype(np.float32)
    op = dict(shape=(B, cin, 0, cout, H, W), mode=0, res_mode=res_mode, scaled=False, prologue=0, xa=f(B, cin, H, W), xb=None,
              w=(0.05 * r.standard_normal((cout, cin, 3, 3))).astype(np.float32), bias=f(cout), res=None, prm=None, gamma=None, beta=None, film=None,
              film2=None)
    if res_mode >= 0:
        Hr, Wr = (H // 2, W // 2) if res_mode == 1 else ((2 * H, 2 * W) if res_mode == 2 else (H, W))
        op["res"] = f(B, cout, Hr, Wr)
    if second:
        op["gamma2"] = (0.5 + r.random(cout)).astype(np.float32)
        op["beta2"] = (0.2 * r.standard_normal(cout)).astype(np.float32)
        op["w2"] = (0.05 * r.standard_normal((second, cout, 3, 3))).astype(np.float32)
        op["bias2"] = f(second)
        if film:
            op["film2"] = (0.2 * r.standard_normal((B, 2 * cout))).astype(np.float32)     # a different row per image
    return op


def _image(op, n):
    """The B = 1 case made of image n."""
    one = dict(op, shape=(1,) + op["shape"][1:], xa=np.ascontiguousarray(op["xa"][n:n + 1]))
    for k in ("res", "film2"):
        if op.get(k) is not None:
            one[k] = np.ascontiguousarray(op[k][n:n + 1])
    return one


def _run9(e, op, hop=0):
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, cin, _, cout, H, W = op["shape"]
    out = np.full((B, cout, H, W), np.nan, np.float32)
    stat = np.full((B, cout, 2), np.nan, np.float64)
    d = _lib.Conv9Desc(B=B, Cin=cin, Cout=cout, H=H, W=W, res_mode=op["res_mode"], hop=hop)
    d.x, d.w, d.bias, d.res, d.prm = _ptr(op["xa"]), _ptr(op["w"]), _ptr(op["bias"]), _ptr(op["res"]), _ptr(op["prm"])
    d.out, d.stat_out = _ptr(out), _ptr(stat)
    out2 = None
    if hop:
        d.Cout2 = op["w2"].shape[0]
        out2 = np.full((B, d.Cout2, H, W), np.nan, np.float32)
        for k in ("gamma2", "beta2", "film2", "w2", "bias2"):
            setattr(d, k, _ptr(op[k]))
        d.out2 = _ptr(out2)
    rc = dbg.dpir_debug_conv9_layer(e.h, C.byref(d))
    return dict(rc=rc, out=out, stat=stat, out2=out2, ran=d.ran_out, err=e.lib.dpir_last_error(e.h) if rc else b"")


def _run3(e, op, route=0, split=0, defer=0):
    """dpir_debug_conv3_layer: the existing routes (tests/test_gpu_conv3_layer.py::_run)."""
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, ca, cb, cout, H, W = op["shape"]
    out = np.empty((B, cout, H, W), np.float32)
    d = _lib.Conv3Desc(B=B, ca=ca, cb=cb, Cout=cout, H=H, W=W, mode=op["mode"], res_mode=op["res_mode"], scaled=0, prologue=op["prologue"],
                       route=route, split=split, defer=defer)
    for k in ("xa", "xb", "w", "bias", "res", "prm", "gamma", "beta", "film"):
        setattr(d, k, _ptr(op[k]))
    d.out = _ptr(out)
    out2 = None
    if defer:
        d.Cout2 = op["w2"].shape[0]
        out2 = np.empty((B, d.Cout2, H, W), np.float32)
        for k in ("gamma2", "beta2", "w2", "bias2"):
            setattr(d, k, _ptr(op[k]))
        d.out2 = _ptr(out2)
    rc = dbg.dpir_debug_conv3_layer(e.h, C.byref(d))
    return dict(rc=rc, out=out, out2=out2, kind=d.stat_kind_out, path=d.path_out, ksplit=d.ksplit_out, err=e.lib.dpir_last_error(e.h) if rc else b"")


_refs = {}


def _reference(key, op, f16_operands):
    k = (key, f16_operands)
    if k not in _refs:
        _refs[k] = cf.Reference(op, f16_operands)
    return _refs[k]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ single layer
@pytest.mark.parametrize("prec", F16)
@pytest.mark.parametrize("res_mode", [-1, 0, 1, 2])
@pytest.mark.parametrize("cout", [32, 64, 96, 512])
@pytest.mark.parametrize("cin", [16, 48, 80])
def test_layer_8x8_against_the_float64_statement(engines, cin, cout, res_mode, prec):
    e = engines(prec)
    name = f"c9_cin{cin}_cout{cout}_res{res_mode}"
    op = _operands(3, cin, cout, 8, 8, seed=1000 + cin * 7 + cout * 3 + res_mode, res_mode=res_mode)
    r = _run9(e, op)
    assert r["rc"] == 0 and r["ran"] == 1, (r["rc"], r["err"])
    assert np.isfinite(r["out"]).all(), "non-finite output (poison left in place?)"
    x1 = prec == "f16x1"
    _reference(name, op, x1).check(r["out"], cf.R[prec], f"{name} B=3 [{prec}] conv9" + (" vs the f16-rounded statement" if x1 else ""))
    cf.check_stats(r["stat"], r["out"], f"{name} [{prec}]")
    again = _run9(e, op)
    assert again["rc"] == 0 and _same_bits(again["out"], r["out"]) and np.array_equal(again["stat"], r["stat"]), "two runs of one case differ"
    for n in range(3):
        one = _run9(e, _image(op, n))
        assert one["rc"] == 0 and one["ran"] == 1, one["err"]
        assert _same_bits(one["out"], r["out"][n:n + 1]), f"image {n} alone differs from image {n} of the batch"
        assert np.array_equal(one["stat"], r["stat"][n:n + 1]), f"statistics of image {n}"


@pytest.mark.parametrize("prec", F16)
def test_grid_of_eight_with_two_channel_tiles_keeps_the_plain_numbering(engines, prec):
    """B = 4, Cout = 64: the grid (8) is a multiple of 8 but the tile count (2) is not -- the XCD-aware numbering is a bijection only for a
    multiple of 8 tiles, so this launch must take the plain order."""
    e = engines(prec)
    op = _operands(4, 48, 64, 8, 8, seed=77, res_mode=0)
    r = _run9(e, op)
    assert r["rc"] == 0, r["err"]
    _reference("c9_grid8", op, prec == "f16x1").check(r["out"], cf.R[prec], f"grid 8, two tiles [{prec}]")
    cf.check_stats(r["stat"], r["out"], f"grid 8, two tiles [{prec}]")


# ------------------------------------------------------------------------------------------------ the hop
class _Pair:
    """Float64 statement of layer 1, GroupNorm32 + FiLM + SiLU, layer 2 (cf.PairReference with the FiLM rows), and the second layer's budget."""

    def __init__(self, op):
        first64 = cf.layer(op, torch.float64)
        op2 = dict(cf.second_stage_op(op, first64.numpy()), film=op["film2"])
        x64 = cf.prologued(op2, torch.float64)
        self.ref = cf.layer(op2, torch.float64, x=x64)
        self.S = cf.budget(op2, x=x64)

    def E(self, got):
        return cf.E(got, self.ref, self.S)


def _unfused(e, op):
    """The existing route on the same operands: split-K conv7 with the combine left to gn_act_small (route 7, defer 1); with FiLM rows, which
    that probe's second stage does not take, the stored first layer through gn_act_small with the rows -- the same bits as the deferred form
    (tests/test_gpu_conv3_layer.py::test_split_k_deferred_into_the_next_prologue)."""
    B, cin, _, cout, H, W = op["shape"]
    if op["film2"] is None:
        r = _run3(e, op, route=7, split=1, defer=1)
        assert r["rc"] == 0 and r["kind"] == 3 and r["path"] == 7 and r["ksplit"] > 1, (r["rc"], r["err"], r["kind"], r["path"], r["ksplit"])
        return r["out2"]
    r = _run3(e, op, route=7, split=1)
    assert r["rc"] == 0 and r["path"] == 7 and r["ksplit"] > 1, (r["rc"], r["err"], r["path"], r["ksplit"])
    op2 = dict(cf.second_stage_op(op, r["out"]), film=op["film2"], shape=(B, cout, 0, op["w2"].shape[0], H, W), scaled=False, res=None, prm=None)
    r2 = _run3(e, op2)
    assert r2["rc"] == 0, r2["err"]
    return r2["out"]


@pytest.mark.parametrize("prec", F16)
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("cout", [32, 256, 512])
def test_hop_against_the_unfused_route(engines, cout, film, prec):
    """1, 8 and 16 channels per GroupNorm group.  Bound: the fused route's error against the float64 pair statement is at most twice the
    unfused route's on the same operands (they differ in the summation order inside K and in the GroupNorm sums)."""
    e = engines(prec)
    op = _operands(3, 64, cout, 8, 8, seed=2000 + cout + int(film), second=32, film=film)
    pair = _Pair(op)
    r = _run9(e, op, hop=1)
    assert r["rc"] == 0 and r["ran"] == 1, (r["rc"], r["err"])
    assert np.isfinite(r["out2"]).all()
    e_fused, at = pair.E(r["out2"])
    e_unfused, _ = pair.E(_unfused(e, op))
    print(f"CONV9HOP cout {cout} film {int(film)} [{prec}]: E fused {e_fused:.3e} at {at}, E unfused {e_unfused:.3e}, ratio {e_fused / e_unfused:.3f}")
    assert e_fused <= 2.0 * e_unfused, (e_fused, e_unfused)
    for n in range(3):
        one = _run9(e, _image(op, n), hop=1)
        assert one["rc"] == 0, one["err"]
        assert _same_bits(one["out2"], r["out2"][n:n + 1]), f"fused out2 of image {n} alone differs from the batch"


def test_hop_reports_h1_outside_the_f16_range():
    """gamma2 = 1e6: h1 after the affine is far beyond 65000 -> the engine reports DPIR_ERR_RANGE at the next synchronisation."""
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    try:
        e.set_precision("f16x3")
        op = _operands(1, 64, 32, 8, 8, seed=5, second=32)
        e.sync()
        op["gamma2"][:] = 1e6
        r = _run9(e, op, hop=1)
        assert r["rc"] == 0, r["err"]
        with pytest.raises(diffpir_amd.EngineRangeError, match="f16 operand range"):
            e.sync()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("shape,hop,text", [
    ((1, 40, 32, 8, 8), 0, b"multiple of 16"),
    ((1, 32, 32, 8, 16), 0, b"square image"),
    ((1, 32, 32, 32, 32), 0, b"8 x 8 layers only"),
    ((1, 32, 96, 8, 8), 1, b"straddle a 32-channel tile"),
])
def test_refused_shapes(engines, shape, hop, text):
    B, cin, cout, H, W = shape
    op = _operands(B, cin, cout, H, W, seed=3, second=32 if hop else 0)
    r = _run9(engines("f16x3"), op, hop=hop)
    assert r["rc"] != 0 and r["ran"] == 0 and text in r["err"], (r["rc"], r["err"])


def test_refused_engines(engines):
    op = _operands(1, 32, 32, 8, 8, seed=4)
    r = _run9(engines("f16x3", grad=True), op)
    assert r["rc"] != 0 and r["ran"] == 0 and b"gradient-mode engine" in r["err"], (r["rc"], r["err"])
    r = _run9(engines("f32"), op)
    assert r["rc"] != 0 and r["ran"] == 0 and b"f32 precision" in r["err"], (r["rc"], r["err"])


# ------------------------------------------------------------------------------------------------ forward level
_FWD_SNIPPET = r"""
import sys, numpy as np, torch
sys.path.insert(0, {root!r})
import diffpir_amd
from oracle import unet_oracle as uo
from tests.gpu_common import make_model
e = diffpir_amd.Engine(0); e.set_precision("f16x3")
make_model(e, uo.ffhq_hp())
g = torch.Generator().manual_seed(78)
x = torch.randn((16, 3, 64, 64), generator=g); t = torch.randint(0, 1000, (16,), generator=g)
xd = e.to_device(x.numpy())
a = e.unet_forward(xd, t.numpy()).numpy()
b = e.unet_forward(xd, t.numpy()).numpy()
assert np.array_equal(a, b), "two forwards of the same input differ"
taps = dict(out=a)
for name in {names!r}:
    taps[name] = e.read_tap(name)
try:
    e.read_tap("input_blocks.7.0#h1")
    taps["has_h1_8x8"] = np.ones(1)
except diffpir_amd.EngineError:
    taps["has_h1_8x8"] = np.zeros(1)
np.savez({out!r}, **taps)
"""


@pytest.fixture(scope="module")
def forwards(tmp_path_factory):
    """FFHQ topology at 64 x 64, B = 16 (8 x 8 layers with 256 channels: 128 workgroups), one process per switch setting.  The threshold is
    pinned to 128 workgroups for the runs with the route on, so the coverage does not move with the default."""
    from oracle import unet_oracle as uo
    hp = uo.ffhq_hp()
    sd = uo.synth_state_dict(hp, 0)
    g = torch.Generator().manual_seed(78)
    x = torch.randn((16, 3, 64, 64), generator=g)
    t = torch.randint(0, 1000, (16,), generator=g)
    sub = [0, 15]
    otaps = {}
    oref = uo.unet_forward(sd, hp, x[sub], t[sub], taps=otaps)
    names = [k for k in otaps if k != "emb"]
    tmp = tmp_path_factory.mktemp("conv9_fwd")
    runs = {}
    for tag, env in (("on", dict(DPIR_CONV9="1", DPIR_CONV9_MIN_WG="128")), ("off", dict(DPIR_CONV9="0")),
                     ("on_nohop", dict(DPIR_CONV9="1", DPIR_CONV9_MIN_WG="128", DPIR_FUSE_H1="0")),
                     ("on_nohop_again", dict(DPIR_CONV9="1", DPIR_CONV9_MIN_WG="128", DPIR_FUSE_H1="0"))):
        out = str(tmp / f"{tag}.npz")
        r = subprocess.run([sys.executable, "-c", _FWD_SNIPPET.format(root=ROOT, names=names, out=out)], cwd=ROOT, env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        runs[tag] = dict(np.load(out))
    return runs, otaps, oref.numpy(), sub


def test_forward_route_on_equals_route_off_to_the_fused_hop_bar(forwards):
    from tests.gpu_common import rel_err
    runs = forwards[0]
    assert runs["on"]["has_h1_8x8"][0] == 0 and runs["off"]["has_h1_8x8"][0] == 1, "the 8 x 8 ResBlocks did not take / leave the conv9 hop"
    err = rel_err(runs["on"]["out"], runs["off"]["out"])
    print(f"conv9 on vs off, FFHQ 64^2 B=16 [f16x3]: rel err {err:.3e}")
    assert err < 5e-6


def test_forward_without_the_hop_is_reproducible(forwards):
    runs = forwards[0]
    assert runs["on_nohop"]["has_h1_8x8"][0] == 1
    assert _same_bits(runs["on_nohop"]["out"], runs["on_nohop_again"]["out"])


def test_forward_block_outputs_meet_the_layer_tolerance(forwards):
    from tests.gpu_common import rel_err
    runs, otaps, oref, sub = forwards
    worst = ("", 0.0)
    for name, tv in otaps.items():
        if name == "emb":
            continue
        got = runs["on"][name].reshape((16,) + tuple(tv.shape[1:]))[sub]
        err = rel_err(got, tv.numpy())
        worst = max(worst, (name, err), key=lambda p: p[1])
        assert err < TOL_LAYER, f"layer {name}: rel err {err:.3e}"
    err = rel_err(runs["on"]["out"][sub], oref)
    print(f"conv9 on, FFHQ 64^2 B=16, images {sub} vs oracle: output {err:.3e}, worst block {worst[0]} {worst[1]:.3e}")
    assert err < TOL_LAYER
