"""-m gpu: conv11 (csrc/conv11.hip), conv7's 8 x 32 geometry with the 16x16x32 MFMA in the main loop, one layer at a time on host operands
(dpir_debug_conv11_layer) against the float64 statement and the per-element budget of tests/conv3_f64.py (R = 8 for f16x3), the fused hop
conv1 -> GroupNorm32 + FiLM + SiLU -> conv2 against the float64 statement of the pair with the unfused route (launch_conv6 + gn_act_small,
dpir_debug_conv3_layer) as the yardstick, and the forward with the route on against DPIR_CONV11=0 and against the oracle.

Shapes are the smallest that reach every path of the kernel: 8 x 32 (one tile) and 16 x 64 (2 x 2 tiles: the halo crosses tiles, all four
image borders; the hop: four workgroups wait for one another), Cin 32 / 64 / 96 (one, two and three two-chunk periods: the period body
alone, both slot parities, both plus the last period), Cout 128 / 256 (one and two co-blocks; the hop also 512: 4, 8 and 16 channels per
GroupNorm group), every residual form and none, three images.

Forward level: FFHQ topology at 64 x 64, B = 16 -- the 64 x 64 layers have 256 workgroups, launch_conv6's whole-K rule, so the plain
epilogue routes; the hop needs 384 and is covered by a second pair of runs at 128 x 128, B = 8 (512 workgroups).

Largest E(kernel) / E(float32) measured on MI355X: 3.607 (R = 8); the hop's fused / unfused error ratios 0.85 - 1.21 (bound 2); forward on vs
off 6.99e-07 / 6.29e-07 (bar 5e-6): profiles/conv11/README.md."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import conv3_f64 as cf

pytestmark = pytest.mark.gpu

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


def _run11(e, op, route=0, ksplit=1, hop=0):
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, cin, _, cout, H, W = op["shape"]
    out = np.full((B, cout, H, W), np.nan, np.float32)
    stat = np.full((B, cout, 2), np.nan, np.float64)
    d = _lib.Conv11Desc(B=B, Cin=cin, Cout=cout, H=H, W=W, res_mode=op["res_mode"], route=route, ksplit=ksplit, hop=hop)
    d.x, d.w, d.bias, d.res, d.prm = _ptr(op["xa"]), _ptr(op["w"]), _ptr(op["bias"]), _ptr(op["res"]), _ptr(op["prm"])
    d.out, d.stat_out = _ptr(out), _ptr(stat)
    out2 = None
    if hop:
        d.Cout2 = op["w2"].shape[0]
        out2 = np.full((B, d.Cout2, H, W), np.nan, np.float32)
        for k in ("gamma2", "beta2", "film2", "w2", "bias2"):
            setattr(d, k, _ptr(op[k]))
        d.out2 = _ptr(out2)
    rc = dbg.dpir_debug_conv11_layer(e.h, C.byref(d))
    return dict(rc=rc, out=out, stat=stat, out2=out2, ran=d.ran_out, err=e.lib.dpir_last_error(e.h) if rc else b"")


def _run3(e, op):
    """dpir_debug_conv3_layer: the forward's existing dispatch (tests/test_gpu_conv3_layer.py::_run)."""
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, ca, cb, cout, H, W = op["shape"]
    out = np.empty((B, cout, H, W), np.float32)
    d = _lib.Conv3Desc(B=B, ca=ca, cb=cb, Cout=cout, H=H, W=W, mode=op["mode"], res_mode=op["res_mode"], scaled=0, prologue=op["prologue"],
                       route=0, split=0, defer=0)
    for k in ("xa", "xb", "w", "bias", "res", "prm", "gamma", "beta", "film"):
        setattr(d, k, _ptr(op[k]))
    d.out = _ptr(out)
    rc = dbg.dpir_debug_conv3_layer(e.h, C.byref(d))
    return dict(rc=rc, out=out, path=d.path_out, err=e.lib.dpir_last_error(e.h) if rc else b"")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_layer(e, name, op):
    r = _run11(e, op)
    assert r["rc"] == 0 and r["ran"] == 11, (r["rc"], r["err"], r["ran"])      # the probe reports that conv11 ran
    assert np.isfinite(r["out"]).all(), "non-finite output (poison left in place?)"
    cf.Reference(op).check(r["out"], cf.R["f16x3"], f"{name} B=3 [f16x3] conv11")
    cf.check_stats(r["stat"], r["out"], f"{name} [f16x3] conv11")
    again = _run11(e, op)
    assert again["rc"] == 0 and _same_bits(again["out"], r["out"]) and np.array_equal(again["stat"], r["stat"]), "two runs of one case differ"
    for n in range(op["shape"][0]):
        one = _run11(e, _image(op, n))
        assert one["rc"] == 0 and one["ran"] == 11, one["err"]
        assert _same_bits(one["out"], r["out"][n:n + 1]), f"image {n} alone differs from image {n} of the batch"
        assert np.array_equal(one["stat"], r["stat"][n:n + 1]), f"statistics of image {n}"
    return r


_SHAPES = [(hw, cin, cout) for hw in ((8, 32), (16, 64)) for cin in (32, 64, 96) for cout in (128, 256)]


@pytest.mark.parametrize("case", range(len(_SHAPES)))
def test_layer_against_the_float64_statement(engines, case):
    """Every (tile count, period count, co-block count); the residual form cycles with the case so that each form meets both tile counts."""
    (H, W), cin, cout = _SHAPES[case]
    res_mode = (case + case // 6) % 4 - 1
    op = _operands(3, cin, cout, H, W, seed=1100 + case, res_mode=res_mode)
    _check_layer(engines("f16x3"), f"c11_{H}x{W}_cin{cin}_cout{cout}_res{res_mode}", op)


@pytest.mark.parametrize("res_mode", [-1, 0, 1, 2])
def test_every_residual_form_on_four_tiles_and_two_co_blocks(engines, res_mode):
    op = _operands(3, 64, 256, 16, 64, seed=1200 + res_mode, res_mode=res_mode)
    _check_layer(engines("f16x3"), f"c11_16x64_cin64_cout256_res{res_mode}", op)


def test_conv7_arm_of_the_probe_on_the_same_operands(engines):
    """Route 7 of the probe (what tools/conv11_layer_time.py times conv11 against) is conv7 on the same planes: same f16 products, another fp32
    summation order inside K, so both meet the budget and they differ by rounding only."""
    e = engines("f16x3")
    op = _operands(3, 96, 256, 16, 64, seed=1300, res_mode=0)
    a, b = _run11(e, op), _run11(e, op, route=7)
    assert a["rc"] == 0 and a["ran"] == 11 and b["rc"] == 0 and b["ran"] == 7, (a["err"], b["err"])
    ref = cf.Reference(op)
    ref.check(a["out"], cf.R["f16x3"], "conv11")
    ref.check(b["out"], cf.R["f16x3"], "conv7 arm")
    d, at = cf.E(a["out"], b["out"].astype(np.float64), ref.S)
    print(f"CONV11 - conv7: {d:.3e} of the budget at {at}")
    assert np.array_equal(a["stat"].shape, b["stat"].shape) and np.isfinite(b["stat"]).all()


# ------------------------------------------------------------------------------------------------ the hop
class _Pair:
    """Float64 statement of layer 1, GroupNorm32 + FiLM + SiLU, layer 2, and the second layer's budget."""

    def __init__(self, op):
        first64 = cf.layer(op, torch.float64)
        op2 = dict(cf.second_stage_op(op, first64.numpy()), film=op["film2"])
        x64 = cf.prologued(op2, torch.float64)
        self.ref = cf.layer(op2, torch.float64, x=x64)
        self.S = cf.budget(op2, x=x64)

    def E(self, got):
        return cf.E(got, self.ref, self.S)


def _unfused(e, op):
    """The existing route on the same operands: launch_conv6's own choice for the first layer (conv7), then the second layer behind
    gn_act_small (prologue 2; every shape here has at most 1024 pixels)."""
    B, cin, _, cout, H, W = op["shape"]
    r = _run3(e, op)
    assert r["rc"] == 0 and r["path"] in (6, 7), (r["rc"], r["err"], r["path"])
    op2 = dict(cf.second_stage_op(op, r["out"]), film=op["film2"], shape=(B, cout, 0, op["w2"].shape[0], H, W), scaled=False, res=None, prm=None, xb=None)
    r2 = _run3(e, op2)
    assert r2["rc"] == 0, r2["err"]
    return r2["out"]


@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("hw,cout", [((8, 32), 128), ((8, 32), 256), ((8, 32), 512), ((16, 64), 128), ((16, 64), 256)])
def test_hop_against_the_unfused_route(engines, hw, cout, film):
    """4, 8 and 16 channels per GroupNorm group; one tile, and 2 x 2 tiles (four workgroups wait for one another).  Bound: the fused route's
    error against the float64 pair statement is at most twice the unfused route's on the same operands (conv9's and conv_up's bound)."""
    e = engines("f16x3")
    H, W = hw
    op = _operands(3, 64, cout, H, W, seed=2100 + cout + H + int(film), second=32, film=film)
    pair = _Pair(op)
    r = _run11(e, op, hop=1)
    assert r["rc"] == 0 and r["ran"] == 12, (r["rc"], r["err"], r["ran"])
    assert np.isfinite(r["out2"]).all()
    e_fused, at = pair.E(r["out2"])
    e_unfused, _ = pair.E(_unfused(e, op))
    print(f"CONV11HOP {H}x{W} cout {cout} film {int(film)} [f16x3]: E fused {e_fused:.3e} at {at}, E unfused {e_unfused:.3e}, ratio {e_fused / e_unfused:.3f}")
    assert e_fused <= 2.0 * e_unfused, (e_fused, e_unfused)
    again = _run11(e, op, hop=1)
    assert again["rc"] == 0 and _same_bits(again["out2"], r["out2"]), "two runs of the hop differ"
    for n in range(3):
        one = _run11(e, _image(op, n), hop=1)
        assert one["rc"] == 0, one["err"]
        assert _same_bits(one["out2"], r["out2"][n:n + 1]), f"fused out2 of image {n} alone differs from the batch"


def test_hop_refuses_groups_that_straddle_waves(engines):
    """Cout = 384: 12 channels per GroupNorm group do not divide the 64 channels of a wave."""
    op = _operands(1, 32, 384, 8, 32, seed=5, second=32)
    r = _run11(engines("f16x3"), op, hop=1)
    assert r["rc"] != 0 and r["ran"] == 0 and b"GroupNorm groups inside a wave's 64 channels" in r["err"], (r["rc"], r["err"])


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("shape,ksplit,text", [
    ((1, 48, 128, 8, 32), 1, b"Cin must be a multiple of 32"),
    ((1, 32, 64, 8, 32), 1, b"Cout must be a multiple of 128"),
    ((1, 32, 128, 8, 16), 1, b"8 x 32 tiles inside the image"),
    ((1, 32, 128, 12, 32), 1, b"8 x 32 tiles inside the image"),
    ((1, 32, 128, 8, 32), 2, b"split-K launches keep conv6"),
])
def test_refused_shapes(engines, shape, ksplit, text):
    B, cin, cout, H, W = shape
    r = _run11(engines("f16x3"), _operands(B, cin, cout, H, W, seed=3), ksplit=ksplit)
    assert r["rc"] != 0 and r["ran"] == 0 and text in r["err"], (r["rc"], r["err"])


def test_refused_engines(engines):
    op = _operands(1, 32, 128, 8, 32, seed=4)
    r = _run11(engines("f16x3", grad=True), op)
    assert r["rc"] != 0 and r["ran"] == 0 and b"gradient-mode forward" in r["err"], (r["rc"], r["err"])
    r = _run11(engines("f32"), op)
    assert r["rc"] != 0 and r["ran"] == 0 and b"f32 precision" in r["err"], (r["rc"], r["err"])
    r = _run11(engines("f16x1"), op)
    assert r["rc"] != 0 and r["ran"] == 0 and b"f16x1 keeps conv7" in r["err"], (r["rc"], r["err"])


# ------------------------------------------------------------------------------------------------ forward level
_FWD_SNIPPET = r"""
import ctypes as C, json, sys, numpy as np, torch
sys.path.insert(0, {root!r})
import diffpir_amd
from diffpir_amd import _lib
from oracle import unet_oracle as uo
from tests.gpu_common import make_model
e = diffpir_amd.Engine(0); e.set_precision("f16x3")
make_model(e, uo.ffhq_hp())
g = torch.Generator().manual_seed(81)
x = torch.randn(({B}, 3, {size}, {size}), generator=g); t = torch.randint(0, 1000, ({B},), generator=g)
xd = e.to_device(x.numpy())
a = e.unet_forward(xd, t.numpy()).numpy()
first = _lib.route_log(e)
b = e.unet_forward(xd, t.numpy()).numpy()
log = _lib.route_log(e)
assert np.array_equal(a, b), "two forwards of the same input differ"
assert log == first, "two forwards of the same input took different routes"
taps = dict(out=a)
for name in {names!r}:
    taps[name] = e.read_tap(name)
c11 = [r for r in first + log if r["kernel"] == 11]       # conv11 launches of the two forwards: plain epilogue, fused hop
taps["launches"] = np.array([sum(r["hop"] == 0 for r in c11), sum(r["hop"] == 1 for r in c11)])
taps["routes"] = np.array(json.dumps(log))
np.savez({out!r}, **taps)
"""


def _forward_runs(tmp, B, size, names):
    runs = {}
    for tag, env in (("on", dict(DPIR_CONV11="1")), ("off", dict(DPIR_CONV11="0"))):
        out = str(tmp / f"{tag}_{size}.npz")
        r = subprocess.run([sys.executable, "-c", _FWD_SNIPPET.format(root=ROOT, names=names, out=out, B=B, size=size)], cwd=ROOT,
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        runs[tag] = dict(np.load(out))
    return runs


@pytest.fixture(scope="module")
def forwards(tmp_path_factory):
    """FFHQ topology at 64 x 64, B = 16: the 64 x 64 layers (128 -> 128, 256 -> 128) have 256 workgroups and route, with the plain epilogue.  One
    process per switch setting, two forwards each (compared bit for bit inside the process)."""
    from oracle import unet_oracle as uo
    hp = uo.ffhq_hp()
    sd = uo.synth_state_dict(hp, 0)
    g = torch.Generator().manual_seed(81)
    x = torch.randn((16, 3, 64, 64), generator=g)
    t = torch.randint(0, 1000, (16,), generator=g)
    sub = [0, 15]
    otaps = {}
    oref = uo.unet_forward(sd, hp, x[sub], t[sub], taps=otaps)
    names = [k for k in otaps if k != "emb"]
    return _forward_runs(tmp_path_factory.mktemp("conv11_fwd"), 16, 64, names), otaps, oref.numpy(), sub


@pytest.fixture(scope="module")
def forwards_hop(tmp_path_factory):
    """The same at 128 x 128, B = 8: the 128 x 128 ResBlocks have 512 workgroups, the hop's 384 are met."""
    return _forward_runs(tmp_path_factory.mktemp("conv11_fwd_hop"), 8, 128, [])


def test_forward_takes_the_routes(forwards, forwards_hop):
    on, off = forwards[0]["on"]["launches"], forwards[0]["off"]["launches"]
    hon, hoff = forwards_hop["on"]["launches"], forwards_hop["off"]["launches"]
    print(f"conv11 launches (plain, hop) in two forwards: 64^2 B=16 {list(on)}, 128^2 B=8 {list(hon)}")
    assert on[0] > 0 and on[1] == 0, "64 x 64 layers at B = 16: 256 workgroups, plain epilogue only"
    assert hon[0] > 0 and hon[1] > 0, "128 x 128 layers at B = 8: 512 workgroups, the hop is taken"
    assert list(off) == [0, 0] and list(hoff) == [0, 0], "DPIR_CONV11=0 must restore the old dispatch"


def _route_class(r):
    """A route-log record -> the kernel class a kernel trace shows for it (template EMIT argument -> hop)."""
    k = r["kernel"]
    if k == 0:
        return "fp32_3x3" if r["ks"] == 3 else "fp32_1x1"
    name = {5: "conv5", 6: "conv6", 7: "conv7", 17: "conv7_narrow", 8: "conv8", 9: "conv9", 11: "conv11", 12: "conv_up", 60: "resolve"}[k]
    return name + "_hop" if r["hop"] else name


@pytest.mark.parametrize("cfg", ["B16_64", "B8_128"])
def test_forward_launches_the_kernels_the_parent_commit_launched(forwards, forwards_hop, cfg):
    """The route log of one default forward, counted per kernel class, against tests/golden/conv_route_counts.json: the per-kernel launch counts of
    a rocprofv3 kernel trace of ONE eager forward of the commit BEFORE the planner existed (kernel names reduced to classes), same topology,
    precision, batch and size.  conv7's three tilings are one class here (the log does not carry the tiling)."""
    import json
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_route_counts.json")))[cfg]
    want = {}
    for k, v in golden.items():
        k = "conv7" if k.startswith("conv7_g") else k
        want[k] = want.get(k, 0) + v
    log = json.loads(str((forwards[0] if cfg == "B16_64" else forwards_hop)["on"]["routes"]))
    got = {}
    for r in log:
        c = _route_class(r)
        got[c] = got.get(c, 0) + 1
    print(f"route classes {cfg}: {dict(sorted(got.items()))}")
    assert got == want
    # split-K combines: every split launch is either finished by launch_conv6_resolve (a `resolve` record of the same layer right behind its
    # convolution's statistics kind 2 / 0) or left to the next layer's fused prologue (kind 3); the parent's trace has `resolve` conv6_reduce launches
    split = [r for r in log if r["ksplit"] > 1 and r["kernel"] in (6, 7)]
    pending = [r for r in split if r["stat_kind"] == 3]
    resolved = {r["layer"] for r in log if r["kernel"] == 60}
    assert len(resolved) == want.get("resolve", 0) and len(split) == len(pending) + len(resolved)
    assert {r["layer"] for r in split if r["stat_kind"] != 3} == resolved and not {r["layer"] for r in pending} & resolved


def test_forward_route_on_equals_route_off_to_the_fused_hop_bar(forwards, forwards_hop):
    from tests.gpu_common import rel_err
    for what, runs in (("64^2 B=16", forwards[0]), ("128^2 B=8", forwards_hop)):
        err = rel_err(runs["on"]["out"], runs["off"]["out"])
        print(f"conv11 on vs off, FFHQ {what} [f16x3]: rel err {err:.3e}")
        assert err < 5e-6


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
    print(f"conv11 on, FFHQ 64^2 B=16, images {sub} vs oracle: output {err:.3e}, worst block {worst[0]} {worst[1]:.3e}")
    assert err < TOL_LAYER
