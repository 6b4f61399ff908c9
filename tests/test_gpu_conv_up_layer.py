"""-m gpu: conv_up (csrc/conv_up.hip), conv1 of an up-sampling ResBlock as four 2x2 phase convolutions of the source image, one layer at a
time on host operands (dpir_debug_conv_up_layer) against the float64 statement and the per-element budget of tests/conv3_f64.py (its layer()
with mode 1: R = 8 for f16x3; f16x1 against the statement with the COMBINED phase weights rounded to f16 after the pack's scale, written
below, with R["f16x1"]), the fused hop conv1 -> GroupNorm32 + FiLM + SiLU -> conv2 against the float64 statement of the pair with the existing
unfused route (dpir_debug_conv3_layer, mode 1) as the yardstick, and the forward with the route on against DPIR_CONV_UP=0 and the oracle.

Shapes are the smallest that reach each path: source 8 x 32 / 16 x 32 / 8 x 64 = one tile, a vertical and a horizontal tile seam; Cin 16 / 48 =
one chunk and three (the weight ring wraps across chunks, odd count); Cout 32 / 64 / 128 / 256 = a block with an idle wave pair, one block,
two and four blocks (with B = 1 and two tiles the grid is a multiple of 8: the XCD-aware numbering); one and three images.

Largest E(kernel) / E(float32) measured on MI355X: 1.232 (f16x3, R = 8), 0.990 (f16x1 against the f16-rounded phase statement, R = 4); the hop's
fused / unfused error ratios 0.84 - 1.26 (bound 2): profiles/conv_up/README.md."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

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


def _operands(B, cin, cout, Hs, Ws, seed, second=0, film=False):
    """conv3_f64's op of a mode-1 layer: xa at the source resolution, shape = (B, ca, cb, Cout, H, W) of the OUTPUT."""
    r = np.random.default_rng(seed)
    f = lambda *s: r.standard_normal(s).astype(np.float32)
    op = dict(shape=(B, cin, 0, cout, 2 * Hs, 2 * Ws), mode=1, res_mode=-1, scaled=False, prologue=0, xa=f(B, cin, Hs, Ws), xb=None,
              w=(0.05 * r.standard_normal((cout, cin, 3, 3))).astype(np.float32), bias=f(cout), res=None, prm=None, gamma=None, beta=None, film=None,
              film2=None)
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
    if op.get("film2") is not None:
        one["film2"] = np.ascontiguousarray(op["film2"][n:n + 1])
    return one


def _run_up(e, op, hop=0, force_hop=1, route=0, res=None):
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, cin, _, cout, H, W = op["shape"]
    out = np.full((B, cout, H, W), np.nan, np.float32)
    stat = np.full((B, cout, 2), np.nan, np.float64)
    d = _lib.ConvUpDesc(B=B, Cin=cin, Cout=cout, Hs=H // 2, Ws=W // 2, hop=hop, force_hop=force_hop, route=route)
    d.x, d.w, d.bias, d.prm, d.res = _ptr(op["xa"]), _ptr(op["w"]), _ptr(op["bias"]), _ptr(op["prm"]), _ptr(res)
    d.out, d.stat_out = _ptr(out), _ptr(stat)
    out2 = None
    if hop:
        d.Cout2 = op["w2"].shape[0]
        out2 = np.full((B, d.Cout2, H, W), np.nan, np.float32)
        for k in ("gamma2", "beta2", "film2", "w2", "bias2"):
            setattr(d, k, _ptr(op[k]))
        d.out2 = _ptr(out2)
    rc = dbg.dpir_debug_conv_up_layer(e.h, C.byref(d))
    return dict(rc=rc, out=out, stat=stat, out2=out2, ran=d.ran_out, err=e.lib.dpir_last_error(e.h) if rc else b"")


def _run3(e, op):
    """dpir_debug_conv3_layer: the existing routes (tests/test_gpu_conv3_layer.py::_run), no slab buffer."""
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


# ------------------------------------------------------------------------------------------------ the statements
def phase_weights(w64):
    """[a][b] -> the 2x2 filter [Cout][Cin][2][2] of output parity (a, b) = (y & 1, x & 1): a 3x3 convolution with zero padding 1 of the
    nearest-x2 up-sampled image reads, for output row 2i + a, the source rows i - 1, i with row weights w[0], w[1] + w[2] (a = 0) or the
    rows i, i + 1 with w[0] + w[1], w[2] (a = 1); the columns combine the same way.  Sums in float64."""
    rows = {0: [w64[:, :, 0:1], w64[:, :, 1:2] + w64[:, :, 2:3]], 1: [w64[:, :, 0:1] + w64[:, :, 1:2], w64[:, :, 2:3]]}
    out = {}
    for a in (0, 1):
        wr = torch.cat(rows[a], dim=2)                                  # [Cout][Cin][2][3]
        cols = {0: [wr[..., 0:1], wr[..., 1:2] + wr[..., 2:3]], 1: [wr[..., 0:1] + wr[..., 1:2], wr[..., 2:3]]}
        for b in (0, 1):
            out[(a, b)] = torch.cat(cols[b], dim=3)
    return out


def phase_layer(x, pw, bias, dt):
    """The four phase convolutions in dtype dt: x at the source resolution (already prologued), pw = phase_weights(...)."""
    B, _, Hs, Ws = x.shape
    y = torch.empty((B, bias.shape[0], 2 * Hs, 2 * Ws), dtype=dt)
    for (a, b), w in pw.items():
        xp = F.pad(x.to(dt), (1 - b, b, 1 - a, a))                      # a = 0: rows i - 1, i (pad above); a = 1: rows i, i + 1 (pad below)
        y[:, :, a::2, b::2] = F.conv2d(xp, w.to(dt))
    return y + bias.to(dt)[None, :, None, None]


class X1Reference:
    """f16x1: the activation operand (float32 as the kernels hold it, at the source resolution) and the COMBINED weights (float64 sums, times
    the pack's power-of-two scale of the combined maximum) rounded to float16 once; float64 statement, budget, float32 baseline."""

    def __init__(self, op):
        src = dict(op, mode=0)
        x = cf._f16(cf.prologued(src, torch.float64))
        pw = phase_weights(torch.from_numpy(op["w"]).to(torch.float64))
        s = float(cf.weight_scale(np.concatenate([v.numpy().astype(np.float32).ravel() for v in pw.values()])))
        # numpy rounds float64 -> float16 in one step (torch goes through float32, which can land on a tie the float64 value was not on)
        pw = {k: torch.from_numpy((v.numpy() * s).astype(np.float16).astype(np.float64)) / s for k, v in pw.items()}
        bias = torch.from_numpy(op["bias"]).to(torch.float64)
        self.ref = phase_layer(x, pw, bias, torch.float64)
        self.S = phase_layer(x.abs(), {k: v.abs() for k, v in pw.items()}, bias.abs(), torch.float64)
        self.base32 = phase_layer(x, pw, bias, torch.float32).numpy()
        self.e32, self.at32 = cf.E(self.base32, self.ref, self.S)

    measure = cf.Reference.measure
    check = cf.Reference.check


_refs = {}


def _reference(key, op, x1):
    k = (key, x1)
    if k not in _refs:
        _refs[k] = X1Reference(op) if x1 else cf.Reference(op)
    return _refs[k]


def test_phase_statement_is_the_3x3_on_the_up_sampled_image():
    """The float64 phase statement (exact weights) equals conv3_f64.layer with mode 1 to float64 rounding: the identity the kernel is built on."""
    op = _operands(2, 16, 32, 8, 32, seed=9)
    pw = phase_weights(torch.from_numpy(op["w"]).to(torch.float64))
    got = phase_layer(cf.prologued(dict(op, mode=0)), pw, torch.from_numpy(op["bias"]).to(torch.float64), torch.float64)
    ref = cf.layer(op, torch.float64)
    assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ single layer, plain epilogue
@pytest.mark.parametrize("prec", F16)
@pytest.mark.parametrize("cout", [32, 64, 128, 256])
@pytest.mark.parametrize("cin", [16, 48])
@pytest.mark.parametrize("src", [(8, 32), (16, 32), (8, 64)])
def test_layer_against_the_float64_statement(engines, src, cin, cout, prec):
    e = engines(prec)
    Hs, Ws = src
    name = f"cu_{Hs}x{Ws}_cin{cin}_cout{cout}"
    op = _operands(3, cin, cout, Hs, Ws, seed=3000 + Hs * 11 + Ws * 5 + cin * 7 + cout * 3)
    r = _run_up(e, op)
    assert r["rc"] == 0 and r["ran"] == 1, (r["rc"], r["err"])
    assert np.isfinite(r["out"]).all(), "non-finite output (poison left in place?)"
    x1 = prec == "f16x1"
    _reference(name, op, x1).check(r["out"], cf.R[prec], f"{name} B=3 [{prec}] conv_up" + (" vs the f16-rounded phase statement" if x1 else ""))
    cf.check_stats(r["stat"], r["out"], f"{name} [{prec}]")
    again = _run_up(e, op)
    assert again["rc"] == 0 and _same_bits(again["out"], r["out"]) and np.array_equal(again["stat"], r["stat"]), "two runs of one case differ"
    for n in range(3):
        one = _run_up(e, _image(op, n))
        assert one["rc"] == 0 and one["ran"] == 1, one["err"]
        assert _same_bits(one["out"], r["out"][n:n + 1]), f"image {n} alone differs from image {n} of the batch"
        assert np.array_equal(one["stat"], r["stat"][n:n + 1]), f"statistics of image {n}"


@pytest.mark.parametrize("prec", F16)
def test_layer_with_a_table_prologue_at_the_source_resolution(engines, prec):
    """GroupNorm + SiLU as a table, applied by act_split BEFORE the up-sampling, as the oracle's ResBlock does."""
    e = engines(prec)
    op = _operands(2, 48, 64, 16, 32, seed=41)
    r = np.random.default_rng(42)
    prm = np.empty((2, 48, 4), np.float32)
    prm[..., 0] = 0.1 * r.standard_normal((2, 48)); prm[..., 1] = 0.5 + r.random((2, 48)); prm[..., 2] = 0.1 * r.standard_normal((2, 48)); prm[..., 3] = 1.0
    op.update(prologue=1, prm=prm)
    got = _run_up(e, op)
    assert got["rc"] == 0 and got["ran"] == 1, got["err"]
    assert np.isfinite(got["out"]).all()
    ref = _reference("cu_table", op, False)
    if prec != "f16x1":
        ref.check(got["out"], cf.R[prec], f"table prologue [{prec}] conv_up")
        return
    # tests/test_gpu_conv3_layer.py's rule for f16x1 behind a prologue: the fp32 SiLU of the kernel and the float64 one of the statement can round to
    # different f16 values, so the bound is the format's -- each operand rounded once, |product error| <= (2^-11 + 2^-11 + 2^-22) |x||w|, and a
    # combined weight is at most the sum of the |w| the budget counts -- plus the fp32 accumulation term
    m = ref.measure(got["out"])
    print(f"CONV3X1 table prologue [f16x1] conv_up: E {m['E']:.3e} at {m['at']} (format bound 2^-10)")
    assert m["E"] <= 2.0 ** -10 + cf.R["f32"] * max(ref.e32, cf.FLOOR), f"E = {m['E']:.3e} at {m['at']}"


# ------------------------------------------------------------------------------------------------ the hop
class _Pair:
    """Float64 statement of conv1 (mode 1), GroupNorm32 + FiLM + SiLU, conv2, and the second layer's budget."""

    def __init__(self, op):
        first64 = cf.layer(op, torch.float64)
        op2 = dict(cf.second_stage_op(op, first64.numpy()), film=op["film2"])
        x64 = cf.prologued(op2, torch.float64)
        self.ref = cf.layer(op2, torch.float64, x=x64)
        self.S = cf.budget(op2, x=x64)

    def E(self, got):
        return cf.E(got, self.ref, self.S)


def _unfused(e, op):
    """The existing route on the same operands: up-sampled planes + launch_conv6 (dpir_debug_conv3_layer, mode 1), then the second layer behind
    gn_act_small (prologue 2) where it takes the shape, else behind the table gn_prm would build (float64 sums of the stored first layer)."""
    B, cin, _, cout, H, W = op["shape"]
    r = _run3(e, op)
    assert r["rc"] == 0 and r["path"] in (6, 7), (r["rc"], r["err"], r["path"])
    op2 = dict(cf.second_stage_op(op, r["out"]), film=op["film2"], shape=(B, cout, 0, op["w2"].shape[0], H, W), scaled=False, res=None, prm=None, xb=None)
    if H * W > 1024:
        v = r["out"].astype(np.float64).reshape(B, 32, -1)
        mean, var = v.mean(axis=2), v.var(axis=2)
        cg = cout // 32
        mean_c, rstd_c = np.repeat(mean, cg, axis=1), np.repeat(1.0 / np.sqrt(var + cf.GN_EPS), cg, axis=1)
        a = rstd_c.astype(np.float32) * op["gamma2"][None]
        b = np.broadcast_to(op["beta2"][None], a.shape).astype(np.float32)
        if op["film2"] is not None:
            sc = np.float32(1.0) + op["film2"][:, :cout]
            a, b = a * sc, b * sc + op["film2"][:, cout:]
        prm = np.stack([mean_c.astype(np.float32), a.astype(np.float32), b.astype(np.float32), np.ones_like(a, dtype=np.float32)], axis=2)
        op2.update(prologue=1, prm=np.ascontiguousarray(prm), gamma=None, beta=None, film=None)
    r2 = _run3(e, op2)
    assert r2["rc"] == 0, r2["err"]
    return r2["out"]


@pytest.mark.parametrize("prec", F16)
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("src,cout", [((8, 32), 128), ((8, 32), 256), ((16, 64), 128)])
def test_hop_against_the_unfused_route(engines, src, cout, film, prec):
    """4 and 8 channels per GroupNorm group; one source tile, and 2 x 2 tiles (8 workgroups wait for one another).  Bound: the fused route's
    error against the float64 pair statement is at most twice the unfused route's on the same operands."""
    e = engines(prec)
    Hs, Ws = src
    op = _operands(3, 48, cout, Hs, Ws, seed=4000 + cout + int(film) + Hs, second=32, film=film)
    pair = _Pair(op)
    r = _run_up(e, op, hop=1)
    assert r["rc"] == 0 and r["ran"] == 2, (r["rc"], r["err"])
    assert np.isfinite(r["out2"]).all()
    e_fused, at = pair.E(r["out2"])
    e_unfused, _ = pair.E(_unfused(e, op))
    print(f"CONVUPHOP src {Hs}x{Ws} cout {cout} film {int(film)} [{prec}]: E fused {e_fused:.3e} at {at}, E unfused {e_unfused:.3e}, ratio {e_fused / e_unfused:.3f}")
    assert e_fused <= 2.0 * e_unfused, (e_fused, e_unfused)
    again = _run_up(e, op, hop=1)
    assert again["rc"] == 0 and _same_bits(again["out2"], r["out2"]), "two runs of the hop differ"
    for n in range(3):
        one = _run_up(e, _image(op, n), hop=1)
        assert one["rc"] == 0, one["err"]
        assert _same_bits(one["out2"], r["out2"][n:n + 1]), f"fused out2 of image {n} alone differs from the batch"


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("shape,hop,force,text", [
    ((1, 16, 32, 8, 16), 0, 1, b"source width must be a multiple of 32"),
    ((1, 16, 32, 4, 32), 0, 1, b"source height must be a multiple of 8"),
    ((1, 40, 32, 8, 32), 0, 1, b"input channels must be a multiple of 16"),
    ((1, 16, 48, 8, 32), 0, 1, b"output channels must be a multiple of 32"),
    ((1, 16, 96, 8, 32), 1, 1, b"must not straddle a wave's 32 channels"),
    ((1, 16, 384, 8, 32), 1, 1, b"must not straddle a wave's 32 channels"),
    ((1, 16, 128, 8, 32), 1, 0, b"too few workgroups for the hop"),
    ((1, 16, 128, 256, 256), 1, 1, b"wait set exceeds half of the resident workgroups"),
])
def test_refused_shapes(engines, shape, hop, force, text):
    B, cin, cout, Hs, Ws = shape
    op = _operands(B, cin, cout, Hs, Ws, seed=3, second=32 if hop else 0)
    r = _run_up(engines("f16x3"), op, hop=hop, force_hop=force)
    assert r["rc"] != 0 and r["ran"] == 0 and text in r["err"], (r["rc"], r["err"])


def test_refused_residual_and_engines(engines):
    op = _operands(1, 16, 32, 8, 32, seed=4)
    r = _run_up(engines("f16x3"), op, res=np.zeros((1, 32, 16, 64), np.float32))
    assert r["rc"] != 0 and r["ran"] == 0 and b"takes no residual" in r["err"], (r["rc"], r["err"])
    r = _run_up(engines("f16x3", grad=True), op)
    assert r["rc"] != 0 and r["ran"] == 0 and b"gradient-mode engine" in r["err"], (r["rc"], r["err"])
    r = _run_up(engines("f32"), op)
    assert r["rc"] != 0 and r["ran"] == 0 and b"f32 precision" in r["err"], (r["rc"], r["err"])


# ------------------------------------------------------------------------------------------------ forward level
_FWD_SNIPPET = r"""
import ctypes as C, sys, numpy as np, torch
sys.path.insert(0, {root!r})
import diffpir_amd
from diffpir_amd import _lib
from oracle import unet_oracle as uo
from tests.gpu_common import make_model
e = diffpir_amd.Engine(0); e.set_precision("f16x3")
make_model(e, uo.ffhq_hp())
g = torch.Generator().manual_seed(79)
x = torch.randn((8, 3, 128, 128), generator=g); t = torch.randint(0, 1000, (8,), generator=g)
xd = e.to_device(x.numpy())
a = e.unet_forward(xd, t.numpy()).numpy()
log = _lib.route_log(e)
b = e.unet_forward(xd, t.numpy()).numpy()
log += _lib.route_log(e)
assert np.array_equal(a, b), "two forwards of the same input differ"
taps = dict(out=a)
for name in {names!r}:
    taps[name] = e.read_tap(name)
ups = [r for r in log if r["kernel"] == 12]       # conv_up launches of the two forwards: plain epilogue, fused hop
taps["launches"] = np.array([sum(r["hop"] == 0 for r in ups), sum(r["hop"] == 3 for r in ups)])
np.savez({out!r}, **taps)
"""


@pytest.fixture(scope="module")
def forwards(tmp_path_factory):
    """FFHQ topology at 128 x 128, B = 8: the up-sampling ResBlocks with a 64 x 64 source (128 channels, 512 workgroups: the hop) and a
    32 x 32 source (256 channels, 256 workgroups: below the hop's 384, the plain epilogue behind gn_act_small); the lower ones (source widths
    16, 8, 4) keep the old route.  One process per switch setting, two forwards each."""
    from oracle import unet_oracle as uo
    hp = uo.ffhq_hp()
    sd = uo.synth_state_dict(hp, 0)
    g = torch.Generator().manual_seed(79)
    x = torch.randn((8, 3, 128, 128), generator=g)
    t = torch.randint(0, 1000, (8,), generator=g)
    sub = [5]
    otaps = {}
    oref = uo.unet_forward(sd, hp, x[sub], t[sub], taps=otaps)
    names = [k for k in otaps if k != "emb"]
    tmp = tmp_path_factory.mktemp("conv_up_fwd")
    runs = {}
    for tag, env in (("on", dict(DPIR_CONV_UP="1")), ("off", dict(DPIR_CONV_UP="0")), ("on_nohop", dict(DPIR_CONV_UP="1", DPIR_FUSE_H1="0"))):
        out = str(tmp / f"{tag}.npz")
        r = subprocess.run([sys.executable, "-c", _FWD_SNIPPET.format(root=ROOT, names=names, out=out)], cwd=ROOT, env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        runs[tag] = dict(np.load(out))
    return runs, otaps, oref.numpy(), sub


def test_forward_takes_the_routes(forwards):
    runs = forwards[0]
    assert list(runs["on"]["launches"]) == [2, 2], "two forwards: one plain and one hop launch each"
    assert list(runs["on_nohop"]["launches"]) == [4, 0], "two forwards without the hop: two plain launches each"
    assert list(runs["off"]["launches"]) == [0, 0], "DPIR_CONV_UP=0 must restore the old dispatch"


def test_forward_route_on_against_route_off(forwards):
    """The on / off difference is recorded, not bounded by a number chosen in advance: both are held to the oracle below."""
    from tests.gpu_common import rel_err
    runs = forwards[0]
    for tag in ("on", "on_nohop"):
        print(f"conv_up {tag} vs off, FFHQ 128^2 B=8 [f16x3]: rel err {rel_err(runs[tag]['out'], runs['off']['out']):.3e}")
        assert np.isfinite(runs[tag]["out"]).all()


@pytest.mark.parametrize("tag", ["on", "on_nohop"])
def test_forward_block_outputs_meet_the_layer_tolerance(forwards, tag):
    from tests.gpu_common import rel_err
    runs, otaps, oref, sub = forwards
    worst = ("", 0.0)
    for name, tv in otaps.items():
        if name == "emb":
            continue
        got = runs[tag][name].reshape((8,) + tuple(tv.shape[1:]))[sub]
        err = rel_err(got, tv.numpy())
        worst = max(worst, (name, err), key=lambda p: p[1])
        assert err < TOL_LAYER, f"layer {name}: rel err {err:.3e}"
    err = rel_err(runs[tag]["out"][sub], oref)
    print(f"conv_up {tag}, FFHQ 128^2 B=8, image {sub} vs oracle: output {err:.3e}, worst block {worst[0]} {worst[1]:.3e}")
    assert err < TOL_LAYER
