"""-m gpu: the attention core (csrc/attn.hip), its backward (csrc/grad.hip: bgemm x4, softmax_rows, softmax_bwd_rows), the GroupNorm statistics and
table (csrc/norm.hip: gn_stats, gn_prm) and the GroupNorm + FiLM + SiLU backward (csrc/grad.hip: gn_bwd_reduce, gn_bwd_apply), one site at a time on
host operands through the product's own launchers (dpir_debug_attention, dpir_debug_groupnorm), against the float64 statements of
tests/attn_gn_f64.py, per element.

What is asserted for each case: the probe succeeds, every output is finite (the output buffers start out as NaN), each output is within
R x the error of the same statement evaluated in float32 on the CPU -- every element against its own magnitude budget --, no guard word around
any output buffer changed, image 0 of the batch equals the same image run alone bit for bit, and a second call equals the first bit for bit.

The cases are the ones the whole-network tests leave out: sharp softmax rows (a running-max rescale with alpha near 0, the winner in the last key
tile, logits near +200, probabilities that underflow), T no multiple of the 32-key tile / of the 64 x 64 and 16-deep tiles of the backward GEMMs,
a block with idle waves (T = 160), T = 1024 and 1000 (sixteen entries per lane in the softmax rows); GroupNorm planes with H W no multiple of 4
(scalar paths), the resampling adjoints, a group that straddles the two sources of a concat, a mean far from zero, zero variance, accumulation
into prior contents, `extra`, and groups split over two and three partial workgroups."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import attn_gn_f64 as ag

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def _bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return (a is None and b is None) or np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ attention
def _attn(e, qkv, dAtt=None, head_ch=64):
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, C3, T = qkv.shape
    out = np.full((B, C3 // 3, T), np.nan, np.float32)
    dqkv = None if dAtt is None else np.full((B, C3, T), np.nan, np.float32)
    d = _lib.AttentionDesc(B=B, C=C3 // 3, T=T, head_ch=head_ch, qkv=_ptr(qkv), dAtt=_ptr(dAtt), out=_ptr(out), dqkv=_ptr(dqkv))
    rc = dbg.dpir_debug_attention(e.h, C.byref(d))
    return dict(rc=rc, out=out, dqkv=dqkv, guard=int(d.guard_bad_out), err=e.lib.dpir_last_error(e.h) if rc else b"")


# name -> (family, T, B, C)
ATTN_CASES = {
    "01_mild_T8": ("mild", 8, 2, 64),
    "02_mild_T36": ("mild", 36, 2, 64),
    "03_mild_T64": ("mild", 64, 2, 64),
    "04_mild_T100": ("mild", 100, 2, 64),
    "05_mild_T160_idle_waves": ("mild", 160, 2, 64),
    "06_mild_T256": ("mild", 256, 2, 64),
    "07_mild_T100_two_heads_odd_batch": ("mild", 100, 3, 128),
    "08_peaked_T36": ("peaked", 36, 2, 64),
    "09_peaked_T100": ("peaked", 100, 2, 64),
    "10_peaked_T256": ("peaked", 256, 2, 64),
    "11_offset200_T100": ("offset200", 100, 2, 64),
    "12_ascending_T100": ("ascending", 100, 2, 64),
    "13_descending_T100": ("descending", 100, 2, 64),
    "14_late_winner_T100": ("late_winner", 100, 2, 64),
    "15_neg_last_tile_T100": ("neg_last_tile", 100, 2, 64),
    "16_mild_T1024": ("mild", 1024, 1, 64),
    "17_mild_T1000": ("mild", 1000, 1, 64),
}


@pytest.mark.parametrize("name", sorted(ATTN_CASES))
def test_attention_against_the_float64_statement(engine, name):
    family, T, B, Cc = ATTN_CASES[name]
    qkv, dA = ag.attn_inputs(family, B, Cc, T, seed=100 + sorted(ATTN_CASES).index(name))
    ref = ag.AttnReference(qkv, dA)
    r = _attn(engine, qkv, dA)
    assert r["rc"] == 0, (r["rc"], r["err"])
    assert np.isfinite(r["out"]).all() and np.isfinite(r["dqkv"]).all(), f"{name}: non-finite output (an element left unwritten?)"
    ref.out.check(r["out"], f"attention {name} out")
    for held, got, what in zip((ref.dq, ref.dk, ref.dv), ag.split_dqkv(r["dqkv"]), ("dq", "dk", "dv")):
        held.check(got, f"attention {name} {what}")
    assert r["guard"] == 0, f"{name}: {r['guard']} guard words around the output buffers changed"
    again = _attn(engine, qkv, dA)
    assert again["rc"] == 0 and again["guard"] == 0
    assert _same(again["out"], r["out"]) and _same(again["dqkv"], r["dqkv"]), f"{name}: two identical calls disagree"
    if B > 1:
        alone = _attn(engine, np.ascontiguousarray(qkv[:1]), np.ascontiguousarray(dA[:1]))
        assert alone["rc"] == 0 and alone["guard"] == 0
        assert _same(alone["out"][0], r["out"][0]) and _same(alone["dqkv"][0], r["dqkv"][0]), f"{name}: image 0 depends on the batch"


def test_attention_refusals(engine):
    qkv, dA = ag.attn_inputs("mild", 1, 64, 36, seed=1)
    r = _attn(engine, qkv, dA, head_ch=32)
    assert r["rc"] != 0 and b"only num_head_channels=64 is built" in r["err"], (r["rc"], r["err"])
    q96 = np.random.default_rng(2).standard_normal((1, 3 * 96, 36)).astype(np.float32)
    r = _attn(engine, q96)
    assert r["rc"] != 0 and b"channels not divisible by head channels" in r["err"], (r["rc"], r["err"])
    # the backward keeps sixteen entries of a row per lane: T <= 1024.  The forward of the same call runs (it has no such limit).
    qkv, dA = ag.attn_inputs("mild", 1, 64, 1025, seed=3)
    r = _attn(engine, qkv, dA)
    assert r["rc"] != 0 and b"T <= 1024" in r["err"], (r["rc"], r["err"])
    r = _attn(engine, qkv)
    assert r["rc"] == 0 and r["guard"] == 0
    ag.Held("attn_fwd", ag.attn_forward(qkv), ag.attn_forward_budget(qkv), ag.attn_forward(qkv, torch.float32)).check(r["out"], "attention T 1025 out")


# ------------------------------------------------------------------------------------------------ GroupNorm
def _gn(e, op):
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, ca, cb, Hs, Ws = op["B"], op["ca"], op["cb"], op["Hs"], op["Ws"]
    Cc = ca + cb
    prm = np.full((B, Cc, 4), np.nan, np.float32)
    stats = np.full((B, 32, 2), np.nan, np.float32)
    bwd = op.get("dA") is not None
    ga = np.full((B, ca, Hs, Ws), np.nan, np.float32) if bwd else None
    gb = np.full((B, cb, Hs, Ws), np.nan, np.float32) if bwd and cb else None
    d = _lib.GroupNormDesc(B=B, ca=ca, cb=cb, Hs=Hs, Ws=Ws, mode=op["mode"], silu=op["silu"], acc_a=op["acc_a"], acc_b=op["acc_b"])
    for k in ("xa", "xb", "gamma", "beta", "film", "dA", "ga_init", "gb_init", "extra"):
        setattr(d, k, _ptr(op.get(k)))
    d.prm_out, d.stats_out, d.ga_out, d.gb_out = _ptr(prm), _ptr(stats), _ptr(ga), _ptr(gb)
    rc = dbg.dpir_debug_groupnorm(e.h, C.byref(d))
    return dict(rc=rc, prm=prm, stats=stats, ga=ga, gb=gb, ns=int(d.ns_out), guard=int(d.guard_bad_out), err=e.lib.dpir_last_error(e.h) if rc else b"")


def _first_image(op):
    one = dict(op, B=1)
    for k in ("xa", "xb", "film", "dA", "ga_init", "gb_init", "extra"):
        if op.get(k) is not None:
            one[k] = np.ascontiguousarray(op[k][:1])
    return one


def _gn_case(shape, kind="mild", seed=0, mode=0, film=True, silu=1, acc=False, extra=False):
    op = ag.gn_inputs(kind, *shape, seed=seed, mode=mode, film=film)
    op["silu"] = silu
    r = np.random.default_rng(seed + 5000)
    if acc:
        op["acc_a"], op["ga_init"] = 1, r.standard_normal(op["xa"].shape).astype(np.float32)
        if op["xb"] is not None:
            op["acc_b"], op["gb_init"] = 1, r.standard_normal(op["xb"].shape).astype(np.float32)
    if extra:
        op["extra"] = r.standard_normal(op["xa"].shape).astype(np.float32)
    return op


GN_CASES = {}
for _i, _kind in enumerate(ag.GN_KINDS):
    for _film in (True, False):
        # H W = 35: the scalar statistics loop and the scalar backward
        GN_CASES[f"1_5x7_{_kind}_{'film' if _film else 'plain'}"] = dict(shape=(2, 64, 0, 5, 7), kind=_kind, film=_film, seed=200 + 2 * _i + _film)
    # float4 paths, three channels per group, odd batch
    GN_CASES[f"2_16x16_c96_{_kind}"] = dict(shape=(3, 96, 0, 16, 16), kind=_kind, seed=220 + _i)
GN_CASES.update({
    # 1024 float4 per plane: the 4-way unrolled statistics loop runs
    "3_64x64_c32": dict(shape=(1, 32, 0, 64, 64), seed=230),
    # the attention block's normalisation: no FiLM, no SiLU (the flag-off branch of the backward)
    "3_64x64_c32_affine": dict(shape=(1, 32, 0, 64, 64), seed=231, film=False, silu=0),
    # 96 channels over two sources of 40 and 56: group 13 (channels 39-41) straddles them
    "4_concat_40_56_8x8": dict(shape=(2, 40, 56, 8, 8), seed=232),
    "5_mode1_up_source_8x8": dict(shape=(2, 64, 0, 8, 8), seed=233, mode=1),
    "6_mode2_pool_source_16x16": dict(shape=(2, 64, 0, 16, 16), seed=234, mode=2),
    "7_accumulate_concat_8x8": dict(shape=(2, 40, 56, 8, 8), seed=235, acc=True),
    "7_accumulate_concat_5x7": dict(shape=(2, 40, 56, 5, 7), seed=236, acc=True),
    "7_extra_accumulate_8x8": dict(shape=(2, 64, 0, 8, 8), seed=237, acc=True, extra=True),
    "7_extra_5x7": dict(shape=(2, 64, 0, 5, 7), seed=238, extra=True),
    # two channels of 8200 per group, three partial workgroups: a share of 5467 rounded up to 5468, a boundary inside the first channel's plane
    "8_82x100_three_parts": dict(shape=(1, 64, 0, 82, 100), seed=239),
    "9_64x80_two_parts": dict(shape=(1, 64, 0, 64, 80), seed=240),
})
GN_PARTS = {"8_82x100_three_parts": 3, "9_64x80_two_parts": 2}


@pytest.mark.parametrize("name", sorted(GN_CASES))
def test_groupnorm_against_the_float64_statement(engine, name):
    kw = dict(GN_CASES[name])
    op = _gn_case(kw.pop("shape"), **kw)
    ref = ag.GnReference(op)
    r = _gn(engine, op)
    assert r["rc"] == 0, (r["rc"], r["err"])
    outs = [r["prm"], r["stats"], r["ga"]] + ([r["gb"]] if op["cb"] else [])
    assert all(np.isfinite(o).all() for o in outs), f"{name}: non-finite output (an element left unwritten?)"
    assert (r["prm"][..., 3] == float(op["silu"])).all()
    ref.y.check(ag.apply_table(op, r["prm"]), f"groupnorm {name} table")
    ref.check_stats(r["stats"], op, f"groupnorm {name} statistics")
    ref.ga.check(r["ga"], f"groupnorm {name} ga")
    if op["cb"]:
        ref.gb.check(r["gb"], f"groupnorm {name} gb")
    Cc, HW = op["ca"] + op["cb"], op["Hs"] * op["Ws"]
    assert r["ns"] == min(64, max(1, -(-(Cc // 32) * HW // 8192))) and r["ns"] == GN_PARTS.get(name, 1), r["ns"]
    assert r["guard"] == 0, f"{name}: {r['guard']} guard words around the output buffers changed"
    again = _gn(engine, op)
    assert again["rc"] == 0 and again["guard"] == 0
    assert all(_same(again[k], r[k]) for k in ("prm", "stats", "ga", "gb")), f"{name}: two identical calls disagree"
    if op["B"] > 1:
        alone = _gn(engine, _first_image(op))
        assert alone["rc"] == 0 and alone["guard"] == 0
        assert all(_same(alone[k][0], r[k][0]) for k in ("prm", "stats", "ga")), f"{name}: image 0 depends on the batch"
        assert not op["cb"] or _same(alone["gb"][0], r["gb"][0]), f"{name}: image 0 depends on the batch"


def test_groupnorm_refusals(engine):
    op = _gn_case((1, 48, 0, 8, 8), seed=1)
    r = _gn(engine, op)
    assert r["rc"] != 0 and b"gn_prm: channel bookkeeping" in r["err"], (r["rc"], r["err"])
    op = _gn_case((1, 32, 0, 7, 8), seed=2, mode=2)
    r = _gn(engine, op)
    assert r["rc"] != 0 and b"pooled source must be even" in r["err"], (r["rc"], r["err"])
