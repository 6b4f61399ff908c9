"""The planner of the 3x3 convolution routes (csrc/conv_plan.cpp, through dpir_debug_conv3_plan / dpir_debug_resblock_plan: no engine, no GPU)
against the Python statement of the dispatch in tests/conv_route_rules.py, which is written from the documents: on a full grid of shapes and
engine states, at every threshold explicitly, with each route switched off, and on the ResBlock kinds of the FFHQ topology."""
import ctypes as C
import itertools

import numpy as np
import pytest

from diffpir_amd import _lib
from tests import conv_route_rules as rr

PLAN_FIELDS = ("kernel", "hop", "geo", "ksplit", "chunks_per_split", "stat_kind", "stat_slots", "refused")
QUERY_DT = np.dtype([(n, np.int32) for n in _lib.CONV3_QUERY_FIELDS] + [("slab_floats", np.int64)])
PLAN_DT = np.dtype([(n, np.int32) for n in PLAN_FIELDS] + [("workgroups", np.int64)])
SLAB = 16 * 1024 * 1024         # the forward's slab buffer, in floats
PREC = {"f32": 0, "f16x3": 1, "f16x1": 2}


def test_struct_layouts():
    assert QUERY_DT.itemsize == C.sizeof(_lib.Conv3Query) and PLAN_DT.itemsize == C.sizeof(_lib.ConvPlan)


def _knobs(**kw):
    k = _lib.ConvKnobs()
    _lib.load_debug().dpir_debug_conv_knobs_default(C.byref(k))
    assert {n: getattr(k, n) for n, _ in k._fields_} == rr.KNOBS, "the built-in defaults are the documented ones"
    for n, v in kw.items():
        setattr(k, n, v)
    return k, dict(rr.KNOBS, **kw)


def _plans(queries, knobs=None, caps=(512, 512, 512)):
    """list of query dicts -> list of plan dicts, one library call"""
    qa = np.zeros(len(queries), QUERY_DT)
    for n in QUERY_DT.names:
        qa[n] = [q.get(n, 0) for q in queries]
    out = np.zeros(len(queries), PLAN_DT)
    rc = _lib.load_debug().dpir_debug_conv3_plan(qa.ctypes.data, len(queries), None if knobs is None else C.byref(knobs), *caps, out.ctypes.data)
    assert rc == 0
    return [dict(zip(PLAN_DT.names, (int(v) for v in row))) for row in out.tolist()]


def _query(B, cin, cout, H, W, prec="f16x3", grad=0, slab=1, hop=0, **kw):
    """A layer as Fwd describes it: the packs load_conv makes, statistics buffers where the output can carry them."""
    p = PREC[prec]
    q = dict(B=B, Cin=cin, Cout=cout, H=H, W=W, precision=p, grad=grad, w16=int(p != 0), w8=0,
             w11=int(p == 1 and cin % 32 == 0 and cout % 128 == 0), conv8_source=0, defer=1, hop=hop, has_res=0,
             stats=int(rr.stat_slots(H, W) > 0 and cout % 32 == 0 and not hop), force_kernel=0, slab_floats=SLAB if slab and not hop else 0)
    q.update(kw)
    return q


def _same(got, want, what):
    if want["refused"]:
        assert got["refused"] == 1, (what, got)
        return
    for k, v in want.items():
        assert got[k] == v, (what, k, got, want)


GRID_B = (1, 2, 3, 4, 5, 8, 16, 32, 64)
GRID_C = (3, 6, 16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 640, 1024)
GRID_HW = [(s, s) for s in (4, 8, 12, 16, 24, 32, 40, 64, 128, 256)] + [(8, 32), (16, 64), (32, 8), (12, 20), (64, 128), (8, 16)]


@pytest.mark.parametrize("cap", [512, 64])
@pytest.mark.parametrize("prec", sorted(PREC))
def test_grid_equals_the_documented_rules(prec, cap):
    caps = (cap, cap, cap)
    queries = [_query(B, cin, cout, H, W, prec, grad, slab, hop)
               for B, cin, cout, (H, W), grad, slab, hop in itertools.product(GRID_B, GRID_C, GRID_C, GRID_HW, (0, 1), (0, 1), (0, 1))]
    plans = _plans(queries, caps=caps)
    kernels = set()
    for q, got in zip(queries, plans):
        _same(got, rr.plan(q, rr.KNOBS, caps), q)
        kernels.add((got["kernel"], got["hop"], got["refused"]))
    if prec == "f32":
        assert kernels == {(0, 0, 0), (0, 0, 1)}
    else:       # the grid reaches every route (conv8 and conv_up have cases of their own below)
        want = {(0, 0, 0), (6, 0, 0), (7, 0, 0), (17, 0, 0), (9, 0, 0), (9, 1, 0), (7, 1, 0), (0, 0, 1)} | ({(11, 0, 0), (11, 1, 0)} if prec == "f16x3" else set())
        assert kernels == want, kernels ^ want


def _one(q, knobs=None, kd=rr.KNOBS, caps=(512, 512, 512)):
    got = _plans([q], knobs, caps)[0]
    _same(got, rr.plan(q, kd, caps), q)
    return got


def test_split_rule_at_255_and_256_workgroups():
    # 16 x 16 geometry, Cout 128: one workgroup per image
    a, b = _one(_query(255, 256, 128, 16, 16, "f16x1")), _one(_query(256, 256, 128, 16, 16, "f16x1"))
    assert (a["kernel"], a["ksplit"], a["workgroups"], a["stat_kind"]) == (7, 2, 510, 3)
    assert (b["kernel"], b["ksplit"], b["workgroups"], b["stat_kind"]) == (7, 1, 256, 1)
    # 8 x 32 geometry: a split launch runs on conv6
    c = _one(_query(15, 256, 256, 32, 64, "f16x1"))
    assert (c["kernel"], c["ksplit"], c["workgroups"]) == (6, 2, 480)


def test_hop_at_383_and_384_workgroups():
    # 64 x 32: 8 tiles per image, Cout 128 -> 8 workgroups per image
    for prec, kernel in (("f16x3", 11), ("f16x1", 7)):
        a, b = _plans([_query(47, 128, 128, 64, 32, prec, hop=1), _query(48, 128, 128, 64, 32, prec, hop=1)])
        assert a["refused"] == 1 and (b["refused"], b["kernel"], b["hop"], b["workgroups"]) == (0, kernel, 1, 384)
    # the wait set: 64 x 128 has 32 tiles per image, half of 64 resident workgroups just holds them; 33 do not fit
    assert _one(_query(16, 128, 128, 64, 128, hop=1), caps=(64, 64, 64))["kernel"] == 11
    assert _one(_query(16, 128, 128, 64, 128, hop=1), caps=(64, 62, 64))["kernel"] == 7       # conv11 refuses, conv7's own capacity allows
    assert _one(_query(16, 128, 128, 64, 128, hop=1), caps=(62, 62, 64))["refused"] == 1


def test_conv9_at_127_and_128_workgroups():
    a, b = _one(_query(127, 64, 32, 8, 8)), _one(_query(128, 64, 32, 8, 8))
    assert (a["kernel"], a["geo"]) == (7, 2) and (b["kernel"], b["workgroups"], b["stat_kind"]) == (9, 128, 2)
    assert _one(_query(8, 512, 512, 8, 8))["kernel"] == 9 and _one(_query(8, 512, 512, 8, 8, grad=1))["kernel"] == 7


@pytest.mark.parametrize("cout,fits64,fits32", [(256, True, True), (384, False, False), (512, True, True), (640, False, False), (1024, True, True), (2048, True, False)])
def test_groups_that_straddle_a_wave(cout, fits64, fits32):
    q = _query(16, 128, cout, 64, 64, hop=1)
    assert (_one(q)["refused"] == 0) == fits64
    q9 = _query(16, 128, cout, 8, 8, hop=1)
    got = _one(q9)
    assert (got["refused"] == 0 and got["kernel"] == 9) == fits32


def test_idle_half_and_narrow():
    assert _one(_query(16, 64, 160, 64, 64, slab=0))["kernel"] == 6        # 160 = 128 + 32 live channels in the last block: at most 64, conv6's idle-half class
    assert _one(_query(16, 64, 192, 64, 64, slab=0))["kernel"] == 6        # 64 live channels: still the idle-half class
    assert _one(_query(16, 64, 200, 64, 64, slab=0))["kernel"] == 7        # 72 live channels: off
    assert _one(_query(16, 64, 160, 16, 16, slab=0))["kernel"] == 7        # the class exists in the 8 x 32 geometry only
    for cout in (3, 6, 32):
        assert _one(_query(16, 128, cout, 64, 64))["kernel"] == 17
    assert _one(_query(16, 128, 6, 16, 16))["kernel"] == 7                 # narrow exists in the 8 x 32 geometry only
    assert _one(_query(16, 128, 33, 64, 64))["kernel"] == 6


def test_slab_too_small_for_the_split():
    q = _query(4, 512, 512, 32, 32)         # 64 workgroups: four slabs of 4 x 512 x 32 x 32 floats
    assert _one(q)["ksplit"] == 4 and _one(dict(q, slab_floats=4 * 4 * 512 * 32 * 32))["ksplit"] == 4
    small = dict(q, slab_floats=4 * 4 * 512 * 32 * 32 - 1)
    got = _one(small)
    assert (got["ksplit"], got["kernel"], got["stat_kind"]) == (1, 7, 1)


def test_conv11_refuses_an_odd_number_of_chunks():
    assert _one(_query(16, 128, 128, 64, 64))["kernel"] == 11
    assert _one(_query(16, 48, 128, 64, 64, w11=1))["kernel"] == 7
    assert _one(_query(16, 128, 128, 64, 64, "f16x1", w11=1))["kernel"] == 7
    assert _one(_query(16, 128, 128, 64, 64, w11=0))["kernel"] == 7


CONV8_Q = dict(w8=1, conv8_source=1, slab=1)


def test_conv8_takes_the_output_layer():
    got = _one(_query(16, 128, 6, 64, 64, **CONV8_Q))
    assert (got["kernel"], got["workgroups"]) == (8, 16 * 2 * 8)
    assert _one(_query(16, 128, 6, 64, 64, grad=1, **CONV8_Q))["kernel"] == 17
    assert _one(_query(16, 128, 6, 64, 64, **dict(CONV8_Q, conv8_source=0)))["kernel"] == 17
    assert _one(_query(16, 320, 6, 64, 64, **CONV8_Q))["kernel"] == 17


@pytest.mark.parametrize("knob,q,on,off", [
    ("conv8", _query(16, 128, 6, 64, 64, **CONV8_Q), 8, 17),
    ("conv9", _query(16, 512, 512, 8, 8), 9, 7),
    ("conv11", _query(16, 128, 128, 64, 64), 11, 7),
])
def test_a_route_switched_off_gives_the_previous_dispatch(knob, q, on, off):
    assert _one(q)["kernel"] == on
    k, kd = _knobs(**{knob: 0})
    got = _one(q, k, kd)
    assert got["kernel"] == off
    if knob == "conv9":     # back on launch_conv6's split-K route: 4 workgroups, 16 slabs, combine left to the consumer
        assert (got["ksplit"], got["stat_kind"]) == (16, 3)


def test_split_knobs_move_all_routes():
    k, kd = _knobs(split_below=384, split_target=512)
    q = _query(16, 128, 128, 64, 64)        # 256 workgroups
    got = _one(q, k, kd)
    assert (got["kernel"], got["ksplit"]) == (6, 2)


# ---------------------------------------------------------------------------------------------------- ResBlocks
def _resblock(q, knobs=None, kd=rr.KNOBS, caps=(512, 512, 512)):
    d = _lib.ResblockQuery(**q)
    out = _lib.ResblockPlan()
    assert _lib.load_debug().dpir_debug_resblock_plan(C.byref(d), None if knobs is None else C.byref(knobs), *caps, C.byref(out)) == 0
    got = dict(up=out.up, skip_emit=out.skip_emit, hop=out.hop)
    for name in ("conv1", "conv2"):
        p = getattr(out, name)
        got[name] = {n: getattr(p, n) for n in PLAN_FIELDS + ("workgroups",)}
    want = rr.resblock(q, kd, caps)
    assert {k: got[k] for k in ("up", "skip_emit", "hop")} == {k: want[k] for k in ("up", "skip_emit", "hop")}, (q, got, want)
    for name in ("conv1", "conv2"):
        for k, v in want[name].items():
            assert got[name][k] == v, (q, name, k, got[name], want[name])
    return got


def _rq(B, cin, cout, size, mode=0, concat=0, prec="f16x3", grad=0):
    return dict(B=B, Cin=cin, Cout=cout, H=size, W=size, mode=mode, concat=concat, precision=PREC[prec], grad=grad, hop_allowed=int(not grad and prec != "f32"),
                arena_words_left=B * 4096, slab_floats=SLAB)


@pytest.mark.parametrize("B,size", [(16, 64), (8, 128)])
def test_resblock_kinds_of_the_ffhq_topology(B, size):
    """The four ResBlock kinds at the top resolution of the two forward-level test configurations (FFHQ: 128 channels there)."""
    hop = B * (size // 32) * (size // 8) >= rr.HOP_MIN_WG       # 256 workgroups at (16, 64^2): no hop; 512 at (8, 128^2)
    plain = _resblock(_rq(B, 128, 128, size))
    assert (plain["up"], plain["skip_emit"], plain["hop"]) == (0, 0, int(hop)) and plain["conv1"]["kernel"] == plain["conv2"]["kernel"] == 11
    assert plain["conv1"]["hop"] == int(hop)
    skip = _resblock(_rq(B, 256, 128, size, concat=1))
    assert (skip["up"], skip["skip_emit"], skip["hop"]) == (0, 1, int(hop)) and skip["conv1"]["kernel"] == 11
    down = _resblock(_rq(B, 128, 128, size, mode=2))
    assert (down["up"], down["skip_emit"], down["hop"]) == (0, 0, 0)
    up = _resblock(_rq(B, 128, 128, size // 2, mode=1))
    wgs = B * (size // 64) * (size // 16) * 2 * 2
    assert up["up"] == int(wgs >= 256) and up["hop"] == (3 if wgs >= rr.HOP_MIN_WG else 0)
    if up["up"]:
        assert up["conv1"]["kernel"] == 12 and up["conv1"]["workgroups"] == wgs
    # 8 x 8 blocks deeper in the same forwards: conv9 with its in-workgroup hop
    deep = _resblock(_rq(B, 512, 512, 8))
    assert (deep["hop"], deep["conv1"]["kernel"], deep["conv2"]["kernel"]) == (2, 9, 9)
    for q in (_rq(B, 128, 128, size, grad=1), _rq(B, 128, 128, size, prec="f32"), _rq(B, 128, 128, size // 2, mode=1, prec="f16x1")):
        _resblock(q)


def test_conv_up_switched_off_and_following_the_split_knob():
    q = _rq(8, 128, 128, 64, mode=1)         # 8 x 2 x 8 x 2 x 2 = 512 workgroups
    assert _resblock(q)["hop"] == 3
    k, kd = _knobs(conv_up=0)
    off = _resblock(q, k, kd)
    assert (off["up"], off["conv1"]["kernel"]) == (0, 11)
    k, kd = _knobs(fuse_h1=0)
    assert _resblock(q, k, kd)["hop"] == 0 and _resblock(_rq(8, 512, 512, 8), k, kd)["hop"] == 0
    small = _rq(4, 128, 128, 64, mode=1)     # 256 workgroups: taken at the default, not with split_below = 384
    assert _resblock(small)["up"] == 1
    k, kd = _knobs(split_below=384)
    assert _resblock(small, k, kd)["up"] == 0
