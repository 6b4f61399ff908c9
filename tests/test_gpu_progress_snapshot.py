"""-m gpu: dpir_progress_snapshot (csrc/progress.hip) on raw arrays against numpy float32, bit for bit: the f32 and uint8 panels at their
column offset of the strip, the masked pair, the per-image max / min, every byte outside the panel left alone, and the argument refusals."""
import ctypes as C

import numpy as np
import pytest

from diffpir_amd.engine import EngineError

pytestmark = pytest.mark.gpu
F = np.float32
SENT_F, SENT_U = F(-7.25), np.uint8(0xA5)
# (B, H, W, P, panels): scalar path with fewer than one wave per image and an odd pitch; the 16-byte path; W % 4 == 0 with a pitch that keeps
# alignment at every panel; the 16-byte path over more than one workgroup per image (64 * 64 / 4 = 1024 groups)
SHAPES = [(3, 5, 7, 11, (0, 5, 10)), (2, 64, 64, 11, (0, 5, 10)), (1, 8, 12, 3, (0, 1, 2))]


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


def to_u8(v):
    return np.rint(np.clip(v, F(0), F(1)) * F(255)).astype(np.uint8)


def expected(x, y, m, strips, p, W):
    """numpy float32 statement of one snapshot into copies of the four strips and the minmax table"""
    f32, u8, mf32, mu8, mm = (None if a is None else a.copy() for a in strips)
    v = x / F(2) + F(0.5)
    cols = slice(p * W, (p + 1) * W)
    if f32 is not None:
        f32[..., cols] = v
    if u8 is not None:
        u8[:, :, cols, :] = to_u8(v).transpose(0, 2, 3, 1)
    if mf32 is not None or mu8 is not None:
        mf = m.astype(F)
        mv = y * mf + (F(1) - mf) * v
        if mf32 is not None:
            mf32[..., cols] = mv
        if mu8 is not None:
            mu8[:, :, cols, :] = to_u8(mv).transpose(0, 2, 3, 1)
    if mm is not None:
        mm[p, :, 0] = v.max(axis=(1, 2, 3))
        mm[p, :, 1] = v.min(axis=(1, 2, 3))
    return f32, u8, mf32, mu8, mm


def run(engine, x, y, m, p, P, want=(True, True, True, True, True)):
    B, _, H, W = x.shape
    host = [np.full((B, 3, H, P * W), SENT_F, F), np.full((B, H, P * W, 3), SENT_U, np.uint8), np.full((B, 3, H, P * W), SENT_F, F),
            np.full((B, H, P * W, 3), SENT_U, np.uint8), np.full((P, B, 2), SENT_F, F)]
    host = [a if w else None for a, w in zip(host, want)]
    dev = [None if a is None else engine.to_device(a) for a in host]
    engine.progress_snapshot(engine.to_device(x), p, P, strip_f32=dev[0], strip_u8=dev[1], y=None if y is None else engine.to_device(y),
                             mask=None if m is None else engine.to_device(m, np.uint8), masked_f32=dev[2], masked_u8=dev[3], minmax=dev[4])
    engine.sync()
    got = [None if d is None else d.numpy() for d in dev]
    exp = expected(x, y, m, host, p, W)
    for name, g, e in zip(("strip_f32", "strip_u8", "masked_f32", "masked_u8", "minmax"), got, exp):
        if g is not None:
            assert g.tobytes() == e.tobytes(), f"{name} differs at panel {p} of {P}: {np.argwhere(g != e)[:4].tolist()}"
    return got


def inputs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, 3, H, W)) * 1.2).astype(F)           # x/2+.5 leaves [0, 1] on both sides: the uint8 clamp is exercised
    y = rng.random((B, 3, H, W)).astype(F)
    m = (rng.random((B, 3, H, W)) < 0.6).astype(np.uint8)
    return x, y, m


@pytest.mark.parametrize("B,H,W,P,panels", SHAPES)
def test_panel_equals_numpy_and_leaves_the_rest_of_the_strip_alone(engine, B, H, W, P, panels):
    x, y, m = inputs(B, H, W, 1)
    for p in panels:
        run(engine, x, y, m, p, P)


@pytest.mark.parametrize("B,H,W,P,panels", SHAPES)
@pytest.mark.parametrize("mask", ["zeros", "ones"])
def test_all_zero_and_all_one_masks(engine, B, H, W, P, panels, mask):
    x, y, _ = inputs(B, H, W, 2)
    m = (np.zeros if mask == "zeros" else np.ones)((B, 3, H, W), np.uint8)
    got = run(engine, x, y, m, panels[1], P)
    cols = slice(panels[1] * W, (panels[1] + 1) * W)
    if mask == "zeros":
        assert got[2][..., cols].tobytes() == got[0][..., cols].tobytes()           # nothing known: the masked panel is the panel
    else:
        assert got[2][..., cols].tobytes() == y.tobytes()                             # everything known: y itself


@pytest.mark.parametrize("B,H,W,P,panels", SHAPES)
def test_minmax_extremes(engine, B, H, W, P, panels):
    """Extremes at the first and the last element of an image, an all-equal image, an all-negative image."""
    rng = np.random.default_rng(3)
    cases = []
    a = rng.uniform(-1, 1, (B, 3, H, W)).astype(F)
    a[:, 0, 0, 0], a[:, -1, -1, -1] = F(5.5), F(-6.5)                  # max first, min last
    cases.append(a)
    b = a.copy()
    b[:, 0, 0, 0], b[:, -1, -1, -1] = F(-6.5), F(5.5)                  # min first, max last
    cases.append(b)
    cases.append(np.full((B, 3, H, W), F(0.3125), F))                  # all equal
    cases.append((-3 - rng.random((B, 3, H, W))).astype(F))            # x/2+.5 < 0 everywhere
    c = rng.uniform(-1, 1, (B, 3, H, W)).astype(F)
    c[0] = F(-1.0)                                                     # one image exactly 0 after x/2+.5, the others mixed
    cases.append(c)
    for x in cases:
        got = run(engine, x, None, None, panels[-1], P, want=(True, False, False, False, True))
        v = x / F(2) + F(0.5)
        assert got[4][panels[-1], :, 0].tobytes() == v.max(axis=(1, 2, 3)).tobytes()
        assert got[4][panels[-1], :, 1].tobytes() == v.min(axis=(1, 2, 3)).tobytes()


def test_every_output_is_optional_and_repeats_are_identical(engine):
    x, y, m = inputs(2, 64, 64, 4)
    a = run(engine, x, y, m, 3, 11, want=(False, True, False, True, False))
    b = run(engine, x, y, m, 3, 11, want=(False, True, False, True, False))
    assert a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes()
    run(engine, x, None, None, 3, 11, want=(True, False, False, False, False))
    run(engine, x, None, None, 3, 11, want=(False, False, False, False, True))


def test_unaligned_pointers_take_the_scalar_path(engine):
    """W % 4 == 0 but x (and the strip) start 4 bytes into their allocations: the 16-byte path may not be taken."""
    B, H, W, P, p = 1, 8, 12, 3, 1
    x, _, _ = inputs(B, H, W, 5)
    xd = engine.empty((x.size + 1,))
    xd.copy_from(np.concatenate([[F(9)], x.ravel()]))
    sd = engine.to_device(np.full((B * 3 * H * P * W + 1,), SENT_F, F))
    engine._check(engine.lib.dpir_progress_snapshot(engine.h, xd.ptr + 4, None, None, p, P, sd.ptr + 4, None, None, None, None, B, H, W))
    engine.sync()
    got = sd.numpy()
    exp = expected(x, None, None, (np.full((B, 3, H, P * W), SENT_F, F), None, None, None, None), p, W)[0]
    assert got[0] == SENT_F and got[1:].tobytes() == exp.tobytes()


def test_argument_refusals_launch_nothing(engine):
    x, y, m = inputs(1, 8, 12, 6)
    xd, yd, md = engine.to_device(x), engine.to_device(y), engine.to_device(m, np.uint8)
    strip = engine.to_device(np.full((1, 3, 8, 36), SENT_F, F))
    for p, P in ((-1, 3), (3, 3), (0, 0)):
        with pytest.raises(EngineError, match="panel"):
            engine.progress_snapshot(xd, p, P, strip_f32=strip)
    for kw in (dict(masked_f32=strip), dict(masked_f32=strip, y=yd), dict(masked_u8=strip, mask=md)):
        with pytest.raises(EngineError, match="masked output needs y and mask"):
            engine.progress_snapshot(xd, 0, 3, **kw)
    with pytest.raises(EngineError, match="B, H and W"):
        engine._check(engine.lib.dpir_progress_snapshot(engine.h, xd.ptr, None, None, 0, 3, strip.ptr, None, None, None, None, 1, 0, 12))
    engine.sync()
    assert (strip.numpy() == SENT_F).all()
