"""-m gpu: dpir_inpaint_step, the fused data side of one inpainting sub-step (csrc/inpaint.hip), against the numpy float32 statement
(tests/inpaint_resample_ref.substep_f32) and against the chain of the existing entries, bit for bit; batch independence; device noise against
dpir_randn and the numpy Philox statement; argument validation."""
import ctypes as C
import itertools

import numpy as np
import pytest

from diffpir_amd import _lib
from diffpir_amd.engine import _ptr
from tests.inpaint_resample_ref import substep_f32

pytestmark = pytest.mark.gpu
f32 = np.float32
# (2,6,6) and (3,20,20): more images than one, totals that are no multiple of a workgroup's 1024 elements; (2,5,7): H*W = 35 is no multiple of 4, the
# scalar path with a partial last group per image (3*35 = 105); the other shapes take the 16-byte path
SHAPES = [(1, 8, 8), (3, 20, 20), (2, 64, 64), (2, 6, 6), (2, 5, 7)]


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


def make_row(es, back, last=0, mix_next=1):
    """Coefficients of the magnitudes a schedule produces (no relation between them is needed: the kernel only applies them)."""
    return dict(t=500, last=last, pos=0, back=back, c1=1.6180340, c2=1.2720196, tau=0.37, sa_t=0.6180339, s1m_t=0.7861513, sa_p=0.72, k1=0.83666,
                q=0.6931, es=es, k2=0.38, sae=0.85837, sb=0.51302, sa_n=0.6180339, s1m_n=0.7861513, mix_next=mix_next, reserved=0)


def c_row(row):
    r = _lib.InpaintRow()
    for f, _ in _lib.InpaintRow._fields_:
        setattr(r, f, row[f])
    return {k: (float(f32(v)) if isinstance(v, float) else v) for k, v in row.items()}, r


def operands(B, H, W, ch, mask_kind, seed):
    rng = np.random.default_rng(seed)
    sh = (B, 3, H, W)
    o = dict(x=rng.standard_normal(sh).astype(f32), eps=rng.standard_normal((B, ch, H, W)).astype(f32), y=rng.random(sh).astype(f32),
             n1=rng.standard_normal(sh).astype(f32), n2=rng.standard_normal(sh).astype(f32), nb=rng.standard_normal(sh).astype(f32),
             nr=rng.standard_normal(sh).astype(f32))
    o["mask"] = {"ones": np.ones(sh, np.uint8), "zeros": np.zeros(sh, np.uint8), "random": (rng.random(sh) < 0.5).astype(np.uint8)}[mask_kind]
    return o


def run_fused(e, o, crow, mode, g, B, H, W, ch, host=True, seed=0, off=0, substep=0, want_x0=True):
    x = e.to_device(o["x"]); eps = e.to_device(o["eps"]); y = e.to_device(o["y"]); m = e.to_device(o["mask"], np.uint8)
    n = {k: (e.to_device(o[k]) if host else None) for k in ("n1", "n2", "nb", "nr")}
    x0 = e.empty((B, 3, H, W)) if want_x0 else None
    e._check(e.lib.dpir_inpaint_step(e.h, x.ptr, eps.ptr, ch, y.ptr, m.ptr, C.byref(crow), mode, g, _ptr(n["n1"]), _ptr(n["n2"]), _ptr(n["nb"]),
                                     _ptr(n["nr"]), seed, off, substep, _ptr(x0), B, H, W))
    return x.numpy(), (x0.numpy() if want_x0 else None)


def run_chain(e, o, row, mode, g, B, H, W, ch):
    """xstart (through the fused call's x0 output) -> dpir_prox_mask -> dpir_renoise -> dpir_ewise set-back -> dpir_repaint_mix."""
    _, crow = c_row(row)
    _, x0h = run_fused(e, o, crow, mode, g, B, H, W, ch)
    numel = B * 3 * H * W
    x = e.to_device(o["x"]); y = e.to_device(o["y"]); m = e.to_device(o["mask"], np.uint8); x0 = e.to_device(x0h)
    st = _lib.Step()
    for f, _ in _lib.Step._fields_:
        setattr(st, f, row[f])
    if mode == 0:
        e._check(e.lib.dpir_prox_mask(e.h, x0.ptr, y.ptr, m.ptr, float(f32(row["tau"])), g, B, H, W))
    n1, n2, nb, nr = (e.to_device(o[k]) for k in ("n1", "n2", "nb", "nr"))
    e._check(e.lib.dpir_renoise(e.h, x.ptr, x0.ptr, C.byref(st), n1.ptr if row["es"] != 0 else None, n2.ptr, B, H, W))
    if row["back"]:
        e._check(e.lib.dpir_ewise(e.h, 2, x.ptr, None, 0, float(f32(row["sae"])), x.ptr, numel))
        e._check(e.lib.dpir_ewise(e.h, 2, nb.ptr, None, 0, float(f32(row["sb"])), nb.ptr, numel))
        e._check(e.lib.dpir_ewise(e.h, 0, x.ptr, nb.ptr, numel, 0.0, x.ptr, numel))
    if mode == 1 and row["mix_next"]:
        nxt = _lib.Step(); nxt.sa_t, nxt.s1m_t = row["sa_n"], row["s1m_n"]
        e._check(e.lib.dpir_repaint_mix(e.h, x.ptr, y.ptr, m.ptr, C.byref(nxt), nr.ptr, B, H, W))
    return x.numpy()


GRID = list(itertools.product((0, 1, 2), (0, 1), (0.0, 0.21), (3, 6), (1.0, 0.7), ("ones", "zeros", "random")))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_step_equals_numpy_float32_statement_and_the_chain_bitwise(engine, B, H, W):
    """mode x back x es x eps_channels x guidance x mask, host noise: the fused pass, the numpy statement and the chain of existing entries."""
    for k, (mode, back, es, ch, g, mk) in enumerate(GRID):
        o = operands(B, H, W, ch, mk, 1000 + k)
        row, crow = c_row(make_row(es, back))
        got, x0 = run_fused(engine, o, crow, mode, g, B, H, W, ch)
        ref, x0r = substep_f32(o["x"], o["eps"][:, :3], o["y"], o["mask"], row, mode, g, o["n1"], o["n2"], o["nb"], o["nr"])
        tag = f"mode {mode} back {back} es {es} ch {ch} g {g} mask {mk}"
        np.testing.assert_array_equal(x0.view(np.uint32), x0r.view(np.uint32), err_msg="x0 " + tag)
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=tag)
        if (B, H, W) != (2, 64, 64) or k % 3 == 2 or k < 36:  # the chain: every grid point on the small shapes (the scalar-tail shape among them); at 64 x 64 all of mode 0 and the random masks of the others
            chain = run_chain(engine, o, row, mode, g, B, H, W, ch)
            np.testing.assert_array_equal(got.view(np.uint32), chain.view(np.uint32), err_msg="chain " + tag)


def test_final_row_only_takes_the_next_mix(engine):
    B, H, W = 3, 20, 20
    o = operands(B, H, W, 6, "random", 5)
    row, crow = c_row(make_row(0.0, 0, last=1))
    for mode in (0, 1, 2):
        got, _ = run_fused(engine, o, crow, mode, 1.0, B, H, W, 6)
        ref, _ = substep_f32(o["x"], o["eps"][:, :3], o["y"], o["mask"], row, mode, 1.0, nr=o["nr"])
        np.testing.assert_array_equal(got, ref)
        if mode != 1:
            np.testing.assert_array_equal(got, o["x"])


@pytest.mark.parametrize("B,H,W", SHAPES[1:])
@pytest.mark.parametrize("host", [True, False])
def test_image_n_of_a_batch_equals_the_image_alone_bitwise(engine, B, H, W, host):
    o = operands(B, H, W, 6, "random", 77)
    _, crow = c_row(make_row(0.21, 1))
    full, _ = run_fused(engine, o, crow, 1, 0.7, B, H, W, 6, host=host, seed=11, off=5, substep=3)
    for n in range(B):
        one = {k: v[n:n + 1] for k, v in o.items()}
        alone, _ = run_fused(engine, one, crow, 1, 0.7, 1, H, W, 6, host=host, seed=11, off=5 + n, substep=3)
        np.testing.assert_array_equal(alone[0], full[n])


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_device_noise_equals_host_noise_fed_dpir_randn(engine, B, H, W):
    """The in-place draws share philox_normal4 and the (seed, image, stream, counter) keying with randn_kernel: bitwise."""
    e = engine
    seed, off, s = 2 ** 40 + 9, 7, 5
    for mode, back, es in ((0, 1, 0.21), (1, 1, 0.0), (1, 0, 0.21)):
        o = operands(B, H, W, 6, "random", 31 + mode)
        for key, stream in (("n1", 1 + 4 * s), ("n2", 2 + 4 * s), ("nb", 2 ** 32 + s), ("nr", 3 + 4 * (s + 1))):
            buf = e.empty((B, 3, H, W))
            e._check(e.lib.dpir_randn(e.h, buf.ptr, seed, stream, off, B, 3, H, W))
            o[key] = buf.numpy()
        _, crow = c_row(make_row(es, back))
        dev, _ = run_fused(e, o, crow, mode, 1.0, B, H, W, 6, host=False, seed=seed, off=off, substep=s)
        host, _ = run_fused(e, o, crow, mode, 1.0, B, H, W, 6, host=True)
        np.testing.assert_array_equal(dev.view(np.uint32), host.view(np.uint32))


def test_set_back_stream_equals_the_numpy_philox_statement(engine):
    """Stream 2^32 + s (the counter's high word) against oracle/philox_oracle.py, to the 4e-6 of the existing Philox test: x = 0 * x + 1 * n_back
    isolates the draw (c1 = c2 = 0 -> x0 = 0; k1 = k2 = sa_p = 0 -> re-noise gives 0)."""
    from oracle import philox_oracle as po
    e = engine
    B, H, W, s, seed, off = 2, 20, 20, 6, 99, 2 ** 33 + 1
    row = make_row(0.0, 1)
    row.update(c1=0.0, c2=0.0, sa_p=0.0, k1=0.0, k2=0.0, sae=0.0, sb=1.0)
    _, crow = c_row(row)
    o = operands(B, H, W, 6, "ones", 3)
    got, _ = run_fused(e, o, crow, 2, 1.0, B, H, W, 6, host=False, seed=seed, off=off, substep=s)
    ref = po.randn(seed, 2 ** 32 + s, off, B, 3 * H * W).reshape(B, 3, H, W)
    np.testing.assert_allclose(got, ref, atol=4e-6, rtol=2e-6)
    other = po.randn(seed, s, off, B, 3 * H * W).reshape(B, 3, H, W)          # not the low word alone
    assert np.abs(got - other).max() > 0.1


def test_null_operands_and_bad_shapes_are_invalid_before_any_launch(engine):
    e = engine
    B, H, W = 1, 8, 8
    o = operands(B, H, W, 6, "ones", 1)
    x = e.to_device(o["x"]); eps = e.to_device(o["eps"]); y = e.to_device(o["y"]); m = e.to_device(o["mask"], np.uint8); n = e.to_device(o["n2"])
    _, crow = c_row(make_row(0.21, 1))
    INVALID = -1            # DPIR_ERR_INVALID

    def call(x_=x.ptr, eps_=eps.ptr, ch=6, y_=y.ptr, m_=m.ptr, row=C.byref(crow), mode=0, n1=n.ptr, n2=n.ptr, nb=n.ptr, nr=n.ptr, s=0, shape=(B, H, W)):
        return e.lib.dpir_inpaint_step(e.h, x_, eps_, ch, y_, m_, row, mode, 1.0, n1, n2, nb, nr, 0, 0, s, None, *shape)
    assert call() == 0
    before = x.numpy().copy()
    for kw in (dict(x_=None), dict(eps_=None), dict(y_=None), dict(m_=None), dict(row=None), dict(ch=4), dict(mode=3), dict(s=-1),
               dict(shape=(0, H, W)), dict(shape=(B, -1, W)), dict(shape=(B, H, 0)), dict(n1=None), dict(nb=None), dict(n2=None),
               dict(mode=1, nr=None)):
        assert call(**kw) == INVALID, kw
    e.sync()
    np.testing.assert_array_equal(x.numpy(), before)
