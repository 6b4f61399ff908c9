"""-m gpu: dpir_ancestral_step, the fused data side of one ancestral inpainting step (csrc/ancestral.hip), against the numpy float32 statement
(tests/ancestral_ref.step_f32): bit for bit where expf is not involved, to expf's last bit where it is; batch independence; device noise
against dpir_randn at the documented streams; argument validation.  The network output has 6 planes per image and x has 3: every shape with
B > 1 exercises the two image strides."""
import ctypes as C
import itertools

import numpy as np
import pytest

from diffpir_amd import _lib, schedule
from diffpir_amd.engine import _ptr
from tests.ancestral_ref import step_f32

pytestmark = pytest.mark.gpu
f32 = np.float32
# (2,64,64): the 16-byte path, more than one workgroup per image; (3,20,20): several images on the 16-byte path, 1200 elements per image (no multiple of a
# workgroup's 1024); (1,9,7): H*W = 63 is no multiple of 4 -- the scalar path with a partial last group (189 = 47 * 4 + 1 elements)
SHAPES = [(2, 64, 64), (3, 20, 20), (1, 9, 7)]
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


def make_row(nonzero=1, mix_next=1, t_index=3):
    """A row of the real schedule (quad, 10 steps: t = 422 at index 3) with the two flags set freely: the kernel only applies them."""
    _, rows, _ = schedule.build_ancestral_rows(iter_num=10)
    row = dict(rows[t_index], nonzero=nonzero, mix_next=mix_next)
    if not row["sa_n"]:
        row.update(sa_n=row["sa_t"], s1m_n=row["s1m_t"])
    return row


def c_row(row):
    r = _lib.AncestralRow()
    for f, _ in _lib.AncestralRow._fields_:
        setattr(r, f, row[f])
    return {k: (float(f32(v)) if isinstance(v, float) else v) for k, v in row.items()}, r


def operands(B, H, W, mask_kind, seed):
    rng = np.random.default_rng(seed)
    sh = (B, 3, H, W)
    out6 = np.concatenate([rng.standard_normal(sh), rng.uniform(-1.2, 1.2, sh)], axis=1).astype(f32)
    o = dict(x=rng.standard_normal(sh).astype(f32), out6=out6, y=rng.random(sh).astype(f32), n=rng.standard_normal(sh).astype(f32),
             nr=rng.standard_normal(sh).astype(f32))
    o["mask"] = {"ones": np.ones(sh, np.uint8), "zeros": np.zeros(sh, np.uint8), "random": (rng.random(sh) < 0.5).astype(np.uint8)}[mask_kind]
    return o


def run_fused(e, o, crow, mode, ddim, B, H, W, host=True, seed=0, off=0, step=0, want_x0=True):
    x = e.to_device(o["x"]); out6 = e.to_device(o["out6"]); y = e.to_device(o["y"]); m = e.to_device(o["mask"], np.uint8)
    n = {k: (e.to_device(o[k]) if host else None) for k in ("n", "nr")}
    x0 = e.empty((B, 3, H, W)) if want_x0 else None
    e._check(e.lib.dpir_ancestral_step(e.h, x.ptr, out6.ptr, 6, y.ptr, m.ptr, C.byref(crow), mode, ddim, _ptr(n["n"]), _ptr(n["nr"]), seed, off, step,
                                       _ptr(x0), B, H, W))
    return x.numpy(), (x0.numpy() if want_x0 else None)


GRID = list(itertools.product((1, 2), (0, 1), (0, 1), (0, 1), ("ones", "zeros", "random")))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_step_equals_the_numpy_float32_statement(engine, B, H, W):
    """mode x ddim x nonzero x mix_next x mask, host noise.  Without the sampler's noise term (nonzero = 0, ddim) every operation is a correctly
    rounded float32 operation: bitwise.  With it, the std factor is expf(0.5 lv): HIP documents expf to 1 ulp, the statement rounds the float64
    value (0.5 ulp), so the factors differ by at most 1.5 ulp, the product s n by at most 2.5 * 2^-23 |s n| after its own rounding, and the
    sum mean + s n by that plus one rounding of the result: |got - ref| <= 2.5 * 2^-23 |s n| + 2^-23 |ref| per element (the accuracy of expf is
    taken from HIP's documentation, not measured here).  Where the mask is 1 the mix replaces the sample and the difference is 0."""
    worst = 0.0
    for k, (mode, ddim, nonzero, mix_next, mk) in enumerate(GRID):
        o = operands(B, H, W, mk, 2000 + k)
        row, crow = c_row(make_row(nonzero, mix_next))
        got, x0 = run_fused(engine, o, crow, mode, ddim, B, H, W)
        ref, x0r, sn = step_f32(o["x"], o["out6"], o["y"], o["mask"], row, mode, ddim, o["n"], o["nr"])
        tag = f"mode {mode} ddim {ddim} nonzero {nonzero} mix_next {mix_next} mask {mk}"
        np.testing.assert_array_equal(x0.view(np.uint32), x0r.view(np.uint32), err_msg="x0 " + tag)
        if ddim or not nonzero:
            np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=tag)
            continue
        bound = 2.5 * EPS * np.abs(sn.astype(np.float64)) + EPS * np.abs(ref.astype(np.float64))
        ratio = float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (tag, ratio)
    print(f"({B},{H},{W}): largest |got - ref| / (2.5 * 2^-23 |s n| + 2^-23 |ref|) over the grid = {worst:.3f}")


@pytest.mark.parametrize("B,H,W", SHAPES[:2])
@pytest.mark.parametrize("host", [True, False])
def test_image_n_of_a_batch_equals_the_image_alone_bitwise(engine, B, H, W, host):
    """x's image stride is 3 H W, the network output's is 6 H W: an image read at the wrong stride does not equal itself run alone."""
    o = operands(B, H, W, "random", 77)
    _, crow = c_row(make_row())
    for mode, ddim in ((1, 0), (1, 1), (2, 0)):
        full, fx0 = run_fused(engine, o, crow, mode, ddim, B, H, W, host=host, seed=11, off=5, step=3)
        for n in range(B):
            one = {k: v[n:n + 1] for k, v in o.items()}
            alone, ax0 = run_fused(engine, one, crow, mode, ddim, 1, H, W, host=host, seed=11, off=5 + n, step=3)
            np.testing.assert_array_equal(alone[0], full[n])
            np.testing.assert_array_equal(ax0[0], fx0[n])


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_device_noise_equals_host_noise_fed_dpir_randn(engine, B, H, W):
    """Streams 4 (step + 1) for the sampler's draw and 3 + 4 (step + 1) for the next step's mix, keyed by (seed, image_offset + b): the in-place
    draws share philox_normal4 with randn_kernel, so the two passes are bitwise equal.  ddim on device draws nothing for the sampler."""
    e = engine
    seed, off, s = 2 ** 40 + 9, 7, 5
    for mode, ddim, nonzero in ((1, 0, 1), (2, 0, 1), (1, 1, 1), (1, 0, 0)):
        o = operands(B, H, W, "random", 31 + mode + 2 * ddim)
        for key, stream in (("n", 4 * (s + 1)), ("nr", 3 + 4 * (s + 1))):
            buf = e.empty((B, 3, H, W))
            e._check(e.lib.dpir_randn(e.h, buf.ptr, seed, stream, off, B, 3, H, W))
            o[key] = buf.numpy()
        _, crow = c_row(make_row(nonzero, 1))
        dev, _ = run_fused(e, o, crow, mode, ddim, B, H, W, host=False, seed=seed, off=off, step=s)
        host, _ = run_fused(e, o, crow, mode, ddim, B, H, W, host=True)
        np.testing.assert_array_equal(dev.view(np.uint32), host.view(np.uint32))
        wrong = dict(o, n=o["nr"], nr=o["n"])                   # the two streams are not interchangeable
        other, _ = run_fused(e, wrong, crow, mode, ddim, B, H, W, host=True)
        if mode == 1 or (not ddim and nonzero):
            assert np.abs(other - dev).max() > 1e-3


def test_null_operands_and_bad_shapes_give_the_documented_codes_before_any_launch(engine):
    e = engine
    B, H, W = 1, 8, 8
    o = operands(B, H, W, "ones", 1)
    x = e.to_device(o["x"]); out6 = e.to_device(o["out6"]); y = e.to_device(o["y"]); m = e.to_device(o["mask"], np.uint8); n = e.to_device(o["n"])
    _, crow = c_row(make_row())
    INVALID, UNSUPPORTED = -1, -5

    def call(x_=x.ptr, o6=out6.ptr, ch=6, y_=y.ptr, m_=m.ptr, row=C.byref(crow), mode=1, n_=n.ptr, nr=n.ptr, s=0, shape=(B, H, W)):
        return e.lib.dpir_ancestral_step(e.h, x_, o6, ch, y_, m_, row, mode, 0, n_, nr, 0, 0, s, None, *shape)
    assert call() == 0
    assert call(mode=2, y_=None, m_=None, nr=None) == 0          # vanilla reads neither y nor mask
    assert call(n_=None, nr=None) == 0                           # device noise
    e.sync()
    before = x.numpy().copy()
    for kw in (dict(x_=None), dict(o6=None), dict(row=None), dict(y_=None), dict(m_=None), dict(mode=0), dict(mode=3), dict(s=-1),
               dict(shape=(0, H, W)), dict(shape=(B, -1, W)), dict(shape=(B, H, 0)), dict(nr=None), dict(n_=None)):
        assert call(**kw) == INVALID, kw
    for ch in (3, 4, 7):
        assert call(ch=ch) == UNSUPPORTED, ch
    assert b"learn_sigma" in e.lib.dpir_last_error(e.h)
    e.sync()
    np.testing.assert_array_equal(x.numpy(), before)
