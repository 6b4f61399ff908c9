"""-m gpu: conv5's small tile (64 output channels x 128 pixels, csrc/conv5.hip) against its 128 x 256 tile and against the float64
statement of a 1x1 convolution, one layer at a time through dpir_debug_conv5_layer (the forward's own dispatch on host operands).

Both tiles run the same K chunks in the same order with the same three MFMAs per product, so they must agree BIT FOR BIT wherever both can
run; the shapes are the smallest that reach every index path of the small tile: one and several pixel tiles, a virtual concat, an output
channel count that is no multiple of 128 (nor of 64 x 2), an odd batch, the GroupNorm prologue, the residual epilogue, and 8 x 8 images
(two whole images per pixel tile, the last tile ragged)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.gpu_common import rel_err

pytestmark = pytest.mark.gpu

# the per-layer bound of the layer-by-layer UNet tests (tests/test_gpu_unet.py TOL_LAYER, max-abs / max-abs via gpu_common.rel_err), which
# the conv5 layers of the f16x3 forward are held to: the split product keeps 22 mantissa bits and accumulates in fp32
TOL_LAYER = 2e-5
SMALL_ON = os.environ.get("DPIR_CONV5_SMALL", "1") != "0"


@pytest.fixture(scope="module", params=["f16x3", "f16x1"])
def eng(request):
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    e.set_precision(request.param)
    e.prec = request.param
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng3():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    e.set_precision("f16x3")
    yield e
    e.close()


def _operands(B, ca, cb, cout, H, W, prm, res, seed, silu=True):
    r = np.random.default_rng(seed)
    c = ca + cb
    op = dict(xa=r.standard_normal((B, ca, H, W)).astype(np.float32),
              xb=r.standard_normal((B, cb, H, W)).astype(np.float32) if cb else None,
              w=(r.standard_normal((cout, c)) * 0.05).astype(np.float32),
              bias=r.standard_normal(cout).astype(np.float32), prm=None, res=None)
    if prm:     # {mean, scale, shift, SiLU flag} per (image, channel); the flag is the same in every row of a table
        t = np.empty((B, c, 4), np.float32)
        t[..., 0] = r.standard_normal((B, c)) * 0.1
        t[..., 1] = 0.5 + r.random((B, c))
        t[..., 2] = r.standard_normal((B, c)) * 0.2
        t[..., 3] = 1.0 if silu else 0.0
        op["prm"] = t
    if res:
        op["res"] = r.standard_normal((B, cout, H, W)).astype(np.float32)
    return op


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _layer(e, op, tile):
    """(return code, output, path that ran: 0 general fp32 kernel, 1 the 128 x 256 tile, 2 the 64 x 128 tile)"""
    from diffpir_amd import _lib
    dbg = _lib.load_debug()
    B, ca, H, W = op["xa"].shape
    cb = 0 if op["xb"] is None else op["xb"].shape[1]
    cout = op["w"].shape[0]
    out = np.empty((B, cout, H, W), np.float32)
    path = C.c_int(-1)
    rc = dbg.dpir_debug_conv5_layer(e.h, B, ca, cb, cout, H, W, tile, _ptr(op["xa"]), _ptr(op["xb"]), _ptr(op["w"]), _ptr(op["bias"]),
                                    _ptr(op["prm"]), _ptr(op["res"]), _ptr(out), C.byref(path))
    return rc, out, path.value


def _f64(op):
    x = op["xa"].astype(np.float64)
    if op["xb"] is not None:
        x = np.concatenate([x, op["xb"].astype(np.float64)], axis=1)
    if op["prm"] is not None:
        t = op["prm"].astype(np.float64)
        x = (x - t[:, :, 0, None, None]) * t[:, :, 1, None, None] + t[:, :, 2, None, None]
        if t[0, 0, 3] != 0:
            x = x / (1.0 + np.exp(-x))
    y = np.einsum("oc,bchw->bohw", op["w"].astype(np.float64), x) + op["bias"].astype(np.float64)[None, :, None, None]
    if op["res"] is not None:
        y = y + op["res"].astype(np.float64)
    return y


# (B, ca, cb, Cout, H, prm, res)
BITWISE = {
    "one_tile_row_two_chunks": (2, 32, 0, 64, 16, False, False),
    "virtual_concat_32_16": (2, 32, 16, 64, 16, False, False),
    "cout_192_odd_batch_prm": (3, 64, 0, 192, 32, True, False),
    "cout_192_odd_batch_res": (3, 64, 0, 192, 32, False, True),
    "cout_192_odd_batch_prm_res": (3, 64, 0, 192, 32, True, True),
    "images_8x8_ragged_last_tile": (5, 32, 0, 64, 8, False, False),
}


@pytest.mark.parametrize("case", sorted(BITWISE))
def test_small_tile_equals_the_large_tile_bit_for_bit(eng, case):
    B, ca, cb, cout, H, prm, res = BITWISE[case]
    op = _operands(B, ca, cb, cout, H, H, prm, res, seed=11)
    rc1, big, p1 = _layer(eng, op, 1)
    rc2, small, p2 = _layer(eng, op, 2)
    assert rc1 == 0 and rc2 == 0 and (p1, p2) == (1, 2), (rc1, rc2, p1, p2, eng.lib.dpir_last_error(eng.h))
    diff = big.view(np.uint32) != small.view(np.uint32)
    print(f"{eng.prec} {case}: {int(diff.sum())} of {diff.size} elements differ")
    assert np.isfinite(big).all() and not diff.any()
    if eng.prec == "f16x3":      # ... and both are the layer: same bound as below
        err = rel_err(small, _f64(op))
        print(f"{eng.prec} {case}: small tile vs float64 {err:.3e}")
        assert err < TOL_LAYER


@pytest.mark.parametrize("B,cin,cout", [(16, 64, 256), (5, 32, 64), (16, 1024, 512)])
def test_8x8_images_against_the_float64_convolution(eng3, B, cin, cout):
    """Two whole 8 x 8 images per pixel tile.  (16, 64, 256) is the smallest launch the dispatch itself puts on the small tile (32
    workgroups), (16, 1024, 512) the FFHQ skip projection at the benched batch that used to run on the fp32 kernel."""
    op = _operands(B, cin, 0, cout, 8, 8, False, False, seed=5)
    ref = _f64(op)
    rc, forced, path = _layer(eng3, op, 2)
    assert rc == 0 and path == 2, (rc, path, eng3.lib.dpir_last_error(eng3.h))
    err = rel_err(forced, ref)
    print(f"B {B} {cin}->{cout} @8x8: small tile vs float64 {err:.3e}")
    assert err < TOL_LAYER
    rc, auto, path = _layer(eng3, op, 0)
    assert rc == 0
    print(f"B {B} {cin}->{cout} @8x8: the dispatch took path {path}, vs float64 {rel_err(auto, ref):.3e}")
    assert rel_err(auto, ref) < TOL_LAYER
    if B == 16:
        assert path == (2 if SMALL_ON else 0)
        if SMALL_ON:
            assert np.array_equal(auto.view(np.uint32), forced.view(np.uint32))
    else:
        assert path == 0          # 3 x 1 workgroups: below the floor, the split-K fp32 kernel as before


def test_shapes_conv5_refuses_still_take_the_fp32_kernel(eng3):
    # H * W no multiple of 4: no float4 stores inside an image
    op = _operands(16, 32, 0, 64, 6, 5, False, False, seed=7)
    rc, out, path = _layer(eng3, op, 0)
    assert rc == 0 and path == 0, (rc, path)
    err = rel_err(out, _f64(op))
    print(f"H*W % 4 != 0: fp32 kernel vs float64 {err:.3e}")
    assert err < TOL_LAYER
    for tile in (1, 2):
        rc, _, _ = _layer(eng3, op, tile)
        assert rc != 0, tile
    # GroupNorm prologue on a channel count that is no multiple of 16: the staged rows are 16 channels per chunk
    op = _operands(16, 24, 0, 256, 16, 16, True, False, seed=8, silu=False)
    for tile in (0, 2):
        rc, out, path = _layer(eng3, op, tile)
        assert rc == 0 and path == 0, (rc, path, tile)
        err = rel_err(out, _f64(op))
        print(f"prm with Cin % 16 != 0 (tile {tile}): fp32 kernel vs float64 {err:.3e}")
        assert err < TOL_LAYER
    # a virtual concat that splits a pair of channel rows: the large tile
    op = _operands(16, 18, 14, 256, 16, 16, False, False, seed=9)
    rc, out, path = _layer(eng3, op, 0)
    assert rc == 0 and path == 1, (rc, path)
    assert rel_err(out, _f64(op)) < TOL_LAYER
    rc, _, _ = _layer(eng3, op, 2)
    assert rc != 0
