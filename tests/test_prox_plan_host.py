"""The plan of the mixed-radix FFT prox (csrc/fft_plan.cpp, through dpir_debug_fft_plan / dpir_debug_prox_layout: no engine, no GPU): the radix
list, the storage permutation with its adjacent aliases, a float64 numpy walk of the very stages the kernels of csrc/fft_mixed.hip run against
np.fft.fft, the refusals, the layout rule on every shape the three older kernel families serve, and the column strips."""
import ctypes as C

import numpy as np
import pytest

from diffpir_amd import _lib

OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -5
FULL_BITREV, HALF_ROWS, HALF_COLS, FULL_DIGITREV = 0, 1, 2, 3
LENGTHS = (8, 24, 36, 44, 52, 62, 93, 96, 160, 224, 352, 480, 1000)
ALLOWED = {2, 3, 4, 5, 7, 11, 13, 17, 19, 23, 29, 31}
CASES = [(N, sf) for N in LENGTHS for sf in range(1, 17) if N % sf == 0]


def plan(N, sf, want_perm=True):
    """(rc, radices, perm)"""
    rad = (C.c_int * 16)()
    n = C.c_int(0)
    perm = np.full(max(N, 1), -1, np.int32)
    rc = _lib.load_debug().dpir_debug_fft_plan(N, sf, rad, 16, C.byref(n), perm.ctypes.data if want_perm else None)
    return rc, list(rad[:n.value]), perm


def layout(H, W, sf, mode=3):
    """(rc, layout, (strip width, count, last), message)"""
    out = [C.c_int(-1) for _ in range(4)]
    msg = C.create_string_buffer(256)
    rc = _lib.load_debug().dpir_debug_prox_layout(H, W, sf, mode, *[C.byref(o) for o in out], msg, 256)
    return rc, out[0].value, tuple(o.value for o in out[1:]), msg.value.decode()


def walk(x, radices, inverse=False):
    """The in-place stages of mixed_fft_lds in float64.  Forward (DIF): blocks of L points, butterflies over the r points m = L / r apart, then the
    twiddle W_L^(j k) on output k of butterfly j.  Inverse (DIT): the stages in reverse order, conjugate twiddle first, conjugate butterfly after."""
    N = len(x)
    d = np.asarray(x, np.complex128).copy()
    sign = 2j if inverse else -2j
    lengths, L = [], N
    for r in radices:
        lengths.append(L)
        L //= r
    for r, L in (reversed(list(zip(radices, lengths))) if inverse else zip(radices, lengths)):
        m = L // r
        k = np.arange(r)
        bf = np.exp(sign * np.pi * np.outer(k, k) / r)                 # [out][in]
        tw = np.exp(sign * np.pi * np.outer(k, np.arange(m)) / L)      # [k][j]
        blocks = d.reshape(N // L, r, m)
        if inverse:
            d = np.einsum("kq,bqj->bkj", bf, blocks * tw[None]).reshape(N)
        else:
            d = (np.einsum("kq,bqj->bkj", bf, blocks) * tw[None]).reshape(N)
    return d


@pytest.mark.parametrize("N,sf", CASES)
def test_radices_permutation_and_walk(N, sf):
    rc, rad, perm = plan(N, sf)
    assert rc == OK
    assert int(np.prod(rad)) == N and set(rad) <= ALLOWED, rad
    tail, t = 1, len(rad)
    while tail < sf:
        t -= 1
        tail *= rad[t]
    assert tail == sf, (rad, sf)                                        # the trailing radices multiply to sf
    assert sorted(perm.tolist()) == list(range(N))                      # a bijection
    f = np.arange(N // sf)
    alias = perm[(f[:, None] + np.arange(sf)[None, :] * (N // sf))]     # [fold group][alias]
    assert np.array_equal(np.sort(alias, axis=1), (alias.min(axis=1) // sf * sf)[:, None] + np.arange(sf)[None, :]), "aliases are sf adjacent positions"
    rng = np.random.default_rng(N * 17 + sf)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    ref = np.fft.fft(x)
    stored = walk(x, rad)
    assert np.abs(stored[perm] - ref).max() <= 1e-12 * np.abs(ref).max()
    back = walk(stored, rad, inverse=True) / N
    assert np.abs(back - x).max() <= 1e-12 * np.abs(x).max()


def test_plan_rejections():
    assert plan(74, 1)[0] == ERR_UNSUPPORTED and plan(2 * 37 * 4, 4)[0] == ERR_UNSUPPORTED
    assert plan(64, 3)[0] == ERR_INVALID and plan(64, 0)[0] == ERR_INVALID
    rc, lay, _, msg = layout(74, 64, 1)
    assert rc == ERR_UNSUPPORTED and "37" in msg, msg
    rc, lay, _, msg = layout(64, 2 * 37 * 4, 4)
    assert rc == ERR_UNSUPPORTED and "37" in msg, msg
    rc, lay, _, msg = layout(64, 64, 3)
    assert rc == ERR_INVALID and msg == "pre_calculate: image size not divisible by sf"
    assert layout(1032, 96, 1)[0] == ERR_UNSUPPORTED and layout(96, 2064, 1)[0] == ERR_UNSUPPORTED       # beyond the LDS bounds
    assert layout(6, 96, 1)[0] == ERR_UNSUPPORTED and layout(96, 96, 32)[0] == ERR_UNSUPPORTED
    assert layout(2048, 16, 1)[:2] == (ERR_UNSUPPORTED, FULL_BITREV) and layout(8, 8, 1)[:2] == (ERR_UNSUPPORTED, FULL_BITREV)      # as before


def test_strict_launch_modes_refuse_what_they_refused():
    """Modes 0 and 1 of dpir_set_prox_launch run the power-of-two families only: the shapes the mixed-radix kernels serve under modes 2 and 3 (the
    default) stay DPIR_ERR_UNSUPPORTED there, with the generic kernels' own message; a non-divisor is invalid under every mode."""
    for H, W, sf in ((96, 96, 1), (48, 48, 3), (96, 96, 3), (24, 36, 1), (64, 96, 2), (64, 64, 16 + 16)):
        for mode in (0, 1):
            rc, lay, _, msg = layout(H, W, sf, mode)
            assert (rc, lay) == (ERR_UNSUPPORTED, FULL_BITREV) and ("power of two" in msg or "sf must be" in msg), (H, W, sf, mode, rc, msg)
    for H, W, sf in ((96, 96, 1), (48, 48, 3), (96, 96, 3), (24, 36, 1), (64, 96, 2)):
        for mode in (2, 3):
            assert layout(H, W, sf, mode)[:2] == (OK, FULL_DIGITREV)
    for mode in range(4):
        assert layout(64, 64, 3, mode)[0] == ERR_INVALID and layout(256, 256, 3, mode)[0] == ERR_INVALID


def _documented(mode, H, W, sf):
    """tests/test_gpu_prox_float64.py's _family, as layouts"""
    if sf in (1, 2, 4) and H == W and H in (256, 512) and mode == 1:
        return HALF_COLS
    if sf in (1, 2, 4) and H == W and H in (64, 256, 512):
        return HALF_ROWS
    return FULL_BITREV


def test_power_of_two_shapes_keep_their_layout():
    from tests import test_gpu_prox_float64 as t
    shapes = {(H, H, sf) for H, sf, B, p in t.FFT4} | {(H, H, sf) for H, sf, p in t.FFT2} | {(H, W, sf) for H, W, sf, B, p in t.GENERIC}
    shapes |= {(H, W, sf) for m, H, W, sf in t.DELTA + t.APPLY}
    assert len(shapes) == 27
    for H, W, sf in sorted(shapes):
        for mode in (0, 1, 2, 3):          # bit 0: wave kernels where they exist; bit 1 (the mixed-radix layout) changes nothing here
            rc, lay, strips, msg = layout(H, W, sf, mode)
            assert (rc, lay) == (OK, _documented(mode & 1, H, W, sf)), (H, W, sf, mode, rc, lay, msg)
            if lay == FULL_BITREV:
                assert strips == (16, W // 16, 16)


@pytest.mark.parametrize("H,W", [(24, 36), (30, 50), (36, 60), (48, 80), (44, 52), (62, 93), (64, 96), (96, 96), (96, 160), (224, 352), (480, 640),
                                 (1020, 2040), (1024, 96), (8, 2046)])
def test_strips_tile_the_width_and_stored_indices_stay_inside(H, W):
    for sf in [s for s in range(1, 17) if H % s == 0 and W % s == 0]:
        rc, lay, (width, count, last), msg = layout(H, W, sf)
        assert (rc, lay) == (OK, FULL_DIGITREV), (H, W, sf, msg)
        assert width % sf == 0 and 1 <= width <= 16 and (width >= 12 or width == sf or sf == 9) and last % sf == 0 and 0 < last <= width
        cover = np.zeros(W, np.int32)
        for s in range(count):
            cover[s * width:s * width + (width if s < count - 1 else last)] += 1
        assert (count - 1) * width + last == W and np.all(cover == 1)
        assert (H + width * (H + 1)) * 8 <= 160 * 1024                   # the W_H table and one strip in LDS
        ph, pw = plan(H, sf)[2], plan(W, sf)[2]
        stored = ph.astype(np.int64)[:, None] * W + pw[None, :]
        assert stored.min() == 0 and stored.max() == H * W - 1 and len(np.unique(stored)) == H * W
        # the sf x sf aliases of (u, v) are one sf x sf tile of the stored plane, inside ONE strip
        u, v = (H // sf) // 2, (W // sf) - 1
        rows = np.sort(ph[u + np.arange(sf) * (H // sf)])
        cols = np.sort(pw[v + np.arange(sf) * (W // sf)])
        assert np.array_equal(rows, rows[0] + np.arange(sf)) and rows[0] % sf == 0
        assert np.array_equal(cols, cols[0] + np.arange(sf)) and cols[0] // width == cols[-1] // width
