"""-m gpu: two parts of the gradient-mode loops' interface that the stepwise == monolithic tests do not pin (dpir_run_dps_loop and
dpir_run_deblur_grad_loop, include/diffpir_engine.h): the Philox stream ids of the device-noise path, and the status code of every refusal.
Tiny topology, 64 x 64, B = 2, 4 NFE, K = 9 for the deblurring program."""
import ctypes as C

import numpy as np
import pytest

import diffpir_amd
from diffpir_amd import _lib, restore
from diffpir_amd.engine import _ptr
from oracle import unet_oracle as uo
from tests.gpu_common import make_model

pytestmark = pytest.mark.gpu

B, SIZE, K, NFE, SEED, OFFSET = 2, 64, 9, 4, 1234, 3
INVALID, STATE, UNSUPPORTED = -1, -4, -5          # dpir_status


def _psf():
    ax = np.arange(K) - K // 2
    ks = [np.exp(-(ax[:, None] ** 2 + (s * ax[None, :]) ** 2) / (2 * std * std)) for std, s in ((1.6, 1.0), (2.4, 0.5))]
    return np.stack([k / k.sum() for k in ks]).astype(np.float32)[:, None]


def _sr(mode, sf):
    return restore.LoopConfig(task="sr", iter_num=NFE, lambda_=6.0, zeta=0.25, sf=sf, sr_mode="cubic", generate_mode=mode)


def _deblur(mode, **kw):
    return restore.LoopConfig(driver="main_ddpir_deblur", task="deblur", iter_num=NFE, lambda_=6.0, zeta=0.25, generate_mode=mode, **kw)


CASES = {
    "sr_DPS_y0": _sr("DPS_y0", 2),
    "sr_DPS_yt": _sr("DPS_yt", 2),
    "sr_DPS_yt_x4": _sr("DPS_yt", 4),
    "deblur_DPS_y0": _deblur("DPS_y0"),
    "deblur_DPS_yt": _deblur("DPS_yt"),
    "deblur_first_order": restore.LoopConfig(driver="main_ddpir_deblur", task="deblur", iter_num=NFE, lambda_=6.0e5, zeta=0.25, eta=0.5,
                                             sub_1_analytic=False),
}


@pytest.fixture(scope="module")
def eng():
    e = diffpir_amd.Engine(0)
    e.set_precision("f16x3")
    e.enable_grad()
    make_model(e, uo.tiny_hp())
    yield e
    e.close()


def documented_streams(cfg, steps):
    """The stream id of every host draw of the mode, in the host's draw order (restore.dps_host_noise_shapes); None where the loop discards the
    draw.  init: 0; p_sample of step i: 4 (i + 1); y_t: 4 (i + 1) + 1; the first-order re-noise: 4 i + 1 and 4 i + 2."""
    out = [0]
    for i, st in enumerate(steps):
        if cfg.generate_mode == "DiffPIR":
            out.append(None)                                  # p_sample's draw, unused for pred_xstart
            if not st["last"]:
                out += [4 * i + 1, 4 * i + 2]
        else:
            out.append(None if st["last"] else 4 * (i + 1))
            if cfg.generate_mode == "DPS_yt" and not st["last"]:
                out.append(4 * (i + 1) + 1)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_device_noise_is_the_documented_philox_streams(eng, name):
    """restore_batch with device noise against the same call fed, as host noise, dpir_randn of the documented (seed, stream, image_offset)."""
    cfg = CASES[name]
    rng = np.random.default_rng(5)
    h = SIZE // cfg.sf
    y = rng.uniform(0, 1, (B, 3, h, h)).astype(np.float32)
    k = _psf() if cfg.task == "deblur" else None
    streams = documented_streams(cfg, restore._steps(cfg)[1])
    assert any(s is None for s in streams) and sum(s is not None for s in streams) >= NFE
    todo = list(streams)

    def f(shape):
        stream = todo.pop(0)
        if stream is None:
            return np.zeros(shape, np.float32)
        out = eng.empty(shape)
        eng._check(eng.lib.dpir_randn(eng.h, out.ptr, SEED, stream, OFFSET, *shape))
        return out.numpy()

    dev = restore.restore_batch(eng, cfg, y, k=k, noise_source="device", seed=SEED, image_offset=OFFSET).numpy()
    host = restore.restore_batch(eng, cfg, y, k=k, noise_source="host", noise_fn=f).numpy()
    assert not todo
    print(f"{name}: device noise vs host-fed dpir_randn streams {streams}: max|diff| {float(np.abs(dev - host).max()):.3e}")
    assert np.isfinite(dev).all()
    assert np.array_equal(dev, host)


def _refusals():
    """(label, entry, variant, descriptor edits, expected status).  The codes are what each entry returned before the two loops shared a body."""
    dps, deb = "dpir_run_dps_loop", "dpir_run_deblur_grad_loop"
    return [
        ("dps: null descriptor", dps, 1, None, INVALID),
        ("deblur: null descriptor", deb, 1, None, INVALID),
        ("dps: variant 2", dps, 2, {}, INVALID),
        ("dps: task deblur", dps, 1, dict(task=restore.TASKS["deblur"]), UNSUPPORTED),
        ("deblur: variant 3", deb, 3, {}, INVALID),
        ("deblur: task sr", deb, 1, dict(task=restore.TASKS["sr_cubic"]), INVALID),
        ("deblur: sf 2", deb, 1, dict(sf=2), INVALID),
        ("deblur: no k_dev", deb, 1, dict(k_dev=None), INVALID),
        ("deblur: kh != kw", deb, 1, dict(kh=9, kw=7), INVALID),
        ("deblur: K even", deb, 1, dict(kh=8, kw=8), INVALID),
        ("deblur: K = 81", deb, 1, dict(kh=81, kw=81), UNSUPPORTED),
        ("deblur: variant 0 without gradient mode", deb, 0, {}, STATE),
        ("dps: variant 0 without gradient mode", dps, 0, {}, STATE),
        ("dps: labels on an unconditional model", dps, 1, dict(labels=True), INVALID),
        ("deblur: labels on an unconditional model", deb, 1, dict(labels=True), INVALID),
    ]


def test_refusals_keep_their_status_codes():
    """The C entries called directly on an engine with the model loaded and no gradient mode: nothing is launched, only the code is read."""
    e = diffpir_amd.Engine(0)
    try:
        e.set_precision("f16x3")
        make_model(e, uo.tiny_hp())
        _, steps, arr = restore._steps(_sr("DPS_yt", 2))
        coefs = (_lib.DpsCoef * len(steps))()
        y = e.empty((B, 3, SIZE, SIZE))
        k = e.empty((B, 1, 81, 81))
        out = e.empty((B, 3, SIZE, SIZE))
        lab = np.zeros(B, np.int64)
        got = []
        for label, entry, variant, edits, want in _refusals():
            d = _lib.LoopDesc()
            d.B, d.H, d.W, d.y_dev = B, SIZE, SIZE, y.ptr
            if entry == "dpir_run_dps_loop":
                d.task, d.sf = restore.TASKS["sr_cubic"], 2
            else:
                d.task, d.sf, d.kh, d.kw, d.k_dev = restore.TASKS["deblur"], 1, K, K, k.ptr
            for key, v in (edits or {}).items():
                if key == "labels":
                    d.labels_host = lab.ctypes.data
                else:
                    setattr(d, key, v)
            head = (e.h, None if edits is None else C.byref(d), arr, coefs, len(steps), variant, 6.0, None, None)
            tail = (out.ptr, None)
            rc = e.lib.dpir_run_dps_loop(*head, 1.0, *tail) if entry == "dpir_run_dps_loop" else e.lib.dpir_run_deblur_grad_loop(*head, *tail)
            msg = (e.lib.dpir_last_error(e.h) or b"").decode()
            print(f"{label}: status {rc} ({msg})")
            got.append((label, rc))
        e.sync()
        assert got == [(r[0], r[4]) for r in _refusals()]
    finally:
        e.close()
