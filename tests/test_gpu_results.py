"""-m gpu: dpir_result_panels (csrc/results.hip) against the plain-numpy statement tests/results_ref.py, bit for bit, with every output
between guard words; its refusals; and the driver end to end with engine_save_results on (the exact set of files, each decoding to the bytes
of degrade.result_panels and of the run's out_u8) and off (the same PSNR, no results directory)."""
import ctypes as C
import os

import numpy as np
import pytest

from diffpir_amd import _lib, degrade as dgr
from diffpir_amd.engine import _ptr
from tests import results_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DPIR_ERR_INVALID = -1
GUARD = 64                                 # guard bytes either side of an output
SENT = np.uint8(0xA5)

# (B, H, W, sf, kh, kw, mode, misalign): the issue's six cases and one more path
CASES = {
    "vector path, sf 1, hidden inset": (3, 32, 32, 1, 5, 5, 0, 0),
    "sf 2, inset 21 x 21 partly under the 12 x 20 paste": (2, 24, 40, 2, 7, 7, 0, 0),
    "sf 4, L width 12": (1, 32, 48, 4, 3, 3, 0, 0),
    "scalar path: width 30, no kernel, output pointers off by one byte": (2, 30, 30, 1, 0, 0, 0, 1),
    "width 12 with output pointers off by one byte: the 4-byte path may not be taken": (1, 8, 12, 1, 2, 2, 0, 1),
    "inpainting strip": (2, 16, 20, 1, 0, 0, 1, 0),
    "inset exactly as wide as the image": (2, 24, 24, 2, 5, 8, 0, 0),
    "W % 4 == 0 but w % 4 != 0: scalar path with an inset": (2, 18, 36, 2, 6, 3, 0, 0),
    "more than one workgroup per image": (1, 64, 64, 2, 9, 9, 0, 0),
}


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


def inputs(B, H, W, sf, kh, kw, seed):
    """y with negatives, values above 1 and the float32 neighbours of (n + 0.5) / 255; random est / gt bytes; a positive kernel"""
    rng = np.random.default_rng(seed)
    h, w = H // sf, W // sf
    y = rng.uniform(-0.25, 1.25, (B, 3, h, w)).astype(np.float32)
    t = R.tie_values()
    pos = rng.choice(y.size, size=t.size, replace=False)
    y.reshape(-1)[pos] = t
    assert (y < 0).any() and (y > 1).any()
    est = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    gt = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    k = (rng.random((B, kh, kw)) + 0.01).astype(np.float32) if kh else None
    return y, est, gt, k


def guarded(engine, nbytes, misalign):
    """a device buffer of SENT bytes with the output at GUARD + misalign"""
    return engine.to_device(np.full(GUARD + misalign + nbytes + GUARD, SENT, np.uint8)), GUARD + misalign


def call(engine, y, est, gt, k, sf, mode, want_L, want_leh, misalign=0):
    B, H, W, _ = gt.shape
    d = _lib.ResultDesc()
    d.B, d.H, d.W, d.sf, d.mode = B, H, W, sf, mode
    kv_d = None
    if k is not None:
        kv = np.stack([R.kernel_bytes(kk) for kk in k])
        d.kh, d.kw = kv.shape[1], kv.shape[2]
        kv_d = engine.to_device(kv)
    nL, nS = B * (H // sf) * (W // sf) * 3, B * H * 3 * W * 3
    (Lb, Lo), (Sb, So) = guarded(engine, nL, misalign), guarded(engine, nS, misalign)
    yd, ed, gd = engine.to_device(y), engine.to_device(est), engine.to_device(gt)
    rc = engine.lib.dpir_result_panels(engine.h, C.byref(d), _ptr(yd), _ptr(kv_d), _ptr(ed), _ptr(gd),
                                       Lb.ptr + Lo if want_L else None, Sb.ptr + So if want_leh else None)
    engine.sync()
    return rc, (Lb.numpy(), Lo, nL), (Sb.numpy(), So, nS)


def check_buffer(buf, off, n, want, name):
    assert (buf[:off] == SENT).all() and (buf[off + n:] == SENT).all(), f"{name}: a guard word was overwritten"
    if want is None:
        assert (buf == SENT).all(), f"{name}: a NULL output was written"
    else:
        got = buf[off:off + n].reshape(want.shape)
        assert got.tobytes() == want.tobytes(), f"{name} differs at {np.argwhere(got != want)[:4].tolist()}"


@pytest.mark.parametrize("name", list(CASES))
def test_panels_equal_the_statement_bit_for_bit(engine, name):
    B, H, W, sf, kh, kw, mode, misalign = CASES[name]
    y, est, gt, k = inputs(B, H, W, sf, kh, kw, 11)
    L, leh = R.panels(y, est, gt, k, sf, "inpaint" if mode else "kernel")
    assert np.array_equal(L, np.uint8((y.clip(0, 1) * 255.).round()).transpose(0, 2, 3, 1))       # the issue's own expression on the float32 y
    for want_L, want_leh in ((True, True), (True, False), (False, True), (False, False)):
        rc, Lr, Sr = call(engine, y, est, gt, k, sf, mode, want_L, want_leh, misalign)
        assert rc == 0, engine.lib.dpir_last_error(engine.h)
        check_buffer(*Lr, L if want_L else None, f"{name}: L")
        check_buffer(*Sr, leh if want_leh else None, f"{name}: LEH")


def test_mode_inpaint_ignores_kernel_bytes_and_the_wrapper_agrees(engine):
    y, est, gt, k = inputs(2, 16, 20, 1, 3, 3, 12)
    L, leh = R.panels(y, est, gt, mode="inpaint")
    rc, Lr, Sr = call(engine, y, est, gt, k, 1, 1, True, True)
    assert rc == 0
    check_buffer(*Lr, L, "L")
    check_buffer(*Sr, leh, "LEH")
    gL, gS = dgr.result_panels(engine, y, est, gt, k=k[:, None], sf=1, mode="inpaint")
    assert gL.tobytes() == L.tobytes() and gS.tobytes() == leh.tobytes()
    y, est, gt, k = inputs(2, 24, 40, 2, 7, 7, 13)
    L, leh = R.panels(y, est, gt, k, 2)
    gL, gS = dgr.result_panels(engine, engine.to_device(y), engine.to_device(est), engine.to_device(gt), k=k[:, None], sf=2)
    assert gL.tobytes() == L.tobytes() and gS.tobytes() == leh.tobytes()
    assert np.array_equal(dgr.kernel_bytes(k[:, None]), np.stack([R.kernel_bytes(kk) for kk in k]))
    gL, gS = dgr.result_panels(engine, y, est, gt, k=k[:, None], sf=2, want_L=False)
    assert gL is None and gS.tobytes() == leh.tobytes()


def test_refusals_launch_nothing(engine):
    y, est, gt, _ = inputs(2, 24, 40, 2, 7, 7, 14)
    rng = np.random.default_rng(15)
    bad = {
        "3 kh > H": (dict(sf=2), rng.random((2, 9, 7)), y, b"3 kh <= H"),
        "3 kw > W": (dict(sf=2), rng.random((2, 7, 14)), y, b"3 kw <= W"),
        "sf does not divide W": (dict(sf=3), None, y, b"sf must be >= 1 and divide"),
        "sf 0": (dict(sf=0), None, y, b"sf must be >= 1"),
        "B 0": (dict(sf=2, B=0), None, y, b"B, H and W must be >= 1"),
        "mode 2": (dict(sf=2, mode=2), None, y, b"mode"),
        "inpainting strip at sf 2": (dict(sf=2, mode=1), None, y, b"sf 1"),
    }
    for what, (over, k, yy, msg) in bad.items():
        d = _lib.ResultDesc()
        d.B, d.H, d.W, d.sf, d.mode = over.get("B", 2), 24, 40, over["sf"], over.get("mode", 0)
        kv_d = None
        if k is not None:
            kv_d = engine.to_device(np.stack([R.kernel_bytes(kk) for kk in k]))
            d.kh, d.kw = k.shape[1], k.shape[2]
        (Lb, Lo), (Sb, So) = guarded(engine, 2 * 24 * 40 * 3, 0), guarded(engine, 2 * 24 * 120 * 3, 0)
        yd, ed, gd = engine.to_device(yy), engine.to_device(est), engine.to_device(gt)
        rc = engine.lib.dpir_result_panels(engine.h, C.byref(d), _ptr(yd), _ptr(kv_d), _ptr(ed), _ptr(gd), Lb.ptr + Lo, Sb.ptr + So)
        err = engine.lib.dpir_last_error(engine.h)
        assert rc == DPIR_ERR_INVALID and b"dpir_result_panels" in err and msg in err, (what, rc, err)
        engine.sync()
        assert (Lb.numpy() == SENT).all() and (Sb.numpy() == SENT).all(), what
    assert engine.lib.dpir_result_panels(engine.h, None, None, None, None, None, None, None) == DPIR_ERR_INVALID
    d = _lib.ResultDesc()
    d.B, d.H, d.W, d.sf = 2, 24, 40, 2
    Sb, So = guarded(engine, 2 * 24 * 120 * 3, 0)
    assert engine.lib.dpir_result_panels(engine.h, C.byref(d), _ptr(engine.to_device(y)), None, None, None, None, Sb.ptr + So) == DPIR_ERR_INVALID
    assert b"est_u8_dev" in engine.lib.dpir_last_error(engine.h)
    with pytest.raises(ValueError, match="does not divide"):
        dgr.result_panels(engine, y, est, gt, sf=3)
    assert engine.lib.dpir_version() == 2
    L, leh = R.panels(y, est, gt, None, 2)                         # still usable
    gL, gS = dgr.result_panels(engine, y, est, gt, sf=2)
    assert gL.tobytes() == L.tobytes() and gS.tobytes() == leh.tobytes()


# ------------------------------------------------------------------------------------------------------------------ the driver
def run_driver(tmp_path, monkeypatch, tag, **over):
    """configs/engine_example.yaml on --synthetic 2 at 4 NFE; returns (PSNR list, recorded result_panels calls, recorded out_u8 arrays, cwd)"""
    import yaml
    from diffpir_amd import main_ddpir, restore
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "engine_example.yaml")))
    cwd = tmp_path / tag
    cwd.mkdir()
    cfg.update(iter_num=4, batch_size=2, cwd=str(cwd))
    cfg.update(over)
    p = cwd / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    panels, outs = [], []
    real_panels, real_restore = dgr.result_panels, restore.restore_batch

    def rec_panels(eng, y, est, gt, **kw):
        out = real_panels(eng, y, est, gt, **kw)
        panels.append((out, kw))
        return out

    def rec_restore(eng, cfg_, y, **kw):
        out = real_restore(eng, cfg_, y, **kw)
        outs.append(kw["out_u8"].numpy())
        return out
    monkeypatch.setattr(dgr, "result_panels", rec_panels)
    monkeypatch.setattr(restore, "restore_batch", rec_restore)
    res = main_ddpir.main(["--opt", str(p), "--synthetic", "2", "--max-sweeps", "1"])
    monkeypatch.setattr(dgr, "result_panels", real_panels)
    monkeypatch.setattr(restore, "restore_batch", real_restore)
    return res, panels, outs, cwd, main_ddpir.result_dir(main_ddpir.parse_config(str(p)))


def decoded(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_driver_saves_the_reference_s_files_for_deblurring(tmp_path, monkeypatch):
    from diffpir_amd import main_ddpir
    on, panels, outs, cwd, out_dir = run_driver(tmp_path, monkeypatch, "on", engine_save_results=True, save_E=True, save_L=True, save_LEH=True)
    off, panels_off, outs_off, cwd_off, _ = run_driver(tmp_path, monkeypatch, "off", save_E=True, save_L=True, save_LEH=True)
    assert on == off and len(on) == 1 and np.isfinite(on[0])         # saving changes no number
    assert panels_off == [] and not os.path.exists(cwd_off / "results") and sorted(os.listdir(cwd_off)) == ["c.yaml"]
    assert outs[0].tobytes() == outs_off[0].tobytes()
    names = ["synth_0000.png", "synth_0001.png"]
    e_pre = "diffusion_ffhq_10m_x1_lambda7.0000_zeta0.3000_"
    want = sorted([e_pre + n for n in names] + ["LR_x1_" + n for n in names] + ["synth_0000_LEH.png", "synth_0001_LEH.png"] +
                  ["motion_kernel_" + n for n in names])
    assert sorted(os.listdir(out_dir)) == want
    assert len(panels) == 1 and len(outs) == 1
    (L, leh), kw = panels[0]
    assert kw["sf"] == 1 and kw["mode"] == "kernel" and L.shape == (2, 256, 256, 3) and leh.shape == (2, 256, 768, 3)
    parsed = main_ddpir.parse_config(str(cwd / "c.yaml"))
    k_all, _ = main_ddpir.make_operators(parsed, 2, 0, 256, 256)
    for b, n in enumerate(names):
        stem = n[:-4]
        assert np.array_equal(decoded(os.path.join(out_dir, e_pre + n)), outs[0][b])
        assert np.array_equal(decoded(os.path.join(out_dir, "LR_x1_" + n)), L[b])
        assert np.array_equal(decoded(os.path.join(out_dir, stem + "_LEH.png")), leh[b])
        pic = decoded(os.path.join(out_dir, "motion_kernel_" + n))
        assert pic.shape == (61, 61) and np.array_equal(pic, R.kernel_picture(k_all[b, 0]))
        assert np.array_equal(leh[b, :, 256:512], outs[0][b]) and np.array_equal(leh[b, :, :256], L[b])      # sf 1: the paste hides the inset


def test_flattened_sweep_saves_one_e_per_point_and_the_rest_once(tmp_path, monkeypatch):
    """engine_batch_sweeps: the first two points of the x4 sweep on two images as two batches of (point, image) rows."""
    from diffpir_amd import main_ddpir
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "engine_example.yaml")))
    cfg.update(task="sr", sf=4, iter_num=4, batch_size=2, cwd=str(tmp_path), engine_batch_sweeps=True, engine_save_results=True, save_E=True,
               save_L=True, save_LEH=True)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    panels, real = [], dgr.result_panels

    def rec(eng, y, est, gt, **kw):
        out = real(eng, y, est, gt, **kw)
        panels.append((out, est.numpy()))
        return out
    monkeypatch.setattr(dgr, "result_panels", rec)
    res = main_ddpir.main(["--opt", str(p), "--synthetic", "2", "--max-sweeps", "2"])
    assert len(res) == 2 and np.all(np.isfinite(res)) and len(panels) == 2
    parsed = main_ddpir.parse_config(str(p))
    out_dir, points = main_ddpir.result_dir(parsed), main_ddpir.sweeps(parsed)[:2]
    names = ["synth_0000.png", "synth_0001.png"]
    e_names = [[f"diffusion_ffhq_10m_x4_lambda{lam:.4f}_zeta{zeta:.4f}_" + n for n in names] for lam, zeta in points]
    assert sorted(os.listdir(out_dir)) == sorted(e_names[0] + e_names[1] + ["LR_x4_" + n for n in names] + [n[:-4] + "_LEH.png" for n in names])
    for s in range(2):                                               # batch s holds point s's two images
        (L, leh), est = panels[s]
        for b, n in enumerate(names):
            assert np.array_equal(decoded(os.path.join(out_dir, e_names[s][b])), est[b])
            if s == 0:
                assert np.array_equal(decoded(os.path.join(out_dir, "LR_x4_" + n)), L[b])
            else:
                assert np.array_equal(decoded(os.path.join(out_dir, n[:-4] + "_LEH.png")), leh[b])          # the last point's strip stays
    assert panels[0][0][1] is None and panels[1][0][0] is None       # no strip at the first point, no L at the last: neither is computed there


def test_driver_saves_the_strip_with_its_inset_for_super_resolution(tmp_path, monkeypatch):
    from diffpir_amd import main_ddpir
    res, panels, outs, cwd, out_dir = run_driver(tmp_path, monkeypatch, "sr", task="sr", sf=4, engine_save_results=True, save_E=True, save_L=True,
                                                 save_LEH=True)
    assert len(res) == 1 and np.isfinite(res[0]) and len(panels) == 1 and len(outs) == 1
    names = ["synth_0000.png", "synth_0001.png"]
    lam = main_ddpir.sweeps(main_ddpir.parse_config(str(cwd / "c.yaml")))[0][0]
    e_pre = f"diffusion_ffhq_10m_x4_lambda{lam:.4f}_zeta0.1000_"
    want = sorted([e_pre + n for n in names] + ["LR_x4_" + n for n in names] + ["synth_0000_LEH.png", "synth_0001_LEH.png"])
    assert sorted(os.listdir(out_dir)) == want                        # no kernel picture: that is the deblurring task's
    (L, leh), kw = panels[0]
    assert kw["sf"] == 4 and L.shape == (2, 64, 64, 3) and leh.shape == (2, 256, 768, 3)
    kh = kw["k"].shape[2]
    for b, n in enumerate(names):
        assert np.array_equal(decoded(os.path.join(out_dir, e_pre + n)), outs[0][b])
        assert np.array_equal(decoded(os.path.join(out_dir, "LR_x4_" + n)), L[b])
        assert np.array_equal(decoded(os.path.join(out_dir, n[:-4] + "_LEH.png")), leh[b])
        assert np.array_equal(leh[b, :64, :64], L[b]) and np.array_equal(leh[b, :, 256:512], outs[0][b])
        inset = np.repeat(np.repeat(R.kernel_bytes(kw["k"][b, 0]), 3, 0), 3, 1)
        assert 3 * kh <= 192                                          # the inset lies right of the 64 x 64 paste: all of it shows
        assert all(np.array_equal(leh[b, :3 * kh, 256 - 3 * kh:256, c], inset) for c in range(3))
        assert np.array_equal(leh[b, 200, 100], L[b, 50, 25])         # the zoom below the inset and the paste


def test_l_only_needs_no_room_for_the_inset(engine, tmp_path, monkeypatch):
    """save_L and save_E without the strip on images smaller than 3 x the kernel (61 x 61 on 128 x 128): the wrapper passes no kernel for an
    L-only call and the driver writes E, L and the kernel picture (tests/test_results_host.py: asking for the strip there is refused ahead of all work)."""
    y, est, gt, _ = inputs(2, 24, 40, 2, 0, 0, 16)
    k = np.random.default_rng(17).random((2, 1, 9, 9)) + 0.01       # 3 x 9 = 27 > 24
    gL, gS = dgr.result_panels(engine, y, est, gt, k=k, sf=2, want_LEH=False)
    assert gS is None and gL.tobytes() == R.l_bytes(y).tobytes()
    from diffpir_amd import main_ddpir
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "engine_example.yaml")))
    assert cfg["save_L"] and cfg["save_E"] and "save_LEH" not in cfg and cfg["kernel_size"] == 61
    cfg.update(iter_num=4, batch_size=2, cwd=str(tmp_path), engine_save_results=True)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    panels, real = [], dgr.result_panels

    def rec(eng, y_, est_, gt_, **kw):
        out = real(eng, y_, est_, gt_, **kw)
        panels.append((out, kw, est_.numpy()))
        return out
    monkeypatch.setattr(dgr, "result_panels", rec)
    res = main_ddpir.main(["--opt", str(p), "--synthetic", "2", "--synthetic-size", "128x128", "--max-sweeps", "1"])
    assert len(res) == 1 and np.isfinite(res[0]) and len(panels) == 1
    (L, leh), kw, est_u8 = panels[0]
    assert leh is None and kw["k"] is None and L.shape == (2, 128, 128, 3)
    out_dir = main_ddpir.result_dir(main_ddpir.parse_config(str(p)))
    names = ["synth_0000.png", "synth_0001.png"]
    e_pre = "diffusion_ffhq_10m_x1_lambda7.0000_zeta0.3000_"
    assert sorted(os.listdir(out_dir)) == sorted([e_pre + n for n in names] + ["LR_x1_" + n for n in names] + ["motion_kernel_" + n for n in names])
    for b, n in enumerate(names):
        assert np.array_equal(decoded(os.path.join(out_dir, "LR_x1_" + n)), L[b])
        assert np.array_equal(decoded(os.path.join(out_dir, e_pre + n)), est_u8[b])
        assert decoded(os.path.join(out_dir, "motion_kernel_" + n)).shape == (61, 61)
