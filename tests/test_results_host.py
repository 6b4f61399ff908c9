"""CPU tests of the saved results (engine_save_results): the four kinds of file name under the three `driver:` values against strings written
out by hand from the reference's lines; the plain-numpy statement tests/results_ref.py against the live util.single2uint / util.tensor2uint
where the reference tree is present, and its composition facts; the writer pool; and the switch."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

from diffpir_amd import _lib, main_ddpir
from oracle import ref_import
from tests import results_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(**kw):
    d = dict(task="deblur", sf=1, model_name="diffusion_ffhq_10m", testset_name="demo_test", generate_mode="DiffPIR", noise_level_img=0.05,
             iter_num=100, eta=0, zeta=0.1, lambda_=1, blur_mode="Gaussian", sr_mode="blur", cwd="", batch_size=2)
    d.update(kw)
    return main_ddpir.Config(d)


# ------------------------------------------------------------------------------------------------------------------ names
def test_file_names_of_main_ddpir():
    """main_ddpir.py:499 / :511 / :299: imsave_batch puts its prefix in front of the WHOLE file name (utils_image.py:168-173)."""
    names = main_ddpir.result_file_names(config(task="deblur"), "69037.png", 7.0, 0.3)
    assert names == ("diffusion_ffhq_10m_x1_lambda7.0000_zeta0.3000_69037.png", "LR_x1_69037.png", "69037_LEH.png", "motion_kernel_69037.png")
    # a .jpg name, and a lambda that needs the :.4f rounding (12 x 0.33335 = 4.0002 -> "4.0002"; 1 / 3 -> "0.3333")
    names = main_ddpir.result_file_names(config(task="sr", sf=4), "ILSVRC2012_val_00000003.jpg", 12 * 0.33335, 1 / 3)
    assert names == ("diffusion_ffhq_10m_x4_lambda4.0002_zeta0.3333_ILSVRC2012_val_00000003.jpg", "LR_x4_ILSVRC2012_val_00000003.jpg",
                     "ILSVRC2012_val_00000003_LEH.jpg", None)
    assert main_ddpir.result_file_names(config(task="sr", sf=4), "a.png", 0.00005, 2.00005)[0] == "diffusion_ffhq_10m_x4_lambda0.0001_zeta2.0000_a.png"
    names = main_ddpir.result_file_names(config(task="inpaint", model_name="256x256_diffusion_uncond"), "a.b.png", 1, 1)
    assert names == ("256x256_diffusion_uncond_x1_lambda1.0000_zeta1.0000_a.b.png", "LR_x1_a.b.png", "a.b256x256_diffusion_uncond_LEH.png", None)


def test_file_names_of_the_standalone_programs():
    """main_ddpir_deblur.py:398, 424, 421, 177 and main_ddpir_inpainting.py:341, 344, 347 (no underscore in front of the strip's model name)."""
    names = main_ddpir.result_file_names(config(task="deblur", driver="main_ddpir_deblur"), "69037.jpg", 7.0, 0.3)
    assert names == ("69037_diffusion_ffhq_10m.jpg", "69037_LR.jpg", "69037_LEH.jpg", "motion_kernel_69037.jpg")
    names = main_ddpir.result_file_names(config(task="inpaint", driver="main_ddpir_inpainting"), "69037.png", 1.0, 1.0)
    assert names == ("69037_diffusion_ffhq_10m.png", "69037_L.png", "69037diffusion_ffhq_10m_LEH.png", None)


def test_the_header_and_the_binding_declare_the_entry():
    assert "dpir_result_panels" in _lib.SIGNATURES and len(_lib.SIGNATURES["dpir_result_panels"][1]) == 8
    hdr = open(os.path.join(ROOT, "include", "diffpir_engine.h")).read()
    decl = re.search(r"\bint dpir_result_panels\(([^)]*)\)", hdr)
    assert decl and len(decl.group(1).split(",")) == 8
    body = re.search(r"typedef struct dpir_result_desc \{(.*?)\} dpir_result_desc;", hdr, re.S).group(1)
    fields = re.findall(r"\b(B|H|W|sf|kh|kw|mode)\b(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in _lib.ResultDesc._fields_] and C.sizeof(_lib.ResultDesc) == 28
    for line in ("main_ddpir.py:508-511", "main_ddpir_deblur.py:412-421", "main_ddpir_inpainting.py:346-347"):
        assert line in hdr
    assert _lib.ABI_VERSION == 2 and "#define DPIR_ABI_VERSION 2" in hdr                      # appended to: no layout moved


# ------------------------------------------------------------------------------------------------------------------ the statement
def measurement(B, h, w, seed):
    rng = np.random.default_rng(seed)
    y = rng.uniform(-0.2, 1.2, (B, 3, h, w)).astype(np.float32)
    t = R.tie_values()
    y.reshape(-1)[:t.size] = t
    return y


@pytest.mark.skipif(not ref_import.available(), reason="reference tree absent")
def test_statement_bytes_are_the_live_single2uint_and_tensor2uint():
    import torch
    ui = ref_import.load().utils_image
    y = measurement(2, 6, 10, 0)
    for b in range(2):
        img_L = np.transpose(y[b], (1, 2, 0))
        assert np.array_equal(ui.single2uint(img_L), R.l_bytes(y)[b])
        assert np.array_equal(ui.tensor2uint(torch.from_numpy(y[b:b + 1].copy())), R.l_bytes(y)[b])       # E: the loop's out_u8 conversion
    k = np.random.default_rng(1).random((7, 7))
    assert np.array_equal(ui.single2uint(k / np.max(k) * 1.0), R.kernel_bytes(k))


def test_ties_round_half_to_even_in_float32():
    t = R.tie_values()
    got = R.l_bytes(np.broadcast_to(t[None, None, None, :], (1, 3, 1, t.size)).astype(np.float32))[0, 0, :, 0]
    want = np.rint(np.clip(t, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    assert got.tolist() == want.tolist()
    assert len(set(got.tolist())) > 8                              # the values straddle the byte boundaries: both sides occur


def strip_inputs(B, H, W, sf, kh, seed):
    rng = np.random.default_rng(seed)
    y = measurement(B, H // sf, W // sf, seed)
    est = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    gt = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    k = rng.random((B, kh, kh)) + 0.01
    return y, est, gt, k


def test_with_sf_1_the_paste_hides_the_inset():
    y, est, gt, k = strip_inputs(2, 24, 24, 1, 5, 2)
    L, leh = R.panels(y, est, gt, k, 1)
    _, plain = R.panels(y, est, gt, None, 1)
    assert np.array_equal(leh, plain) and np.array_equal(leh[:, :, :24], L)
    assert np.array_equal(leh, R.panels(y, est, gt, mode="inpaint")[1])
    assert np.array_equal(leh[:, :, 24:48], est) and np.array_equal(leh[:, :, 48:], gt)


def test_with_sf_2_the_inset_shows_exactly_outside_the_paste():
    B, H, W, sf, kh = 2, 24, 40, 2, 7                             # inset 21 x 21 at columns [19, 40), paste 12 x 20: they overlap in [0,12) x [19,20)
    y, est, gt, k = strip_inputs(B, H, W, sf, kh, 3)
    L, leh = R.panels(y, est, gt, k, sf)
    _, plain = R.panels(y, est, gt, None, sf)
    h, w = H // sf, W // sf
    inset = np.zeros((H, W), bool)
    inset[:3 * kh, W - 3 * kh:] = True
    inset[:h, :w] = False
    assert inset[:h, w:].any() and not inset[:h, W - 3 * kh:w].any()
    for b in range(B):
        kv = np.repeat(np.repeat(R.kernel_bytes(k[b]), 3, 0), 3, 1)
        p0 = leh[b, :, :W]
        assert np.array_equal(p0[:h, :w], L[b])
        assert np.array_equal(p0[~inset], plain[b, :, :W][~inset])
        want = np.zeros((H, W), np.uint8)
        want[:3 * kh, W - 3 * kh:] = kv
        assert all(np.array_equal(p0[..., c][inset], want[inset]) for c in range(3))
        assert np.array_equal(plain[b, 15, 39], L[b, 7, 19]) and np.array_equal(plain[b, 23, 22], L[b, 11, 11])       # the zoom reads (Y // sf, X // sf)
    assert R.kernel_bytes(k[0]).max() == 255


def test_an_inset_as_wide_as_the_image_works_and_a_taller_one_raises():
    y, est, gt, k = strip_inputs(1, 24, 21, 1, 7, 4)              # 3 kw == W
    y2 = measurement(1, 12, 7, 4)
    est2, gt2 = est[:, :, :14], gt[:, :, :14]
    k2 = np.random.default_rng(5).random((1, 4, 4)) + 0.01        # H 24, W 14 at sf 2; 3 kw = 12 <= 14
    R.panels(y, est, gt, k, 1)
    _, leh = R.panels(np.ascontiguousarray(y2), est2, gt2, np.random.default_rng(6).random((1, 8, 4)), 2)       # 3 kh == H
    assert leh.shape == (1, 24, 42, 3)
    yw = measurement(1, 12, 6, 7)
    _, leh = R.panels(yw, est[:, :, :12], gt[:, :, :12], k2, 2)   # 3 kw == W == 12: the inset spans the whole row above the paste's right edge
    kv = np.repeat(np.repeat(R.kernel_bytes(k2[0]), 3, 0), 3, 1)
    assert np.array_equal(leh[0, :12, 6:12, 0], kv[:, 6:]) and np.array_equal(leh[0, :12, :6], R.l_bytes(yw)[0])
    with pytest.raises(ValueError):
        R.panels(y2, est2, gt2, np.ones((1, 9, 4)), 2)            # 3 kh = 27 > 24
    with pytest.raises(ValueError):
        R.panels(y2, est2, gt2, np.ones((1, 4, 5)), 2)            # 3 kw = 15 > 14


def test_kernel_picture_saturates_and_rounds():
    """k x 51000 has no exact .5 tie inside [0, 255] for a binary float k (51000 = 2^3 x 6375), so half-to-even never decides; the rest does."""
    k = np.array([[0.0, 0.00099, 0.00101], [0.00001, 0.004, 0.006], [-1.0, 1.0, 0.00499]])
    want = np.array([[0, 50, 52], [1, 204, 255], [0, 255, 254]], np.uint8)          # 50.49, 51.51, 0.51, 204, 306, -51000, 51000, 254.49
    assert np.array_equal(R.kernel_picture(k), want) and np.array_equal(main_ddpir.kernel_picture(k), want)
    k32 = np.random.default_rng(10).random((9, 9)).astype(np.float32) / 81
    assert np.array_equal(main_ddpir.kernel_picture(k32), R.kernel_picture(k32)) and main_ddpir.kernel_picture(k32).dtype == np.uint8


# ------------------------------------------------------------------------------------------------------------------ the writer pool
def test_writer_pool_writes_every_file(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(8)
    files = {}
    rw = main_ddpir.ResultWriter(files_per_batch=3, workers=3)
    assert rw.q.maxsize == 6 and len(rw.threads) == 3
    for i in range(20):                                          # more than the queue holds: submit blocks and goes on
        a = rng.integers(0, 256, (9, 12, 3) if i % 2 else (9, 12), dtype=np.uint8)
        files[str(tmp_path / "deep" / "er" / f"f{i}.png")] = a
        rw.submit(str(tmp_path / "deep" / "er" / f"f{i}.png"), a)
    rw.drain()
    for path, a in files.items():
        img = Image.open(path)
        assert img.mode == ("RGB" if a.ndim == 3 else "L")
        assert np.array_equal(np.asarray(img), a)
    rw.submit(str(tmp_path / "again.png"), files[str(tmp_path / "deep" / "er" / "f0.png")])           # usable after a drain
    rw.drain()
    assert os.path.exists(tmp_path / "again.png")
    rw.close()
    assert not rw.threads
    assert len(main_ddpir.ResultWriter(1, workers=100).threads) == main_ddpir.ResultWriter.MAX_WORKERS == 8


def test_a_worker_s_exception_surfaces_from_drain():
    seen, lock = [], threading.Lock()

    def writer(path, array):
        with lock:
            seen.append(path)
        if path == "bad":
            raise OSError("disk full")
    rw = main_ddpir.ResultWriter(2, workers=2, writer=writer)
    for p in ("a", "bad", "b", "c"):
        rw.submit(p, None)
    with pytest.raises(OSError, match="disk full"):
        rw.drain()
    assert sorted(seen) == ["a", "b", "bad", "c"]               # the other files were still written
    assert not rw.threads                                          # a failed drain ends the pool


# ------------------------------------------------------------------------------------------------------------------ the switch
def batch_arrays(n, H, W, sf):
    rng = np.random.default_rng(9)
    return dict(est_u8=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), L_u8=rng.integers(0, 256, (n, H // sf, W // sf, 3), dtype=np.uint8),
                leh_u8=rng.integers(0, 256, (n, H, 3 * W, 3), dtype=np.uint8), k=rng.random((n, 1, 5, 5)))


def test_with_the_switch_off_nothing_is_written():
    calls = []
    for extra in (dict(), dict(engine_save_results=False)):
        cfg = config(save_E=True, save_L=True, save_LEH=True, **extra)
        assert main_ddpir.result_options(cfg) == (False, False, False, False)
        assert main_ddpir.emit_results(cfg, ["a.png", "b.png"], 7.0, 0.3, submit=lambda *a: calls.append(a), **batch_arrays(2, 8, 8, 1)) == []
        assert main_ddpir.make_result_writer(cfg, 8, 8) is None
    assert calls == []
    cfg = config(engine_save_results=True, save_E=False, save_L=False)
    assert main_ddpir.result_options(cfg) == (False, False, False, False) and main_ddpir.make_result_writer(cfg, 8, 8) is None


def test_emit_results_writes_the_expected_set(tmp_path):
    cfg = config(engine_save_results=True, save_E=True, save_L=True, save_LEH=True, cwd=str(tmp_path))
    assert main_ddpir.result_options(cfg) == (True, True, True, True)
    assert main_ddpir.result_options(config(engine_save_results=True, save_E=True)) == (True, False, False, True)      # save_LEH defaults to false
    assert main_ddpir.result_options(config(engine_save_results=True, save_E=True, task="sr")) == (True, False, False, False)
    arrays, got = batch_arrays(2, 8, 8, 1), {}
    paths = main_ddpir.emit_results(cfg, ["a.png", "b.jpg"], 7.0, 0.3, submit=lambda p, a: got.__setitem__(p, a), **arrays)
    d = main_ddpir.result_dir(cfg)
    assert d.startswith(str(tmp_path)) and sorted(paths) == sorted(got)
    want = {"motion_kernel_a.png": R.kernel_picture(arrays["k"][0, 0]), "diffusion_ffhq_10m_x1_lambda7.0000_zeta0.3000_a.png": arrays["est_u8"][0],
            "LR_x1_a.png": arrays["L_u8"][0], "a_LEH.png": arrays["leh_u8"][0],
            "motion_kernel_b.jpg": R.kernel_picture(arrays["k"][1, 0]), "diffusion_ffhq_10m_x1_lambda7.0000_zeta0.3000_b.jpg": arrays["est_u8"][1],
            "LR_x1_b.jpg": arrays["L_u8"][1], "b_LEH.jpg": arrays["leh_u8"][1]}
    assert {os.path.relpath(p, d) for p in got} == set(want)
    for name, a in want.items():
        assert np.array_equal(got[os.path.join(d, name)], a), name
    assert got[os.path.join(d, "motion_kernel_a.png")].ndim == 2


def test_rows_of_a_flattened_sweep_write_l_once_and_the_strip_at_the_last_point():
    cfg = config(task="sr", sf=2, engine_save_results=True, save_E=True, save_L=True, save_LEH=True)
    arrays, got = batch_arrays(4, 8, 8, 2), []
    # rows: (point 0, image a), (point 0, image b), (point 1, image a), (point 1, image b) of a two-point sweep
    main_ddpir.emit_results(cfg, ["a.png", "b.png", "a.png", "b.png"], [2.0, 2.0, 3.0, 3.0], [0.1] * 4, submit=lambda p, a: got.append((os.path.basename(p), a)),
                            first=[True, True, False, False], last=[False, False, True, True], **arrays)
    names = [n for n, _ in got]
    assert len(set(names)) == len(names) == 8                      # no path twice: nothing can race inside a batch
    assert sorted(names) == sorted(["diffusion_ffhq_10m_x2_lambda2.0000_zeta0.1000_a.png", "diffusion_ffhq_10m_x2_lambda2.0000_zeta0.1000_b.png",
                                    "diffusion_ffhq_10m_x2_lambda3.0000_zeta0.1000_a.png", "diffusion_ffhq_10m_x2_lambda3.0000_zeta0.1000_b.png",
                                    "LR_x2_a.png", "LR_x2_b.png", "a_LEH.png", "b_LEH.png"])
    by = dict(got)
    assert np.array_equal(by["LR_x2_a.png"], arrays["L_u8"][0]) and np.array_equal(by["b_LEH.png"], arrays["leh_u8"][3])


def test_a_strip_whose_inset_cannot_fit_is_refused_before_any_work():
    cfg = config(engine_save_results=True, save_LEH=True, kernel_size=61, use_DIY_kernel=True, kernel_std=3.0)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="save_LEH"):
        main_ddpir.make_result_writer(cfg, 128, 256)             # 3 x 61 = 183 > 128
    assert np.array_equal(np.random.get_state()[1], state)        # the probe of the kernel size leaves numpy's generator alone
    rw = main_ddpir.make_result_writer(cfg, 256, 256)
    assert rw.q.maxsize == 2 * 2 * 2 and len(rw.threads) == 4     # two batches of (strip + kernel picture) x batch_size 2
    rw.close()


class FakeDevice:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


def test_the_kernel_is_passed_only_with_the_strip_and_unused_panels_are_not_asked_for(monkeypatch):
    """save_L without save_LEH on images smaller than 3 x the kernel: the PSFs are the strip's inset, so they do not reach the engine (whose
    3 kh <= H refusal would otherwise end the run after the batch was restored) and the L files are written.  In a flattened sweep a batch that
    holds no first / last point does not compute L / the strip at all."""
    arrays, calls, got = batch_arrays(2, 8, 8, 1), [], []

    def fake_panels(eng, y, est, gt, k=None, sf=1, mode="kernel", want_L=True, want_LEH=True):
        calls.append(dict(k=k, sf=sf, mode=mode, want_L=want_L, want_LEH=want_LEH))
        return (arrays["L_u8"] if want_L else None), (arrays["leh_u8"] if want_LEH else None)
    monkeypatch.setattr(main_ddpir.dgr, "result_panels", fake_panels)

    class RW:
        @staticmethod
        def submit(p, a):
            got.append(os.path.basename(p))
    k = np.random.default_rng(11).random((2, 1, 5, 5))              # 3 x 5 = 15 > 8
    est = FakeDevice(arrays["est_u8"])
    cfg = config(engine_save_results=True, save_E=True, save_L=True)
    assert main_ddpir.make_result_writer(config(engine_save_results=True, save_E=True, save_L=True, kernel_size=61, kernel_std=3.0), 8, 8).close() is None
    main_ddpir.save_results(None, cfg, RW, ["a.png", "b.png"], 7.0, 0.3, None, est, None, k)
    assert calls == [dict(k=None, sf=1, mode="kernel", want_L=True, want_LEH=False)]
    assert sorted(got) == sorted(["LR_x1_a.png", "LR_x1_b.png", "motion_kernel_a.png", "motion_kernel_b.png",
                                  "diffusion_ffhq_10m_x1_lambda7.0000_zeta0.3000_a.png", "diffusion_ffhq_10m_x1_lambda7.0000_zeta0.3000_b.png"])
    del calls[:]
    cfg = config(engine_save_results=True, save_E=True, save_L=True, save_LEH=True)
    main_ddpir.save_results(None, cfg, RW, ["a.png", "b.png"], 7.0, 0.3, None, est, None, k)
    assert calls[0]["k"] is k and calls[0]["want_L"] and calls[0]["want_LEH"]
    main_ddpir.save_results(None, config(task="inpaint", engine_save_results=True, save_LEH=True), RW, ["a.png", "b.png"], 1.0, 1.0, None, est, None, None)
    assert calls[1] == dict(k=None, sf=1, mode="inpaint", want_L=False, want_LEH=True)
    del calls[:], got[:]
    sweep = config(task="sr", sf=2, engine_save_results=True, save_E=True, save_L=True, save_LEH=True)
    for first, last, want in (([True, True], [False, False], (True, False)), ([False, False], [False, False], None),
                              ([False, True], [True, False], (True, True)), ([False, False], [True, True], (False, True))):
        main_ddpir.save_results(None, sweep, RW, ["a.png", "b.png"], [2.0, 3.0], [0.1, 0.1], None, est, None, k, first=first, last=last)
        if want is None:
            assert calls == []                                         # a batch of middle points: E only
        else:
            c = calls.pop()
            assert (c["want_L"], c["want_LEH"]) == want and (c["k"] is k) == want[1] and calls == []
