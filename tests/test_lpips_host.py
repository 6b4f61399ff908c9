"""CPU: the host side of LPIPS (diffpir_amd/lpips.py, the driver's calc_LPIPS switch, the ABI table) and proof that the float64 checker of
tests/lpips_f64.py rejects planted defects, each on its own."""
import logging
import os
import re

import numpy as np
import pytest
import torch

from diffpir_amd import _lib, lpips as lp, main_ddpir as drv
from tests import lpips_f64 as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd():
    return lp.synth_weights(3)


def _torchvision_layout(sd):
    out = {k: torch.from_numpy(v) for k, v in sd.items() if k.startswith("features.")}
    out["classifier.0.bias"] = torch.zeros(4)                  # the file holds the classifier too: ignored
    return out


def _heads_layout(sd):
    return {f"lin{k}.model.1.weight": torch.from_numpy(sd[f"lin{k}.weight"]).view(1, -1, 1, 1) for k in range(5)}


def _full_layout(sd):
    out = {}
    for k, v in sd.items():
        if k.startswith("features."):
            i, leaf = k.split(".")[1:]
            s = 1 + sum(int(i) >= b for b in (4, 9, 16, 23))
            out[f"net.slice{s}.{i}.{leaf}"] = torch.from_numpy(v)
    for k in range(5):
        w = torch.from_numpy(sd[f"lin{k}.weight"]).view(1, -1, 1, 1)
        out[f"lin{k}.model.1.weight"] = w
        out[f"lins.{k}.model.1.weight"] = w
    out["scaling_layer.shift"] = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
    out["scaling_layer.scale"] = torch.tensor([.458, .448, .450]).view(1, 3, 1, 1)
    return out


def test_spec_is_vgg16_features_and_five_heads(sd):
    spec = lp.vgg_spec()
    convs = [s for s in spec if s[2] == "w"]
    assert len(convs) == 13 and len([s for s in spec if s[2] == "lin"]) == 5
    assert [int(k.split(".")[1]) for k, _, _ in convs] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert sum(int(np.prod(shape)) for _, shape, kind in spec if kind in ("w", "b")) == 14_714_688
    assert [shape[0] for _, shape, kind in spec if kind == "lin"] == [64, 128, 256, 512, 512]
    assert set(sd) == {k for k, _, _ in spec} and all(sd[k].shape == shape and sd[k].dtype == np.float32 for k, shape, _ in spec)
    assert all((sd[f"lin{k}.weight"] >= 0).all() for k in range(5))
    again = lp.synth_weights(3)
    assert all(np.array_equal(sd[k], again[k]) for k in sd) and not np.array_equal(sd["features.0.weight"], lp.synth_weights(4)["features.0.weight"])
    # 2 * MAC of the 13 convolutions: about 80 GFLOP per image PAIR at 256 x 256
    assert lp.trunk_flops(256, 256) == 40_089_157_632 and lp.trunk_flops(16, 16) == lp.trunk_flops(256, 256) / 256
    assert 2 * lp.trunk_flops(256, 256) == pytest.approx(80e9, rel=5e-3)


def test_three_key_layouts_load_to_identical_arrays(sd, tmp_path):
    a = lp.canonical({**_torchvision_layout(sd), **_heads_layout(sd)})
    b = lp.canonical(_full_layout(sd))
    torch.save(_torchvision_layout(sd), tmp_path / "vgg16.pth")
    torch.save(_heads_layout(sd), tmp_path / "heads.pth")
    torch.save(_full_layout(sd), tmp_path / "full.pth")
    c = lp.load_weights(str(tmp_path / "vgg16.pth"), str(tmp_path / "heads.pth"))
    d = lp.load_weights(str(tmp_path / "full.pth"))
    for got in (a, b, c, d, lp.canonical(sd)):
        assert list(got) == [k for k, _, _ in lp.vgg_spec()]
        for k in sd:
            assert got[k].dtype == np.float32 and got[k].shape == sd[k].shape and np.array_equal(got[k], sd[k]), k


def test_missing_misshaped_and_foreign_scaling_raise_and_name_the_key(sd):
    bad = dict(sd)
    del bad["features.17.bias"]
    with pytest.raises(KeyError, match=r"features\.17\.bias"):
        lp.canonical(bad)
    with pytest.raises(KeyError, match=r"lin0\.weight"):
        lp.canonical(_torchvision_layout(sd))                    # the trunk alone: heads missing
    bad = dict(sd)
    bad["features.5.weight"] = np.zeros((128, 64, 1, 1), np.float32)
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        lp.canonical(bad)
    bad = _full_layout(sd)
    bad["lin3.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        lp.canonical(bad)
    bad = _full_layout(sd)
    bad["scaling_layer.shift"] = torch.tensor([.030, -.088, -.188]).view(1, 3, 1, 1)
    with pytest.raises(ValueError, match=r"scaling_layer\.shift"):
        lp.canonical(bad)


# ------------------------------------------------------------------------------------------------------------------ the statement
def _pair(H, W, B=1, kind="noise"):
    x0, gt_u8 = L.make_pair(H, W, B, kind)
    return x0, L.gt_single(gt_u8)


def test_statement_sanity(sd):
    x0, gt = _pair(32, 32, B=2)
    assert x0.min() < 0 and x0.max() > 1
    s_xx, taps = L.lpips(sd, x0, x0)
    assert np.all(s_xx == 0.0)
    assert [t.shape for t in taps] == [(4, 64, 32, 32), (4, 128, 16, 16), (4, 256, 8, 8), (4, 512, 4, 4), (4, 512, 2, 2)]
    assert all((t >= 0).all() for t in taps)
    s_ab, _ = L.lpips(sd, x0, gt)
    s_ba, _ = L.lpips(sd, gt, x0)
    np.testing.assert_allclose(s_ab, s_ba, rtol=1e-12)
    assert np.all(s_ab > 0)
    s1, _ = L.lpips(sd, x0[1:], gt[1:])
    np.testing.assert_allclose(s1, s_ab[1:], rtol=1e-12)


@pytest.fixture(scope="module")
def refs(sd):
    """(x0, gt, float64 statement, float32 statement) of a noisy and a one-pixel pair at 40 x 56 (5 -> 2 and 7 -> 3 floors)."""
    out = {}
    for kind in ("noise", "pixel"):
        x0, gt = _pair(40, 56, kind=kind)
        out[kind] = (x0, gt, L.lpips(sd, x0, gt), L.lpips(sd, x0, gt, torch.float32))
    return out


def test_float32_statement_passes_its_own_checker(refs):
    for kind, (x0, gt, r64, r32) in refs.items():
        s = L.check(r32[0], r32[1], r64, r32, f"float32 statement, {kind}")
        assert s["score_rel32"] <= L.SCORE_CAP


@pytest.mark.parametrize("defect", ["pool_ceil", "tap_before_relu", "shift_sign"])
def test_checker_rejects_a_planted_trunk_defect(sd, refs, defect):
    x0, gt, r64, r32 = refs["noise"]
    score, taps = L.lpips(sd, x0, gt, torch.float32, defect=defect)
    assert not L.ok(score, taps, r64, r32)


def test_checker_rejects_the_epsilon_inside_the_square_root(sd):
    """sqrt(s + 1e-10) differs from sqrt(s) + 1e-10 only where the channel norm is small: a last convolution scaled down to 1e-7 puts relu5_3
    there (norms ~1e-6).  The taps are untouched by this defect; the score catches it."""
    small = dict(sd)
    small["features.28.weight"] = sd["features.28.weight"] * np.float32(1e-7)
    small["features.28.bias"] = sd["features.28.bias"] * np.float32(1e-7)
    x0, gt = _pair(40, 56)
    r64, r32 = L.lpips(small, x0, gt), L.lpips(small, x0, gt, torch.float32)
    assert L.ok(r32[0], r32[1], r64, r32)
    score, taps = L.lpips(small, x0, gt, torch.float32, defect="eps_inside_sqrt")
    assert L.stats(score, taps, r64, r32)["margin"] <= 1.0
    assert not L.ok(score, taps, r64, r32)


def test_checker_rejects_the_expanded_head_on_a_one_pixel_pair(sd, refs):
    x0, gt, r64, r32 = refs["pixel"]
    assert 0 < r64[0][0] < 1e-5                                  # the score is a tiny fraction of the three sums
    score, taps = L.lpips(sd, x0, gt, torch.float32, defect="expanded_head")
    assert L.stats(score, taps, r64, r32)["margin"] <= 1.0       # same taps
    assert not L.ok(score, taps, r64, r32)


# ------------------------------------------------------------------------------------------------------------------ driver and ABI
class _NoEngine:
    def load_lpips(self, sd):
        raise AssertionError("no weights may be loaded when the files are absent")


def test_driver_without_weight_files_warns_once_and_runs_as_before(tmp_path, caplog):
    cfg = drv.Config(dict(calc_LPIPS=True, cwd=str(tmp_path)))
    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        assert drv.setup_lpips(_NoEngine(), cfg) is False
        drv.log_batch(1, 30.0, None, 0.0)
    warns = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warns) == 1 and "calc_LPIPS" in warns[0].getMessage() and "vgg16-397923af.pth" in warns[0].getMessage() \
        and "lpips_vgg.pth" in warns[0].getMessage()
    assert [r.getMessage() for r in caplog.records if r.levelno == logging.INFO] == ["batch   1--> PSNR: 30.0000dB"]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        assert drv.setup_lpips(_NoEngine(), drv.Config(dict(calc_LPIPS=False, cwd=str(tmp_path)))) is False      # key off: silent
        assert drv.setup_lpips(_NoEngine(), drv.Config(dict(cwd=str(tmp_path)))) is False
        drv.log_batch(2, 30.0, 0.12345, 0.5)
    assert not [r for r in caplog.records if r.levelno == logging.WARNING]
    assert caplog.records[-1].getMessage() == "batch   2--> PSNR: 30.0000dB; LPIPS: 0.1235; ave LPIPS: 0.5000"


def test_driver_finds_the_weight_files_by_their_yaml_keys(sd, tmp_path):
    zoo = tmp_path / "model_zoo"
    zoo.mkdir()
    torch.save(_torchvision_layout(sd), zoo / "vgg16-397923af.pth")
    torch.save(_heads_layout(sd), zoo / "my_heads.pth")
    cfg = drv.Config(dict(calc_LPIPS=True, cwd=str(tmp_path), lpips_lin_path="my_heads.pth"))
    assert [os.path.basename(p) for p in lp.find_weight_files(cfg)] == ["vgg16-397923af.pth", "my_heads.pth"]
    loaded = []

    class Eng:
        def load_lpips(self, s):
            loaded.append(s)
    assert drv.setup_lpips(Eng(), cfg) is True
    assert len(loaded) == 1 and all(np.array_equal(loaded[0][k], sd[k]) for k in sd)


def test_abi_has_the_lpips_entries_and_is_still_version_2():
    names = {"dpir_lpips_load", "dpir_lpips", "dpir_lpips_keep_taps", "dpir_lpips_read_tap"}
    assert names <= set(_lib.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "diffpir_engine.h")).read()
    assert names <= set(re.findall(r"\b(dpir_[a-z0-9_]+)\s*\(", hdr))
    assert "#define DPIR_ABI_VERSION 2" in hdr and _lib.ABI_VERSION == 2
    lib = _lib.load()
    assert lib.dpir_version() == 2 and all(hasattr(lib, n) for n in names)
