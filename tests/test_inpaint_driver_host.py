"""CPU tests of driver='main_ddpir_inpainting': what it admits and refuses, its start coefficients, the sub-step row table and the host-noise
draw order against scalars recorded from the standalone program (tests/golden/inpaint_resample.npz), and the test-side restatement of the
loop against that program's x_0."""
import os

import numpy as np
import pytest
import torch

from diffpir_amd import restore, schedule
from oracle import unet_oracle as uo
from tests import inpaint_resample_ref as ref
from tests.gpu_common import seeded_noise_fn_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["diffpir_u1", "diffpir_u2_eta", "diffpir_u3", "repaint_u2", "vanilla_u2"]
f32 = np.float32


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("inpaint_resample")
    assert sorted(str(c) for c in g["cases"]) == CASES
    return g


def test_driver_admits_and_refuses():
    LC = restore.LoopConfig
    for mode in ("DiffPIR", "repaint", "vanilla"):
        for U in (1, 2, 5):
            LC(task="inpaint", driver="main_ddpir_inpainting", generate_mode=mode, iter_num_U=U, iter_num=20).check_supported()
    with pytest.raises(NotImplementedError):
        LC(task="inpaint", driver="main_ddpir_inpainting", sub_1_analytic=False).check_supported()
    with pytest.raises(NotImplementedError):
        LC(task="inpaint", driver="main_ddpir_inpainting", model_output_type="pred_x_prev").check_supported()
    with pytest.raises(NotImplementedError):
        LC(task="inpaint", driver="main_ddpir_inpainting", generate_mode="DPS_y0").check_supported()
    for task in ("deblur", "sr"):
        with pytest.raises(ValueError):
            LC(task=task, driver="main_ddpir_inpainting").check_supported()
    with pytest.raises(ValueError, match=":227"):
        LC(task="inpaint", driver="main_ddpir_inpainting", iter_num=9).check_supported()
    LC(task="inpaint", driver="main_ddpir_inpainting", iter_num=10).check_supported()
    # every other driver keeps its refusals
    with pytest.raises(NotImplementedError):
        LC(task="inpaint", iter_num_U=2).check_supported()
    with pytest.raises(NotImplementedError):
        LC(task="deblur", driver="main_ddpir_deblur", iter_num_U=2).check_supported()
    with pytest.raises(ValueError):
        LC(task="inpaint", driver="main_ddpir_deblur").check_supported()
    LC(task="inpaint", iter_num=6).check_supported()            # the default driver has no schedule-length bound
    with pytest.raises(ValueError):
        LC(task="inpaint", driver="nope").check_supported()


@pytest.mark.parametrize("level,init", [(12.75 / 255, "max"), (0.0, "max"), (25.0 / 255, 120.0)])
def test_start_coefficients_are_the_t_y_initialisation(level, init):
    """main_ddpir_inpainting.py:190-193 in numpy float32 on the driver tables; the default driver's pair is untouched."""
    cfg = restore.LoopConfig(task="inpaint", driver="main_ddpir_inpainting", noise_level_img=level, noise_init_img=init, iter_num=20)
    dt = schedule.DriverTables.make()
    t_start = restore.t_start_of(cfg, dt.reduced)
    t_y = schedule.find_nearest(dt.reduced, 2 * level)
    eff = f32(dt.sqrt_ac[t_start]) / f32(dt.sqrt_ac[t_y])
    sb = np.sqrt(f32(dt.sqrt_1m_ac[t_start]) * f32(dt.sqrt_1m_ac[t_start]) - (eff * eff) * (f32(dt.sqrt_1m_ac[t_y]) * f32(dt.sqrt_1m_ac[t_y])))
    assert eff.dtype == f32 and sb.dtype == f32
    got = restore.start_coefficients(cfg, dt)
    assert (f32(got[0]), f32(got[1])) == (eff, sb)
    cfg.driver = "main_ddpir"
    got = restore.start_coefficients(cfg, dt)
    assert (f32(got[0]), f32(got[1])) == (f32(dt.sqrt_ac[t_start]), f32(dt.sqrt_1m_ac[t_start]))


@pytest.mark.parametrize("name", CASES)
def test_row_table_equals_the_programs_recorded_scalars_bitwise(fx, name):
    cfg = ref.loop_config(ref.case_config(fx, name))
    dt, rows, arr = restore._inpaint_rows(cfg)
    n = len(fx[name + ".t_i"])
    visited = len(set(zip(fx[name + ".t_i"].tolist(), fx[name + ".last"].tolist(), np.arange(n) // cfg.iter_num_U)))
    assert len(rows) == n == visited * cfg.iter_num_U
    assert [r["t"] for r in rows] == fx[name + ".t_i"].tolist()
    assert [-1 if r["t_im1"] is None else r["t_im1"] for r in rows] == fx[name + ".t_im1"].tolist()
    assert [r["last"] for r in rows] == fx[name + ".last"].tolist()
    assert [r["back"] for r in rows] == fx[name + ".back"].tolist()
    for key, col in (("tau", "rho"), ("q", "q")):
        np.testing.assert_array_equal(np.array([r[key] for r in rows], f32).view(np.uint32), fx[f"{name}.{col}"].view(np.uint32), err_msg=key)
    # the set-back pair where the program formed it (rows with back); the table carries it on every non-final row
    bk = fx[name + ".back"].astype(bool)
    for key in ("sae", "sb"):
        np.testing.assert_array_equal(np.array([r[key] for r in rows], f32)[bk].view(np.uint32), fx[f"{name}.{key}"][bk].view(np.uint32), err_msg=key)
    assert all(r.get("sb_arg", 0.0) >= 0.0 for r in rows)
    assert [r["pos"] for r in rows] == (np.arange(n) // cfg.iter_num_U).tolist()
    assert [r["mix_next"] for r in rows] == [1] * (n - 1) + [0]
    for i, r in enumerate(rows):            # the ctypes table holds the same float32 values
        assert (arr[i].t, arr[i].last, arr[i].back, arr[i].pos) == (r["t"], r["last"], r["back"], r["pos"])
        assert f32(arr[i].sb) == f32(r["sb"]) and f32(arr[i].sae) == f32(r["sae"]) and f32(arr[i].tau) == f32(r["tau"])
    assert int(fx[name + ".t_start"]) == restore.t_start_of(cfg, dt.reduced)


def test_set_back_root_is_exactly_zero_when_the_timestep_repeats():
    """quad skipping with iter_num > T/2 visits a timestep twice in a row: sae = 1 and the square root's argument is exactly 0."""
    _, rows, _ = schedule.build_inpaint_rows(iter_num=700, iter_num_U=2, sigma=0.05, lambda_=1.0, zeta=1.0)
    same = [r for r in rows if not r["last"] and r["t_im1"] == r["t"]]
    assert same and all(r["sb"] == 0.0 and r["sae"] == 1.0 for r in same)
    assert all(r.get("sb_arg", 0.0) >= 0.0 for r in rows)


@pytest.mark.parametrize("name", CASES)
def test_host_noise_shapes_equal_the_programs_draws(fx, name):
    cfg = ref.loop_config(ref.case_config(fx, name))
    _, rows, _ = restore._inpaint_rows(cfg)
    shapes = restore.inpaint_host_noise_shapes(cfg, rows, 2, 64, 64)
    assert [tuple(s) for s in shapes] == [tuple(s) for s in fx[name + ".draw_shapes"].tolist()]
    # the drawer consumes exactly that sequence
    seen = []
    out = restore.draw_inpaint_host_noise(lambda s: (seen.append(tuple(s)), np.full(s, len(seen), f32))[1], cfg, rows, 2, 64, 64)
    assert seen == [tuple(s) for s in shapes]
    assert out["init"][0].flat[0] == 1 and out["init"][1].flat[0] == len(seen) // 2 + 1
    assert (out["back"] is not None) == (cfg.iter_num_U > 1) and (out["rp"] is not None) == (cfg.generate_mode == "repaint")


@pytest.fixture(scope="module")
def restated(fx):
    """x_0 of the restatement for every case, computed once."""
    hp = uo.tiny_hp()
    sd = uo.synth_state_dict(hp, 0)
    out = {}
    with torch.no_grad():
        for name in CASES:
            cfg = ref.case_config(fx, name)
            out[name] = ref.restore_ref(sd, hp, cfg, fx["y"], fx["mask"], seeded_noise_fn_torch(cfg["seed"]))
    return out


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_programs_x0(fx, restated, name):
    """The same torch operations in the same order as the program the generator executed.  On the generating machine the result is bitwise at
    torch's default thread count (and at 2 and 4 threads); the thread count moves ATen's convolution / GEMM reductions, and with
    torch.set_num_threads(1) the restatement's own x_0 moves by max|d| = 1.82e-6 (diffpir_u1; 4.2e-7 .. 1.55e-6 on the other four cases).
    The bound is twice that spread of the restatement against itself."""
    spread = 1.82e-6
    d = float(np.abs(restated[name] - fx[name + ".x0"]).max())
    print(f"{name}: max|restatement - program| = {d:.3e} (bound {2 * spread:.2e})")
    assert d <= 2 * spread


def test_generator_still_finds_its_statements():
    from oracle import ref_import
    if not ref_import.available() or not os.path.exists(os.path.join(ref_import.REF_ROOT, "main_ddpir_inpainting.py")):
        pytest.skip("reference tree absent")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_inpaint_resample", os.path.join(ROOT, "tools", "gen_golden_inpaint_resample.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    p = m.pieces()
    assert len(p["schedule"]) >= 6 and len(p["body"]) >= 8
    src = "\n".join(__import__("ast").unparse(n) for n in p["body"])
    for needle in ("t_y", "iter_num_U", "sqrt_alpha_effective", "x_0", "progress_seq"):
        assert needle in src, needle
