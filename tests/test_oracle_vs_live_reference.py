"""CPU: the reference's OWN loop -- `test_rho`, taken out of the reference's main_ddpir.py with `ast` and executed unmodified
(oracle/ref_exec.py) -- against the oracle restatement.  What the executed reference produced is stored as data in
tests/golden/executed_reference.npz (oracle/gen_golden_executed.py re-executes it where the reference tree is at hand), so these tests
run on every checkout of the repository."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as uo, diffpir_oracle as do
from oracle.gen_golden_executed import case, seeded


@pytest.fixture(scope="module")
def tiny():
    hp = uo.tiny_hp()
    return hp, uo.synth_state_dict(hp, 0)


def test_the_pieces_executed_are_the_reference_lines_and_the_one_edit_is_one_statement(golden):
    ex = golden("executed_reference")
    lines = {piece: tuple(int(v) for v in ex[f"lines_{piece}"]) for piece in ("schedule", "freeze", "test_rho", "sweep")}
    assert lines["schedule"] == (184, 200) and lines["freeze"] == (236, 239) and lines["test_rho"] == (249, 536) and lines["sweep"] == (548, 580)
    assert int(ex["n_stmt_test_rho"]) - int(ex["n_stmt_test_rho_deblur"]) == 1 and int(ex["n_dropped"]) == 1 and bool(ex["dropped_is_q1"])     # SURVEY quirk Q1, nothing else
    # as shipped, a deblur batch cannot pass that statement
    with pytest.raises(RuntimeError):
        torch.einsum('ab,cd->abcd', torch.eye(3), torch.zeros(2, 5, 5))


@pytest.mark.parametrize("name", ["deblur", "inpaint", "sr_cubic", "repaint", "dps_yt"])
def test_oracle_equals_the_executed_reference_loop(tiny, golden, name):
    hp, sd = tiny
    ex = golden("executed_reference")
    cfg, y, k, mask, seed = case(golden, name)
    ty = torch.from_numpy(y)
    tk = None if k is None else torch.from_numpy(k)
    tm = None if mask is None else torch.from_numpy(mask).float()
    ref = ex[f"out_{name}"]
    if name == "dps_yt":
        ora = do.restore_dps_y0(sd, hp, cfg, ty, noise_fn=seeded(seed)).numpy()
    else:
        with torch.no_grad():
            ora = do.restore(sd, hp, cfg, ty, k=tk, mask=tm, noise_fn=seeded(seed)).numpy()
    d = float(np.abs(ora - ref).max())
    print(f"{name}: oracle vs executed test_rho max |diff| {d:.3e} (output range [{ref.min():.2f}, {ref.max():.2f}])")
    assert np.isfinite(ref).all() and d <= 5e-6
    if name == "dps_yt":
        _, steps = do.step_tables(cfg)
        assert all(float(st["tau"]) == float(ex["dps_yt_rhos"][st["t_i"]]) for st in steps)       # the table DPS_yt divides by, bit for bit


@pytest.mark.parametrize("task", ["deblur", "sr"])
def test_engine_schedule_and_sweep_equal_the_executed_reference(golden, task):
    """The PRODUCT's host logic against the reference executed live: `diffpir_amd.main_ddpir.sweeps` (the lambda / zeta the YAML driver hands to
    the loop) and `diffpir_amd.schedule.build_steps` (the per-step t_i and tau the engine uploads) versus what the reference's own sweep +
    test_rho visit -- every `t_i` it calls the denoiser at and every `tau` it passes to `data_solution`, recorded by executing
    main_ddpir.py:548-580 over a stand-in network (oracle/ref_exec.reference_step_trace, stored in tests/golden/executed_reference.npz)."""
    from oracle.gen_golden_executed import stored_yaml_for
    from diffpir_amd import main_ddpir as drv, schedule
    yd = stored_yaml_for(task, iter_num=20)
    ex = golden("executed_reference")
    ts, taus = ex[f"ts_{task}"], ex[f"taus_{task}"]
    cfg = drv.Config(dict(yd))
    cfg.noise_level_img = cfg.noise_level_img / 255.0
    cfg.sigma = max(0.001, cfg.noise_level_img)
    sw = drv.sweeps(cfg)
    assert len(sw) == (11 if task == "sr" else 1)
    n = 20
    assert len(ts) == n * len(sw) and len(taus) == (n - 1) * len(sw)
    for i, (lambda_, zeta) in enumerate(sw):
        _, steps, _ = schedule.build_steps(iter_num=n, sigma=cfg.sigma, lambda_=lambda_, zeta=zeta)
        assert [st["t"] for st in steps] == list(ts[i * n:(i + 1) * n])
        assert [np.float32(st["tau"]) for st in steps if not st["last"]] == list(taus[i * (n - 1):(i + 1) * (n - 1)])
