"""-m gpu: model_output_type 'pred_x_prev' under driver 'main_ddpir' (dpir_run_ancestral_loop: RePaint-style / plain ancestral inpainting) against
x_0 of the live program (tests/golden/ancestral.npz), against the unfused stepwise loop, and its invariances: graph replay, device noise,
sharding, the progress strip and the uint8 output."""
import numpy as np
import pytest
import torch

from diffpir_amd import restore, script_util
from oracle import unet_oracle as uo, diffpir_oracle as do
from tests import ancestral_ref as ref
from tests.gpu_common import make_model, seeded_noise_fn_np

pytestmark = pytest.mark.gpu
CASES = ["repaint_q10", "repaint_u1000", "vanilla_q10_ddim", "vanilla_u1000"]


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tiny(engine):
    return make_model(engine, uo.tiny_hp())


@pytest.fixture(scope="module")
def diffusion():
    return script_util.create_gaussian_diffusion(steps=1000, learn_sigma=True)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ancestral")


def _cfg(fx, name, **over):
    c = ref.case_config(fx, name)
    return ref.loop_config(c, **over), c["seed"]


def _host(engine, cfg, fx, seed, **kw):
    return restore.restore_batch(engine, cfg, fx["y"], mask=fx["mask"], noise_source="host", noise_fn=seeded_noise_fn_np(seed), **kw)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("graph", [False, True])
def test_loop_matches_the_live_programs_x0(engine, tiny, fx, name, graph):
    """The bounds tests/test_gpu_loop.py holds the inpainting loops to."""
    cfg, seed = _cfg(fx, name)
    out = _host(engine, cfg, fx, seed, use_graph=graph).numpy()
    want, gt = fx[name + ".x0"], fx["gt"]
    err = float(np.abs(out - want).max())
    dpsnr = abs(restore.psnr_batch(out * 2 - 1, gt * 2 - 1) - restore.psnr_batch(want * 2 - 1, gt * 2 - 1))
    print(f"{name} graph={graph}: max|engine - program| {err:.3e}, |dPSNR| {dpsnr:.2e} dB")
    assert err < 2e-3
    assert dpsnr < 1e-3


@pytest.mark.parametrize("name", CASES)
def test_fused_loop_equals_the_stepwise_loop_bitwise(engine, tiny, diffusion, fx, name):
    """dpir_run_ancestral_loop against dpir_repaint_mix -> model_fn 'pred_x_prev' (dpir_p_sample) on the same host noise stream."""
    model, _ = tiny
    cfg, seed = _cfg(fx, name)
    fused = _host(engine, cfg, fx, seed).numpy()
    sw = restore.restore_batch_stepwise(model, diffusion, cfg, engine.to_device(fx["y"]), mask=engine.to_device(fx["mask"], np.uint8),
                                        noise_fn=seeded_noise_fn_np(seed)).numpy()
    np.testing.assert_array_equal(fused, sw)


@pytest.mark.parametrize("name", ["repaint_q10", "vanilla_q10_ddim"])
def test_graph_replay_twice_is_bitwise_identical(engine, tiny, fx, name):
    cfg, seed = _cfg(fx, name)
    a, b, c = (_host(engine, cfg, fx, seed, use_graph=g).numpy() for g in (True, True, False))
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("name", ["repaint_q10", "vanilla_u1000"])
def test_device_noise_loop_equals_host_noise_loop_fed_the_philox_draws(engine, tiny, fx, name):
    """Streams: 0 init; 3 + 4 s the mix ahead of step s; 4 (s + 1) the sampler's draw of step s; image = image_offset + n.  The host-noise loop
    fed dpir_randn's draws at those streams equals the device-noise loop bit for bit, and those draws are the numpy Philox statement's
    (oracle/philox_oracle.py) to the tolerance tests/test_gpu_ops.py holds dpir_randn to (atol 4e-6, rtol 2e-6: logf / sinpif / cospif)."""
    from oracle import philox_oracle as po
    e = engine
    cfg, _ = _cfg(fx, name)
    _, rows, _ = restore._ancestral_rows(cfg)
    B, H, W, seed, off, n = 2, 64, 64, 4242, 3, len(rows)
    dev = restore.restore_batch(e, cfg, fx["y"], mask=fx["mask"], noise_source="device", seed=seed, image_offset=off, use_graph=True).numpy()

    def dr(stream):
        buf = e.empty((B, 3, H, W))
        e._check(e.lib.dpir_randn(e.h, buf.ptr, seed, stream, off, B, 3, H, W))
        got = buf.numpy()
        np.testing.assert_allclose(got, po.randn(seed, stream, off, B, 3 * H * W).reshape(B, 3, H, W), atol=4e-6, rtol=2e-6)
        return got
    rp = cfg.generate_mode == "repaint"
    pre = dict(init=dr(0), ps=np.stack([dr(4 * (s + 1)) for s in range(n)]), rp=np.stack([dr(3 + 4 * s) for s in range(n)]) if rp else None)
    host = restore.restore_batch(e, cfg, fx["y"], mask=fx["mask"], noise_source="host", predrawn=pre).numpy()
    np.testing.assert_array_equal(dev, host)
    # not by accident: another seed gives another image
    other = restore.restore_batch(e, cfg, fx["y"], mask=fx["mask"], noise_source="device", seed=seed + 1, image_offset=off).numpy()
    assert np.abs(other - dev).max() > 1e-3


@pytest.mark.parametrize("name", ["repaint_q10", "vanilla_u1000"])
def test_sharding_invariance_bitwise(engine, tiny, fx, name):
    cfg, _ = _cfg(fx, name)
    both = restore.restore_batch(engine, cfg, fx["y"], mask=fx["mask"], noise_source="device", seed=7, image_offset=10).numpy()
    for n in range(2):
        one = restore.restore_batch(engine, cfg, fx["y"][n:n + 1], mask=fx["mask"][n:n + 1], noise_source="device", seed=7, image_offset=10 + n).numpy()
        np.testing.assert_array_equal(one[0], both[n])


@pytest.mark.parametrize("name", ["repaint_q10", "vanilla_q10_ddim"])
@pytest.mark.parametrize("graph", [False, True])
def test_progress_strip_equals_the_stepwise_strip_and_ends_in_the_result(engine, tiny, diffusion, fx, name, graph):
    """Ten steps, ten panels.  In repaint mode the fused pass applies the next step's mix before x reaches memory: the panel shows x before it."""
    model, _ = tiny
    cfg, seed = _cfg(fx, name)
    pm, ps = restore.Progress(masked=True), restore.Progress(masked=True)
    f, u = _host(engine, cfg, fx, seed, use_graph=graph, return_u8=True, progress=pm)
    plain = _host(engine, cfg, fx, seed, use_graph=graph).numpy()
    restore.restore_batch_stepwise(model, diffusion, cfg, engine.to_device(fx["y"]), mask=engine.to_device(fx["mask"], np.uint8),
                                   noise_fn=seeded_noise_fn_np(seed), progress=ps)
    assert len(pm.panels) == 10 and pm.panels == ps.panels and pm.panels[-1] == (999, 0)
    for key in ("strip_f32", "strip_u8", "masked_f32", "masked_u8", "minmax"):
        np.testing.assert_array_equal(getattr(pm, key), getattr(ps, key), err_msg=key)
    assert pm.strip_f32[..., -64:].tobytes() == f.numpy().tobytes() == plain.tobytes()          # arming changes nothing
    assert pm.strip_u8[:, :, -64:, :].tobytes() == u.numpy().tobytes()


def test_u1000_progress_keeps_the_final_panel(engine, tiny, fx):
    cfg, seed = _cfg(fx, "repaint_u1000")
    pg = restore.Progress()
    f = _host(engine, cfg, fx, seed, use_graph=True, progress=pg).numpy()
    assert pg.panels[-1] == (999, 0)
    assert pg.strip_f32[..., -64:].tobytes() == f.tobytes()


@pytest.mark.parametrize("name", ["repaint_u1000", "vanilla_q10_ddim"])
def test_u8_output_is_the_finalize_conversion_of_the_f32_result(engine, tiny, fx, name):
    """dpir_finalize writes both outputs from one x; its uint8 conversion is utils_image.tensor2uint_batch's (tests/test_gpu_ops.py)."""
    cfg, seed = _cfg(fx, name)
    f, u = _host(engine, cfg, fx, seed, use_graph=True, return_u8=True)
    np.testing.assert_array_equal(u.numpy(), do.tensor2uint_batch(torch.from_numpy(f.numpy())))
    # skip_dead_final_eval is ignored: the final evaluation is live
    g = _host(engine, cfg, fx, seed, use_graph=True, skip_dead_final_eval=True).numpy()
    np.testing.assert_array_equal(g, f.numpy())


def test_loop_refuses_what_it_cannot_run_before_any_launch(engine, tiny, fx):
    import ctypes as C
    from diffpir_amd import _lib
    e = engine
    cfg, _ = _cfg(fx, "repaint_q10")
    dt, rows, arr = restore._ancestral_rows(cfg)
    y, m = e.to_device(fx["y"]), e.to_device(fx["mask"], np.uint8)
    out = e.empty((2, 3, 64, 64))
    d, _ = restore._loop_desc(cfg, 2, 64, 64, 1, restore.start_coefficients(cfg, dt), y, None, m)
    call = lambda n=len(rows), ps=None: e.lib.dpir_run_ancestral_loop(e.h, C.byref(d), arr, n, ps, out.ptr, None)        # noqa: E731
    assert call() == 0
    e.sync()
    assert call(n=0) == -1
    assert call(n=len(rows) - 1) == -1                      # mix_next must be 0 on the last row only
    d.generate_mode = 0
    assert call() == -1 and b":417" in e.lib.dpir_last_error(e.h)
    d.generate_mode = 1
    d.task = 0
    assert call() == -1
    d.task = 2
    assert call(ps=y.ptr) == -1                             # host sampler noise without noise_init_dev / noise_rp_dev
    # an armed table of the wrong length
    pd = _lib.ProgressDesc()
    tab = (C.c_int32 * 3)(0, -1, -1)
    strip = e.empty((2, 3, 64, 64))
    pd.panel_of_step_host, pd.n_entries, pd.n_panels, pd.strip_f32 = tab, 3, 1, strip.ptr
    e._check(e.lib.dpir_set_progress(e.h, C.byref(pd)))
    assert call() == -1
    assert call() == 0                                      # the arming lasted for one call
    e.sync()
