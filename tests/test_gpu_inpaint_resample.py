"""-m gpu: driver='main_ddpir_inpainting' (dpir_run_inpaint_loop: resampling, iter_num_U >= 1) against x_0 of the standalone program
(tests/golden/inpaint_resample.npz), against the unfused stepwise loop, and its invariances: graph replay, device noise, sharding, the dead
final evaluations, and U = 1 against dpir_run_loop."""
import numpy as np
import pytest
import torch

from diffpir_amd import restore, script_util
from oracle import unet_oracle as uo, diffpir_oracle as do
from tests import inpaint_resample_ref as ref
from tests.gpu_common import make_model, seeded_noise_fn_np

pytestmark = pytest.mark.gpu
CASES = ["diffpir_u1", "diffpir_u2_eta", "diffpir_u3", "repaint_u2", "vanilla_u2"]


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
def fx(golden):
    return golden("inpaint_resample")


def _cfg(fx, name, **over):
    c = ref.case_config(fx, name)
    cfg = ref.loop_config(c)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg, c["seed"]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("graph", [False, True])
def test_loop_matches_the_standalone_programs_x0(engine, tiny, fx, name, graph):
    """The bounds tests/test_gpu_loop.py holds the default driver's inpainting loops to."""
    cfg, seed = _cfg(fx, name)
    out = restore.restore_batch(engine, cfg, fx["y"], mask=fx["mask"], noise_source="host", noise_fn=seeded_noise_fn_np(seed), use_graph=graph).numpy()
    want, gt = fx[name + ".x0"], fx["gt"]
    err = float(np.abs(out - want).max())
    dpsnr = abs(restore.psnr_batch(out * 2 - 1, gt * 2 - 1) - restore.psnr_batch(want * 2 - 1, gt * 2 - 1))
    print(f"{name} graph={graph}: max|engine - program| {err:.3e}, |dPSNR| {dpsnr:.2e} dB")
    assert err < 2e-3
    assert dpsnr < 1e-3


@pytest.mark.parametrize("name", ["diffpir_u1", "diffpir_u3", "repaint_u2"])
def test_fused_loop_equals_the_stepwise_loop_bitwise(engine, tiny, fx, name):
    model, _ = tiny
    diffusion = script_util.create_gaussian_diffusion(steps=1000, learn_sigma=True)
    for U in ((1, 3) if name == "repaint_u2" else (None,)):
        cfg, seed = _cfg(fx, name, **({} if U is None else {"iter_num_U": U}))
        fused = restore.restore_batch(engine, cfg, fx["y"], mask=fx["mask"], noise_source="host", noise_fn=seeded_noise_fn_np(seed)).numpy()
        sw = restore.restore_batch_stepwise(model, diffusion, cfg, engine.to_device(fx["y"]), mask=engine.to_device(fx["mask"], np.uint8),
                                            noise_fn=seeded_noise_fn_np(seed)).numpy()
        np.testing.assert_array_equal(fused, sw)


def test_graph_replay_twice_is_bitwise_identical(engine, tiny, fx):
    cfg, seed = _cfg(fx, "diffpir_u3")
    run = lambda g: restore.restore_batch(engine, cfg, fx["y"], mask=fx["mask"], noise_source="host", noise_fn=seeded_noise_fn_np(seed),     # noqa: E731
                                          use_graph=g).numpy()
    a, b, c = run(True), run(True), run(False)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("name", ["diffpir_u2_eta", "repaint_u2"])
def test_device_noise_loop_equals_host_noise_loop_fed_the_numpy_philox_draws(engine, tiny, fx, name):
    """Streams: 0 init; 1 + 4s eta, 2 + 4s zeta, 3 + 4s repaint, 2^32 + s set-back for sub-step ordinal s; image = image_offset + n."""
    from oracle import philox_oracle as po
    cfg, _ = _cfg(fx, name)
    _, rows, _ = restore._inpaint_rows(cfg)
    B, H, W, seed, off = 2, 64, 64, 4242, 3
    dev = restore.restore_batch(engine, cfg, fx["y"], mask=fx["mask"], noise_source="device", seed=seed, image_offset=off, use_graph=True).numpy()
    dr = lambda stream: po.randn(seed, stream, off, B, 3 * H * W).reshape(B, 3, H, W)       # noqa: E731
    n = len(rows)
    pre = dict(init=dr(0), n1=np.stack([dr(1 + 4 * s) for s in range(n)]) if cfg.eta != 0 else None, n2=np.stack([dr(2 + 4 * s) for s in range(n)]),
               back=np.stack([dr(2 ** 32 + s) for s in range(n)]), rp=np.stack([dr(3 + 4 * s) for s in range(n)]) if cfg.generate_mode == "repaint" else None)
    host = restore.restore_batch(engine, cfg, fx["y"], mask=fx["mask"], noise_source="host", predrawn=pre).numpy()
    err = float(np.abs(dev - host).max())
    print(f"{name}: device-Philox loop vs host-noise loop fed the numpy Philox draws: max|diff| {err:.3e}")
    assert err < 1.3e-5


@pytest.mark.parametrize("name", ["diffpir_u3", "repaint_u2"])
def test_sharding_invariance_bitwise(engine, tiny, fx, name):
    cfg, _ = _cfg(fx, name)
    both = restore.restore_batch(engine, cfg, fx["y"], mask=fx["mask"], noise_source="device", seed=7, image_offset=10).numpy()
    for n in range(2):
        one = restore.restore_batch(engine, cfg, fx["y"][n:n + 1], mask=fx["mask"][n:n + 1], noise_source="device", seed=7, image_offset=10 + n).numpy()
        np.testing.assert_array_equal(one[0], both[n])


@pytest.mark.parametrize("name", ["diffpir_u3", "repaint_u2"])
@pytest.mark.parametrize("graph", [False, True])
def test_skip_dead_final_eval_and_u8_output(engine, tiny, fx, name, graph):
    cfg, seed = _cfg(fx, name)
    kw = dict(mask=fx["mask"], noise_source="host", use_graph=graph)
    f, u = restore.restore_batch(engine, cfg, fx["y"], noise_fn=seeded_noise_fn_np(seed), return_u8=True, **kw)
    np.testing.assert_array_equal(u.numpy(), do.tensor2uint_batch(torch.from_numpy(f.numpy())))
    g = restore.restore_batch(engine, cfg, fx["y"], noise_fn=seeded_noise_fn_np(seed), skip_dead_final_eval=True, **kw).numpy()
    np.testing.assert_array_equal(g, f.numpy())


@pytest.mark.parametrize("mode", ["DiffPIR", "vanilla"])
def test_u1_with_forced_start_equals_dpir_run_loop_bitwise(engine, tiny, fx, mode):
    """With iter_num_U = 1 this driver differs from the default one through the start coefficients only: with sa_start / s1m_start forced to the
    default driver's pair, dpir_run_inpaint_loop equals dpir_run_loop bit for bit (host noise; batch-shaped draws fed to both)."""
    kw = dict(task="inpaint", iter_num=10, noise_level_img=float(fx["noise_level_img"]), lambda_=1.0, zeta=0.4, eta=0.3, generate_mode=mode)
    base = restore.LoopConfig(**kw)
    new = restore.LoopConfig(driver="main_ddpir_inpainting", **kw)
    dt, steps, _ = restore._steps(base)
    _, rows, _ = restore._inpaint_rows(new)
    assert [s["t"] for s in steps] == [r["t"] for r in rows]
    rng = np.random.default_rng(3)
    sh = (len(rows), 2, 3, 64, 64)
    init, n1, n2 = (rng.standard_normal(s).astype(np.float32) for s in (sh[1:], sh, sh))
    nl = sum(1 for s in steps if not s["last"])
    a = restore.restore_batch(engine, base, fx["y"], mask=fx["mask"], noise_source="host", predrawn=(init, n1[:nl], n2[:nl])).numpy()
    b = restore._restore_inpaint_resample(engine, new, fx["y"], fx["mask"], None, "host", None, 0, 0, False, False, None, None, False, None,
                                          dict(init=init, n1=n1, n2=n2, back=None, rp=None), _start=restore.start_coefficients(base, dt)).numpy()
    np.testing.assert_array_equal(a, b)
