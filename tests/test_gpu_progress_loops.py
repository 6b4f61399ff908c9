"""-m gpu: the progressive strip out of the four whole-loop entries (dpir_set_progress) against restore_batch_stepwise's numpy panels, bit for
bit; the last panel against the call's own output; arming leaves the result and the graph cache alone and lasts for one call; and the two
cases of tests/golden/progress*.npz (the standalone inpainting program's own progress_img) at the per-panel bound of tests/progress_ref.py."""
import ctypes as C

import numpy as np
import pytest

import diffpir_amd
from diffpir_amd import _lib, restore, script_util
from diffpir_amd.engine import EngineError
from oracle import unet_oracle as uo
from tests import inpaint_resample_ref as ref, progress_ref as pr
from tests.gpu_common import make_model, seeded_noise_fn_np

pytestmark = pytest.mark.gpu
FIELDS = ("strip_f32", "strip_u8", "masked_f32", "masked_u8", "minmax")

# dpir_run_loop (default driver; 12 NFE quad: 12 panels, one per step)
RUN_LOOP = {
    "deblur": dict(task="deblur", iter_num=12, lambda_=7.0, zeta=0.3),
    "sr_blur": dict(task="sr", iter_num=12, lambda_=6.0, zeta=0.25, sf=4),
    "sr_cubic": dict(task="sr", iter_num=12, lambda_=6.0, zeta=0.25, sf=4, sr_mode="cubic", inIter=2, gamma=0.5),
    "inpaint_repaint": dict(task="inpaint", iter_num=12, noise_level_img=0.0, lambda_=1.0, zeta=1.0, generate_mode="repaint"),
}
# dpir_run_inpaint_loop (driver main_ddpir_inpainting; 12 NFE: 12 row groups)
INPAINT_LOOP = {
    "DiffPIR_u2": dict(generate_mode="DiffPIR", iter_num_U=2),
    "repaint_u2": dict(generate_mode="repaint", iter_num_U=2),
    "vanilla": dict(generate_mode="vanilla", iter_num_U=1),
}


@pytest.fixture(scope="module")
def eng():
    e = diffpir_amd.Engine(0)
    model, sd = make_model(e, uo.tiny_hp())
    yield e, model, sd
    e.close()


@pytest.fixture(scope="module")
def grad_eng():
    e = diffpir_amd.Engine(0)
    e.set_precision("f16x3")
    e.enable_grad()
    model, sd = make_model(e, uo.tiny_hp())
    yield e, model, sd
    e.close()


@pytest.fixture(scope="module")
def diffusion():
    return script_util.create_gaussian_diffusion(steps=1000, learn_sigma=True)


def _inputs(golden, name):
    g, ops = golden("loops"), golden("operators")
    if name == "deblur":
        return g["deblur_y"], g["deblur_k"], None
    if name.startswith("inpaint"):
        return g["inpaint_y"], None, g["inpaint_mask"]
    return g["sr_y"], np.stack([ops["k_bic4"], ops["k_bic4"]])[:, None].astype(np.float32), None


def _same(a: restore.Progress, b: restore.Progress, label):
    assert a.panels == b.panels, label
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (label, f)
        if x is not None:
            assert x.shape == y.shape and x.dtype == y.dtype, (label, f, x.shape, y.shape)
            assert x.tobytes() == y.tobytes(), f"{label}: {f} differs at {np.argwhere(x != y)[:4].tolist()}"


def _pair(e, model, diffusion, cfg, y, k, mask, seed, graph, masked):
    """(monolithic Progress, stepwise Progress, monolithic x_0, stepwise x_0)"""
    dev = lambda a, dt=np.float32: None if a is None else e.to_device(a, dt)        # noqa: E731
    pm, ps = restore.Progress(masked=masked), restore.Progress(masked=masked)
    mono = restore.restore_batch(e, cfg, y, k=k, mask=mask, noise_source="host", noise_fn=seeded_noise_fn_np(seed), use_graph=graph, progress=pm).numpy()
    step = restore.restore_batch_stepwise(model, diffusion, cfg, dev(y), k=dev(k), mask=dev(mask, np.uint8), noise_fn=seeded_noise_fn_np(seed),
                                          progress=ps).numpy()
    return pm, ps, mono, step


@pytest.mark.parametrize("name", list(RUN_LOOP))
@pytest.mark.parametrize("graph", [False, True])
def test_run_loop_strip_equals_the_stepwise_strip(eng, diffusion, golden, name, graph):
    e, model, _ = eng
    y, k, mask = _inputs(golden, name)
    cfg = restore.LoopConfig(**RUN_LOOP[name])
    pm, ps, mono, step = _pair(e, model, diffusion, cfg, y, k, mask, 31, graph, masked=mask is not None)
    W = mono.shape[3]                                      # 32; 64 for the x4 super-resolution cases
    assert len(pm.panels) == 12 and pm.strip_f32.shape == (2, 3, W, 12 * W) and pm.strip_u8.shape == (2, W, 12 * W, 3)
    _same(pm, ps, f"{name} graph={graph}")
    assert pm.strip_f32[..., -W:].tobytes() == mono.tobytes()


@pytest.mark.parametrize("name", list(INPAINT_LOOP))
@pytest.mark.parametrize("graph", [False, True])
def test_inpaint_loop_strip_equals_the_stepwise_strip(eng, diffusion, golden, name, graph):
    e, model, _ = eng
    g = golden("progress")
    cfg = restore.LoopConfig(task="inpaint", driver="main_ddpir_inpainting", iter_num=12, noise_level_img=float(g["noise_level_img"]), lambda_=1.0,
                             zeta=0.6, eta=0.3, **INPAINT_LOOP[name])
    pm, ps, mono, step = _pair(e, model, diffusion, cfg, g["y"], None, g["mask"], 32, graph, masked=True)
    assert len(pm.panels) == 12
    _same(pm, ps, f"{name} graph={graph}")
    assert mono.tobytes() == step.tobytes()
    assert pm.strip_f32[..., -64:].tobytes() == mono.tobytes()


def test_dps_loop_strip_equals_the_stepwise_strip(grad_eng, diffusion, golden):
    e, model, _ = grad_eng
    y = golden("dps")["dps_y"]
    cfg = restore.LoopConfig(task="sr", iter_num=10, lambda_=6.0, zeta=0.25, sf=4, sr_mode="cubic", generate_mode="DPS_y0")
    pm, ps, mono, step = _pair(e, model, diffusion, cfg, y, None, None, 33, False, masked=False)
    assert len(pm.panels) == 10
    _same(pm, ps, "DPS_y0")
    assert mono.tobytes() == step.tobytes() and pm.strip_f32[..., -mono.shape[3]:].tobytes() == mono.tobytes()


def test_deblur_grad_loop_strip_equals_the_stepwise_strip(grad_eng, diffusion, golden):
    e, model, _ = grad_eng
    g = golden("loops")
    ax = np.arange(9) - 4                                               # two 9 x 9 Gaussian PSFs (the reflect-padded operator needs K / 2 < H)
    k = np.stack([np.exp(-(ax[:, None] ** 2 + (st * ax[None, :]) ** 2) / (2 * sd * sd)) for sd, st in ((1.6, 1.0), (2.4, 0.5))])
    k = (k / k.sum(axis=(1, 2), keepdims=True))[:, None].astype(np.float32)
    cfg = restore.LoopConfig(driver="main_ddpir_deblur", task="deblur", iter_num=10, lambda_=6.0, zeta=0.25, generate_mode="DPS_yt")
    pm, ps, mono, step = _pair(e, model, diffusion, cfg, g["deblur_y"], k, None, 34, False, masked=False)
    assert len(pm.panels) == 10
    _same(pm, ps, "deblur DPS_yt")
    assert mono.tobytes() == step.tobytes() and pm.strip_f32[..., -32:].tobytes() == mono.tobytes()


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("loop", ["run_loop", "inpaint_loop"])
def test_last_panel_is_the_calls_own_output(eng, golden, loop, skip):
    e, _, _ = eng
    g = golden("loops")
    if loop == "run_loop":
        cfg = restore.LoopConfig(task="inpaint", iter_num=12, noise_level_img=0.0, lambda_=1.0, zeta=1.0)
    else:
        cfg = restore.LoopConfig(task="inpaint", driver="main_ddpir_inpainting", iter_num=12, noise_level_img=0.0, lambda_=1.0, zeta=1.0, iter_num_U=2,
                                 generate_mode="repaint")
    pg = restore.Progress()
    f, u = restore.restore_batch(e, cfg, g["inpaint_y"], mask=g["inpaint_mask"], noise_source="host", noise_fn=seeded_noise_fn_np(35), use_graph=True,
                                 skip_dead_final_eval=skip, return_u8=True, progress=pg)
    W = f.shape[3]
    assert pg.strip_f32[..., -W:].tobytes() == f.numpy().tobytes()
    assert pg.strip_u8[:, :, -W:, :].tobytes() == u.numpy().tobytes()
    assert pg.panels[-1] == (999, 0)


@pytest.mark.parametrize("loop", ["run_loop", "inpaint_loop"])
def test_arming_leaves_the_result_and_the_graph_cache_alone(golden, loop):
    g = golden("loops")
    if loop == "run_loop":
        cfg, kw = restore.LoopConfig(task="deblur", iter_num=12, lambda_=7.0, zeta=0.3), dict(k=g["deblur_k"])
        y = g["deblur_y"]
    else:
        cfg = restore.LoopConfig(task="inpaint", driver="main_ddpir_inpainting", iter_num=12, noise_level_img=0.0, lambda_=1.0, zeta=1.0, iter_num_U=2,
                                 generate_mode="repaint")
        y, kw = g["inpaint_y"], dict(mask=g["inpaint_mask"])
    sizes, outs = [], []
    for order in (("plain", "armed"), ("armed", "plain")):          # on a fresh engine each: also the FIRST (capturing) call may be the armed one
        e = diffpir_amd.Engine(0)
        try:
            make_model(e, uo.tiny_hp())
            for what in order:
                pg = restore.Progress(masked=loop == "inpaint_loop") if what == "armed" else None
                outs.append(restore.restore_batch(e, cfg, y, noise_source="device", seed=5, use_graph=True, progress=pg, **kw).numpy())
                sizes.append(e.graph_cache_size())
        finally:
            e.close()
    assert all(o.tobytes() == outs[0].tobytes() for o in outs)
    assert sizes[0] == sizes[1] == sizes[2] == sizes[3] and sizes[0] >= 1, sizes


def test_arming_is_one_shot_and_mismatches_are_refused(eng, golden):
    e, _, _ = eng
    g = golden("loops")
    cfg = restore.LoopConfig(task="inpaint", iter_num=12, noise_level_img=0.0, lambda_=1.0, zeta=1.0)
    _, steps, arr = restore._steps(cfg)
    table, panels = restore.progress_table(cfg, steps)
    P = len(panels)
    sent = np.full((2, 3, 32, P * 32), np.float32(-7.25), np.float32)
    strip = e.to_device(sent)

    def arm(tab, masked=None):
        d = _lib.ProgressDesc()
        t = (C.c_int32 * len(tab))(*tab)
        d.panel_of_step_host, d.n_entries, d.n_panels, d.strip_f32 = t, len(tab), P, strip.ptr
        if masked is not None:
            d.masked_f32 = masked.ptr
        return e.lib.dpir_set_progress(e.h, C.byref(d))

    run = lambda c=cfg, **kw: restore.restore_batch(e, c, g["inpaint_y"], mask=g["inpaint_mask"], noise_source="device", seed=1, **kw)      # noqa: E731
    # a table of the wrong length: refused before anything is launched, and the arming is gone afterwards
    e._check(arm(table[:-1]))
    with pytest.raises(EngineError, match="armed 11 entries for a loop of 12"):
        run()
    run()
    e.sync()
    assert strip.numpy().tobytes() == sent.tobytes()
    # armed once: the first call fills the strip, a second call without re-arming leaves a sentinel-filled strip untouched
    e._check(arm(table))
    first = run().numpy()
    got = strip.numpy()
    assert got[..., -32:].tobytes() == first.tobytes() and not (got == np.float32(-7.25)).any()
    strip.copy_from(sent)
    run()
    e.sync()
    assert strip.numpy().tobytes() == sent.tobytes()
    # NULL disarms; entries outside [-1, n_panels) are refused; a masked strip needs a loop with a mask
    e._check(arm(table))
    e._check(e.lib.dpir_set_progress(e.h, None))
    run()
    e.sync()
    assert strip.numpy().tobytes() == sent.tobytes()
    assert arm([P] + table[1:]) == -1 and arm([-2] + table[1:]) == -1
    dcfg = restore.LoopConfig(task="deblur", iter_num=12, lambda_=7.0, zeta=0.3)
    e._check(arm(table, masked=strip))
    with pytest.raises(EngineError, match="masked progress strip needs the mask"):
        restore.restore_batch(e, dcfg, g["deblur_y"], k=g["deblur_k"], noise_source="device", seed=1)
    with pytest.raises(ValueError, match="needs a mask"):
        restore.restore_batch(e, dcfg, g["deblur_y"], k=g["deblur_k"], noise_source="device", seed=1, progress=restore.Progress(masked=True))
    e.sync()
    assert strip.numpy().tobytes() == sent.tobytes()


@pytest.mark.parametrize("name", pr.CASES)
@pytest.mark.parametrize("graph", [False, True])
def test_strip_matches_the_standalone_programs_progress_img(eng, golden, name, graph):
    """Per panel max|engine - program| <= 2e-3 max(1, max|panel of the program|) (tests/progress_ref.py BOUND).  Measured maxima:
    profiles/progress/README.md."""
    e, _, _ = eng
    g = pr.load(golden)
    c = pr.case_config(g, name)
    cfg = ref.loop_config(c)
    pg = restore.Progress(masked=True)
    restore.restore_batch(e, cfg, g["y"], mask=g["mask"], noise_source="host", noise_fn=seeded_noise_fn_np(c["seed"]), use_graph=graph, progress=pg)
    assert pg.panels == list(zip(g[name + ".panel_seq"].tolist(), g[name + ".panel_t"].tolist()))
    want = pr.fixture_strip(g, name)
    errs = pr.per_panel_errors(pg.strip_f32, want, len(pg.panels))
    print(f"{name} graph={graph}: per panel max|engine - program| " + " ".join(f"{a:.2e}" for a, _ in errs))
    assert all(a <= b for a, b in errs), errs
    # the masked strip against the program's own blend of ITS panels (main_ddpir_inpainting.py:361-366), same bound
    m = np.tile(g["mask"].astype(np.float32), (1, 1, 1, len(pg.panels)))
    yt = np.tile(g["y"], (1, 1, 1, len(pg.panels)))
    merr = pr.per_panel_errors(pg.masked_f32, yt * m + (np.float32(1) - m) * want, len(pg.panels))
    assert all(a <= b for a, b in merr), merr
    v = pg.strip_f32.reshape(2, 3, 64, len(pg.panels), 64)
    assert pg.minmax[:, :, 0].tobytes() == v.max(axis=(1, 2, 4)).T.copy().tobytes() and pg.minmax[:, :, 1].tobytes() == v.min(axis=(1, 2, 4)).T.copy().tobytes()
