"""-m gpu: per-image (lambda, zeta, noise level) and per-image noise keys in one batch (dpir_run_loop_per_image, restore.PerImage, the YAML key
engine_batch_sweeps).

The yardstick is the existing uniform path, which the rest of the suite pins to the reference and to float64: a per-image row performs the same
float32 operations in the same order as a uniform call at that row's values, so every comparison is np.testing.assert_array_equal unless it says
otherwise.  The shapes are the smallest that reach each kernel family (CASES); all run on the tiny topology (tests/gpu_common.make_model(engine,
uo.tiny_hp())), also at 256 x 256 and 512 x 512."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

from diffpir_amd import restore, synth
from oracle import unet_oracle as uo
from tests.gpu_common import make_model, seeded_noise_fn_np

pytestmark = pytest.mark.gpu

# three rows that differ in all three fields; row 1 has zeta = 0 (k2 = 0: no fresh noise).  B = 2 cases take the first two.
LAM, ZET, NL = [7.0, 3.5, 11.0], [0.3, 0.0, 0.6], [12.75 / 255, 5.0 / 255, 20.0 / 255]
IDX = [41, 7, 2 ** 33 + 5]          # global image numbers: not consecutive, not ascending, one beyond 2^32
SEED = 11

DEBLUR, SR, INP = dict(task="deblur"), dict(task="sr", sf=4), dict(task="inpaint")
# name -> (synthetic case, B, H, LoopConfig keywords): what each one reaches is in its comment
CASES = {
    "deblur32": ("deblur", 3, 32, dict(DEBLUR, iter_num=4)),                              # fft.hip, unfused step
    "deblur64": ("deblur", 3, 64, dict(DEBLUR, iter_num=4)),                              # fft2, fused step
    "deblur64_g09": ("deblur", 3, 64, dict(DEBLUR, iter_num=4, guidance_scale=0.9)),      # fft2, unfused data_solution
    "deblur256": ("deblur", 3, 256, dict(DEBLUR, iter_num=3)),                            # fft4, fused
    "deblur256_g09": ("deblur", 3, 256, dict(DEBLUR, iter_num=3, guidance_scale=0.9)),    # fft4, unfused
    "sr256": ("sr", 3, 256, dict(SR, iter_num=3)),                                        # fft4 alias fold
    "sr64": ("sr", 2, 64, dict(SR, iter_num=4)),                                          # fft2 alias fold
    "deblur512": ("deblur", 2, 512, dict(DEBLUR, iter_num=3)),                            # the 512-point instantiation
    "deblur64_eta": ("deblur", 2, 64, dict(DEBLUR, iter_num=4, eta=0.7)),                 # the eta draw
    "inpaint32": ("inpaint", 3, 32, dict(INP, iter_num=4)),                               # prox_mask
    "repaint32": ("inpaint", 2, 32, dict(INP, iter_num=4, generate_mode="repaint")),      # the repaint stream
    "cubic64": ("sr", 2, 64, dict(SR, iter_num=4, sr_mode="cubic", inIter=2, gamma=0.5)),  # IBP
}


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    make_model(e, uo.tiny_hp())
    yield e
    e.close()


_DATA, _RUNS = {}, {}


def _data(name):
    if name not in _DATA:
        task, B, H, kw = CASES[name]
        _DATA[name] = synth.make_case(task, B, H, H, seed=23, sf=kw.get("sf", 1), ksize=9)
    return _DATA[name]


def _run(engine, name, graph, per_image, over=None, noise="device", progress=None, data=None, **extra):
    d = data or _data(name)
    cfg = restore.LoopConfig(**dict(CASES[name][3], **(over or {})))
    if noise == "host":
        extra = dict(extra, noise_source="host", noise_fn=seeded_noise_fn_np(5))
    return restore.restore_batch(engine, cfg, d["y"], k=d["k"], mask=d["mask"], seed=SEED, use_graph=graph, per_image=per_image,
                                 progress=progress, **extra).numpy()


def _full(B):
    return restore.PerImage(lambda_=LAM[:B], zeta=ZET[:B], noise_level_img=NL[:B], image_index=IDX[:B])


def _row_values(j):
    return dict(lambda_=LAM[j], zeta=ZET[j], noise_level_img=NL[j])


def _pair(engine, name, graph, noise="device"):
    """(the per-image batch, [comparator of row j: the same rows under LoopConfig uniform at row j's values, the same noise keys]), computed once"""
    key = (name, graph, noise)
    if key not in _RUNS:
        B = CASES[name][1]
        full = _run(engine, name, graph, _full(B), noise=noise)
        refs = [_run(engine, name, graph, restore.PerImage(image_index=IDX[:B]), over=_row_values(j), noise=noise) for j in range(B)]
        _RUNS[key] = (full, refs)
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------- (a) dpir_randn_indexed
@pytest.mark.parametrize("stream", [0, 2 ** 32 + 3])
def test_randn_indexed_rows_equal_randn_at_that_offset(engine, stream):
    idx = np.array([7, 7, 2 ** 33 + 1], np.int64)
    out, one = engine.empty((3, 3, 16, 16)), engine.empty((1, 3, 16, 16))
    engine._check(engine.lib.dpir_randn_indexed(engine.h, out.ptr, 1234, stream, idx.ctypes.data_as(C.POINTER(C.c_int64)), 3, 3, 16, 16))
    rows = out.numpy()
    for b in range(3):
        engine._check(engine.lib.dpir_randn(engine.h, one.ptr, 1234, stream, int(idx[b]), 1, 3, 16, 16))
        np.testing.assert_array_equal(rows[b], one.numpy()[0])
    np.testing.assert_array_equal(rows[0], rows[1])
    assert np.abs(rows[0] - rows[2]).max() > 0.1 and np.isfinite(rows).all()


# ---------------------------------------------------------------------------------------------- (b) the loop, per-image parameters
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(CASES))
def test_row_equals_the_uniform_call_at_its_own_values(engine, name, graph):
    full, refs = _pair(engine, name, graph)
    assert np.isfinite(full).all()
    for j, ref in enumerate(refs):
        np.testing.assert_array_equal(full[j], ref[j], err_msg=f"{name} graph={graph}: row {j}")
    # the parameters do reach the result: row 1 under row 0's values is another image
    assert np.abs(refs[0][1] - refs[1][1]).max() > 1e-4


# ---------------------------------------------------------------------------------------------- (c) index semantics
@pytest.mark.parametrize("name", ["deblur64", "inpaint32"])
def test_image_index_semantics(engine, name):
    B, o = CASES[name][1], 100
    plain = _run(engine, name, True, None, image_offset=o)
    np.testing.assert_array_equal(_run(engine, name, True, restore.PerImage(image_index=o + np.arange(B))), plain)
    d = _data(name)
    twice = {f: None if d[f] is None else np.ascontiguousarray(np.repeat(d[f][:1], 2, axis=0)) for f in ("y", "k", "mask")}
    two = _run(engine, name, True, restore.PerImage(lambda_=[5.0, 5.0], zeta=[0.2, 0.2], image_index=[o, o]), data=twice)
    np.testing.assert_array_equal(two[0], two[1])
    np.testing.assert_array_equal(two[0], _run(engine, name, True, None, over=dict(lambda_=5.0, zeta=0.2), data=twice, image_offset=o)[0])


# ---------------------------------------------------------------------------------------------- (d) host noise: the table alone
@pytest.mark.parametrize("name", ["deblur32", "deblur64"])
def test_host_noise_rows(engine, name):
    full, refs = _pair(engine, name, False, noise="host")
    for j, ref in enumerate(refs):
        np.testing.assert_array_equal(full[j], ref[j], err_msg=f"{name} host noise: row {j}")
    assert np.abs(refs[0][1] - refs[1][1]).max() > 1e-4


# ---------------------------------------------------------------------------------------------- (e) graph cache
def test_uniform_and_per_image_steps_never_share_a_captured_graph():
    """On an engine of its own (the cache is capped and least-recently-used; the module's engine has filled it)."""
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    try:
        make_model(e, uo.tiny_hp())
        size = lambda: e.lib.dpir_graph_cache_size(e.h)
        name, B = "deblur64", CASES["deblur64"][1]
        n0 = size()
        u1 = _run(e, name, True, None)
        n1 = size()
        p = _run(e, name, True, _full(B))
        n2 = size()
        u3 = _run(e, name, True, None)
        n3 = size()
        np.testing.assert_array_equal(u1, u3)
        for j in range(B):
            ref = _run(e, name, False, restore.PerImage(image_index=IDX[:B]), over=_row_values(j))
            np.testing.assert_array_equal(p[j], ref[j])
        assert n0 == 0 and n1 > n0, (n0, n1)
        assert n2 - n1 == n1 - n0 and n3 == n2, f"cache sizes {n0} -> {n1} (uniform) -> {n2} (per-image) -> {n3} (uniform again)"
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- (f) progress
def test_progress_strip_rows(engine):
    name, B = "deblur64", CASES["deblur64"][1]
    pg = restore.Progress()
    _run(engine, name, True, _full(B), progress=pg)
    assert pg.strip_u8.shape[0] == B and len(pg.panels) >= 1
    for j in range(B):
        pj = restore.Progress()
        _run(engine, name, True, restore.PerImage(image_index=IDX[:B]), over=_row_values(j), progress=pj)
        np.testing.assert_array_equal(pg.strip_u8[j], pj.strip_u8[j])
        np.testing.assert_array_equal(pg.strip_f32[j], pj.strip_f32[j])


# ---------------------------------------------------------------------------------------------- (g) the YAML driver
_DRIVE = {}


def _drive(tmp_path, batch_sweeps, batch_size):
    """The x4 super-resolution sweep (its first three points) on two synthetic images, 3 NFE, device noise -> the driver's result list."""
    import yaml
    from diffpir_amd import main_ddpir as drv
    key = (batch_sweeps, batch_size)
    if key not in _DRIVE:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        cfg = yaml.safe_load(open(os.path.join(root, "configs", "sweep_batch_example.yaml")))
        cfg.update(iter_num=3, engine_noise="device", engine_batch_sweeps=batch_sweeps, batch_size=batch_size)
        assert cfg["task"] == "sr" and cfg["sf"] == 4
        p = tmp_path / f"c_{int(batch_sweeps)}_{batch_size}.yaml"
        p.write_text(yaml.safe_dump(cfg))
        _DRIVE[key] = drv.main(["--opt", str(p), "--synthetic", "2", "--max-sweeps", "3"])
    return _DRIVE[key]


def test_driver_uniform_batches_equal_the_sequential_run_exactly(tmp_path):
    seq = _drive(tmp_path, False, 2)
    flat = _drive(tmp_path, True, 2)            # every batch is one point's two images: B = 2, uniform inside
    assert len(seq) == 3 and all(np.isfinite(seq))
    assert flat == seq, (flat, seq)


def test_driver_mixed_batches_within_the_parity_bar(tmp_path):
    seq = _drive(tmp_path, False, 2)
    flat = _drive(tmp_path, True, 3)            # (0,0) (0,1) (1,0) | (1,1) (2,0) (2,1): points mix inside a batch, B = 3
    print("sequential", seq, "flattened at batch_size 3", flat)
    assert len(flat) == len(seq)
    # the project's parity bar (README): 1e-3 dB on the average PSNR.  A change of B moves an output by less than 1e-4
    # (tests/test_gpu_loop.py, shard invariance), far inside it.
    assert max(abs(a - b) for a, b in zip(flat, seq)) <= 1e-3


# ---------------------------------------------------------------------------------------------- (h) sharding
def test_restore_sharded_world_1_equals_restore_batch(engine):
    from diffpir_amd import dist as ddist
    name, B = "deblur64", CASES["deblur64"][1]
    d = _data(name)
    full, _ = _pair(engine, name, True)
    cfg = restore.LoopConfig(**CASES[name][3])
    u8, f32 = ddist.restore_sharded(engine, cfg, d["y"], k=d["k"], rank=0, world=1, seed=SEED, use_graph=True, per_image=_full(B))
    np.testing.assert_array_equal(f32.numpy(), full)
    assert u8.shape == (B, 64, 64, 3)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, collective, ret):
    """One rank of a sharded per-image batch (B = 3: a ragged split), in the style of tests/test_gpu_dist.py."""
    two_devices = collective == "rccl"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank if two_devices else 0), HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.environ.pop("DIFFPIR_COLLECTIVE", None)
    import diffpir_amd
    from diffpir_amd import dist as ddist
    r, lr, w = ddist.init(collective)
    eng = diffpir_amd.Engine(lr)
    ddist.attach(eng)
    make_model(eng, uo.tiny_hp())
    d = synth.make_case("deblur", 3, 32, 32, seed=31, ksize=9)
    cfg = restore.LoopConfig(task="deblur", iter_num=4)
    u8, _ = ddist.restore_sharded(eng, cfg, d["y"], k=d["k"], rank=r, world=w, seed=9, use_graph=True, per_image=_full(3))
    ret[rank] = u8.numpy().tobytes()
    ddist.shutdown()
    eng.close()


def _two_ranks_equal_one(collective):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    one, two = mgr.dict(), mgr.dict()
    mp.spawn(_rank, args=(1, _free_port(), collective, one), nprocs=1, join=True)
    mp.spawn(_rank, args=(2, _free_port(), collective, two), nprocs=2, join=True)
    assert len(one[0]) == 3 * 32 * 32 * 3
    assert two[0] == one[0] and two[1] == one[0]


def test_two_ranks_on_one_gpu_slice_the_per_image_arrays():
    _two_ranks_equal_one("gloo")


def test_rccl_two_ranks_two_devices_slice_the_per_image_arrays():
    from diffpir_amd.engine import device_count
    n = device_count()
    if n < 2:
        pytest.skip(f"RCCL with two ranks needs two GPUs: dpir_device_count() = {n} on this box")
    _two_ranks_equal_one("rccl")
