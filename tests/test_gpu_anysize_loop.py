"""-m gpu: the restoration loop at an image size that is no power of two (48 x 80, the tiny topology of stride 4, B = 2, 8 NFE), whose FFT data step
runs on the mixed-radix kernels (csrc/fft_mixed.hip): deblurring and sr-blur at sf 2 and 3 through restore_batch against the oracle pair
(tests/gpu_common.py::fft_prox_parity, nfe = 8: |dPSNR| <= 1e-3 dB flat), graph against eager and the per-image loop against the uniform one bit for
bit.  In front of them, forward-only checks of the same model at the same shapes (and one FFHQ-topology forward at 96 x 160) against
oracle.unet_forward at tests/test_gpu_unet.py's tolerance: they pass or fail independently of the prox.

tests/golden/operators_x23.npz holds the reference's x2 and x3 bicubic PSFs (kernels/kernels_bicubicx234.mat[0, 0] and [0, 1], 25 x 25 float32,
read once with scipy.io.loadmat) as k_bic2 and k_bic3."""
import os

import numpy as np
import pytest
import torch

from diffpir_amd import restore, synth
from oracle import unet_oracle as uo, diffpir_oracle as do
from tests.gpu_common import make_model, seeded_noise_fn_np, oracle_pair, fft_prox_parity, rel_err

pytestmark = pytest.mark.gpu

TOL_OUT = 2e-5          # tests/test_gpu_unet.py
H, W, B, NFE = 48, 80, 2, 8
W3 = 96                 # sf 3 needs a width divisible by 3 and by the stride


@pytest.fixture(scope="module")
def engine():
    import diffpir_amd
    e = diffpir_amd.Engine(0)          # launch mode 3, the default: the power-of-two families plus the mixed-radix kernels
    yield e
    e.close()


@pytest.fixture(scope="module")
def tiny(engine):
    return make_model(engine, uo.tiny_hp())


_CASES = {}


def _case(name):
    """name -> (LoopConfig keywords, oracle config, data)"""
    if name not in _CASES:
        if name == "deblur":
            d = synth.make_case("deblur", B, H, W, seed=31, ksize=9)
            kw = dict(task="deblur", iter_num=NFE, lambda_=7.0, zeta=0.3)
        else:
            sf = int(name[-1])
            w = W if sf == 2 else W3
            d = synth.make_case("sr", B, H, w, seed=32 + sf, sf=sf, sr_mode="cubic")        # the measurement only: the PSF is the reference's own
            ops = np.load(os.path.join(os.path.dirname(__file__), "golden", "operators_x23.npz"))
            d["k"] = np.broadcast_to(ops[f"k_bic{sf}"], (B, 1, 25, 25)).astype(np.float32).copy()
            kw = dict(task="sr", iter_num=NFE, lambda_=6.0, zeta=0.25, sf=sf)
        ocfg = do.LoopConfig(kw["task"], NFE, 12.75 / 255, kw["lambda_"], kw["zeta"], sf=kw.get("sf", 1))
        _CASES[name] = (kw, ocfg, d)
    return _CASES[name]


@pytest.mark.parametrize("h,w", [(H, W), (H, W3)])
def test_tiny_forward_at_the_loop_shapes(engine, tiny, h, w):
    _, sd = tiny
    g = torch.Generator().manual_seed(h + w)
    x, t = torch.randn(B, 3, h, w, generator=g), torch.tensor([321, 17])
    out = engine.unet_forward(engine.to_device(x.numpy()), t.numpy()).numpy()
    err = rel_err(out, uo.unet_forward(sd, uo.tiny_hp(), x, t).numpy())
    print(f"tiny forward {h}x{w}: rel err {err:.3e}")
    assert err < TOL_OUT


def test_ffhq_forward_at_96x160():
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    try:
        _, sd = make_model(e, uo.ffhq_hp())
        g = torch.Generator().manual_seed(5)
        x, t = torch.randn(1, 3, 96, 160, generator=g), torch.tensor([250])
        out = e.unet_forward(e.to_device(x.numpy()), t.numpy()).numpy()
        err = rel_err(out, uo.unet_forward(sd, uo.ffhq_hp(), x, t).numpy())
        print(f"ffhq forward 96x160: rel err {err:.3e}")
        assert err < TOL_OUT
    finally:
        e.close()


@pytest.mark.parametrize("name,seed", [("deblur", 71), ("sr2", 72), ("sr3", 73)])
def test_loop_vs_oracle(engine, tiny, name, seed):
    kw, ocfg, d = _case(name)
    _, sd = tiny
    out = restore.restore_batch(engine, restore.LoopConfig(**kw), d["y"], k=d["k"], noise_source="host", noise_fn=seeded_noise_fn_np(seed),
                                use_graph=True).numpy()
    ref, exact = oracle_pair("anysize_" + name, sd, uo.tiny_hp(), ocfg, d["y"], d["k"], seed)
    fft_prox_parity(out, ref, d["gt"], f"{name} {d['gt'].shape[2]}x{d['gt'].shape[3]}", exact=exact, nfe=NFE)


@pytest.mark.parametrize("name", ["deblur", "sr2"])
def test_graph_equals_eager_and_per_image_equals_uniform(engine, tiny, name):
    kw, _, d = _case(name)
    cfg = restore.LoopConfig(**kw)
    yd, kd = engine.to_device(d["y"]), engine.to_device(d["k"])
    run = lambda **k: restore.restore_batch(engine, cfg, yd, k=kd, noise_source="device", seed=7, **k).numpy()
    graph, eager = run(use_graph=True), run(use_graph=False)
    assert np.isfinite(graph).all()
    np.testing.assert_array_equal(graph, eager)
    rows = restore.PerImage(lambda_=[kw["lambda_"]] * B, zeta=[kw["zeta"]] * B, noise_level_img=[cfg.noise_level_img] * B)
    for use_graph in (True, False):
        np.testing.assert_array_equal(run(use_graph=use_graph, per_image=rows), graph)
