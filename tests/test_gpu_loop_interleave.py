"""-m gpu: the graph-capable loops interleaved on ONE engine.  One step driver and one captured-step cache serve dpir_run_loop,
dpir_run_inpaint_loop and dpir_run_ancestral_loop; every other loop test runs one kind of loop per engine state.  Here four calls of three kinds
and two shapes (32 x 32, 64 x 64) alternate: each must keep computing the same bits, replayed or eager, and the cache must settle."""
import numpy as np
import pytest

from diffpir_amd import restore
from oracle import unet_oracle as uo
from tests import ancestral_ref, inpaint_resample_ref
from tests.gpu_common import make_model

pytestmark = pytest.mark.gpu
SEED = 4242


def _calls(golden):
    """(name, config, inputs): (a) dpir_run_loop deblur DiffPIR, (b) dpir_run_loop inpainting repaint, (c) dpir_run_inpaint_loop repaint with
    iter_num_U = 2, (d) dpir_run_ancestral_loop repaint -- the shapes and step counts of test_gpu_loop / _inpaint_resample / _ancestral_loop."""
    g, ir, an = golden("loops"), golden("inpaint_resample"), golden("ancestral")
    c = inpaint_resample_ref.loop_config(inpaint_resample_ref.case_config(ir, "repaint_u2"))
    c.iter_num_U = 2
    d = ancestral_ref.loop_config(ancestral_ref.case_config(an, "repaint_q10"))
    assert c.driver == "main_ddpir_inpainting" and c.generate_mode == "repaint" and d.model_output_type == "pred_x_prev" and d.generate_mode == "repaint"
    return [
        ("a", restore.LoopConfig(task="deblur", iter_num=6, lambda_=7.0, zeta=0.3), dict(y=g["deblur_y"], k=g["deblur_k"])),
        ("b", restore.LoopConfig(task="inpaint", iter_num=6, noise_level_img=0.0, lambda_=1.0, zeta=1.0, generate_mode="repaint"),
         dict(y=g["inpaint_y"], mask=g["inpaint_mask"])),
        ("c", c, dict(y=ir["y"], mask=ir["mask"])),
        ("d", d, dict(y=an["y"], mask=an["mask"])),
    ]


def test_interleaved_loops_keep_their_bits_and_the_cache_settles(golden):
    import diffpir_amd
    e = diffpir_amd.Engine(0)
    try:
        make_model(e, uo.tiny_hp())
        calls = _calls(golden)
        rounds, sizes = [], []
        for graph in (True, True, True, False):
            outs = {}
            for name, cfg, inp in calls:
                outs[name] = restore.restore_batch(e, cfg, inp["y"], k=inp.get("k"), mask=inp.get("mask"), noise_source="device", seed=SEED,
                                                   use_graph=graph).numpy()
                assert e.graph_cache_size() <= 16
            rounds.append(outs)
            sizes.append(e.graph_cache_size())
        print(f"interleave: graph cache after rounds 1..4 = {sizes}")
        for name, _, _ in calls:
            assert np.isfinite(rounds[0][name]).all()
            for r in range(1, 4):
                np.testing.assert_array_equal(rounds[r][name], rounds[0][name], err_msg=f"call {name}, round {r + 1} against round 1")
        # four different calls: not the same image four times
        assert len({rounds[0][n].tobytes() for n, _, _ in calls}) == 4
        # round 1 may still grow the workspace and strand its early captures; from round 2 on every step is found
        assert sizes[2] == sizes[1], sizes
        assert sizes[3] == sizes[2], sizes          # the eager round captures nothing
    finally:
        e.close()
