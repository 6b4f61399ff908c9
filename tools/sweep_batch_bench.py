"""Times the reference's 11-point super-resolution lambda sweep (main_ddpir.py:548-580) two ways on one engine:

  sequential : what the YAML driver does by default -- one restore_batch call per sweep point over the whole test set (11 calls at B = 5);
  flattened  : `engine_batch_sweeps: true` -- the 55 (point, image) pairs cut into batches of 16 (16, 16, 16, 7) with per-image lambda / zeta
               (main_ddpir.run_batched_sweeps, restore.PerImage).

Workload: FFHQ topology with synthetic weights, sr-blur x4 at 256 x 256, 100 NFE, captured step graph, device noise, 5 synthetic images.  Both paths
include what the driver does around the loop (degradation, metrics).  Every shape is warmed first; the two paths then alternate --reps times in this one
process, each timed with a host clock around work that ends in engine.sync().  Prints one JSON line; profiles/sweep_batch/README.md keeps the result.

    python tools/sweep_batch_bench.py [--nfe 100] [--images 5] [--batch 16] [--reps 3] [--points 11]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Single:
    """the one-rank answers of diffpir_amd.dist that the driver's batch functions ask for"""
    @staticmethod
    def shard_range(n, rank, world):
        return 0, n

    @staticmethod
    def all_gather_results(local, n, rank, world, engine=None):
        return local


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nfe", type=int, default=100)
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--precision", default="f16x3")
    args = ap.parse_args()
    import logging
    logging.disable(logging.INFO)
    from diffpir_amd import Engine, degrade as dgr, restore, script_util, utils_model, weights
    from diffpir_amd import main_ddpir as drv

    config = drv.parse_config(os.path.join(ROOT, "configs", "sweep_batch_example.yaml"))
    config.iter_num, config.batch_size = args.nfe, args.batch
    points = drv.sweeps(config)[:args.points]
    eng = Engine(0)
    eng.set_precision(args.precision)
    margs = utils_model.create_argparser(dict(model_path="", num_channels=128, num_res_blocks=1, attention_resolutions="16")).parse_args([])
    model, _ = script_util.create_model_and_diffusion(**script_util.args_to_dict(margs, script_util.model_and_diffusion_defaults().keys()), engine=eng)
    model.load_state_dict(weights.synth_state_dict("ffhq"))
    imgs, _ = drv.load_images(config, args.images)
    H, W = imgs.shape[1], imgs.shape[2]
    cache = {}

    def sequential():
        """the default driver path: per point, the test set in batches of batch_size (here one batch of all images)"""
        out = []
        for lambda_, zeta in points:
            cfg = drv.loop_config(config, lambda_, zeta)
            vals = []
            for i0 in range(0, len(imgs), config.batch_size):
                gt = imgs[i0:i0 + config.batch_size]
                k_all, mask_all = drv.make_operators(config, len(gt), i0, H, W)
                y, ops = dgr.degrade(eng, config.task, gt, k=k_all, mask=mask_all, noise_level_img=config.noise_level_img, sf=config.sf,
                                     sr_mode=config.sr_mode, seed=config.seed + 1, image_offset=i0)
                o = restore.restore_batch(eng, cfg, y, k=ops.get("k"), noise_source="device", seed=config.seed, image_offset=i0, use_graph=True, _cache=cache)
                vals += list(dgr.metrics(eng, o, ops["gt"])[0])
            out.append(float(np.mean(vals)))
        eng.sync()
        return out

    def flattened():
        out = drv.run_batched_sweeps(eng, config, points, imgs, _Single, 0, 1, True, cache)
        eng.sync()
        return out

    ref_seq, ref_flat = sequential(), flattened()            # warm every shape: B = 5 and B = 16 / 7, uniform and per-image step graphs
    times = {"sequential": [], "flattened": []}
    for _ in range(args.reps):
        for name, fn in (("sequential", sequential), ("flattened", flattened)):
            eng.sync()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    s, f = np.array(times["sequential"]), np.array(times["flattened"])
    n_runs = len(points) * len(imgs)
    print(json.dumps({
        "workload": f"ffhq topology, synthetic weights, sr-blur x4, {H}x{W}, {args.nfe} NFE, graph, device noise, {len(imgs)} images x {len(points)} points, {args.precision}",
        "sequential_s": [round(v, 4) for v in s], "flattened_s": [round(v, 4) for v in f],
        "sequential_median_s": round(float(np.median(s)), 4), "flattened_median_s": round(float(np.median(f)), 4),
        "sequential_spread_s": round(float(s.max() - s.min()), 4), "flattened_spread_s": round(float(f.max() - f.min()), 4),
        "ratio_sequential_over_flattened": round(float(np.median(s) / np.median(f)), 4),
        "restorations_per_s": {"sequential": round(n_runs / float(np.median(s)), 3), "flattened": round(n_runs / float(np.median(f)), 3)},
        "flattened_batches": [len(b) for b in drv.flatten_sweeps(len(points), len(imgs), args.batch)],
        "max_abs_dpsnr_dB": float(np.max(np.abs(np.array(ref_seq) - np.array(ref_flat)))),
        "graph_cache_size": int(eng.lib.dpir_graph_cache_size(eng.h)),
    }))
    eng.close()


if __name__ == "__main__":
    main()
