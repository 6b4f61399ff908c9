"""Build-machine only: tests/golden/ancestral.npz from the reference program itself, model_output_type 'pred_x_prev'.

This file holds no line of that program.  It runs the live `test_rho` of main_ddpir.py through oracle.ref_exec.run_test_rho as it stands: the
reference's own configs/inpaint.yaml with the case's overrides, the tiny synthetic UNet (oracle.ref_exec.build_unet), one batch of two 64 x 64
images with a box mask and a random mask.  torch.randn_like is routed to a seeded generator that records the shape of every draw; the
`diffusion` object handed to the program is a proxy whose `p_sample` / `ddim_sample` record their timestep tensor and input and then call the
real methods, which is how t_i of every step and the first step's input are read out, where the program's model_fn delivers them.

For `vanilla_u1000` the tool also iterates the reference's `diffusion.p_sample` from t_start down to 0 on the program's own first input and
the same draws, asserts bit equality with the program's x_0 on the CPU, and stores that array: plain DDPM ancestral sampling is what the
program computes in that mode.

The fixture holds arrays and scalars only: the shared inputs, and per case the settings, the noise seed, the shapes of the draws in order,
t_i of every step, t_start and x_0.

    python tools/gen_golden_ancestral.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_exec, unet_oracle as uo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ancestral.npz")
NOISE_LEVEL = 12.75 / 255.0
# noise_init_img in /255 units as in the YAML files ('max': t_start = T - 1).  20.0 puts t_start at 45: every timestep from there down to 0 is visited
CASES = {
    "repaint_q10": dict(generate_mode="repaint", skip_type="quad", iter_num=10, ddim_sample=False, noise_init_img="max", seed=201),
    "vanilla_q10_ddim": dict(generate_mode="vanilla", skip_type="quad", iter_num=10, ddim_sample=True, noise_init_img="max", seed=202),
    "repaint_u1000": dict(generate_mode="repaint", skip_type="uniform", iter_num=1000, ddim_sample=False, noise_init_img=20.0, seed=203),
    "vanilla_u1000": dict(generate_mode="vanilla", skip_type="uniform", iter_num=1000, ddim_sample=False, noise_init_img=20.0, seed=204),
}


def inputs():
    """Two 64 x 64 images: smooth synthetic ground truth, a box mask and a random mask, y = masked gt + noise in [0, 1], masked again."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float32) / 64
    gt = np.stack([np.stack([0.5 + 0.4 * np.sin(5.0 * xx * (c + 1) + b) * np.cos(3.0 * yy + c) for c in range(3)]) for b in range(2)]).astype(np.float32)
    mask = np.ones((2, 3, 64, 64), np.uint8)
    mask[0, :, 18:46, 14:42] = 0
    mask[1] = (rng.random((1, 64, 64)) < 0.5).astype(np.uint8)
    m = mask.astype(np.float32)
    y = (gt * m) * 2 - 1 + rng.normal(0, NOISE_LEVEL * 2, gt.shape).astype(np.float32)
    y = ((y / 2 + 0.5) * m).astype(np.float32)
    return gt, y, mask


def _nhwc(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1)))


def run_case(case, y01, mask, model, diffusion):
    g = torch.Generator().manual_seed(case["seed"])
    shapes, draws, calls = [], [], []

    def noise_fn(t):
        shapes.append(tuple(t.shape))
        n = torch.randn(t.shape, generator=g, dtype=torch.float32)
        draws.append(n)
        return n

    def recorder(name):
        # the sampler the program's model_fn reaches: its timestep tensor and its input are read where they arrive, then the real method runs
        def call(net, x, t, **kw):
            assert bool((t == t[0]).all())
            calls.append((int(t[0]), x.detach().clone(), name))
            return getattr(diffusion, name)(net, x, t, **kw)
        return call

    B = y01.shape[0]
    yd = ref_exec.yaml_for("inpaint", iter_num=case["iter_num"], skip_type=case["skip_type"], generate_mode=case["generate_mode"],
                           model_output_type="pred_x_prev", ddim_sample=case["ddim_sample"], iter_num_U=1, noise_level_img=NOISE_LEVEL * 255.0,
                           noise_init_img=case["noise_init_img"], num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, batch_size=B)
    batch = (torch.zeros((B, 64, 64, 3), dtype=torch.uint8), _nhwc(y01), [f"{i}.png" for i in range(B)], torch.ones((B, 1, 1, 1, 1)),
             _nhwc(mask.astype(np.float32)))
    spy = ref_exec._Proxy(diffusion, p_sample=recorder("p_sample"), ddim_sample=recorder("ddim_sample"))
    outs, config, _ = ref_exec.run_test_rho(yd, [batch], model, spy, noise_fn=noise_fn)
    assert len(outs) == 1 and all(c[2] == ("ddim_sample" if case["ddim_sample"] else "p_sample") for c in calls)
    x0 = outs[0].numpy().copy()
    out = dict(x0=x0, draw_shapes=np.array(shapes, np.int64), t_start=np.int64(int(config.t_start)), t_i=np.array([c[0] for c in calls], np.int64))
    for k, v in case.items():
        out["cfg_" + k] = np.array(v)
    if case["skip_type"] == "uniform":
        ts = out["t_i"]
        assert 30 <= int(config.t_start) <= 60 and ts[0] == int(config.t_start) and (np.diff(ts) == -1).all() and ts[-1] == 0, (config.t_start, ts)
    if case["generate_mode"] == "vanilla" and not case["ddim_sample"]:
        # plain ancestral sampling: the reference's p_sample iterated on the program's first input with the program's draws (draw 0 is the init)
        x = calls[0][1]
        with ref_exec.patched_randn_like(lambda t, it=iter(draws[1:]): next(it)):
            for t in out["t_i"]:
                x = diffusion.p_sample(model, x, torch.tensor([int(t)] * B), clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs={})["sample"]
        ps = (x / 2 + 0.5).numpy()
        assert np.array_equal(ps.view(np.uint32), x0.view(np.uint32)), float(np.abs(ps - x0).max())
        out["psample_x0"] = ps
    return out


def main():
    hp = uo.tiny_hp()
    model, diffusion = ref_exec.build_unet(hp, uo.synth_state_dict(hp, 0))
    gt, y, mask = inputs()
    out = dict(gt=gt, y=y, mask=mask, noise_level_img=np.float64(NOISE_LEVEL), cases=np.array(sorted(CASES)))
    for name in sorted(CASES):
        with torch.no_grad():
            r = run_case(CASES[name], y, mask, model, diffusion)
        for k, v in r.items():
            out[f"{name}.{k}"] = v
        print(name, "steps", len(r["t_i"]), "t_start", int(r["t_start"]), "draws", len(r["draw_shapes"]), "x0 range", float(r["x0"].min()), float(r["x0"].max()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
