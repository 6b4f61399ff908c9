"""Build-machine only: tests/golden/inpaint_resample.npz from the standalone inpainting program itself.

This file holds no line of that program.  It takes, with `ast` at run time, two pieces of main_ddpir_inpainting.py -- the schedule statements
of main() (`betas = ...` through `t_start = ...`) and, out of test_rho's per-image loop, the statements from `t_y = ...` through the end of
the `for i in range(len(seq))` loop -- and executes them, compiled under the program's file name and line numbers, in a namespace it fills:
the tiny synthetic UNet (oracle.ref_exec.build_unet), one image's y in [-1, 1] and its mask, the settings of the case.  torch.randn_like is
routed to a seeded generator (oracle.ref_exec.patched_randn_like); `torch.sqrt` and `utils_model.model_fn` are wrapped by recorders that
call the real functions, which is how the per-sub-step scalars are read out while the loop runs.

The fixture holds arrays and scalars only: the shared inputs, and per case the settings, the noise seed, the shapes of the draws in order,
(t_i, t_im1, rho, sae, sb, back, last) of every sub-step and x_0 of both images.

    python tools/gen_golden_inpaint_resample.py
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_exec, ref_import, unet_oracle as uo  # noqa: E402

PROGRAM = os.path.join(ref_import.REF_ROOT, "main_ddpir_inpainting.py")
OUT = os.path.join(ROOT, "tests", "golden", "inpaint_resample.npz")
NOISE_LEVEL = 12.75 / 255.0
# name -> settings; noise_init_img in /255 units as in the YAML files ('max': t_start = T - 1)
CASES = {
    "diffpir_u1": dict(generate_mode="DiffPIR", iter_num_U=1, eta=0.0, zeta=1.0, lambda_=1.0, guidance_scale=1.0, noise_init_img="max", seed=101),
    "diffpir_u3": dict(generate_mode="DiffPIR", iter_num_U=3, eta=0.0, zeta=1.0, lambda_=1.0, guidance_scale=1.0, noise_init_img="max", seed=102),
    "repaint_u2": dict(generate_mode="repaint", iter_num_U=2, eta=0.0, zeta=1.0, lambda_=1.0, guidance_scale=1.0, noise_init_img="max", seed=103),
    "vanilla_u2": dict(generate_mode="vanilla", iter_num_U=2, eta=0.0, zeta=1.0, lambda_=1.0, guidance_scale=1.0, noise_init_img="max", seed=104),
    "diffpir_u2_eta": dict(generate_mode="DiffPIR", iter_num_U=2, eta=0.5, zeta=0.3, lambda_=7.0, guidance_scale=1.0, noise_init_img=120.0, seed=105),
}
ITER_NUM, T = 10, 1000


def _assigned(node):
    return ref_exec._names_assigned(node)


def pieces():
    """{'schedule': [...], 't_start_max': stmt, 'noise_init': stmt, 'body': [...], 'lines': {...}} from the program's source."""
    with open(PROGRAM) as f:
        tree = ast.parse(f.read(), filename=PROGRAM)
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    body = main.body
    i0 = next(i for i, n in enumerate(body) if "betas" in _assigned(n))
    ts = [i for i, n in enumerate(body) if "t_start" in _assigned(n)]
    ini = [i for i, n in enumerate(body) if "noise_inti_img" in _assigned(n)]
    assert len(ts) == 2 and len(ini) == 1 and i0 < ini[0] < ts[0] < ts[1], (i0, ini, ts)
    rho = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == "test_rho")
    per_image = next(n for n in rho.body if isinstance(n, ast.For) and "L_paths" in ast.unparse(n.iter))
    j0 = next(i for i, n in enumerate(per_image.body) if "t_y" in _assigned(n))
    j1 = next(i for i, n in enumerate(per_image.body) if isinstance(n, ast.For) and "len(seq)" in ast.unparse(n.iter))
    assert j0 < j1
    p = dict(schedule=body[i0:ini[0]], noise_init=body[ini[0]], t_start_level=body[ts[0]], between=body[ts[0] + 1:ts[1]], t_start_max=body[ts[1]],
             body=per_image.body[j0:j1 + 1])
    p["lines"] = dict(schedule=(body[i0].lineno, body[ts[1]].end_lineno), body=(per_image.body[j0].lineno, per_image.body[j1].end_lineno))
    return p


def _exec(nodes, ns):
    exec(compile(ast.Module(body=list(nodes), type_ignores=[]), PROGRAM, "exec"), ns)


def inputs():
    """Two 64 x 64 images: smooth synthetic ground truth, a box mask and a random mask, y = masked gt + noise, masked again (the program's
    :177-183 in the engine's [0, 1] convention)."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float32) / 64
    gt = np.stack([np.stack([0.5 + 0.4 * np.sin(6.0 * xx * (c + 1) + b) * np.cos(4.0 * yy + c) for c in range(3)]) for b in range(2)]).astype(np.float32)
    mask = np.ones((2, 3, 64, 64), np.uint8)
    mask[0, :, 20:44, 16:40] = 0
    mask[1] = (rng.random((1, 64, 64)) < 0.5).astype(np.uint8)
    m = mask.astype(np.float32)
    y = (gt * m) * 2 - 1 + rng.normal(0, NOISE_LEVEL * 2, gt.shape).astype(np.float32)
    y = ((y / 2 + 0.5) * m).astype(np.float32)
    return gt, y, mask


def run_case(case, y01, mask, model, diffusion):
    ns_ref = ref_import.load()
    p = pieces()
    g = torch.Generator().manual_seed(case["seed"])
    shapes = []

    def noise_fn(t):
        shapes.append(tuple(t.shape))
        return torch.randn(t.shape, generator=g, dtype=torch.float32)
    x0s, trace = [], None
    for b in range(y01.shape[0]):
        rec = []
        ns = dict(np=np, device=torch.device("cpu"), model=model, diffusion=diffusion,
                  beta_start=0.1 / 1000, beta_end=20 / 1000, num_train_timesteps=T, iter_num=ITER_NUM, skip=T // ITER_NUM, skip_type="quad",
                  noise_level_img=NOISE_LEVEL, noise_level_model=NOISE_LEVEL, sigma=max(0.001, NOISE_LEVEL), model_out_type="pred_xstart",
                  sub_1_analytic=True, ddim_sample=False, log_process=False, save_progressive=False, show_img=False,
                  **{k: case[k] for k in ("generate_mode", "iter_num_U", "eta", "zeta", "lambda_", "guidance_scale")})

        def sqrt(v, ns=ns, rec=rec):
            out = torch.sqrt(v)
            if "seq" in ns and out.ndim == 0:
                rec.append(("sqrt", ns["i"], ns["u"], float(out), float(ns["sqrt_alpha_effective"])))
            return out

        def model_fn(x, ns=ns, rec=rec, **kw):
            rec.append(("model_fn", ns["i"], ns["u"], int(ns["t_i"])))
            return ns_ref.utils_model.model_fn(x, **kw)
        ns["torch"] = ref_exec._Proxy(torch, sqrt=sqrt)
        ns["utils_model"] = ref_exec._Proxy(ns_ref.utils_model, model_fn=model_fn)
        _exec(p["schedule"], ns)
        if case["noise_init_img"] == "max":
            _exec([p["noise_init"], p["t_start_level"]] + p["between"] + [p["t_start_max"]], ns)
        else:
            ns["noise_inti_img"] = float(case["noise_init_img"]) / 255
            _exec([p["t_start_level"]], ns)
        ns["y"] = torch.from_numpy(y01[b:b + 1]) * 2 - 1
        ns["mask"] = torch.from_numpy(mask[b:b + 1].astype(np.float32))
        with ref_exec.patched_randn_like(noise_fn):
            _exec(p["body"], ns)
        x0s.append(ns["x_0"].detach().numpy().copy())
        # per sub-step scalars from the records
        subs = [(r[1], r[2], r[3]) for r in rec if r[0] == "model_fn"]
        seq, rhos = ns["seq"], ns["rhos"].numpy()
        rows = []
        for (i, u, t_i) in subs:
            last = seq[i] == seq[-1]
            sq = [r for r in rec if r[0] == "sqrt" and r[1] == i and r[2] == u]
            back = (not last) and u < case["iter_num_U"] - 1
            assert len(sq) == (0 if last else 2 + back), (i, u, len(sq))
            t_im1 = -1 if last else int(ns_ref.utils_model.find_nearest(ns["reduced_alpha_cumprod"], ns["sigmas"][seq[i + 1]].cpu().numpy()))
            rows.append((t_i, t_im1, rhos[t_i], np.float32(sq[2][4]) if back else np.float32(0), np.float32(sq[2][3]) if back else np.float32(0),
                         int(back), int(last), np.float32(sq[1][3]) if not last else np.float32(0)))
        if trace is None:
            trace, t_start = rows, int(ns["t_start"])
        else:
            assert rows == trace
    cols = list(zip(*trace))
    out = dict(x0=np.concatenate(x0s), draw_shapes=np.array(shapes, np.int64), t_start=np.int64(t_start),
               t_i=np.array(cols[0], np.int64), t_im1=np.array(cols[1], np.int64), rho=np.array(cols[2], np.float32), sae=np.array(cols[3], np.float32),
               sb=np.array(cols[4], np.float32), back=np.array(cols[5], np.int64), last=np.array(cols[6], np.int64), q=np.array(cols[7], np.float32))
    for k, v in case.items():
        out["cfg_" + k] = np.array(v)
    return out


def main():
    hp = uo.tiny_hp()
    model, diffusion = ref_exec.build_unet(hp, uo.synth_state_dict(hp, 0))
    gt, y, mask = inputs()
    out = dict(gt=gt, y=y, mask=mask, noise_level_img=np.float64(NOISE_LEVEL), iter_num=np.int64(ITER_NUM), cases=np.array(sorted(CASES)))
    for name in sorted(CASES):
        with torch.no_grad():
            r = run_case(CASES[name], y, mask, model, diffusion)
        for k, v in r.items():
            out[f"{name}.{k}"] = v
        print(name, "rows", len(r["t_i"]), "draws", len(r["draw_shapes"]), "x0 range", float(r["x0"].min()), float(r["x0"].max()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
