"""Build-machine only: tests/golden/progress.npz (+ one panel file per case) from the standalone inpainting program itself.

Like tools/gen_golden_inpaint_resample.py, whose `pieces()` / `_exec` machinery it reuses, this file holds no line of that program: the
schedule statements of main() and the per-image statements from `t_y = ...` through the end of the `for i in range(len(seq))` loop are taken
with `ast` at run time and executed in a namespace filled here -- this time with save_progressive = True, so that the loop's own
`if save_progressive and (seq[i] in progress_seq)` block (main_ddpir_inpainting.py:304-309) fills progress_img.

The fixture holds arrays and scalars only: the shared inputs and settings, and per case its settings, seq, t_start, the (seq[i], t_i) of
every panel and the program's progress_img panels of both images.  The panels of a case go to their own file
(tests/golden/progress.<case>.npz): 2 x 11 x 64 x 64 x 3 floats are 1.03 MiB before compression and a committed file may not exceed 1 MiB.

Each case is checked against the CPU float32 statement (tests/progress_ref.py) at the bound the tests use, panel by panel.

    python tools/gen_golden_progress.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_exec, ref_import, unet_oracle as uo  # noqa: E402
from tools import gen_golden_inpaint_resample as gen  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden")
ITER_NUM, T = 20, 1000
CASES = {
    "diffpir_u2": dict(generate_mode="DiffPIR", iter_num_U=2, eta=0.0, zeta=1.0, lambda_=1.0, guidance_scale=1.0, noise_init_img="max", seed=201),
    # t_start below T - 1: the skipped steps drop their panels
    "repaint_u2_init120": dict(generate_mode="repaint", iter_num_U=2, eta=0.0, zeta=1.0, lambda_=1.0, guidance_scale=1.0, noise_init_img=120.0, seed=202),
}
MAX_FILE = 1 << 20


def run_case(case, y01, mask, model, diffusion):
    ns_ref = ref_import.load()
    p = gen.pieces()
    g = torch.Generator().manual_seed(case["seed"])
    noise_fn = lambda t: torch.randn(t.shape, generator=g, dtype=torch.float32)     # noqa: E731
    imgs, trace = [], None
    for b in range(y01.shape[0]):
        rec = []
        ns = dict(np=np, device=torch.device("cpu"), model=model, diffusion=diffusion,
                  beta_start=0.1 / 1000, beta_end=20 / 1000, num_train_timesteps=T, iter_num=ITER_NUM, skip=T // ITER_NUM, skip_type="quad",
                  noise_level_img=gen.NOISE_LEVEL, noise_level_model=gen.NOISE_LEVEL, sigma=max(0.001, gen.NOISE_LEVEL), model_out_type="pred_xstart",
                  sub_1_analytic=True, ddim_sample=False, save_progressive=True, log_process=False, show_img=False, progress_img=[],
                  **{k: case[k] for k in ("generate_mode", "iter_num_U", "eta", "zeta", "lambda_", "guidance_scale")})

        def model_fn(x, ns=ns, rec=rec, **kw):
            rec.append((ns["i"], int(ns["t_i"])))
            return ns_ref.utils_model.model_fn(x, **kw)
        ns["utils_model"] = ref_exec._Proxy(ns_ref.utils_model, model_fn=model_fn)
        ns["torch"] = torch
        gen._exec(p["schedule"], ns)
        if case["noise_init_img"] == "max":
            gen._exec([p["noise_init"], p["t_start_level"]] + p["between"] + [p["t_start_max"]], ns)
        else:
            ns["noise_inti_img"] = float(case["noise_init_img"]) / 255
            gen._exec([p["t_start_level"]], ns)
        ns["y"] = torch.from_numpy(y01[b:b + 1]) * 2 - 1
        ns["mask"] = torch.from_numpy(mask[b:b + 1].astype(np.float32))
        with ref_exec.patched_randn_like(noise_fn):
            gen._exec(p["body"], ns)
        seq, t_of_i = list(ns["seq"]), dict(rec)
        # the steps that kept a panel, by the program's own test, in order: progress_img has one entry per such step
        kept = [(int(seq[i]), t_of_i[i]) for i in sorted(t_of_i) if seq[i] in ns["progress_seq"]]
        assert len(kept) == len(ns["progress_img"]), (len(kept), len(ns["progress_img"]))
        np.testing.assert_array_equal(ns["progress_img"][-1], np.transpose(ns["x_0"].numpy()[0], (1, 2, 0)))
        imgs.append(np.stack([np.asarray(a, np.float32) for a in ns["progress_img"]]))
        if trace is None:
            trace = dict(seq=np.array(seq, np.int64), t_start=np.int64(ns["t_start"]), panel_seq=np.array([k[0] for k in kept], np.int64),
                         panel_t=np.array([k[1] for k in kept], np.int64))
        else:
            assert [k[0] for k in kept] == list(trace["panel_seq"])
    meta = dict(trace)
    for k, v in case.items():
        meta["cfg_" + k] = np.array(v)
    return meta, np.stack(imgs)         # [B,P,H,W,3]


def main():
    from tests import progress_ref as pr
    hp = uo.tiny_hp()
    sd = uo.synth_state_dict(hp, 0)
    model, diffusion = ref_exec.build_unet(hp, sd)
    gt, y, mask = gen.inputs()
    out = dict(gt=gt, y=y, mask=mask, noise_level_img=np.float64(gen.NOISE_LEVEL), iter_num=np.int64(ITER_NUM), cases=np.array(sorted(CASES)))
    per_case = {}
    for name in sorted(CASES):
        with torch.no_grad():
            meta, imgs = run_case(CASES[name], y, mask, model, diffusion)
        for k, v in meta.items():
            out[f"{name}.{k}"] = v
        per_case[name] = {f"{name}.progress_img": imgs}
        print(name, "panels", imgs.shape[1], list(zip(meta["panel_seq"].tolist(), meta["panel_t"].tolist())), "t_start", int(meta["t_start"]))
    path = os.path.join(OUT_DIR, "progress.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for name, d in per_case.items():
        path = os.path.join(OUT_DIR, f"progress.{name}.npz")
        np.savez_compressed(path, **d)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= MAX_FILE, "a committed file may not exceed 1 MiB"
    # the CPU float32 statement against what was just written, at the tests' bound
    g = dict(out)
    for d in per_case.values():
        g.update(d)
    for name in sorted(CASES):
        c = pr.case_config(g, name)
        from tests import inpaint_resample_ref as ref
        strip, panels = pr.panels_ref(sd, hp, ref.loop_config(c), y, mask, pr.seeded(c["seed"]))
        assert panels == list(zip(g[name + ".panel_seq"].tolist(), g[name + ".panel_t"].tolist())), panels
        errs = pr.per_panel_errors(strip, pr.fixture_strip(g, name), len(panels))
        print(name, "CPU float32 statement vs the program, per panel max|d|:", " ".join(f"{e:.2e}" for e, _ in errs),
              "| bounds", " ".join(f"{b:.2e}" for _, b in errs))
        assert all(e <= b for e, b in errs), name


if __name__ == "__main__":
    main()
