"""tests/golden/executed_reference.npz + tests/golden/reference_configs.json: what the reference's OWN code produced when it was executed
(oracle/ref_exec.py), stored as data so that tests/test_oracle_vs_live_reference.py runs wherever the repository is checked out:

  * `out_<case>`            : test_rho (taken out of main_ddpir.py with `ast`, executed unmodified; deblur with the one-statement edit of
                              SURVEY quirk Q1) on the tiny topology for the five loop cases of `CASES` (`case()`);
  * `dps_yt_rhos`           : the rhos table of a DPS_yt YAML (main_ddpir.py:274-286, executed);
  * `ts_<task>`, `taus_<task>` : every t_i the denoiser is called at and every tau handed to data_solution over the reference's sweep
                              (main_ddpir.py:548-580) for a 20-NFE deblur / sr YAML (ref_exec.reference_step_trace);
  * `lines_<piece>`, `n_stmt_test_rho`, `n_stmt_test_rho_deblur`, `n_dropped`, `dropped_is_q1` : where the executed pieces sit in
                              main_ddpir.py, the line counts of test_rho as executed for sr / inpaint and for deblur, how many lines the
                              deblur edit removes and whether the first is quirk Q1's einsum (numbers and flags only: no source text);
  * reference_configs.json  : the key / value pairs of the reference's configs/{deblur,inpaint,sisr}.yaml (yaml.safe_load).

TEST INFRASTRUCTURE ONLY; build container only (needs the reference tree, oracle/ref_import.py).
    python -m oracle.gen_golden_executed
"""
import json
import os

import numpy as np
import torch

from . import diffpir_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DIFFPIR_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
CASES = ("deblur", "inpaint", "sr_cubic", "repaint", "dps_yt")


def seeded(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda like: torch.randn(like.shape, generator=g, dtype=torch.float32)


def stored_configs():
    """{file name: key / value pairs} of the reference's configs/*.yaml, as stored in tests/golden/reference_configs.json."""
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fh:
        return json.load(fh)


def stored_yaml_for(task, **over):
    """ref_exec.yaml_for over the stored configs: the reference's configs/<task>.yaml as a dict, LPIPS and file output off, overrides."""
    d = dict(stored_configs()[{"deblur": "deblur", "sr": "sisr", "inpaint": "inpaint"}[task] + ".yaml"])
    d.update(calc_LPIPS=False, save_L=False, save_E=False)
    d.update(over)
    return d


def case(golden, name):
    """(oracle LoopConfig, y, k, mask, seed) of one loop case; `golden(name)` loads tests/golden/<name>.npz."""
    g = golden("loops")
    k = mask = None
    if name == "deblur":
        cfg, y, k, seed = do.LoopConfig("deblur", 5, 12.75 / 255, 7.0, 0.3, eta=0.7), g["deblur_y"], g["deblur_k"], 43
    elif name == "inpaint":
        cfg, y, mask, seed = do.LoopConfig("inpaint", 6, 0.0, 1.0, 1.0), g["inpaint_y"], g["inpaint_mask"], 44
    elif name == "repaint":
        cfg, y, mask, seed = do.LoopConfig(task="inpaint", iter_num=6, noise_level_img=0.0, lambda_=1.0, zeta=1.0, generate_mode="repaint"), g["inpaint_y"], g["inpaint_mask"], 45
    elif name == "sr_cubic":
        cfg, y, seed = do.LoopConfig("sr", 5, 12.75 / 255, 6.0, 0.25, sf=4, sr_mode="cubic", inIter=2, gamma=0.5), g["sr_y"], 46
        k = np.stack([golden("operators")["k_bic4"]] * 2)[:, None]
    elif name == "dps_yt":      # the mode whose rhos come from sqrt(beta / alpha), main_ddpir.py:279-283 -- at the reference's own lambda
        cfg, y, seed = do.LoopConfig("sr", 10, 12.75 / 255, 6.0, 0.25, sf=4, sr_mode="cubic", generate_mode="DPS_yt"), g["sr_y"], 82
        k = np.stack([golden("operators")["k_bic4"]] * 2)[:, None]
    else:
        raise ValueError(name)
    return cfg, y, k, mask, seed


def main():
    import ast
    import yaml
    from . import ref_exec, ref_import, unet_oracle as uo
    golden = lambda n: np.load(os.path.join(ROOT, "tests", "golden", n + ".npz"))
    out = {}
    hp = uo.tiny_hp()
    model, diffusion = ref_exec.build_unet(hp, uo.synth_state_dict(hp, 0))
    for name in CASES:
        cfg, y, k, mask, seed = case(golden, name)
        tk = None if k is None else torch.from_numpy(k)
        tm = None if mask is None else torch.from_numpy(mask).float()
        out[f"out_{name}"] = ref_exec.restore_ref(model, diffusion, cfg, torch.from_numpy(y), k=tk, mask=tm, noise_fn=seeded(seed)).numpy()
        print(name, "executed test_rho: range", float(out[f"out_{name}"].min()), float(out[f"out_{name}"].max()), flush=True)
    out["dps_yt_rhos"] = ref_exec.reference_tables(ref_exec.yaml_for("sr", iter_num=10, lambda_=6.0, zeta=0.25, generate_mode="DPS_yt",
                                                                     sr_mode="cubic"))["rhos"]
    for task in ("deblur", "sr"):
        out[f"ts_{task}"], out[f"taus_{task}"] = ref_exec.reference_step_trace(ref_exec.yaml_for(task, iter_num=20), (1, 3, 8, 8), sweep=True)
    p = ref_exec.main_pieces()
    for piece, (a, b) in p["lines"].items():
        out[f"lines_{piece}"] = np.array([a, b], np.int64)
    a, b = ast.unparse(p["test_rho"][0]).splitlines(), ast.unparse(p["test_rho_deblur"][0]).splitlines()
    out["n_stmt_test_rho"], out["n_stmt_test_rho_deblur"] = np.array(len(a)), np.array(len(b))
    gone = [l for l in a if l not in b]
    out["n_dropped"] = np.array(len(gone))
    out["dropped_is_q1"] = np.array(bool(gone) and "k_4d = torch.einsum('ab,cd->abcd'" in gone[0])
    np.savez_compressed(os.path.join(OUT, "executed_reference.npz"), **out)
    cfgs = {}
    for f in ("deblur.yaml", "inpaint.yaml", "sisr.yaml"):
        with open(os.path.join(ref_import.REF_ROOT, "configs", f)) as fh:
            cfgs[f] = yaml.safe_load(fh)
    with open(os.path.join(OUT, "reference_configs.json"), "w") as fh:
        json.dump(cfgs, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", sorted(out))


if __name__ == "__main__":
    main()
