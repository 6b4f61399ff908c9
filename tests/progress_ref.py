"""Test-side float32 statement of the progressive panels of the standalone inpainting program (main_ddpir_inpainting.py:302-309 inside the loop
of :231-300), pinned to the live program by tests/golden/progress*.npz (tools/gen_golden_progress.py executes the program's own statements).

The loop is the one of tests/inpaint_resample_ref.py: oracle.unet_oracle's UNet for eps and substep_f32 for the data side of every sub-step,
numpy float32 with one rounding per operation.  A panel is x/2+.5 after the LAST sub-step of its timestep and BEFORE the next sub-step's
repaint mix, so the mix is applied here at the top of a sub-step (as the program does, :244-246) and never inside substep_f32."""
import numpy as np
import torch

from oracle import unet_oracle as uo
from tests import inpaint_resample_ref as ref

f32 = np.float32
BOUND = 2e-3        # tests/test_gpu_inpaint_resample.py holds x_0 of the same loop to it; a panel is the same quantity earlier in the loop
CASES = ("diffpir_u2", "repaint_u2_init120")


def load(golden):
    """The fixture: progress.npz (inputs, settings, seq, the (seq[i], t_i) of every panel) merged with the per-case panel files (one committed
    file may not exceed 1 MiB, and one case's 2 x P x 64 x 64 x 3 floats nearly fill that)."""
    g = dict(golden("progress"))
    for name in CASES:
        g.update(golden("progress." + name))
    return g


def case_config(g, name):
    c = {k.split(".cfg_")[1]: g[k][()] for k in g if k.startswith(name + ".cfg_")}
    return dict(generate_mode=str(c["generate_mode"]), iter_num_U=int(c["iter_num_U"]), eta=float(c["eta"]), zeta=float(c["zeta"]),
                lambda_=float(c["lambda_"]), guidance_scale=float(c["guidance_scale"]), seed=int(c["seed"]),
                noise_init_img="max" if str(c["noise_init_img"]) == "max" else float(c["noise_init_img"]),
                iter_num=int(g["iter_num"]), noise_level_img=float(g["noise_level_img"]))


def seeded(seed):
    gen = torch.Generator().manual_seed(seed)
    return lambda shape: torch.randn(tuple(shape), generator=gen, dtype=torch.float32).numpy()


def panels_ref(sd, hp, cfg, y01, mask_u8, noise_fn):
    """(strip [B,3,H,P W] float32, [(seq value, t_i), ...]) of the loop `cfg` (a restore.LoopConfig, driver main_ddpir_inpainting)."""
    from diffpir_amd import restore
    dt, rows, _ = restore._inpaint_rows(cfg)
    table, panels = restore.progress_table(cfg, rows)
    B, _, H, W = y01.shape
    nz = restore.draw_inpaint_host_noise(noise_fn, cfg, rows, B, H, W)
    mode = restore.GENERATE_MODES[cfg.generate_mode]
    sa0, s1m0 = restore.start_coefficients(cfg, dt)
    y, m = y01.astype(f32), mask_u8.astype(f32)
    x = f32(sa0) * (f32(2) * (y * m) - f32(1)) + f32(s1m0) * nz["init"]
    out = []
    pick = lambda a, s: None if a is None else a[s]         # noqa: E731
    for s, r in enumerate(rows):
        if mode == 1:                                       # :244-246
            known = f32(r["sa_t"]) * (f32(2) * y - f32(1)) + f32(r["s1m_t"]) * nz["rp"][s]
            x = known * m + (f32(1) - m) * x
        if not r["last"]:
            with torch.no_grad():
                eps = uo.unet_forward(sd, hp, torch.from_numpy(x), torch.tensor([r["t"]] * B))[:, :3].numpy()
            x, _ = ref.substep_f32(x, eps, y, mask_u8, dict(r, mix_next=0), mode, cfg.guidance_scale, n1=pick(nz["n1"], s), n2=nz["n2"][s],
                                   nb=pick(nz["back"], s))
        if table[s] >= 0:
            out.append(x / f32(2) + f32(0.5))               # :303
    return np.concatenate(out, axis=3), panels


def fixture_strip(g, name):
    """The reference's progress_img of case `name` ([B,P,H,W,3], as the program keeps them) as a strip [B,3,H,P W]."""
    p = g[name + ".progress_img"]
    B, P, H, W, _ = p.shape
    return np.ascontiguousarray(p.transpose(0, 4, 2, 1, 3).reshape(B, 3, H, P * W))


def per_panel_errors(strip, want, P):
    """[(max|strip - want|, bound)] per panel, bound = BOUND max(1, max|panel of want|)"""
    W = strip.shape[3] // P
    out = []
    for p in range(P):
        a, b = strip[..., p * W:(p + 1) * W], want[..., p * W:(p + 1) * W]
        out.append((float(np.abs(a - b).max()), BOUND * max(1.0, float(np.abs(b).max()))))
    return out
