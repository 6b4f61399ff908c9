"""Test-side restatement of the standalone inpainting program's loop (main_ddpir_inpainting.py:190-303), pinned to the live program by
tests/golden/inpaint_resample.npz (tools/gen_golden_inpaint_resample.py executes the program's own statements).

Two parts:
  * restore_ref   -- the per-image float32 torch loop over oracle.unet_oracle's UNet: t_y initialisation, iter_num_U sub-steps per visited
                     timestep, [repaint mix] -> model_fn -> [masked prox] -> re-noise -> [set-back], in the program's operation order;
  * substep_f32   -- one sub-step's data side in numpy float32, one rounding per operation: what dpir_inpaint_step computes.
"""
import numpy as np
import torch

from oracle import diffpir_oracle as do

f32 = np.float32


def case_config(g, name):
    """The settings of fixture case `name` as a dict (noise_init_img: 'max' or a level in /255 units)."""
    c = {k.split(".cfg_")[1]: g[k][()] for k in g.files if k.startswith(name + ".cfg_")}
    out = dict(generate_mode=str(c["generate_mode"]), iter_num_U=int(c["iter_num_U"]), eta=float(c["eta"]), zeta=float(c["zeta"]),
               lambda_=float(c["lambda_"]), guidance_scale=float(c["guidance_scale"]), seed=int(c["seed"]),
               noise_init_img="max" if str(c["noise_init_img"]) == "max" else float(c["noise_init_img"]),
               iter_num=int(g["iter_num"]), noise_level_img=float(g["noise_level_img"]))
    return out


def loop_config(cfg):
    from diffpir_amd import restore
    return restore.LoopConfig(task="inpaint", driver="main_ddpir_inpainting", iter_num=cfg["iter_num"], iter_num_U=cfg["iter_num_U"],
                              noise_level_img=cfg["noise_level_img"], lambda_=cfg["lambda_"], zeta=cfg["zeta"], eta=cfg["eta"],
                              guidance_scale=cfg["guidance_scale"], generate_mode=cfg["generate_mode"], noise_init_img=cfg["noise_init_img"])


def restore_ref(sd, hp, cfg, y01, mask_u8, noise_fn, T=1000):
    """x_0 [B,3,H,W] of main_ddpir_inpainting.py:190-303, one image at a time; noise_fn(like) -> tensor, called in the program's order."""
    dt, dtab = do.DriverTables(T=T), do.DiffusionTables(T)
    sa, s1m, red = dt.sqrt_ac, dt.sqrt_1m_ac, dt.reduced
    sigma = max(0.001, cfg["noise_level_img"])
    sigmas = torch.tensor([red[T - 1 - i] for i in range(T)])
    rhos = torch.tensor([cfg["lambda_"] * (sigma ** 2) / ((s1m[i] / sa[i]) ** 2) for i in range(T)])                 # :203-211
    seq = do.make_seq(T, cfg["iter_num"], "quad")
    t_start = T - 1 if cfg["noise_init_img"] == "max" else do.find_nearest(red, 2 * float(cfg["noise_init_img"]) / 255)
    U, mode, eta, zeta, gs = cfg["iter_num_U"], cfg["generate_mode"], cfg["eta"], cfg["zeta"], cfg["guidance_scale"]
    draw = noise_fn
    outs = []
    for b in range(y01.shape[0]):
        y = torch.from_numpy(y01[b:b + 1]) * 2 - 1
        mask = torch.from_numpy(mask_u8[b:b + 1].astype(np.float32))
        t_y = do.find_nearest(red, 2 * cfg["noise_level_img"])                                                       # :190
        sae = sa[t_start] / sa[t_y]
        x = sae * y + torch.sqrt(s1m[t_start] ** 2 - sae ** 2 * s1m[t_y] ** 2) * draw(y)                            # :191-193
        for i in range(len(seq)):
            curr_sigma = sigmas[seq[i]].cpu().numpy()
            t_i = do.find_nearest(red, curr_sigma)
            if t_i > t_start:
                continue
            last = seq[i] == seq[-1]
            for u in range(U):
                if mode == "repaint":                                                                                # :244-246
                    x = (sa[t_i] * y + s1m[t_i] * draw(x)) * mask + (1 - mask) * x
                x0 = do.model_fn_xstart(sd, hp, x, curr_sigma * 255, dt, dtab, noise_fn=noise_fn)                     # :250
                if mode == "DiffPIR" and not last:                                                                   # :267-268
                    x0_p = (mask * y + rhos[t_i].float() * x0).div(mask + rhos[t_i])
                    x0 = x0 + gs * (x0_p - x0)
                if not last:                                                                                         # :288-293
                    t_im1 = do.find_nearest(red, sigmas[seq[i + 1]].cpu().numpy())
                    eps = (x - sa[t_i] * x0) / s1m[t_i]
                    eta_sigma = eta * s1m[t_im1] / s1m[t_i] * torch.sqrt(dt.betas[t_i])
                    x = sa[t_im1] * x0 + np.sqrt(1 - zeta) * (torch.sqrt(s1m[t_im1] ** 2 - eta_sigma ** 2) * eps + eta_sigma * draw(x)) \
                        + np.sqrt(zeta) * s1m[t_im1] * draw(x)
                if u < U - 1 and not last:                                                                           # :296-300
                    sae = sa[t_i] / sa[t_im1]
                    x = sae * x + torch.sqrt(s1m[t_i] ** 2 - sae ** 2 * s1m[t_im1] ** 2) * draw(x)
        outs.append((x / 2 + 0.5).numpy())                                                                   # :303
    return np.concatenate(outs)


def substep_f32(x, eps, y01, mask_u8, row, mode, guidance, n1=None, n2=None, nb=None, nr=None):
    """One sub-step's data side in float32, one rounding per operation.  row: a dict of schedule.build_inpaint_rows (or the same keys);
    mode 0 DiffPIR / 1 repaint / 2 vanilla.  Returns (x_new, clamped x0 before the prox or None on a final row)."""
    x, eps, y = x.astype(f32), eps.astype(f32), y01.astype(f32)
    m = mask_u8.astype(f32)
    r = {k: f32(v) for k, v in row.items() if isinstance(v, (float, np.floating))}
    g = f32(guidance)
    x0c = None
    if not row["last"]:
        a = np.minimum(np.maximum(r["c1"] * x - r["c2"] * eps, f32(-1)), f32(1))
        x0c = a.copy()
        if mode == 0:
            num = m * (f32(2) * y - f32(1)) + r["tau"] * a
            xp = num / (m + r["tau"])
            a = a + g * (xp - a)
        e = (x - r["sa_t"] * a) / r["s1m_t"]
        inner = r["q"] * e
        if r["es"] != 0:
            inner = inner + r["es"] * n1.astype(f32)
        x = r["sa_p"] * a + r["k1"] * inner
        x = x + r["k2"] * n2.astype(f32)
        if row["back"]:
            x = r["sae"] * x + r["sb"] * nb.astype(f32)
    if mode == 1 and row["mix_next"]:
        known = r["sa_n"] * (f32(2) * y - f32(1)) + r["s1m_n"] * nr.astype(f32)
        x = known * m + (f32(1) - m) * x
    assert x.dtype == f32
    return x, x0c
