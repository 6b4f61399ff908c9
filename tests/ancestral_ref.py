"""Test-side restatement of main_ddpir.py's loop under model_output_type 'pred_x_prev' (main_ddpir.py:312-315, 341-366, 470; task inpaint,
generate_mode repaint / vanilla, iter_num_U 1), pinned to the live program by tests/golden/ancestral.npz (tools/gen_golden_ancestral.py runs
the program's own test_rho).

Two parts:
  * restore_ref -- the float32 torch loop over oracle.unet_oracle's UNet and oracle.diffpir_oracle.p_sample_prev_and_start: init, then per
                   visited timestep [repaint mix ->] x = p_sample(x) (or ddim_sample, eta = 0);
  * step_f32    -- one step's data side in numpy float32, one rounding per operation, the std factor exp(0.5 lv) computed in float64 and
                   rounded once: what dpir_ancestral_step computes (to expf's last bit).
"""
import numpy as np
import torch

from oracle import diffpir_oracle as do

f32 = np.float32


def case_config(g, name):
    """The settings of fixture case `name` as a dict (noise_init_img: 'max' or a level in /255 units)."""
    c = {k.split(".cfg_")[1]: g[k][()] for k in g.files if k.startswith(name + ".cfg_")}
    return dict(generate_mode=str(c["generate_mode"]), skip_type=str(c["skip_type"]), iter_num=int(c["iter_num"]), ddim_sample=bool(c["ddim_sample"]),
                seed=int(c["seed"]), noise_init_img="max" if str(c["noise_init_img"]) == "max" else float(c["noise_init_img"]),
                noise_level_img=float(g["noise_level_img"]))


def loop_config(cfg, **over):
    from diffpir_amd import restore
    kw = dict(task="inpaint", model_output_type="pred_x_prev", iter_num=cfg["iter_num"], skip_type=cfg["skip_type"],
              noise_level_img=cfg["noise_level_img"], generate_mode=cfg["generate_mode"], ddim_sample=cfg["ddim_sample"],
              noise_init_img=cfg["noise_init_img"], lambda_=1.0, zeta=1.0)
    kw.update(over)
    return restore.LoopConfig(**kw)


def restore_ref(sd, hp, cfg, y01, mask_u8, noise_fn, T=1000):
    """x_0 [B,3,H,W] of the program; noise_fn(like) -> tensor, called in the program's order (init, then per step [mix], sampler).  y and mask
    enter with the strides the program's DataLoader path gives them (oracle.diffpir_oracle.loader_strides)."""
    dt, dtab = do.DriverTables(T=T), do.DiffusionTables(T)
    sa, s1m, red = dt.sqrt_ac, dt.sqrt_1m_ac, dt.reduced
    y = do.loader_strides(torch.from_numpy(y01))
    mask = do.loader_strides(torch.from_numpy(mask_u8.astype(np.float32)))
    seq = do.make_seq(T, cfg["iter_num"], cfg["skip_type"])
    t_start = T - 1 if cfg["noise_init_img"] == "max" else do.find_nearest(red, 2 * float(cfg["noise_init_img"]) / 255)
    x = y * mask                                                                                # :314
    x = sa[t_start] * (2 * x - 1) + s1m[t_start] * noise_fn(x)                                   # :315
    for i in range(len(seq)):
        t_i = do.find_nearest(red, red[T - 1 - seq[i]].numpy())                                  # :342-344
        if t_i > t_start:
            continue
        if cfg["generate_mode"] == "repaint":                                                   # :356-358
            x = (sa[t_i] * (2 * y - 1) + s1m[t_i] * noise_fn(x)) * mask + (1 - mask) * x
        x, _ = do.p_sample_prev_and_start(sd, hp, x, t_i, dtab, noise_fn(x), ddim=cfg["ddim_sample"])   # :365-366
    return (x / 2 + 0.5).numpy()                                                                 # :470


def step_f32(x, out6, y01, mask_u8, row, mode, ddim, n=None, nr=None):
    """One step's data side in float32, one rounding per operation.  row: a dict of schedule.build_ancestral_rows (or the same keys); mode 1 repaint /
    2 vanilla.  Returns (x_new, clamped x0, s n) with s = float32(exp(0.5 lv) in float64): the term whose last bit expf decides (zeros where the
    sampler's draw is not used)."""
    x, eps, v = x.astype(f32), out6[:, :3].astype(f32), out6[:, 3:6].astype(f32)
    r = {k: f32(val) for k, val in row.items() if isinstance(val, (float, np.floating))}
    a = np.minimum(np.maximum(r["c1"] * x - r["c2"] * eps, f32(-1)), f32(1))
    sn = np.zeros_like(x)
    if ddim:
        e2 = (r["c1"] * x - a) / r["c2"]
        o = a * r["sa_prev"] + r["s1m_prev"] * e2
    else:
        frac = (v + f32(1)) / f32(2)
        lv = frac * r["max_log"] + (f32(1) - frac) * r["min_log"]
        mean = r["pc1"] * a + r["pc2"] * x
        s = np.exp((f32(0.5) * lv).astype(np.float64)).astype(f32)
        nz = f32(1.0 if row["nonzero"] else 0.0)
        sn = (nz * s) * n.astype(f32)
        o = mean + sn
    if mode == 1 and row["mix_next"]:
        m = mask_u8.astype(f32)
        known = r["sa_n"] * (f32(2) * y01.astype(f32) - f32(1)) + r["s1m_n"] * nr.astype(f32)
        o = known * m + (f32(1) - m) * o
    assert o.dtype == f32 and a.dtype == f32
    return o, a, sn
