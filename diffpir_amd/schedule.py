"""Host-side schedule tables and per-step scalars of the DiffPIR loop (numpy only).

Mirrors main_ddpir.py:184-190 (float32 driver tables), :274-286 (sigmas / rhos), :327-344 + :451
(timestep sequence), :454-456 (re-noise coefficients) and the float64 tables of
guided_diffusion/gaussian_diffusion.py:27-35,133-151 used by eps -> x0 (:328-333).
Everything here is a few thousand scalar operations per batch; it is evaluated once, before the
loop, instead of 12 host<->device crossings per step in the reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

from . import _lib


@dataclass
class DriverTables:
    """main_ddpir.py:184-190.  np.cumprod on a float32 array is a sequential float32 product,
    which is what the reference gets from np.cumprod(torch_tensor_float32)."""
    T: int
    betas: np.ndarray
    alphas_cumprod: np.ndarray
    sqrt_ac: np.ndarray
    sqrt_1m_ac: np.ndarray
    reduced: np.ndarray

    @staticmethod
    def make(beta_start=0.0001, beta_end=0.02, T=1000) -> "DriverTables":
        # The reference evaluates these 1000-entry tables with torch CPU ops (main_ddpir.py:184-190);
        # torch.sqrt(float32) is not correctly rounded on every entry, so the same ops are used here
        # (host-side scalar prep) to obtain bit-identical tables.
        import torch
        betas = torch.from_numpy(np.linspace(beta_start, beta_end, T, dtype=np.float32))
        alphas = 1.0 - betas
        ac = torch.as_tensor(np.cumprod(alphas.numpy(), axis=0))
        s_ac = torch.sqrt(ac)
        s_1m = torch.sqrt(1. - ac)
        red = torch.div(s_1m, s_ac)
        return DriverTables(T, betas.numpy(), ac.numpy(), s_ac.numpy(), s_1m.numpy(), red.numpy())


@dataclass
class DiffusionTables:
    """GaussianDiffusion.__init__ float64 tables (gaussian_diffusion.py:133-151), linear schedule :27-35."""
    sqrt_recip_ac: np.ndarray
    sqrt_recipm1_ac: np.ndarray
    # posterior q(x_{t-1} | x_t, x_0) and the learned-range variance bounds (gaussian_diffusion.py:153-167, 268-276): p_sample of
    # the DPS modes (model_out_type 'pred_x_prev_and_start')
    posterior_mean_coef1: np.ndarray = None
    posterior_mean_coef2: np.ndarray = None
    posterior_log_variance_clipped: np.ndarray = None
    log_betas: np.ndarray = None
    alphas_cumprod_prev: np.ndarray = None

    @staticmethod
    def make(T=1000) -> "DiffusionTables":
        scale = 1000 / T
        betas = np.linspace(scale * 0.0001, scale * 0.02, T, dtype=np.float64)
        ac = np.cumprod(1.0 - betas, axis=0)
        ac_prev = np.append(1.0, ac[:-1])
        post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
        return DiffusionTables(np.sqrt(1.0 / ac), np.sqrt(1.0 / ac - 1),
                               betas * np.sqrt(ac_prev) / (1.0 - ac), (1.0 - ac_prev) * np.sqrt(1.0 - betas) / (1.0 - ac),
                               np.log(np.append(post_var[1], post_var[1:])), np.log(betas), ac_prev)

    def ddim_coef(self, t: int):
        """ddim_sample(eta = 0) (gaussian_diffusion.py:568-580): (sqrt(alpha_bar_prev), sqrt(1 - alpha_bar_prev - sigma^2)) with sigma = 0,
        evaluated in float32 as the reference does on its _extract_into_tensor(...).float() tensors."""
        abp = np.float32(self.alphas_cumprod_prev[t])
        return np.sqrt(abp, dtype=np.float32), np.sqrt(np.float32(np.float32(1.0) - abp) - np.float32(0.0), dtype=np.float32)

    def dps_coef(self, t: int):
        """(posterior_mean_coef1, posterior_mean_coef2, min_log, max_log) at t as float32 (_extract_into_tensor(...).float())."""
        return (np.float32(self.posterior_mean_coef1[t]), np.float32(self.posterior_mean_coef2[t]),
                np.float32(self.posterior_log_variance_clipped[t]), np.float32(self.log_betas[t]))

    def c1c2(self, t: int):
        return np.float32(self.sqrt_recip_ac[t]), np.float32(self.sqrt_recipm1_ac[t])


def find_nearest(array, value) -> int:
    """utils/utils_model.py:202-205."""
    array = np.asarray(array)
    return int(np.abs(array - value).argmin())


def make_seq(T: int, iter_num: int, skip_type: str = "quad") -> List[int]:
    """main_ddpir.py:327-335."""
    if skip_type == "uniform":
        skip = T // iter_num
        seq = [i * skip for i in range(iter_num)]
        if skip > 1:
            seq.append(T - 1)
        return seq
    if skip_type != "quad":
        raise ValueError(f"unknown skip_type {skip_type}")
    s = np.sqrt(np.linspace(0, T ** 2, iter_num))
    seq = [int(v) for v in list(s)]
    seq[-1] = seq[-1] - 1
    return seq


def progress_seq(seq, program: str = "main_ddpir") -> List[int]:
    """The seq values whose steps keep a panel of the progressive strip (save_progressive), literally as the reference builds them:
    main_ddpir.py:336-338 = main_ddpir_deblur.py:252-254 = main_ddpir_sisr.py:275-277 (`max(., 1)`, seq[-1] appended only when it is not
    last already) and main_ddpir_inpainting.py:227-228 (no max: raises for fewer than 10 entries; seq[-1] appended unconditionally)."""
    seq = list(seq)
    if program == "main_ddpir_inpainting":
        if len(seq) < 10:
            raise ValueError("main_ddpir_inpainting.py:227 `progress_seq = seq[::(len(seq)//10)]` raises for a schedule of fewer than 10 entries "
                             f"(got {len(seq)}): there is no behaviour to mirror")
        ps = seq[::(len(seq) // 10)]
        ps.append(seq[-1])
        return ps
    if program not in ("main_ddpir", "main_ddpir_deblur", "main_ddpir_sisr"):
        raise ValueError(f"unknown program {program!r}")
    ps = seq[::max(len(seq) // 10, 1)]
    if ps[-1] != seq[-1]:
        ps.append(seq[-1])
    return ps


def progress_panels(seq, visited, program: str = "main_ddpir") -> List[int]:
    """For every visited step -- `visited` lists the indices i into seq that the loop does not skip (t_i <= t_start; the `continue` of
    main_ddpir_deblur.py:262-263 / main_ddpir_inpainting.py:236-237 precedes the snapshot block), one entry per timestep, not per
    resampling sub-step -- its panel index in the strip, or -1.  Membership is by VALUE (`seq[i] in progress_seq`, main_ddpir_deblur.py:361,
    main_ddpir_inpainting.py:304), so every occurrence of a duplicated seq value keeps a panel; the final step (seq[i] == seq[-1]) always does."""
    ps = progress_seq(seq, program)
    out, p = [], 0
    for i in visited:
        if seq[i] in ps:
            out.append(p)
            p += 1
        else:
            out.append(-1)
    return out


def build_steps(*, iter_num: int, sigma: float, lambda_: float, zeta: float, eta: float = 0.0,
                skip_type: str = "quad", T: int = 1000, beta_start=0.0001, beta_end=0.02,
                t_start: int = None, generate_mode: str = "DiffPIR", model_output_type: str = "pred_xstart"):
    """Returns (DriverTables, list of python dicts, ctypes Step array) for one (lambda, zeta) setting.

    sigma = max(0.001, noise_level_img/255) (main_ddpir.py:141).  generate_mode / model_output_type select the sigma_k table the
    rhos are built from (main_ddpir.py:279-283): sigma_bar_t only for (pred_xstart, DiffPIR), sqrt(beta_t / alpha_t) otherwise --
    which is what generate_mode DPS_yt divides its step by (:443)."""
    dt = DriverTables.make(beta_start, beta_end, T)
    dtab = DiffusionTables.make(T)
    if t_start is None:
        t_start = T - 1
    seq = make_seq(T, iter_num, skip_type)
    # sigmas[i] = reduced[T-1-i]; rhos[i] = lambda*sigma^2/sigma_k[i]^2, sigma_k = s1m/sa, evaluated with
    # torch 0-dim float32 tensors like main_ddpir.py:277-286 (python-float / tensor = reciprocal * scalar)
    import torch
    t_s1m, t_sa = torch.from_numpy(dt.sqrt_1m_ac), torch.from_numpy(dt.sqrt_ac)
    if model_output_type == "pred_xstart" and generate_mode == "DiffPIR":
        sigma_ks = t_s1m / t_sa                           # main_ddpir.py:279-280
    else:
        t_betas = torch.from_numpy(dt.betas)
        sigma_ks = torch.sqrt(t_betas / (1.0 - t_betas))  # main_ddpir.py:282-283 (alphas = 1.0 - betas, :186)
    rhos = (lambda_ * (sigma ** 2) / (sigma_ks ** 2)).float().numpy()
    t_list = [find_nearest(dt.reduced, dt.reduced[T - 1 - s]) for s in seq]
    steps = []
    for i, t_i in enumerate(t_list):
        if t_i > t_start:
            continue                                      # main_ddpir.py:346-347
        last = seq[i] == seq[-1]
        c1, c2 = dtab.c1c2(t_i)
        st = dict(t=t_i, last=int(last), c1=float(c1), c2=float(c2), tau=float(rhos[t_i]),
                  sa_t=float(dt.sqrt_ac[t_i]), s1m_t=float(dt.sqrt_1m_ac[t_i]),
                  sa_p=0.0, k1=0.0, q=0.0, es=0.0, k2=0.0, t_im1=None, seq_i=i, seq=seq[i])
        if not last:
            t_p = t_list[i + 1]
            # main_ddpir.py:454-456 with 0-dim float32 tensors
            s1m_p, s1m_t = t_s1m[t_p], t_s1m[t_i]
            es = eta * s1m_p / s1m_t * torch.sqrt(torch.from_numpy(dt.betas)[t_i])
            q = torch.sqrt(s1m_p ** 2 - es ** 2)
            k2 = np.sqrt(zeta) * s1m_p
            st.update(sa_p=float(dt.sqrt_ac[t_p]), k1=float(np.float32(np.sqrt(1 - zeta))), q=float(q), es=float(es),
                      k2=float(k2), t_im1=t_p)
        steps.append(st)
    arr = (_lib.Step * len(steps))()
    for i, st in enumerate(steps):
        for f, _ in _lib.Step._fields_:
            setattr(arr[i], f, st[f])
    return dt, steps, arr


IMAGE_FIELDS = ("tau", "k1", "k2")          # what (lambda, zeta, sigma) reach of a step; every other field is shared by the batch


def build_image_table(*, lambda_, zeta, sigma, **kw):
    """Per-image (lambda, zeta, sigma) for one batch: lambda_, zeta and sigma are length-B sequences, every other keyword is build_steps' own and
    holds for the whole call.  Returns ((dt, steps, arr) of image 0's triple, float32 [n_steps, B, 4] of (tau, k1, k2, 0)) -- the table of
    dpir_run_loop_per_image.  build_steps is called once per distinct triple and its tau / k1 / k2 are copied: the numbers are the uniform
    path's own, none of main_ddpir.py:277-286, 454-456 is restated here.  ValueError when any other field of a step differs between triples."""
    lam, zet, sig = [float(v) for v in lambda_], [float(v) for v in zeta], [float(v) for v in sigma]
    if not lam or not (len(lam) == len(zet) == len(sig)):
        raise ValueError(f"lambda_, zeta and sigma must be sequences of one length B >= 1 (got {len(lam)}, {len(zet)}, {len(sig)})")
    built = {}
    for triple in zip(lam, zet, sig):
        if triple not in built:
            built[triple] = build_steps(lambda_=triple[0], zeta=triple[1], sigma=triple[2], **kw)
    first = built[(lam[0], zet[0], sig[0])]
    shared = [f for f, _ in _lib.Step._fields_ if f not in IMAGE_FIELDS]
    for triple, (_, steps, arr) in built.items():
        if len(steps) != len(first[1]):
            raise ValueError(f"(lambda, zeta, sigma) = {triple}: {len(steps)} steps, image 0 has {len(first[1])}")
        for i in range(len(steps)):
            for f in shared:
                if getattr(arr[i], f) != getattr(first[2][i], f):
                    raise ValueError(f"step {i}: field {f!r} differs between (lambda, zeta, sigma) = {triple} and image 0's "
                                     f"({getattr(arr[i], f)!r} != {getattr(first[2][i], f)!r}); only tau, k1 and k2 may depend on them")
    table = np.zeros((len(first[1]), len(lam), 4), np.float32)
    for b, triple in enumerate(zip(lam, zet, sig)):
        arr = built[triple][2]
        for i in range(table.shape[0]):
            table[i, b, :3] = [getattr(arr[i], f) for f in IMAGE_FIELDS]      # the ctypes array holds the float32 values the engine reads
    return first, table


def build_ancestral_rows(*, iter_num: int, skip_type: str = "quad", T: int = 1000, beta_start=0.0001, beta_end=0.02, t_start: int = None):
    """One row per visited step of main_ddpir.py:341-470 under model_output_type pred_x_prev, task inpaint, generate_mode repaint / vanilla,
    iter_num_U 1: returns (DriverTables, list of python dicts, ctypes AncestralRow array).  seq, t_i and the `t_i > t_start` skip are
    build_steps' (:327-347).  A step is x = model_fn(x, 'pred_x_prev') and nothing else, so a row holds p_sample's coefficients at t_i as
    utils_model.model_fn forms them for dpir_p_sample (DiffusionTables.c1c2 / dps_coef / ddim_coef: float64 tables cast to float32), the mix
    pair (sa, s1m)[t_i] of :356-358 from the driver's float32 tables, and the next row's pair for the mix the fused pass applies ahead of the
    next denoiser call.  There is no `last` flag: the final step is live (t = 0: nonzero = 0).  rhos (:284) are never read in these modes."""
    dt = DriverTables.make(beta_start, beta_end, T)
    dtab = DiffusionTables.make(T)
    if t_start is None:
        t_start = T - 1
    seq = make_seq(T, iter_num, skip_type)
    t_list = [find_nearest(dt.reduced, dt.reduced[T - 1 - s]) for s in seq]
    rows = []
    for i, t_i in enumerate(t_list):
        if t_i > t_start:
            continue                                      # main_ddpir.py:346-347
        c1, c2 = dtab.c1c2(t_i)
        pc1, pc2, min_log, max_log = dtab.dps_coef(t_i)
        sa_prev, s1m_prev = dtab.ddim_coef(t_i)
        rows.append(dict(t=t_i, nonzero=int(t_i != 0), mix_next=0, reserved=0, c1=float(c1), c2=float(c2), pc1=float(pc1), pc2=float(pc2),
                         min_log=float(min_log), max_log=float(max_log), sa_prev=float(sa_prev), s1m_prev=float(s1m_prev),
                         sa_t=float(dt.sqrt_ac[t_i]), s1m_t=float(dt.sqrt_1m_ac[t_i]), sa_n=0.0, s1m_n=0.0, seq_i=i, seq=seq[i]))
    for r, nxt in zip(rows[:-1], rows[1:]):
        r.update(mix_next=1, sa_n=nxt["sa_t"], s1m_n=nxt["s1m_t"])
    arr = (_lib.AncestralRow * len(rows))()
    for i, r in enumerate(rows):
        for f, _ in _lib.AncestralRow._fields_:
            setattr(arr[i], f, r[f])
    return dt, rows, arr


def build_inpaint_rows(*, iter_num: int, iter_num_U: int, sigma: float, lambda_: float, zeta: float, eta: float = 0.0,
                       skip_type: str = "quad", T: int = 1000, beta_start=0.0001, beta_end=0.02, t_start: int = None):
    """One row per sub-step (i, u) of the standalone inpainting program (main_ddpir_inpainting.py:200-300), model_out_type pred_xstart:
    returns (DriverTables, list of python dicts, ctypes InpaintRow array).  Every coefficient is formed with 0-dim float32 torch tensors in
    that program's operation order; rhos come from sigma_ks = s1m / sa in every generate_mode (:205-209 branch on model_out_type only).
    A row carries the set-back pair (sae, sb) of :298-300 with its `back` flag (u < U - 1) and the next row's (sa, s1m) for the repaint
    mix the fused pass applies ahead of the next denoiser call."""
    import torch
    if iter_num_U < 1:
        raise ValueError("iter_num_U must be >= 1")
    dt = DriverTables.make(beta_start, beta_end, T)
    dtab = DiffusionTables.make(T)
    if t_start is None:
        t_start = T - 1
    seq = make_seq(T, iter_num, skip_type)
    if len(seq) < 10:
        raise ValueError("main_ddpir_inpainting.py:227 `progress_seq = seq[::(len(seq)//10)]` raises for a schedule of fewer than 10 entries "
                         f"(got {len(seq)}): there is no behaviour to mirror")
    t_s1m, t_sa, t_betas = torch.from_numpy(dt.sqrt_1m_ac), torch.from_numpy(dt.sqrt_ac), torch.from_numpy(dt.betas)
    rhos = (lambda_ * (sigma ** 2) / ((t_s1m / t_sa) ** 2)).float().numpy()          # :206, :209
    t_list = [find_nearest(dt.reduced, dt.reduced[T - 1 - s]) for s in seq]          # :232-234
    rows, pos = [], -1
    for i, t_i in enumerate(t_list):
        if t_i > t_start:
            continue                                                                  # :236-237
        pos += 1
        last = seq[i] == seq[-1]
        c1, c2 = dtab.c1c2(t_i)
        base = dict(t=t_i, last=int(last), pos=pos, back=0, c1=float(c1), c2=float(c2), tau=float(rhos[t_i]), sa_t=float(dt.sqrt_ac[t_i]),
                    s1m_t=float(dt.sqrt_1m_ac[t_i]), sa_p=0.0, k1=0.0, q=0.0, es=0.0, k2=0.0, sae=0.0, sb=0.0, sa_n=0.0, s1m_n=0.0,
                    mix_next=0, reserved=0, t_im1=None, u=0, seq_i=i, seq=seq[i])
        if not last:
            t_p = t_list[i + 1]
            s1m_p, s1m_t = t_s1m[t_p], t_s1m[t_i]
            es = eta * s1m_p / s1m_t * torch.sqrt(t_betas[t_i])                       # :291
            q = torch.sqrt(s1m_p ** 2 - es ** 2)                                      # :292
            k2 = np.sqrt(zeta) * s1m_p                                                # :293
            sae = t_sa[t_i] / t_sa[t_p]                                               # :298
            arg = s1m_t ** 2 - sae ** 2 * s1m_p ** 2                                  # :299-300
            assert float(arg) >= 0.0, (t_i, t_p, float(arg))
            base.update(sa_p=float(dt.sqrt_ac[t_p]), k1=float(np.float32(np.sqrt(1 - zeta))), q=float(q), es=float(es), k2=float(k2),
                        sae=float(sae), sb=float(torch.sqrt(arg)), sb_arg=float(arg), t_im1=t_p)
        for u in range(iter_num_U):
            rows.append(dict(base, u=u, back=int(not last and u < iter_num_U - 1)))
    for r, nxt in zip(rows[:-1], rows[1:]):
        r.update(mix_next=1, sa_n=nxt["sa_t"], s1m_n=nxt["s1m_t"])
    arr = (_lib.InpaintRow * len(rows))()
    for i, r in enumerate(rows):
        for f, _ in _lib.InpaintRow._fields_:
            setattr(arr[i], f, r[f])
    return dt, rows, arr
