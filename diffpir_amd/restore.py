"""One batch of the DiffPIR restoration loop (main_ddpir.py:259-470) on the HIP engine.

Two entry points with identical results:
  * restore_batch          -- the fast path: host builds the per-step scalar table once, then ONE call
                              into dpir_run_loop (optionally a cached hipGraph) does init -> N x
                              (UNet -> prox -> re-noise) -> finalize without returning to Python.
  * restore_batch_stepwise -- the reference's loop body, line for line, calling the drop-in plugs
                              (utils_model.model_fn, utils_sisr.pre_calculate, dpir_prox_fft_apply, ...).
                              Exists to show (and test) that the reference loop runs unmodified
                              against the engine's operator surface.
Noise: noise_source="host" draws N(0,1) on the host in the reference's order (SURVEY.md 8 a-R: init,
then per step p_sample / n1 / n2) through `noise_fn(shape) -> np.ndarray` and uploads what the loop
consumes; noise_source="device" uses the engine's Philox stream keyed by (seed, global image index,
draw index), which makes results independent of how a batch is sharded across GPUs.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace
from typing import Callable, Optional

import numpy as np

from . import _lib
from .engine import Engine, DeviceArray, _ptr, EngineError
from .schedule import build_image_table, build_steps, find_nearest

TASKS = {"deblur": 0, "sr_blur": 1, "inpaint": 2, "sr_cubic": 3}


@dataclass
class LoopConfig:
    """The YAML keys that reach the loop (configs/*.yaml; derived fields main_ddpir.py:138-158)."""
    task: str = "deblur"               # deblur | sr | inpaint
    iter_num: int = 100
    noise_level_img: float = 12.75 / 255.0     # already /255 (main_ddpir.py:138)
    lambda_: float = 7.0
    zeta: float = 0.3
    eta: float = 0.0
    guidance_scale: float = 1.0
    sf: int = 1
    sr_mode: str = "blur"
    inIter: int = 1
    gamma: float = 0.01
    skip_type: str = "quad"
    num_train_timesteps: int = 1000
    beta_start: float = 0.0001
    beta_end: float = 0.02
    generate_mode: str = "DiffPIR"
    model_output_type: str = "pred_xstart"
    sub_1_analytic: bool = True
    ddim_sample: bool = False
    iter_num_U: int = 1
    noise_init_img: object = "max"      # 'max' -> t_start = T-1, else a noise level in /255 units (main_ddpir.py:197-200)
    skip_noise_model_t: bool = False    # main_ddpir.py:192-195, 391
    # which reference program's semantics the loop follows: "main_ddpir" (every task; refuses the gradient modes for deblurring, as that
    # program does) or "main_ddpir_deblur" (the standalone deblurring program: the reflect-padded blur operator in DPS_y0 / DPS_yt / the
    # first-order data step, its t_y initialisation of x in every mode, one image's own residual norm) or "main_ddpir_inpainting" (the
    # standalone inpainting program: the same t_y initialisation and the resampling of iter_num_U sub-steps per timestep)
    driver: str = "main_ddpir"

    @property
    def sigma(self):
        return max(0.001, self.noise_level_img)

    def engine_task(self) -> int:
        if self.task == "deblur":
            return TASKS["deblur"]
        if self.task == "inpaint":
            return TASKS["inpaint"]
        if self.task == "sr":
            return TASKS["sr_blur"] if self.sr_mode == "blur" else TASKS["sr_cubic"]
        raise ValueError(f"unknown task {self.task}")

    def check_supported(self):
        if self.driver not in DRIVERS:
            raise ValueError(f"driver={self.driver!r}: expected one of {DRIVERS}")
        if self.driver == "main_ddpir_deblur":
            if self.task != "deblur":
                raise ValueError("driver='main_ddpir_deblur' is the standalone deblurring program: task must be 'deblur'")
            if self.generate_mode not in ("DiffPIR", "DPS_y0", "DPS_yt") or self.model_output_type != "pred_xstart" or self.iter_num_U != 1:
                raise NotImplementedError("driver='main_ddpir_deblur' runs generate_mode DiffPIR (sub_1_analytic true or false), DPS_y0 and DPS_yt with "
                                          "model_output_type=pred_xstart, iter_num_U=1")
            return
        if self.driver == "main_ddpir_inpainting":
            if self.task != "inpaint":
                raise ValueError("driver='main_ddpir_inpainting' is the standalone inpainting program: task must be 'inpaint'")
            if not self.sub_1_analytic:
                raise NotImplementedError("sub_1_analytic=false is a `pass` under a TODO in main_ddpir_inpainting.py:280-283")
            if self.generate_mode not in ("DiffPIR", "repaint", "vanilla") or self.model_output_type != "pred_xstart":
                raise NotImplementedError("driver='main_ddpir_inpainting' runs generate_mode DiffPIR / repaint / vanilla with "
                                          "model_output_type=pred_xstart (pred_x_prev is not on the accelerated path), any iter_num_U >= 1")
            if int(self.iter_num_U) < 1:
                raise ValueError("iter_num_U must be >= 1")
            # skip_noise_model_t has nothing to select here: the program pins noise_model_t = 0 (main_ddpir_inpainting.py:89), so the test at :266 holds on
            # every step and the key is ignored, true or false
            from .schedule import make_seq
            n = len(make_seq(self.num_train_timesteps, self.iter_num, self.skip_type))
            if n < 10:
                raise ValueError(f"main_ddpir_inpainting.py:227 `progress_seq = seq[::(len(seq)//10)]` raises for a schedule of {n} entries "
                                 "(fewer than 10): there is no behaviour to mirror")
            return
        if self.model_output_type == "pred_x_prev":
            self._check_ancestral()
            return
        # ddim_sample is accepted: with model_output_type=pred_xstart it selects the same x0 prediction and the same number
        # of RNG draws as p_sample (utils_model.py:219-240; tests/golden/model_fn.npz).  iter_num_U > 1 cannot be mirrored:
        # the reference raises IndexError on `seq[i+1]` at its last step (main_ddpir.py:448-451 with u < iter_num_U-1).
        if not self.sub_1_analytic and not (self.generate_mode == "DiffPIR" and self.task == "sr"):
            # main_ddpir.py:420-430: the first-order data step differentiates through degrade_op, which only exists for task sr
            # (Resizer) in a runnable form (deblur: SURVEY Q1; inpaint: "TODO first order solver for inpainting")
            raise NotImplementedError("sub_1_analytic=false is implemented for generate_mode DiffPIR, task 'sr'")
        if self.generate_mode not in GENERATE_MODES or self.model_output_type != "pred_xstart" or self.iter_num_U != 1:
            raise NotImplementedError("only generate_mode in (DiffPIR, repaint, vanilla), model_output_type=pred_xstart, "
                                      "iter_num_U=1 are on the accelerated path (SURVEY.md 8f); the gradient-based modes DPS_y0 / DPS_yt and "
                                      "sub_1_analytic=false exist for task sr")
        if self.generate_mode in ("DPS_y0", "DPS_yt"):
            # main_ddpir.py:370-373, 433-445.  Runnable in the reference for task 'sr' only: the deblurring operator raises at :302
            #  and the inpainting branch never defines xt.
            if self.task != "sr":
                raise NotImplementedError("generate_mode DPS_y0 / DPS_yt are implemented for task 'sr' (the only one the reference can run)")
        elif self.generate_mode != "DiffPIR" and self.task != "inpaint":
            # main_ddpir.py:448: outside DiffPIR mode x is only re-noised for inpainting; other tasks would leave x untouched
            raise NotImplementedError("generate_mode repaint / vanilla are inpainting modes in the reference")

    def is_ancestral(self) -> bool:
        """driver main_ddpir with model_output_type pred_x_prev: the ancestral loops (dpir_run_ancestral_loop)."""
        return self.driver == "main_ddpir" and self.model_output_type == "pred_x_prev"

    def _check_ancestral(self):
        """model_output_type pred_x_prev under driver main_ddpir (main_ddpir.py:355-366): task inpaint with generate_mode repaint (RePaint-style
        ancestral sampling) or vanilla (plain DDPM ancestral sampling), iter_num_U 1.  Everything else has no behaviour to mirror."""
        if self.task != "inpaint":
            # main_ddpir.py:375 assigns the sample to x0, which nothing reads without 'pred_xstart' (:387, :448): x never changes
            raise NotImplementedError("model_output_type=pred_x_prev: only task 'inpaint' updates x from the sample (main_ddpir.py:365-366); "
                                      "for the other tasks the reference leaves x untouched")
        if self.generate_mode == "DiffPIR":
            raise NotImplementedError("model_output_type=pred_x_prev with generate_mode DiffPIR: the reference reads an unbound `tau` at "
                                      "main_ddpir.py:417 (it is assigned in the pred_xstart branch only, :389)")
        if self.generate_mode not in ("repaint", "vanilla"):
            raise NotImplementedError("model_output_type=pred_x_prev runs generate_mode repaint / vanilla (the reference asserts the inpainting "
                                      "modes at main_ddpir.py:154)")
        if int(self.iter_num_U) != 1:
            raise NotImplementedError("model_output_type=pred_x_prev with iter_num_U > 1: the reference reads an unbound `t_im1` at "
                                      "main_ddpir.py:465 (it is assigned in the pred_xstart re-noise only, :451)")
        # sub_1_analytic, lambda_, zeta, eta and guidance_scale are never read in these two modes (:384-445 has no branch for them)


DRIVERS = ("main_ddpir", "main_ddpir_deblur", "main_ddpir_inpainting")
GENERATE_MODES = {"DiffPIR": 0, "repaint": 1, "vanilla": 2, "DPS_y0": 3, "DPS_yt": 4}


@dataclass
class PerImage:
    """Per-image hyper-parameters of one restore_batch call: a batch may hold the same picture several times under different (lambda, zeta), or
    pictures of different noise levels -- the sweep of main_ddpir.py:548-580 as rows of full batches.  lambda_, zeta, noise_level_img: None (the
    LoopConfig's value for every image) or length-B sequences in LoopConfig's units; image_index: None (image_offset + b) or length-B ints, the
    global image number that keys each row's device noise.  Row b equals what a uniform call at its own values computes for that image."""
    lambda_: object = None
    zeta: object = None
    noise_level_img: object = None
    image_index: object = None

    def has_scalars(self) -> bool:
        return self.lambda_ is not None or self.zeta is not None or self.noise_level_img is not None

    def check(self, B: int):
        for name in ("lambda_", "zeta", "noise_level_img", "image_index"):
            v = getattr(self, name)
            if v is not None and len(v) != B:
                raise ValueError(f"PerImage.{name}: {len(v)} values for a batch of {B} images")

    def rows(self, lo: int, hi: int) -> "PerImage":
        """the rows [lo, hi) of a sharded batch"""
        cut = lambda v: None if v is None else list(v)[lo:hi]
        return PerImage(cut(self.lambda_), cut(self.zeta), cut(self.noise_level_img), cut(self.image_index))


def check_per_image(cfg: "LoopConfig", per_image: PerImage):
    """What has no per-image form, refused before the device is touched."""
    if cfg.driver != "main_ddpir":
        raise NotImplementedError(f"per_image: driver={cfg.driver!r} runs the standalone program's own loop, which has no per-image form")
    if cfg.generate_mode in ("DPS_y0", "DPS_yt"):
        raise NotImplementedError("per_image: the DPS modes have no per-image form")
    if cfg.is_ancestral():
        raise NotImplementedError("per_image: model_output_type=pred_x_prev reads none of lambda, zeta and the noise level inside the loop; there is "
                                  "nothing to vary per image (dpir_run_ancestral_loop has no per-image form)")
    if not cfg.sub_1_analytic:
        raise NotImplementedError("per_image: sub_1_analytic=false normalises its step by one residual norm of the whole batch (main_ddpir.py:425-427)")
    if cfg.skip_noise_model_t and per_image.noise_level_img is not None:
        raise NotImplementedError("per_image: skip_noise_model_t with a per-image noise level -- noise_model_t (main_ddpir.py:192) would differ per image")


def _image_table(cfg: "LoopConfig", per_image: PerImage, B: int):
    """((dt, steps, arr), table) of schedule.build_image_table for this call: _steps' keywords with the three per-image sequences filled in."""
    T = cfg.num_train_timesteps
    _steps(cfg)                                    # the uniform path's own checks (skip_noise_model_t against iter_num)
    t_start = None
    if cfg.noise_init_img != "max" or cfg.skip_noise_model_t:
        from .schedule import DriverTables
        t_start = t_start_of(cfg, DriverTables.make(cfg.beta_start, cfg.beta_end, T).reduced)
    every = lambda v, default: [default] * B if v is None else [float(x) for x in v]
    sigma = [max(0.001, v) for v in every(per_image.noise_level_img, cfg.noise_level_img)]         # LoopConfig.sigma per image
    return build_image_table(lambda_=every(per_image.lambda_, cfg.lambda_), zeta=every(per_image.zeta, cfg.zeta), sigma=sigma,
                             iter_num=cfg.iter_num, eta=cfg.eta, skip_type=cfg.skip_type, T=T, beta_start=cfg.beta_start, beta_end=cfg.beta_end,
                             t_start=t_start, generate_mode=cfg.generate_mode, model_output_type=cfg.model_output_type)


@dataclass
class Progress:
    """The progressive "process" strip of one restoration call (the reference's save_progressive / log_process / save_progressive_mask:
    main_ddpir_deblur.py:359-371, 400-406, main_ddpir_inpainting.py:302-313, 349-371).  Request: u8 (also the uint8 strips), masked (also the
    strips with the known pixels pasted back; needs a mask).  After the call: panels = [(seq value, t_i), ...] in strip order; strip_f32
    [B,3,H,P W] = x/2+.5 of each panel side by side, strip_u8 [B,H,P W,3]; masked_f32 / masked_u8 in the same layouts; minmax [P,B,2] =
    (np.max, np.min) of each image's panel -- numpy arrays on the host."""
    u8: bool = True
    masked: bool = False
    panels: list = None
    strip_f32: np.ndarray = None
    strip_u8: np.ndarray = None
    masked_f32: np.ndarray = None
    masked_u8: np.ndarray = None
    minmax: np.ndarray = None

    def log_lines(self, b: int):
        """log_process: one line per panel for image b, the reference's format (main_ddpir_deblur.py:368, main_ddpir_inpainting.py:311)."""
        return ["{:>4d}, steps: {:>4d}, np.max(x_show): {:.4f}, np.min(x_show): {:.4f}".format(s, t, self.minmax[p, b, 0], self.minmax[p, b, 1])
                for p, (s, t) in enumerate(self.panels)]


def progress_table(cfg: LoopConfig, entries):
    """(panel index or -1 for every step / row dict of build_steps / build_inpaint_rows, [(seq value, t_i) of each panel]).  An inpainting
    row group (the iter_num_U sub-steps of one timestep) keeps its panel on its last row: the snapshot follows the whole `for u` loop."""
    from .schedule import make_seq, progress_panels
    seq = make_seq(cfg.num_train_timesteps, cfg.iter_num, cfg.skip_type)
    visited = []
    for st in entries:
        if not visited or visited[-1] != st["seq_i"]:
            visited.append(st["seq_i"])
    of_i = dict(zip(visited, progress_panels(seq, visited, cfg.driver)))
    table, panels = [], []
    for j, st in enumerate(entries):
        closes = j + 1 == len(entries) or entries[j + 1]["seq_i"] != st["seq_i"]
        p = of_i[st["seq_i"]] if closes else -1
        table.append(p)
        if p >= 0:
            panels.append((int(st["seq"]), int(st["t"])))
    return table, panels


class _ArmedProgress:
    """Allocates the strips, arms the next whole-loop call (dpir_set_progress) and, after it, downloads them into the Progress object."""

    def __init__(self, engine: Engine, progress: Progress, cfg: LoopConfig, entries, B: int, H: int, W: int, has_mask: bool):
        if progress.masked and not has_mask:
            raise ValueError("Progress(masked=True) needs a mask (the inpainting task)")
        self.progress, self.engine = progress, engine
        table, self.panels = progress_table(cfg, entries)
        P = len(self.panels)
        self.f32 = engine.empty((B, 3, H, P * W))
        self.u8 = engine.empty((B, H, P * W, 3), np.uint8) if progress.u8 else None
        self.mf32 = engine.empty((B, 3, H, P * W)) if progress.masked else None
        self.mu8 = engine.empty((B, H, P * W, 3), np.uint8) if progress.masked and progress.u8 else None
        self.mm = engine.empty((P, B, 2))
        self.table = (C.c_int32 * len(table))(*table)
        d = _lib.ProgressDesc()
        d.panel_of_step_host, d.n_entries, d.n_panels = self.table, len(table), P
        d.strip_f32, d.strip_u8, d.masked_f32, d.masked_u8, d.minmax_dev = self.f32.ptr, _ptr(self.u8), _ptr(self.mf32), _ptr(self.mu8), self.mm.ptr
        engine._check(engine.lib.dpir_set_progress(engine.h, C.byref(d)))

    def finish(self):
        pg = self.progress
        pg.panels = self.panels
        pg.strip_f32, pg.minmax = self.f32.numpy(), self.mm.numpy()
        pg.strip_u8 = None if self.u8 is None else self.u8.numpy()
        pg.masked_f32 = None if self.mf32 is None else self.mf32.numpy()
        pg.masked_u8 = None if self.mu8 is None else self.mu8.numpy()


def _arm(engine, progress, cfg, entries, B, H, W, has_mask):
    return None if progress is None else _ArmedProgress(engine, progress, cfg, entries, B, H, W, has_mask)


class _HostProgress:
    """restore_batch_stepwise's side of Progress: x is downloaded at the panel steps and x/2+.5, the uint8 conversion, the masked blend and
    max / min are formed in numpy float32 -- deliberately NOT dpir_progress_snapshot, so that the stepwise path is the yardstick of the kernel."""

    def __init__(self, progress: Progress, cfg: LoopConfig, entries, y, mask):
        self.pg = progress
        self.table, self.panels = progress_table(cfg, entries)
        if progress.masked and mask is None:
            raise ValueError("Progress(masked=True) needs a mask (the inpainting task)")
        self.y = y.numpy() if progress.masked else None
        self.m = mask.numpy().astype(np.float32) if progress.masked else None
        self.f32, self.mf32 = [], []

    def take(self, j: int, x):
        """after step / row j (call with j = -1 freely)"""
        if j < 0 or self.table[j] < 0:
            return
        v = x.numpy() / np.float32(2) + np.float32(0.5)
        self.f32.append(v)
        if self.pg.masked:
            self.mf32.append(self.y * self.m + (np.float32(1) - self.m) * v)

    @staticmethod
    def _u8(strip):
        return np.ascontiguousarray(np.rint(np.clip(strip, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1))

    def finish(self):
        pg = self.pg
        pg.panels = self.panels
        pg.strip_f32 = np.concatenate(self.f32, axis=3)
        pg.minmax = np.stack([np.stack([v.max(axis=(1, 2, 3)), v.min(axis=(1, 2, 3))], axis=1) for v in self.f32]).astype(np.float32)
        pg.strip_u8 = self._u8(pg.strip_f32) if pg.u8 else None
        pg.masked_f32 = np.concatenate(self.mf32, axis=3) if pg.masked else None
        pg.masked_u8 = self._u8(pg.masked_f32) if pg.masked and pg.u8 else None


def t_start_of(cfg: LoopConfig, reduced) -> int:
    """main_ddpir.py:197-200: the timestep the forward-noised initial image is placed at; steps above it are skipped (:346)."""
    if cfg.noise_init_img == "max":
        return cfg.num_train_timesteps - 1
    return find_nearest(reduced, 2 * float(cfg.noise_init_img) / 255)


def start_coefficients(cfg: LoopConfig, dt):
    """(sa, s1m) of the initial x = sa (2y - 1) + s1m randn_like(y), float32.  main_ddpir.py:315 places y at t_start as if it were clean;
    main_ddpir_deblur.py:228-231 and main_ddpir_inpainting.py:190-193 noise it from its own level t_y up to t_start, on the driver's float32 tables."""
    t_start = t_start_of(cfg, dt.reduced)
    sa, s1m = np.float32(dt.sqrt_ac[t_start]), np.float32(dt.sqrt_1m_ac[t_start])
    if cfg.driver not in ("main_ddpir_deblur", "main_ddpir_inpainting"):
        return sa, s1m
    t_y = find_nearest(dt.reduced, 2 * cfg.noise_level_img)
    eff = np.float32(sa / np.float32(dt.sqrt_ac[t_y]))
    s1m_y = np.float32(dt.sqrt_1m_ac[t_y])
    return eff, np.sqrt(np.float32(np.float32(s1m * s1m) - np.float32(np.float32(eff * eff) * np.float32(s1m_y * s1m_y))), dtype=np.float32)


def _steps(cfg: LoopConfig):
    T = cfg.num_train_timesteps
    t_start = None
    if cfg.noise_init_img != "max" or cfg.skip_noise_model_t:
        from .schedule import DriverTables
        red = DriverTables.make(cfg.beta_start, cfg.beta_end, T).reduced
        t_start = t_start_of(cfg, red)
        if cfg.skip_noise_model_t:
            # main_ddpir.py:391 compares the LOOP INDEX with T - noise_model_t; the branch it guards (a switch to pred_x_prev that
            # persists for the rest of the run, :407-413) is dead for every iter_num below that bound -- and not mirrored beyond it
            noise_model_t = find_nearest(red, 2 * cfg.noise_level_img)
            if cfg.iter_num > T - noise_model_t:
                raise NotImplementedError("skip_noise_model_t with iter_num > T - noise_model_t selects the reference's pred_x_prev "
                                          "fallback (main_ddpir.py:407-413), which is not on the accelerated path")
    return build_steps(iter_num=cfg.iter_num, sigma=cfg.sigma, lambda_=cfg.lambda_, zeta=cfg.zeta, eta=cfg.eta,
                       skip_type=cfg.skip_type, T=T, beta_start=cfg.beta_start, beta_end=cfg.beta_end, t_start=t_start,
                       generate_mode=cfg.generate_mode, model_output_type=cfg.model_output_type)


def draw_host_noise(noise_fn: Callable, steps, shape, need_n1: bool, repaint: bool = False):
    """Consume noise_fn in the reference's order; keep only what the loop uses.  Per step: [repaint mix], p_sample, then
    (unless last) the eta draw and the zeta draw (main_ddpir.py:355-358, gaussian_diffusion.py:430, main_ddpir.py:454-456)."""
    init = np.asarray(noise_fn(shape), dtype=np.float32)
    n_re = sum(1 for s in steps if not s["last"])
    n1 = np.empty((n_re,) + tuple(shape), np.float32) if need_n1 else None
    n2 = np.empty((n_re,) + tuple(shape), np.float32)
    nrp = np.empty((len(steps),) + tuple(shape), np.float32) if repaint else None
    j = 0
    for i, s in enumerate(steps):
        if repaint:
            nrp[i] = noise_fn(shape)
        noise_fn(shape)                                   # p_sample's randn_like (gaussian_diffusion.py:430), unused
        if not s["last"]:
            a = noise_fn(shape)
            if need_n1:
                n1[j] = a
            n2[j] = noise_fn(shape)
            j += 1
    return (init, n1, n2, nrp) if repaint else (init, n1, n2)


def _dev(engine, a, dtype, keep: list):
    """a as a device array (a numpy array is uploaded), held in `keep` so that it outlives the asynchronous call; None stays None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        a = engine.to_device(a, dtype)
    keep.append(a)
    return a


def _loop_desc(cfg: LoopConfig, B, H, W, sf, start, y, k=None, mask=None, labels=None, seed=0, image_offset=0, use_graph=False,
               skip_dead_final_eval=False):
    """(_lib.LoopDesc without its noise pointers, the int64 label array or None) for every whole-loop entry.  start: (sa, s1m) of the initial x.
    The descriptor holds only the ADDRESS of the labels: the caller keeps the returned array until the engine call has returned."""
    d = _lib.LoopDesc()
    d.task = cfg.engine_task()
    d.B, d.H, d.W, d.sf = B, H, W, sf
    if k is not None:
        d.kh, d.kw = k.shape[2], k.shape[3]
    d.in_iter, d.gamma, d.guidance = cfg.inIter, cfg.gamma, cfg.guidance_scale
    d.sa_start, d.s1m_start = [float(v) for v in start]
    d.y_dev, d.k_dev, d.mask_dev = _ptr(y), _ptr(k), _ptr(mask)
    lab = None
    if labels is not None:
        lab = np.ascontiguousarray(labels, dtype=np.int64)
        d.labels_host = lab.ctypes.data
    d.seed, d.image_offset = seed, image_offset
    d.use_graph, d.skip_dead_final_eval = int(use_graph), int(skip_dead_final_eval)
    d.generate_mode = GENERATE_MODES[cfg.generate_mode]
    d.first_order = 0 if cfg.sub_1_analytic else 1
    # config.ddim_sample reaches model_fn(..., 'pred_x_prev_and_start') (main_ddpir.py:371-373): only the gradient-mode loops read it
    d.ddim_sample = 1 if cfg.ddim_sample else 0
    return d, lab


def _host_noise(noise_source, noise_fn, predrawn=None) -> bool:
    """Whether the call feeds host noise; a host-noise call must bring noise_fn or draws made ahead."""
    if noise_source == "host":
        if predrawn is None and noise_fn is None:
            raise EngineError("noise_source='host' needs noise_fn")
        return True
    if noise_source != "device":
        raise ValueError("noise_source must be 'host' or 'device'")
    return False


def _outputs(engine, B, H, W, out_f32, out_u8, return_u8):
    if out_f32 is None:
        out_f32 = engine.empty((B, 3, H, W))
    if out_u8 is None and return_u8:
        out_u8 = engine.empty((B, H, W, 3), np.uint8)
    return out_f32, out_u8


def _call_loop(engine, progress, cfg, entries, B, H, W, has_mask, call):
    """One whole-loop engine call with the progress request, if any, armed before it and downloaded after it."""
    armed = _arm(engine, progress, cfg, entries, B, H, W, has_mask)
    engine._check(call())
    if armed:
        armed.finish()


def restore_batch(engine: Engine, cfg: LoopConfig, y, k=None, mask=None, labels=None, noise_source="device",
                  noise_fn: Optional[Callable] = None, seed: int = 0, image_offset: int = 0, use_graph: bool = False,
                  skip_dead_final_eval: bool = False, out_f32=None, out_u8=None, return_u8: bool = False, _cache: dict = None,
                  predrawn=None, progress: Optional[Progress] = None, per_image: Optional[PerImage] = None):
    """y: [B,3,h,w] in [0,1]; k: [B,1,kh,kw]; mask: uint8 [B,3,H,W] -- device arrays (or numpy, uploaded).
    Returns a DeviceArray [B,3,H,W] = x_0 in [0,1] (un-clamped, main_ddpir.py:470), and the u8 NHWC
    array as well when return_u8.  progress: a Progress request, filled with the progressive strip of this call (every driver and mode).
    per_image: a PerImage -- lambda / zeta / noise level and the noise key per image (dpir_run_loop_per_image); the closed-form DiffPIR /
    repaint / vanilla loop of driver main_ddpir only.  Host noise and progress work unchanged; the caller orders the rows."""
    cfg.check_supported()
    if per_image is not None:
        check_per_image(cfg, per_image)
    if cfg.driver == "main_ddpir_inpainting":
        return _restore_inpaint_resample(engine, cfg, y, mask, labels, noise_source, noise_fn, seed, image_offset, use_graph, skip_dead_final_eval,
                                         out_f32, out_u8, return_u8, _cache, predrawn, progress=progress)
    if cfg.is_ancestral():
        return _restore_ancestral(engine, cfg, y, mask, labels, noise_source, noise_fn, seed, image_offset, use_graph, out_f32, out_u8, return_u8,
                                  _cache, predrawn, progress=progress)
    if cfg.driver == "main_ddpir_deblur" and (cfg.generate_mode != "DiffPIR" or not cfg.sub_1_analytic):
        if predrawn is not None or mask is not None or use_graph:
            raise NotImplementedError("the deblurring program's gradient modes take host noise through noise_fn, no mask and no step graph")
        return _restore_grad(engine, cfg, y, k, labels, noise_source, noise_fn, seed, image_offset, skip_dead_final_eval, out_f32, out_u8, return_u8,
                             progress=progress)
    if cfg.generate_mode in ("DPS_y0", "DPS_yt"):
        if predrawn is not None or mask is not None:
            raise NotImplementedError("DPS modes take host noise through noise_fn (their draw order differs from the DiffPIR loop's) and no mask")
        return _restore_grad(engine, cfg, y, None, labels, noise_source, noise_fn, seed, image_offset, skip_dead_final_eval, out_f32, out_u8, return_u8,
                             progress=progress)
    keep = []
    y = _dev(engine, y, np.float32, keep); k = _dev(engine, k, np.float32, keep); mask = _dev(engine, mask, np.uint8, keep)
    B, _, h, w = y.shape
    table = index = None
    if per_image is not None:
        per_image.check(B)
        if per_image.has_scalars():
            (dt, steps, arr), tab = _image_table(cfg, per_image, B)
            table = np.ascontiguousarray(tab, np.float32)
        if per_image.image_index is not None:
            index = np.ascontiguousarray(per_image.image_index, dtype=np.int64)
    if table is None:
        dt, steps, arr = _steps(cfg)
    H, W = h * cfg.sf, w * cfg.sf
    d, lab = _loop_desc(cfg, B, H, W, cfg.sf, start_coefficients(cfg, dt), y, k, mask, labels, seed, image_offset, use_graph, skip_dead_final_eval)
    if _host_noise(noise_source, noise_fn, predrawn):
        rp = cfg.generate_mode == "repaint"
        # predrawn: (init, n1, n2[, nrp]) already drawn in the reference's order (sharded runs)
        drawn = predrawn if predrawn is not None else draw_host_noise(noise_fn, steps, (B, 3, H, W), cfg.eta != 0, repaint=rp)
        init, n1, n2 = drawn[:3]
        d.noise_rp_dev = _ptr(_dev(engine, drawn[3] if rp else None, None, keep))
        d.noise_init_dev, d.noise_n2_dev = _dev(engine, init, None, keep).ptr, _dev(engine, n2, None, keep).ptr
        d.noise_n1_dev = _ptr(_dev(engine, n1, None, keep))
    out_f32, out_u8 = _outputs(engine, B, H, W, out_f32, out_u8, return_u8)
    if table is None and index is None:
        call = lambda: engine.lib.dpir_run_loop(engine.h, C.byref(d), arr, len(steps), _ptr(out_f32), _ptr(out_u8))
    else:
        call = lambda: engine.lib.dpir_run_loop_per_image(
            engine.h, C.byref(d), arr, len(steps), None if table is None else table.ctypes.data_as(C.POINTER(_lib.ImageStep)),
            None if index is None else index.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(out_f32), _ptr(out_u8))
    _call_loop(engine, progress, cfg, steps, B, H, W, mask is not None, call)
    if _cache is not None:
        _cache["keep"] = keep
    else:
        engine.sync()
    return (out_f32, out_u8) if return_u8 else out_f32


def dps_host_noise_shapes(cfg: LoopConfig, steps, B: int, H: int, W: int):
    """Shapes of the reference's randn_like draws in the DPS modes, in call order: init, then per step the sampler's draw
    (gaussian_diffusion.py:430 / :577, every step incl. the dead final one) and, DPS_yt on non-final steps, the y_t draw (main_ddpir.py:440)."""
    h, w = H // cfg.sf, W // cfg.sf
    shapes = [(B, 3, H, W)]
    for st in steps:
        shapes.append((B, 3, H, W))
        if cfg.generate_mode == "DPS_yt" and not st["last"]:
            shapes.append((B, 3, h, w))
        if cfg.driver == "main_ddpir_deblur" and cfg.generate_mode == "DiffPIR" and not st["last"]:
            shapes += [(B, 3, H, W)] * 2          # the re-noise's two draws (main_ddpir_deblur.py:346-347), analytic and first-order alike
    return shapes


def _inpaint_rows(cfg: LoopConfig):
    from .schedule import DriverTables, build_inpaint_rows
    t_start = None
    if cfg.noise_init_img != "max":
        t_start = t_start_of(cfg, DriverTables.make(cfg.beta_start, cfg.beta_end, cfg.num_train_timesteps).reduced)
    return build_inpaint_rows(iter_num=cfg.iter_num, iter_num_U=int(cfg.iter_num_U), sigma=cfg.sigma, lambda_=cfg.lambda_, zeta=cfg.zeta, eta=cfg.eta,
                              skip_type=cfg.skip_type, T=cfg.num_train_timesteps, beta_start=cfg.beta_start, beta_end=cfg.beta_end, t_start=t_start)


def inpaint_host_noise_shapes(cfg: LoopConfig, rows, B: int, H: int, W: int):
    """Shapes of the standalone inpainting program's randn_like draws, in call order.  The program restores one image at a time, so every draw
    is (1,3,H,W) and the whole sequence repeats per image: init (main_ddpir_inpainting.py:193), then per sub-step [the repaint mix, :245],
    p_sample's unused draw (gaussian_diffusion.py:430) and, on non-final steps, the eta and zeta draws (:293, both always drawn) and the
    set-back draw where u < iter_num_U - 1 (:300)."""
    one = (1, 3, H, W)
    per = [one]
    for r in rows:
        per += [one] * ((cfg.generate_mode == "repaint") + 1 + (0 if r["last"] else 2 + r["back"]))
    return per * B


def draw_inpaint_host_noise(noise_fn: Callable, cfg: LoopConfig, rows, B: int, H: int, W: int):
    """Consume noise_fn in the order of inpaint_host_noise_shapes and keep what the loop uses, batch-shaped:
    dict(init [B,3,H,W]; n1 (eta != 0) / n2 / back (iter_num_U > 1) / rp (repaint) [n_rows,B,3,H,W], or None)."""
    rp, n = cfg.generate_mode == "repaint", len(rows)
    full = (n, B, 3, H, W)
    out = dict(init=np.empty((B, 3, H, W), np.float32), n1=np.zeros(full, np.float32) if cfg.eta != 0 else None, n2=np.zeros(full, np.float32),
               back=np.zeros(full, np.float32) if any(r["back"] for r in rows) else None, rp=np.zeros(full, np.float32) if rp else None)
    one = (1, 3, H, W)
    for b in range(B):
        out["init"][b] = np.asarray(noise_fn(one), np.float32)[0]
        for s, r in enumerate(rows):
            if rp:
                out["rp"][s, b] = np.asarray(noise_fn(one), np.float32)[0]
            noise_fn(one)                                   # p_sample's randn_like, unused
            if r["last"]:
                continue
            a = np.asarray(noise_fn(one), np.float32)[0]
            if out["n1"] is not None:
                out["n1"][s, b] = a
            out["n2"][s, b] = np.asarray(noise_fn(one), np.float32)[0]
            if r["back"]:
                out["back"][s, b] = np.asarray(noise_fn(one), np.float32)[0]
    return out


def _restore_inpaint_resample(engine, cfg, y, mask, labels, noise_source, noise_fn, seed, image_offset, use_graph, skip_dead_final_eval,
                              out_f32, out_u8, return_u8, _cache, predrawn, _start=None, progress=None):
    """driver 'main_ddpir_inpainting' (main_ddpir_inpainting.py:190-303): dpir_run_inpaint_loop, one fused data pass per sub-step.
    predrawn: the dict of draw_inpaint_host_noise (sharded runs).  _start: (sa, s1m) instead of the t_y initialisation (tests)."""
    if mask is None:
        raise EngineError("inpainting needs a mask")
    dt, rows, arr = _inpaint_rows(cfg)
    keep = []
    y, mask = _dev(engine, y, np.float32, keep), _dev(engine, mask, np.uint8, keep)
    B, _, H, W = y.shape
    d, lab = _loop_desc(cfg, B, H, W, 1, start_coefficients(cfg, dt) if _start is None else _start, y, None, mask, labels, seed, image_offset,
                        use_graph, skip_dead_final_eval)
    nback = None
    if _host_noise(noise_source, noise_fn, predrawn):
        if predrawn is None:
            predrawn = draw_inpaint_host_noise(noise_fn, cfg, rows, B, H, W)
        dn = {k_: _dev(engine, v, np.float32, keep) for k_, v in predrawn.items()}
        d.noise_init_dev, d.noise_n1_dev, d.noise_n2_dev, d.noise_rp_dev = _ptr(dn["init"]), _ptr(dn["n1"]), _ptr(dn["n2"]), _ptr(dn["rp"])
        nback = dn["back"]
    out_f32, out_u8 = _outputs(engine, B, H, W, out_f32, out_u8, return_u8)
    _call_loop(engine, progress, cfg, rows, B, H, W, True,
               lambda: engine.lib.dpir_run_inpaint_loop(engine.h, C.byref(d), arr, len(rows), _ptr(nback), _ptr(out_f32), _ptr(out_u8)))
    if _cache is not None:
        _cache["keep"] = keep
    else:
        engine.sync()
    return (out_f32, out_u8) if return_u8 else out_f32


def _ancestral_rows(cfg: LoopConfig):
    from .schedule import DriverTables, build_ancestral_rows
    t_start = None
    if cfg.noise_init_img != "max":
        t_start = t_start_of(cfg, DriverTables.make(cfg.beta_start, cfg.beta_end, cfg.num_train_timesteps).reduced)
    return build_ancestral_rows(iter_num=cfg.iter_num, skip_type=cfg.skip_type, T=cfg.num_train_timesteps, beta_start=cfg.beta_start,
                                beta_end=cfg.beta_end, t_start=t_start)


def ancestral_host_noise_shapes(cfg: LoopConfig, rows, B: int, H: int, W: int):
    """Shapes of the reference's randn_like draws under model_output_type pred_x_prev, in call order: init (main_ddpir.py:315), then per step
    [the repaint mix, :357] and the sampler's draw (gaussian_diffusion.py:430 / :577; ddim consumes it too).  All batch-shaped."""
    return [(B, 3, H, W)] * (1 + len(rows) * ((cfg.generate_mode == "repaint") + 1))


def draw_ancestral_host_noise(noise_fn: Callable, cfg: LoopConfig, rows, B: int, H: int, W: int):
    """Consume noise_fn in the order of ancestral_host_noise_shapes: dict(init [B,3,H,W]; ps [n_rows,B,3,H,W]; rp (repaint) likewise, or None)."""
    shape, rp = (B, 3, H, W), cfg.generate_mode == "repaint"
    draw = lambda: np.asarray(noise_fn(shape), dtype=np.float32)
    out = dict(init=draw(), ps=np.empty((len(rows),) + shape, np.float32), rp=np.empty((len(rows),) + shape, np.float32) if rp else None)
    for s in range(len(rows)):
        if rp:
            out["rp"][s] = draw()
        out["ps"][s] = draw()
    return out


def _restore_ancestral(engine, cfg, y, mask, labels, noise_source, noise_fn, seed, image_offset, use_graph, out_f32, out_u8, return_u8, _cache,
                       predrawn, progress=None):
    """model_output_type 'pred_x_prev' of driver 'main_ddpir' (main_ddpir.py:355-366, task inpaint, generate_mode repaint / vanilla):
    dpir_run_ancestral_loop, one fused data pass per step.  predrawn: the dict of draw_ancestral_host_noise (sharded runs)."""
    if mask is None:
        raise EngineError("inpainting needs a mask")
    dt, rows, arr = _ancestral_rows(cfg)
    keep = []
    y, mask = _dev(engine, y, np.float32, keep), _dev(engine, mask, np.uint8, keep)
    B, _, H, W = y.shape
    d, lab = _loop_desc(cfg, B, H, W, 1, start_coefficients(cfg, dt), y, None, mask, labels, seed, image_offset, use_graph, False)
    nps = None
    if _host_noise(noise_source, noise_fn, predrawn):
        if predrawn is None:
            predrawn = draw_ancestral_host_noise(noise_fn, cfg, rows, B, H, W)
        dn = {k_: _dev(engine, v, np.float32, keep) for k_, v in predrawn.items()}
        d.noise_init_dev, d.noise_rp_dev = _ptr(dn["init"]), _ptr(dn["rp"])
        nps = dn["ps"]
    out_f32, out_u8 = _outputs(engine, B, H, W, out_f32, out_u8, return_u8)
    _call_loop(engine, progress, cfg, rows, B, H, W, True,
               lambda: engine.lib.dpir_run_ancestral_loop(engine.h, C.byref(d), arr, len(rows), _ptr(nps), _ptr(out_f32), _ptr(out_u8)))
    if _cache is not None:
        _cache["keep"] = keep
    else:
        engine.sync()
    return (out_f32, out_u8) if return_u8 else out_f32


def draw_grad_host_noise(noise_fn: Callable, cfg: LoopConfig, steps, B: int, H: int, W: int):
    """Host noise of the gradient-mode loops, consumed in the order of dps_host_noise_shapes; image n uses slice n of every batch-shaped draw.
    DPS_y0 / DPS_yt: dict(init [B,3,H,W], ps [n_steps,B,3,H,W], yt [n_steps,B,3,H/sf,W/sf] (DPS_yt; zeros where a step has no y_t draw) or None);
    the first-order data step of the deblurring program: dict(init, n1, n2) of draw_host_noise (no re-noising in the DPS modes, main_ddpir.py:448)."""
    if cfg.generate_mode == "DiffPIR":
        init, n1, n2 = draw_host_noise(noise_fn, steps, (B, 3, H, W), cfg.eta != 0)
        return dict(init=init, n2=n2, n1=n1)
    shapes = iter(dps_host_noise_shapes(cfg, steps, B, H, W))
    draw = lambda: np.asarray(noise_fn(next(shapes)), dtype=np.float32)
    yt_mode = cfg.generate_mode == "DPS_yt"
    init, ps, yt = draw(), [], []
    for st in steps:
        ps.append(draw())
        yt.append(draw() if yt_mode and not st["last"] else np.zeros((B, 3, H // cfg.sf, W // cfg.sf), np.float32))
    return dict(init=init, ps=np.stack(ps), yt=np.stack(yt) if yt_mode else None)


def _restore_grad(engine, cfg, y, k, labels, noise_source, noise_fn, seed, image_offset, skip_dead_final_eval, out_f32, out_u8, return_u8, progress=None):
    """The gradient modes: generate_mode DPS_y0 / DPS_yt of driver 'main_ddpir' (task sr; main_ddpir.py:370-373, 433-445: dpir_run_dps_loop over
    the Resizer) and DPS_y0 / DPS_yt / DiffPIR with sub_1_analytic false of driver 'main_ddpir_deblur' (dpir_run_deblur_grad_loop over the
    reflect-padded blur, k [B,1,K,K]).  One loop body in the engine; the driver picks the entry and the initialisation (start_coefficients)."""
    from .schedule import DiffusionTables
    deblur = cfg.driver == "main_ddpir_deblur"
    variant = {"DPS_y0": 0, "DPS_yt": 1, "DiffPIR": 2}[cfg.generate_mode]
    if variant == 0 and not engine.grad:
        raise EngineError("generate_mode DPS_y0 needs Engine.enable_grad() before the model is loaded")
    if deblur and k is None:
        raise EngineError("the deblurring program needs the PSFs k [B,1,K,K]")
    dt, steps, arr = _steps(cfg)
    dtab = DiffusionTables.make(cfg.num_train_timesteps)
    coefs = (_lib.DpsCoef * len(steps))()
    for i, st in enumerate(steps):
        coefs[i].pc1, coefs[i].pc2, coefs[i].min_log, coefs[i].max_log = [float(v) for v in dtab.dps_coef(st["t"])]
        coefs[i].sa_prev, coefs[i].s1m_prev = [float(v) for v in dtab.ddim_coef(st["t"])]
    if deblur and cfg.sf != 1:
        cfg = replace(cfg, sf=1)                    # the deblurring program has no scale factor: the key is ignored
    keep = []
    y, k = _dev(engine, y, np.float32, keep), _dev(engine, k, np.float32, keep)
    B, _, h, w = y.shape
    H, W = h * cfg.sf, w * cfg.sf
    d, lab = _loop_desc(cfg, B, H, W, cfg.sf, start_coefficients(cfg, dt), y, k, None, labels, seed, image_offset, False, skip_dead_final_eval)
    nps = nyt = None
    if _host_noise(noise_source, noise_fn):
        dn = {k_: _dev(engine, v, None, keep) for k_, v in draw_grad_host_noise(noise_fn, cfg, steps, B, H, W).items()}
        d.noise_init_dev, d.noise_n1_dev, d.noise_n2_dev = _ptr(dn["init"]), _ptr(dn.get("n1")), _ptr(dn.get("n2"))
        nps, nyt = dn.get("ps"), dn.get("yt")
    out_f32, out_u8 = _outputs(engine, B, H, W, out_f32, out_u8, return_u8)
    head = (engine.h, C.byref(d), arr, coefs, len(steps), variant, float(cfg.lambda_), _ptr(nps), _ptr(nyt))
    if deblur:
        call = lambda: engine.lib.dpir_run_deblur_grad_loop(*head, _ptr(out_f32), _ptr(out_u8))
    else:
        call = lambda: engine.lib.dpir_run_dps_loop(*head, 1.0, _ptr(out_f32), _ptr(out_u8))
    _call_loop(engine, progress, cfg, steps, B, H, W, False, call)
    engine.sync()
    return (out_f32, out_u8) if return_u8 else out_f32


def restore_batch_stepwise(model, diffusion, cfg: LoopConfig, y, k=None, mask=None, noise_fn: Callable = None, labels=None,
                           progress: Optional[Progress] = None):
    """The reference's loop body (main_ddpir.py:291-470) against the drop-in plugs, host-fed noise.  Every branch the monolithic
    loops implement: the DiffPIR analytic step, the first-order data step (sub_1_analytic: false), DPS_y0 and DPS_yt -- the latter
    three written with the reference's own expressions on device arrays (`xt - norm_grad * 1.`, ...)."""
    from . import utils_model, utils_sisr as sr
    from .utils_resizer import Resizer
    eng: Engine = model.engine
    cfg.check_supported()
    if cfg.driver == "main_ddpir_inpainting":
        return _stepwise_inpaint_resample(model, diffusion, cfg, y, mask, noise_fn, labels, progress)
    if cfg.is_ancestral():
        return _stepwise_ancestral(model, diffusion, cfg, y, mask, noise_fn, labels, progress)
    dt, steps, arr = _steps(cfg)
    hp = None if progress is None else _HostProgress(progress, cfg, steps, y, mask)
    B, _, h, w = y.shape
    H, W = h * cfg.sf, w * cfg.sf
    shape = (B, 3, H, W)
    lib, hnd = eng.lib, eng.h
    x = eng.empty(shape)
    dps = "DPS" in cfg.generate_mode
    deb = cfg.driver == "main_ddpir_deblur"      # main_ddpir_deblur.py's loop body: Tx as degrade_op, measurement y in [0, 1], t_y initialisation
    # (3) initialize x (main_ddpir.py:293-315)
    if cfg.task == "sr":
        degrade_op = Resizer(shape, 1 / cfg.sf, engine=eng)
        src = eng.empty(shape)
        eng._check(lib.dpir_bicubic_up(hnd, _ptr(y), src.ptr, cfg.sf, B, h, w))
        xs = src.numpy()
    elif cfg.task == "deblur":
        xs = y.numpy()
        if deb:
            from .utils_deblur import BlurOperator
            degrade_op = BlurOperator(k, engine=eng)            # Tx (main_ddpir_deblur.py:307-311, 317-321)
    else:
        xs = y.numpy() * mask.numpy().astype(np.float32)
    sa0, s1m0 = start_coefficients(cfg, dt)                     # main_ddpir.py:315 / main_ddpir_deblur.py:228-231
    n0 = np.asarray(noise_fn(shape), np.float32)
    x.copy_from(sa0 * (np.float32(2) * xs - np.float32(1)) + s1m0 * n0)
    if cfg.task in ("sr", "deblur") and not (cfg.task == "sr" and cfg.sr_mode == "cubic") and not dps and cfg.sub_1_analytic:
        FB, FBC, F2B, FBFy = sr.pre_calculate(y, k, cfg.sf, engine=eng)
    kwargs = {} if labels is None else {"y": labels}
    # the sampler's randn_like (gaussian_diffusion.py:430 / :577) and the loop's own draws come from ONE host stream, in call order
    draw = lambda like: eng.to_device(np.asarray(noise_fn(like.shape), np.float32))
    utils_model.set_randn_like(draw)
    try:
        for i, st in enumerate(steps):
            if hp:
                hp.take(i - 1, x)                               # the panel of the step before: x as that step left it
            curr_sigma = dt.reduced[st["t"]]
            t_i = st["t"]
            if cfg.generate_mode == "repaint":                  # main_ddpir.py:355-358
                nr = eng.to_device(np.asarray(noise_fn(shape), np.float32))
                eng._check(lib.dpir_repaint_mix(hnd, x.ptr, _ptr(y), _ptr(mask), C.byref(arr[i]), nr.ptr, B, H, W))
            if dps:                                             # main_ddpir.py:370-373
                x = x.requires_grad_()
                xt, x0 = utils_model.model_fn(x, noise_level=curr_sigma * 255, model_out_type="pred_x_prev_and_start", model_diffusion=model,
                                              diffusion=diffusion, ddim_sample=cfg.ddim_sample, alphas_cumprod=dt.alphas_cumprod, **kwargs)
            else:
                x0 = utils_model.model_fn(x, noise_level=curr_sigma * 255, model_out_type="pred_xstart", model_diffusion=model,
                                          diffusion=diffusion, ddim_sample=cfg.ddim_sample, alphas_cumprod=dt.alphas_cumprod, **kwargs)
                noise_fn(shape)                                 # p_sample's draw (unused for pred_xstart)
            if st["last"]:
                continue
            tau = np.float32(st["tau"])                         # rhos[t_i]
            if cfg.generate_mode == "DPS_y0":                   # main_ddpir.py:434-438 / main_ddpir_deblur.py:323-327
                measurement = y if deb else 2 * y - 1
                norm_grad, norm = utils_model.grad_and_value(operator=degrade_op, x=x, x_hat=x0, measurement=measurement)
                x = xt - norm_grad * 1.
                x = x.detach_()
                continue
            if cfg.generate_mode == "DPS_yt":                   # main_ddpir.py:439-445
                y_t = dt.sqrt_ac[t_i] * (2 * y - 1) + dt.sqrt_1m_ac[t_i] * draw(y)
                if deb:                                         # main_ddpir_deblur.py:331
                    y_t = y_t / 2 + 0.5
                measurement = y_t
                norm_grad, norm = utils_model.grad_and_value(operator=degrade_op, x=xt, x_hat=xt, measurement=measurement)
                x = xt - norm_grad * cfg.lambda_ * norm / tau * 0.35
                x = x.detach_()
                continue
            if cfg.generate_mode != "DiffPIR":
                pass                                            # no data-fidelity step outside DiffPIR mode (main_ddpir.py:385)
            elif not cfg.sub_1_analytic:                        # main_ddpir.py:420-430 (task sr)
                x0 = x0.requires_grad_()
                measurement = y if deb else 2 * y - 1           # main_ddpir_deblur.py:312
                norm_grad, norm = utils_model.grad_and_value(operator=degrade_op, x=x0, x_hat=x0, measurement=measurement)
                x0 = x0 - norm_grad * norm / tau
                x0 = x0.detach_()
            elif cfg.task == "inpaint":
                eng._check(lib.dpir_prox_mask(hnd, x0.ptr, _ptr(y), _ptr(mask), float(tau), cfg.guidance_scale, B, H, W))
            elif cfg.task == "deblur" or cfg.sr_mode == "blur":
                # main_ddpir.py:395-400 / main_ddpir_deblur.py:291-295 through the entry that replaces those lines as a whole (dpir_prox_fft_apply):
                # the kernels and the roundings of dpir_run_loop's data step, which on the half-spectrum layouts at guidance_scale 1 writes
                # 2 data_solution(.) - 1 without forming x0 + 1 (. - x0).  (Forming the blend on the host from sr.data_solution's output differs
                # from that by an ulp of x0 -- enough to separate the two loops' progress panels, which are compared bit for bit.)
                eng._check(lib.dpir_prox_fft_apply(hnd, FB.spectra.handle, x0.ptr, float(tau), float(cfg.guidance_scale)))
            else:
                eng._check(lib.dpir_prox_ibp(hnd, x0.ptr, _ptr(y), float(tau), cfg.gamma, cfg.inIter, cfg.sf, B, H, W))
            n1 = eng.to_device(np.asarray(noise_fn(shape), np.float32))
            n2 = eng.to_device(np.asarray(noise_fn(shape), np.float32))
            eng._check(lib.dpir_renoise(hnd, x.ptr, x0.ptr, C.byref(arr[i]), n1.ptr, n2.ptr, B, H, W))
    finally:
        utils_model.set_randn_like(None)
    if hp:
        hp.take(len(steps) - 1, x)
        hp.finish()
    out = eng.empty(shape)
    eng._check(lib.dpir_finalize(hnd, x.ptr, out.ptr, None, B, H, W))
    eng.sync()
    return out


def _stepwise_inpaint_resample(model, diffusion, cfg: LoopConfig, y, mask, noise_fn, labels, progress=None):
    """main_ddpir_inpainting.py:190-303 over the drop-in plugs, one launch per expression: the unfused statement of dpir_run_inpaint_loop.
    Host noise is taken through draw_inpaint_host_noise (the program's per-image draw order)."""
    from . import utils_model
    eng: Engine = model.engine
    dt, rows, arr = _inpaint_rows(cfg)
    hp = None if progress is None else _HostProgress(progress, cfg, rows, y, mask)
    B, _, H, W = y.shape
    shape, numel = (B, 3, H, W), B * 3 * H * W
    lib, hnd = eng.lib, eng.h
    nz = draw_inpaint_host_noise(noise_fn, cfg, rows, B, H, W)
    sa0, s1m0 = start_coefficients(cfg, dt)                     # :190-193
    x = eng.empty(shape)
    xs = y.numpy() * mask.numpy().astype(np.float32)            # y arrives masked: the identity (what init_x_kernel does)
    x.copy_from(sa0 * (np.float32(2) * xs - np.float32(1)) + s1m0 * nz["init"])
    kwargs = {} if labels is None else {"y": labels}
    steps = (_lib.Step * len(rows))()
    for s, r in enumerate(rows):
        for f, _ in _lib.Step._fields_:
            setattr(steps[s], f, r[f])
    for s, r in enumerate(rows):
        if hp:
            hp.take(s - 1, x)                               # :302-309 of the row group that just ended, ahead of this row's mix
        if cfg.generate_mode == "repaint":                  # :244-246
            nr = eng.to_device(nz["rp"][s])
            eng._check(lib.dpir_repaint_mix(hnd, x.ptr, _ptr(y), _ptr(mask), C.byref(steps[s]), nr.ptr, B, H, W))
        x0 = utils_model.model_fn(x, noise_level=dt.reduced[r["t"]] * 255, model_out_type="pred_xstart", model_diffusion=model,
                                  diffusion=diffusion, ddim_sample=cfg.ddim_sample, alphas_cumprod=dt.alphas_cumprod, **kwargs)
        if r["last"]:
            continue
        if cfg.generate_mode == "DiffPIR":                  # :267-268
            eng._check(lib.dpir_prox_mask(hnd, x0.ptr, _ptr(y), _ptr(mask), float(np.float32(r["tau"])), cfg.guidance_scale, B, H, W))
        n1 = None if nz["n1"] is None else eng.to_device(nz["n1"][s])
        n2 = eng.to_device(nz["n2"][s])
        eng._check(lib.dpir_renoise(hnd, x.ptr, x0.ptr, C.byref(steps[s]), _ptr(n1), n2.ptr, B, H, W))       # :288-293
        if r["back"]:                                       # :296-300
            nb = eng.to_device(nz["back"][s])
            eng._check(lib.dpir_ewise(hnd, 2, x.ptr, None, 0, float(np.float32(r["sae"])), x.ptr, numel))
            eng._check(lib.dpir_ewise(hnd, 2, nb.ptr, None, 0, float(np.float32(r["sb"])), nb.ptr, numel))
            eng._check(lib.dpir_ewise(hnd, 0, x.ptr, nb.ptr, numel, 0.0, x.ptr, numel))
    if hp:
        hp.take(len(rows) - 1, x)
        hp.finish()
    out = eng.empty(shape)
    eng._check(lib.dpir_finalize(hnd, x.ptr, out.ptr, None, B, H, W))
    eng.sync()
    return out


def _stepwise_ancestral(model, diffusion, cfg: LoopConfig, y, mask, noise_fn, labels, progress=None):
    """main_ddpir.py:312-315, 341-366, 470 under model_output_type pred_x_prev over the drop-in plugs (dpir_repaint_mix, model_fn 'pred_x_prev' ->
    dpir_p_sample): the unfused statement of dpir_run_ancestral_loop.  One host noise stream in call order: init, [mix], the sampler's draw."""
    from . import utils_model
    eng: Engine = model.engine
    dt, rows, arr = _ancestral_rows(cfg)
    hp = None if progress is None else _HostProgress(progress, cfg, rows, y, mask)
    B, _, H, W = y.shape
    shape = (B, 3, H, W)
    lib, hnd = eng.lib, eng.h
    x = eng.empty(shape)
    xs = y.numpy() * mask.numpy().astype(np.float32)            # :314
    sa0, s1m0 = start_coefficients(cfg, dt)
    x.copy_from(sa0 * (np.float32(2) * xs - np.float32(1)) + s1m0 * np.asarray(noise_fn(shape), np.float32))    # :315
    kwargs = {} if labels is None else {"y": labels}
    utils_model.set_randn_like(lambda like: eng.to_device(np.asarray(noise_fn(like.shape), np.float32)))
    try:
        for s, r in enumerate(rows):
            if hp:
                hp.take(s - 1, x)                               # the panel of the step before, ahead of this step's mix
            if cfg.generate_mode == "repaint":                  # :356-358
                st = _lib.Step()
                st.sa_t, st.s1m_t = r["sa_t"], r["s1m_t"]
                nr = eng.to_device(np.asarray(noise_fn(shape), np.float32))
                eng._check(lib.dpir_repaint_mix(hnd, x.ptr, _ptr(y), _ptr(mask), C.byref(st), nr.ptr, B, H, W))
            x = utils_model.model_fn(x, noise_level=dt.reduced[r["t"]] * 255, model_out_type="pred_x_prev", model_diffusion=model,
                                     diffusion=diffusion, ddim_sample=cfg.ddim_sample, alphas_cumprod=dt.alphas_cumprod, **kwargs)    # :365-366
    finally:
        utils_model.set_randn_like(None)
    if hp:
        hp.take(len(rows) - 1, x)
        hp.finish()
    out = eng.empty(shape)
    eng._check(lib.dpir_finalize(hnd, x.ptr, out.ptr, None, B, H, W))
    eng.sync()
    return out


def psnr_batch(a: np.ndarray, b: np.ndarray, max_pixel=2.0, eps=1e-10) -> float:
    """utils/utils_image.py:601-610 on numpy arrays in [-1,1]."""
    mse = np.mean((a.astype(np.float32) - b.astype(np.float32)) ** 2, axis=(1, 2, 3), dtype=np.float32)
    with np.errstate(divide="ignore"):
        v = np.where(mse == 0, np.inf, 20 * np.log10(max_pixel / np.sqrt(mse + np.float32(eps))))
    v = np.where(np.isnan(v), 0.0, v)
    return float(np.mean(v))
