"""Float64 statements of the deblurring program's measurement operator (csrc/blur.hip) and a torch-CPU restatement of the loop body of
main_ddpir_deblur.py for its four modes.  A helper, not a test; nothing here calls the engine, and nothing reads the reference tree.

The operator (main_ddpir_deblur.py:179-180, 307-311):  F.conv2d(ReflectionPad2d(K // 2)(x * xa + xb), eye(3) (x) k), with x * xa + xb formed in
float32 (the kernel's own first step, exact for xa = 0.5) and everything after it in the requested dtype; the adjoint is torch.autograd.grad of
that.  eye(3) (x) k only adds exact zeros from the other two channels, so the convolution is evaluated per channel (groups), and in blocks of output
rows so that torch's im2col buffer stays small at K = 61: the same sums either way.

Checker constants.  The plane-wise checker of tests/ops_f64.py (e_p <= max(K o_p, FLOOR), o_p = torch's own float32 evaluation against float64)
is used with that module's K_RATIO = 8 and FLOOR = 0 unchanged.  Measured on the MI355X over the six shapes of tests/test_gpu_blur_operator.py
(every plane, forward and adjoint): see MEASURED below.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import diffpir_oracle as do
from tests.ops_f64 import K_RATIO, FLOOR      # noqa: F401  (re-exported: the constants the operator tests run with)

# worst e_p / o_p per shape (B, H, W, K) on the MI355X, (forward, adjoint), first green run: the existing K_RATIO = 8 is used to 23 % at most,
# so no constant of its own is needed for the 3 721-term sums.  (The forward ratio is 1.000 throughout: the kernel's ascending-tap fmaf chain
# and torch's float32 convolution round alike on these inputs.)
MEASURED = {(1, 7, 9, 13): (1.000, 1.677), (2, 24, 40, 5): (1.000, 1.709), (3, 32, 32, 31): (1.000, 1.374), (1, 64, 64, 61): (1.000, 1.276),
            (1, 16, 16, 1): (0.0, 0.0), (2, 256, 256, 61): (1.000, 1.810)}


# ------------------------------------------------------------------------------------------------------------------ operator
def _conv_rows(pad, w, H, W, K):
    """Depthwise valid correlation of pad [1, P, H + K - 1, W + K - 1] with w [P, 1, K, K], in row blocks (im2col of at most ~32 M elements)."""
    rows = max(1, min(H, (1 << 25) // max(1, K * K * W)))
    out = [F.conv2d(pad[:, :, r:r + min(rows, H - r) + K - 1], w, groups=w.shape[0]) for r in range(0, H, rows)]
    return out[0] if len(out) == 1 else torch.cat(out, dim=2)


def blur_reflect(x, k, xa=0.5, xb=0.5, dtype=torch.float64):
    """x [B, 3, H, W] float32 tensor, k [B, 1, K, K] -> Tx(x) [B, 3, H, W] in `dtype`.  Differentiable w.r.t. x."""
    B, C, H, W = x.shape
    K = k.shape[-1]
    v = (x.float() * np.float32(xa) + np.float32(xb)).to(dtype)
    pad = torch.nn.ReflectionPad2d(K // 2)(v).reshape(1, B * C, H + K - 1, W + K - 1)
    w = k.to(dtype).reshape(B, 1, 1, K, K).expand(B, C, 1, K, K).reshape(B * C, 1, K, K)
    return _conv_rows(pad, w, H, W, K).reshape(B, C, H, W)


def blur_reflect_adjoint(g, k, xa=0.5, dtype=torch.float64):
    """torch.autograd.grad of blur_reflect w.r.t. x with cotangent g (the operator is affine: the point of linearisation does not matter)."""
    x = torch.zeros(g.shape, dtype=torch.float32, requires_grad=True)
    # x * xa is formed in float32 inside blur_reflect; for the adjoint in `dtype` the scaling has to be differentiated in `dtype` as well
    xd = x.to(dtype)
    B, C, H, W = g.shape
    K = k.shape[-1]
    pad = torch.nn.ReflectionPad2d(K // 2)(xd * xa).reshape(1, B * C, H + K - 1, W + K - 1)
    w = k.to(dtype).reshape(B, 1, 1, K, K).expand(B, C, 1, K, K).reshape(B * C, 1, K, K)
    out = _conv_rows(pad, w, H, W, K).reshape(B, C, H, W)
    return torch.autograd.grad(out, xd, g.to(dtype))[0]


def grad_and_value(x_hat, measurement, k, dtype=torch.float64):
    """utils_model.grad_and_value(operator=Tx, x=x_hat, x_hat=x_hat, measurement) per image: (norm_grad [B, 3, H, W], norm [B])."""
    xr = x_hat.float().clone().requires_grad_()
    diff = measurement.to(dtype) - blur_reflect(xr, k, dtype=dtype)
    norms = torch.stack([torch.linalg.norm(diff[n]) for n in range(diff.shape[0])])
    return torch.autograd.grad(norms.sum(), xr)[0], norms.detach()


# ------------------------------------------------------------------------------------------------------------------ the program's loop
def start_coefficients(cfg: do.LoopConfig, dt):
    """main_ddpir_deblur.py:228-231 on the driver's float32 tables."""
    t_start = cfg.t_start(dt)
    t_y = do.find_nearest(dt.reduced, 2 * cfg.noise_level_img)
    eff = dt.sqrt_ac[t_start] / dt.sqrt_ac[t_y]
    return eff, torch.sqrt(dt.sqrt_1m_ac[t_start] ** 2 - eff ** 2 * dt.sqrt_1m_ac[t_y] ** 2)


def restore_deblur(sd, hp, cfg: do.LoopConfig, y, k2d, noise_fn, exact_prox=False, grad_dtype=None):
    """main_ddpir_deblur.py:225-360 for ONE image: y [1, 3, H, W] in [0, 1], k2d [K, K].  cfg.generate_mode DiffPIR (cfg.sub_1_analytic True:
    the closed-form prox, :286-295; False: the first-order data step, :305-314), DPS_y0 (:323-327) or DPS_yt (:329-336).  noise_fn(like) is
    called in the program's randn_like order.  Returns x_0 = x / 2 + 0.5 (:360)."""
    dt, steps = do.step_tables(cfg)
    dtab = do.DiffusionTables(cfg.T)
    y = y.float()
    t_start = cfg.t_start(dt)
    k2d = k2d.float()
    k_4d = torch.einsum('ab,cd->abcd', torch.eye(3), k2d)                                    # :179-180
    p = k2d.shape[0] // 2

    def Tx(v):                                                                               # :307-311, :317-321
        return F.conv2d(torch.nn.ReflectionPad2d(p)(v / 2 + 0.5), k_4d)

    sa, s1m = start_coefficients(cfg, dt)
    x = sa * (2 * y - 1) + s1m * noise_fn(y)                                                 # :230-231
    pre = None
    if cfg.generate_mode == "DiffPIR" and cfg.sub_1_analytic:
        kt = k2d[None, None]
        pre = do.pre_calculate(y.double(), kt.double(), 1) if exact_prox else do.pre_calculate(y, kt, 1)     # :236
    for st in steps:
        t_i = st["t_i"]
        if t_i > t_start:                                                                    # :262-263
            continue
        if "DPS" in cfg.generate_mode:                                                       # :270-273
            x = x.detach().requires_grad_()
            xt, x0 = do.p_sample_prev_and_start(sd, hp, x, t_i, dtab, noise_fn(x), ddim=cfg.ddim_sample)
        else:                                                                                # :275-276
            x0 = do.model_fn_xstart(sd, hp, x, st["curr_sigma"] * 255, dt, dtab, noise_fn)
        if st["last"]:                                                                       # :284, :339
            continue
        if cfg.generate_mode == "DPS_y0":                                                    # :323-327
            norm = torch.linalg.norm(y - Tx(x0))
            norm_grad = torch.autograd.grad(outputs=norm, inputs=x)[0]
            x = (xt - norm_grad * 1.).detach()
            continue
        if cfg.generate_mode == "DPS_yt":                                                    # :329-336
            y_t = dt.sqrt_ac[t_i] * (2 * y - 1) + dt.sqrt_1m_ac[t_i] * noise_fn(y)
            y_t = y_t / 2 + 0.5
            xt = xt.detach().requires_grad_()
            norm = torch.linalg.norm(y_t - Tx(xt))
            norm_grad = torch.autograd.grad(outputs=norm, inputs=xt)[0]
            x = (xt - norm_grad * cfg.lambda_ * norm / st["tau"] * 0.35).detach()
            continue
        if cfg.sub_1_analytic:                                                               # :286-295
            x0 = do.prox_fft(x0, pre, st["tau"].repeat(1, 1, 1, 1), 1, cfg.guidance_scale, exact=exact_prox)
        else:                                                                                # :305-314
            x0 = x0.detach().requires_grad_()
            norm = torch.linalg.norm(y - Tx(x0))
            norm_grad = torch.autograd.grad(outputs=norm, inputs=x0)[0]
            x0 = (x0 - norm_grad * norm / st["tau"]).detach()
        n1 = noise_fn(x)                                                                     # :346-347
        n2 = noise_fn(x)
        x = do.renoise(x, x0, dt, t_i, st["t_im1"], cfg.eta, cfg.zeta, n1, n2)
    return x.detach() / 2 + 0.5


def image_noise_fn(seed, B, n, shapes=None):
    """The host noise of image n of a batch of B: every draw is made batch-shaped from one seeded stream, in call order, and image n takes
    slice n (what the engine's loop does with its host-fed noise).  shapes: a list that receives the batch shape of every draw."""
    gen = torch.Generator().manual_seed(seed)

    def fn(like):
        shp = (B,) + tuple(like.shape[1:])
        if shapes is not None:
            shapes.append(shp)
        return torch.randn(shp, generator=gen, dtype=torch.float32)[n:n + 1]
    return fn


def restore_deblur_batch(sd, hp, cfg, y, k, seed, exact_prox=False, shapes=None):
    """The program run once per image of the batch (its norm is that image's own), each with its slices of the batch-shaped noise."""
    B = y.shape[0]
    return torch.cat([restore_deblur(sd, hp, cfg, y[n:n + 1], k[n, 0], image_noise_fn(seed, B, n, shapes if n == 0 else None), exact_prox)
                      for n in range(B)])
