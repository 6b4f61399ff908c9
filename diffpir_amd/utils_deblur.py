"""The measurement operator of the reference's standalone deblurring program (main_ddpir_deblur.py:307-311, 317-321) as a plug:

    Tx = BlurOperator(k, engine=eng)
    norm_grad, norm = utils_model.grad_and_value(operator=Tx, x=x, x_hat=x0, measurement=y)

Tx(x) = F.conv2d(ReflectionPad2d(K // 2)(x / 2 + 0.5), eye(3) (x) k): a dense K x K cross-correlation with reflection padding, one PSF
per image shared by its three channels (csrc/blur.hip).  The `motionblur` PSF generators of the reference's utils_deblur are not part of
this package: any normalised PSF array is accepted.
"""
from __future__ import annotations

import numpy as np

from .engine import DeviceArray, Engine, EngineError, _ptr, default_engine


class BlurOperator:
    """k: a 2-D PSF [K, K] (broadcast to the batch at the first call) or per-image PSFs [B, 1, K, K] / [B, K, K]; numpy or DeviceArray."""

    xa = 0.5        # Tx starts with x / 2 + 0.5 (main_ddpir_deblur.py:308, 318)
    xb = 0.5

    def __init__(self, k, engine: Engine = None):
        self.engine = engine if engine is not None else (k.engine if isinstance(k, DeviceArray) else default_engine())
        self._host = None
        if isinstance(k, DeviceArray):
            if len(k.shape) != 4 or k.shape[1] != 1:
                raise EngineError(f"device PSFs must be [B, 1, K, K], got {k.shape}")
            self.k = k
        else:
            a = np.asarray(k.detach().cpu().numpy() if hasattr(k, "detach") else k, dtype=np.float32)
            if a.ndim == 2:
                self._host, self.k = a, None            # uploaded once the batch size is known
            elif a.ndim == 3:
                self.k = self.engine.to_device(a[:, None])
            elif a.ndim == 4 and a.shape[1] == 1:
                self.k = self.engine.to_device(a)
            else:
                raise EngineError(f"PSF must be [K, K], [B, K, K] or [B, 1, K, K], got {a.shape}")
        self.kh, self.kw = (self._host.shape if self.k is None else self.k.shape[2:])

    def psf(self, B: int) -> DeviceArray:
        if self.k is None or (self._host is not None and self.k.shape[0] != B):
            self.k = self.engine.to_device(np.broadcast_to(self._host, (B, 1) + self._host.shape))
        if self.k.shape[0] != B:
            raise EngineError(f"{self.k.shape[0]} PSFs for a batch of {B}")
        return self.k

    def forward(self, x):
        B, C, H, W = x.shape
        if C != 3:
            raise EngineError("BlurOperator works on [B, 3, H, W] images")
        e = self.engine
        out = e.empty((B, 3, H, W))
        e._check(e.lib.dpir_blur_reflect(e.h, _ptr(x), self.psf(B).ptr, self.kh, self.kw, self.xa, self.xb, out.ptr, B, H, W))
        return out

    __call__ = forward

    def transpose(self, g):
        """The adjoint of `forward` (what torch.autograd.grad(Tx(x), x, g) returns): 0.5 R^T C^T g."""
        B, C, H, W = g.shape
        if C != 3:
            raise EngineError("BlurOperator works on [B, 3, H, W] images")
        e = self.engine
        out = e.empty((B, 3, H, W))
        e._check(e.lib.dpir_blur_reflect_adjoint(e.h, _ptr(g), self.psf(B).ptr, self.kh, self.kw, self.xa, out.ptr, B, H, W))
        return out
