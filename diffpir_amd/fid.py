"""FID (host side): the FID Inception-v3's schema, BatchNorm folding, weight loading, synthetic weights, and the Fréchet distance.

The paper's tables have a FID column beside PSNR and LPIPS (reference README.md:119-141), computed with `pytorch-fid`: the `pool3` features
(2048 per image) of its FID Inception-v3 for the restored set and for the ground-truth set give a mean and a covariance each, and the two
Gaussians a Fréchet distance.  The engine computes the features (csrc/fid.hip, dpir_fid_features); mean, covariance and the distance are
float64 on the host, here.  Neither `pytorch-fid` nor `torchvision` is a dependency: `load_weights` reads the file pytorch-fid downloads
(pt_inception-2015-12-05-6726825d.pth) with torch.load.

Canonical keys (what dpir_fid_load takes): <layer>.weight [Cout,Cin,KH,KW] and <layer>.bias [Cout] for the 94 layers of `inception_spec()`,
the eval-mode BatchNorm (eps = 1e-3) folded into them in float64 and rounded once.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

BN_EPS = 1e-3
FEATURES = 2048
SIDE = 299
DEFAULT_FILE = "pt_inception-2015-12-05-6726825d.pth"
# the 13 tensors dpir_fid_read_tap serves ahead of the features: (channels, side)
TAP_SHAPES = ((64, 73), (192, 35), (256, 35), (288, 35), (288, 35), (768, 17), (768, 17), (768, 17), (768, 17), (768, 17), (1280, 8), (2048, 8),
              (2048, 8))


class Layer(NamedTuple):
    name: str
    cin: int
    cout: int
    kernel: Tuple[int, int]
    stride: int
    padding: Tuple[int, int]
    in_hw: Tuple[int, int]
    out_hw: Tuple[int, int]


def inception_spec() -> List[Layer]:
    """The 94 BasicConv layers in execution order (convolution without bias -> BatchNorm eps 1e-3 -> ReLU), with the sizes the fixed
    299 x 299 entry gives them."""
    out: List[Layer] = []

    def conv(name, cin, cout, hw, k=(1, 1), s=1, p=(0, 0)):
        k = (k, k) if isinstance(k, int) else k
        p = (p, p) if isinstance(p, int) else p
        o = ((hw[0] + 2 * p[0] - k[0]) // s + 1, (hw[1] + 2 * p[1] - k[1]) // s + 1)
        out.append(Layer(name, cin, cout, k, s, p, hw, o))
        return o

    def pool_s2(hw):
        return ((hw[0] - 3) // 2 + 1, (hw[1] - 3) // 2 + 1)

    hw = conv("Conv2d_1a_3x3", 3, 32, (SIDE, SIDE), 3, 2)
    hw = conv("Conv2d_2a_3x3", 32, 32, hw, 3)
    hw = conv("Conv2d_2b_3x3", 32, 64, hw, 3, 1, 1)
    hw = pool_s2(hw)
    hw = conv("Conv2d_3b_1x1", 64, 80, hw)
    hw = conv("Conv2d_4a_3x3", 80, 192, hw, 3)
    hw = pool_s2(hw)
    c = 192
    for n, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
        conv(f"{n}.branch1x1", c, 64, hw)
        conv(f"{n}.branch5x5_1", c, 48, hw)
        conv(f"{n}.branch5x5_2", 48, 64, hw, 5, 1, 2)
        conv(f"{n}.branch3x3dbl_1", c, 64, hw)
        conv(f"{n}.branch3x3dbl_2", 64, 96, hw, 3, 1, 1)
        conv(f"{n}.branch3x3dbl_3", 96, 96, hw, 3, 1, 1)
        conv(f"{n}.branch_pool", c, pf, hw)
        c = 224 + pf
    n = "Mixed_6a"
    conv(f"{n}.branch3x3", c, 384, hw, 3, 2)
    conv(f"{n}.branch3x3dbl_1", c, 64, hw)
    conv(f"{n}.branch3x3dbl_2", 64, 96, hw, 3, 1, 1)
    hw = conv(f"{n}.branch3x3dbl_3", 96, 96, hw, 3, 2)
    c = 384 + 96 + c
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        conv(f"{n}.branch1x1", c, 192, hw)
        conv(f"{n}.branch7x7_1", c, c7, hw)
        conv(f"{n}.branch7x7_2", c7, c7, hw, (1, 7), 1, (0, 3))
        conv(f"{n}.branch7x7_3", c7, 192, hw, (7, 1), 1, (3, 0))
        conv(f"{n}.branch7x7dbl_1", c, c7, hw)
        conv(f"{n}.branch7x7dbl_2", c7, c7, hw, (7, 1), 1, (3, 0))
        conv(f"{n}.branch7x7dbl_3", c7, c7, hw, (1, 7), 1, (0, 3))
        conv(f"{n}.branch7x7dbl_4", c7, c7, hw, (7, 1), 1, (3, 0))
        conv(f"{n}.branch7x7dbl_5", c7, 192, hw, (1, 7), 1, (0, 3))
        conv(f"{n}.branch_pool", c, 192, hw)
    n = "Mixed_7a"
    conv(f"{n}.branch3x3_1", c, 192, hw)
    conv(f"{n}.branch3x3_2", 192, 320, hw, 3, 2)
    conv(f"{n}.branch7x7x3_1", c, 192, hw)
    conv(f"{n}.branch7x7x3_2", 192, 192, hw, (1, 7), 1, (0, 3))
    conv(f"{n}.branch7x7x3_3", 192, 192, hw, (7, 1), 1, (3, 0))
    hw = conv(f"{n}.branch7x7x3_4", 192, 192, hw, 3, 2)
    c = 320 + 192 + c
    for n in ("Mixed_7b", "Mixed_7c"):
        conv(f"{n}.branch1x1", c, 320, hw)
        conv(f"{n}.branch3x3_1", c, 384, hw)
        conv(f"{n}.branch3x3_2a", 384, 384, hw, (1, 3), 1, (0, 1))
        conv(f"{n}.branch3x3_2b", 384, 384, hw, (3, 1), 1, (1, 0))
        conv(f"{n}.branch3x3dbl_1", c, 448, hw)
        conv(f"{n}.branch3x3dbl_2", 448, 384, hw, 3, 1, 1)
        conv(f"{n}.branch3x3dbl_3a", 384, 384, hw, (1, 3), 1, (0, 1))
        conv(f"{n}.branch3x3dbl_3b", 384, 384, hw, (3, 1), 1, (1, 0))
        conv(f"{n}.branch_pool", c, 192, hw)
        c = 2048
    return out


def macs() -> int:
    """Multiply-accumulates of the 94 convolutions for ONE image: 5 711 168 096 (the 5.71 G that torchvision's model table lists for
    inception_v3 under "GFLOPS" counts multiply-accumulates, its 2 M of `fc` included)."""
    return sum(l.cin * l.cout * l.kernel[0] * l.kernel[1] * l.out_hw[0] * l.out_hw[1] for l in inception_spec())


def flops() -> float:
    """FLOPs (2 * MAC, the convention of lpips.trunk_flops) of the 94 convolutions for ONE image: 11.42e9 whatever the image's own size (the
    entry is resized to 299 x 299)."""
    return 2.0 * macs()


RAW_LEAVES = ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")


def synth_weights(seed: int = 0, raw: bool = False) -> Dict[str, np.ndarray]:
    """Seeded stand-in weights (tests and timing only; never a metric): He-scaled normal convolutions, BatchNorm gamma around 1, small beta
    and running mean, running variance around 1.  numpy PCG64 streams keyed by (seed, tensor index) like lpips.synth_weights.
    raw=False: the canonical folded dict; raw=True: pytorch-fid's own key layout (<layer>.conv.weight, <layer>.bn.*), float32."""
    sd = {}
    idx = 0
    for l in inception_spec():
        shape = (l.cout, l.cin) + l.kernel
        for leaf in RAW_LEAVES:
            rng = np.random.default_rng([seed, idx])
            idx += 1
            if leaf == "conv.weight":
                v = rng.standard_normal(shape, dtype=np.float32) * np.float32(math.sqrt(2.0 / (l.cin * l.kernel[0] * l.kernel[1])))
            elif leaf == "bn.weight":
                v = np.float32(1) + (rng.random(l.cout, dtype=np.float32) * 2 - 1) * np.float32(0.1)
            elif leaf == "bn.running_var":
                v = np.float32(1) + (rng.random(l.cout, dtype=np.float32) * 2 - 1) * np.float32(0.2)
            else:
                v = (rng.random(l.cout, dtype=np.float32) * 2 - 1) * np.float32(0.05)
            sd[f"{l.name}.{leaf}"] = np.ascontiguousarray(v, dtype=np.float32)
    return sd if raw else canonical(sd)


def fold_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """Eval-mode BatchNorm folded into the convolution in float64 and rounded once: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)."""
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    wf = np.asarray(w, np.float64) * scale[:, None, None, None]
    bf = np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * scale
    return np.ascontiguousarray(wf, dtype=np.float32), np.ascontiguousarray(bf, dtype=np.float32)


def _np(v) -> np.ndarray:
    if hasattr(v, "detach"):
        v = v.detach().cpu().float().numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


def canonical(sd) -> Dict[str, np.ndarray]:
    """pytorch-fid's raw layout (<layer>.conv.weight, <layer>.bn.{weight,bias,running_mean,running_var}; fc.*, AuxLogits.* and
    num_batches_tracked are ignored) or the already folded one (<layer>.weight, <layer>.bias) -> the folded dict, validated.
    KeyError names the first missing key, ValueError the first mis-shaped one."""
    out = {}
    for l in inception_spec():
        wshape = (l.cout, l.cin) + l.kernel

        def get(key, shape):
            if key not in sd:
                raise KeyError(f"FID Inception weights: key missing: {key}")
            a = _np(sd[key])
            if tuple(a.shape) != shape:
                raise ValueError(f"FID Inception weights: key {key}: shape {tuple(a.shape)}, expected {shape}")
            return a

        if f"{l.name}.conv.weight" in sd or f"{l.name}.weight" not in sd:
            w = get(f"{l.name}.conv.weight", wshape)
            g, b, m, v = (get(f"{l.name}.bn.{leaf}", (l.cout,)) for leaf in ("weight", "bias", "running_mean", "running_var"))
            w, b = fold_bn(w, g, b, m, v)
        else:
            w, b = get(f"{l.name}.weight", wshape), get(f"{l.name}.bias", (l.cout,))
        out[f"{l.name}.weight"], out[f"{l.name}.bias"] = w, b
    return out


def load_weights(path: str) -> Dict[str, np.ndarray]:
    """torch.load the file and return the canonical folded dict."""
    import torch
    sd = torch.load(path, map_location="cpu")
    if hasattr(sd, "state_dict"):
        sd = sd.state_dict()
    return canonical(sd)


def find_weight_file(config) -> str:
    """The file the driver loads for calc_FID: <cwd>/model_zoo/<fid_inception_path> (default: the name pytorch-fid downloads it under)."""
    return os.path.join(config.get("cwd", "") or "", "model_zoo", config.get("fid_inception_path", DEFAULT_FILE))


class FidStats:
    """Accumulates feature rows [n, d]; mu and sigma as pytorch-fid forms them (np.mean(axis=0), np.cov(rowvar=False)), float64."""

    def __init__(self):
        self.rows: List[np.ndarray] = []

    def add(self, feats):
        f = np.asarray(feats, np.float64)
        self.rows.append(f.reshape(-1, f.shape[-1]))

    def __len__(self):
        return sum(len(r) for r in self.rows)

    @property
    def features(self) -> np.ndarray:
        return np.concatenate(self.rows, 0)

    @property
    def mu(self) -> np.ndarray:
        return np.mean(self.features, axis=0)

    @property
    def sigma(self) -> np.ndarray:
        return np.atleast_2d(np.cov(self.features, rowvar=False))


def frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """pytorch-fid's calculate_frechet_distance: |mu1 - mu2|^2 + tr s1 + tr s2 - 2 tr sqrtm(s1 s2).  A non-finite square root is retried with
    eps I added to both covariances; a complex one is an error when its diagonal's imaginary part exceeds 1e-3, else its real part is taken."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError(f"frechet_distance: shapes differ: mu {mu1.shape} / {mu2.shape}, sigma {sigma1.shape} / {sigma2.shape}")
    diff = mu1 - mu2
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    if isinstance(covmean, tuple):               # older scipy returns (sqrtm, error estimate)
        covmean = covmean[0]
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
        if isinstance(covmean, tuple):
            covmean = covmean[0]
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"frechet_distance: imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def fid_from_features(a, b) -> float:
    """FID of two feature sets [n, d] (at least 2 rows each)."""
    sa, sb = FidStats(), FidStats()
    sa.add(a)
    sb.add(b)
    if len(sa) < 2 or len(sb) < 2:
        raise ValueError("fid_from_features: a covariance needs at least 2 rows per set")
    return frechet_distance(sa.mu, sa.sigma, sb.mu, sb.sigma)
