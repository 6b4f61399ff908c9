"""LPIPS v0.1, net='vgg' (host side): the VGG16 trunk's schema, weight loading and synthetic weights for dpir_lpips_load.

The reference evaluates `loss_fn_vgg = lpips.LPIPS(net='vgg')` on (x_0*2-1, img_H/255*2-1) after every batch (main_ddpir.py:250-251,
489-493).  That module is a fixed scaling layer, the 13 convolutions of torchvision's VGG16 `features` and five bias-free 1x1 heads;
the engine runs all of it (csrc/lpips.hip).  Neither `lpips` nor `torchvision` is a dependency: `load_weights` reads the two files those
packages download (torchvision's vgg16-397923af.pth and the package's weights/v0.1/vgg.pth) with torch.load, or one file holding a whole
`lpips.LPIPS(net='vgg').state_dict()`.

Canonical keys (what dpir_lpips_load takes): features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias} (OIHW) and lin{0..4}.weight [C].
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Tuple

import numpy as np

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# torchvision vgg16 cfg 'D': 64,64,M,128,128,M,256,256,256,M,512,512,512,M,512,512,512 (no pool behind the last convolution in LPIPS)
PLAN = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
TAP_AFTER_CONV = (2, 4, 7, 10, 13)                # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (1-based convolution numbers)
TAP_CHANNELS = (64, 128, 256, 512, 512)
# lpips' vgg16 wrapper copies features[0:4], [4:9], [9:16], [16:23], [23:30] into slice1..5 under their ORIGINAL indices
_SLICE_OF = {i: 1 + sum(i >= b for b in (4, 9, 16, 23)) for i in FEATURE_INDEX}


def vgg_spec() -> List[Tuple[str, Tuple[int, ...], str]]:
    """(canonical key, shape, kind) of everything dpir_lpips_load takes: 13 convolutions (kind 'w' / 'b'), then five heads ('lin')."""
    spec, cin, convs = [], 3, iter(FEATURE_INDEX)
    for c in PLAN:
        if c == "M":
            continue
        i = next(convs)
        spec.append((f"features.{i}.weight", (c, cin, 3, 3), "w"))
        spec.append((f"features.{i}.bias", (c,), "b"))
        cin = c
    for k, c in enumerate(TAP_CHANNELS):
        spec.append((f"lin{k}.weight", (c,), "lin"))
    return spec


def trunk_flops(H: int, W: int) -> float:
    """FLOPs (2 * MAC) of the 13 convolutions for ONE image at H x W (an image pair costs twice this)."""
    total, cin, h, w = 0.0, 3, H, W
    for c in PLAN:
        if c == "M":
            h, w = h // 2, w // 2
            continue
        total += 2.0 * 9 * cin * c * h * w
        cin = c
    return total


def synth_weights(seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded stand-in weights (tests and timing only; never a metric): He-scaled normal convolutions, small biases, non-negative heads.
    numpy PCG64 streams keyed by (seed, tensor index) like weights.synth_state_dict."""
    sd = {}
    for idx, (key, shape, kind) in enumerate(vgg_spec()):
        rng = np.random.default_rng([seed, idx])
        if kind == "w":
            v = rng.standard_normal(shape, dtype=np.float32) * np.float32(math.sqrt(2.0 / (shape[1] * 9)))
        elif kind == "b":
            v = (rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(0.05)
        else:
            v = rng.random(shape, dtype=np.float32) * np.float32(0.1)
        sd[key] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def _np(v) -> np.ndarray:
    if hasattr(v, "detach"):
        v = v.detach().cpu().float().numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


def canonical(sd) -> Dict[str, np.ndarray]:
    """Any of the three layouts (or the canonical one, or a merge of them) -> the canonical dict, validated.
      * torchvision vgg16:            features.N.{weight,bias}  (classifier.* is ignored)
      * lpips.LPIPS(net='vgg'):       net.slice{1..5}.N.{weight,bias}, lin{k}.model.1.weight [1,C,1,1], scaling_layer.{shift,scale}
      * the package's heads-only file: lin{k}.model.1.weight
    KeyError names the first missing key, ValueError the first mis-shaped one; scaling_layer buffers that are not the v0.1 constants
    raise ValueError (the engine's scaling layer is those constants)."""
    out = {}
    for name, const in (("shift", SHIFT), ("scale", SCALE)):
        key = f"scaling_layer.{name}"
        if key in sd:
            got = _np(sd[key]).reshape(-1)
            if got.shape != (3,) or not np.array_equal(got, np.asarray(const, np.float32)):
                raise ValueError(f"{key} = {got.tolist()} is not the LPIPS v0.1 constant {list(const)}: the engine's scaling layer is fixed")
    for key, shape, kind in vgg_spec():
        if kind == "lin":
            k = key[3]
            cands = (key, f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight")
        else:
            i, leaf = key.split(".")[1:]
            cands = (key, f"net.slice{_SLICE_OF[int(i)]}.{i}.{leaf}")
        src = next((c for c in cands if c in sd), None)
        if src is None:
            raise KeyError(f"LPIPS weights: key missing: {key} (also looked for {', '.join(cands[1:])})")
        a = _np(sd[src])
        if kind == "lin":
            if a.size != shape[0] or a.ndim not in (1, 4) or (a.ndim == 4 and a.shape != (1, shape[0], 1, 1)):
                raise ValueError(f"LPIPS weights: key {src}: shape {tuple(a.shape)}, expected [1,{shape[0]},1,1] or [{shape[0]}]")
            a = a.reshape(-1)
        elif tuple(a.shape) != shape:
            raise ValueError(f"LPIPS weights: key {src}: shape {tuple(a.shape)}, expected {shape}")
        out[key] = np.ascontiguousarray(a)
    return out


def load_weights(*paths: str) -> Dict[str, np.ndarray]:
    """torch.load every path, merge the state dicts (later files win) and return the canonical dict."""
    import torch
    merged = {}
    for p in paths:
        sd = torch.load(p, map_location="cpu")
        if hasattr(sd, "state_dict"):
            sd = sd.state_dict()
        merged.update(sd)
    return canonical(merged)


def find_weight_files(config) -> Tuple[str, ...]:
    """The files the driver loads for calc_LPIPS, under <cwd>/model_zoo: YAML keys lpips_vgg_path (default vgg16-397923af.pth, torchvision's
    trunk) and lpips_lin_path (default lpips_vgg.pth, the package's weights/v0.1/vgg.pth heads; a full LPIPS state dict here serves both).
    Returns the paths that exist, trunk first; load_weights says which key is missing when they do not hold everything."""
    zoo = os.path.join(config.get("cwd", "") or "", "model_zoo")
    trunk = os.path.join(zoo, config.get("lpips_vgg_path", "vgg16-397923af.pth"))
    lin = os.path.join(zoo, config.get("lpips_lin_path", "lpips_vgg.pth"))
    return tuple(p for p in (trunk, lin) if os.path.exists(p))
