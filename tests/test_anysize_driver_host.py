"""Host side of the any-size driver path (no GPU): modcrop against the reference's definition (utils_image.py:538-551: the top-left
H - H % sf by W - W % sf, a copy), --synthetic-size parsing, and the image loader that applies both."""
import argparse
import types

import numpy as np
import pytest

from diffpir_amd import main_ddpir as drv


def _reference_modcrop(img_in, scale):
    """utils_image.modcrop, restated"""
    img = np.copy(img_in)
    if img.ndim == 2:
        H, W = img.shape
        return img[:H - H % scale, :W - W % scale]
    if img.ndim == 3:
        H, W, C = img.shape
        return img[:H - H % scale, :W - W % scale, :]
    raise ValueError("Wrong img ndim: [{:d}].".format(img.ndim))


@pytest.mark.parametrize("shape", [(321, 481, 3), (320, 480, 3), (17, 5), (8, 8, 1), (7, 9, 3)])
@pytest.mark.parametrize("sf", [1, 2, 3, 4, 5, 8])
def test_modcrop_equals_the_reference_definition(shape, sf):
    img = np.random.default_rng(sum(shape) + sf).integers(0, 256, shape).astype(np.uint8)
    got, want = drv.modcrop(img, sf), _reference_modcrop(img, sf)
    assert got.shape == want.shape and np.array_equal(got, want) and got.dtype == np.uint8
    assert got.shape[0] % sf == 0 and got.shape[1] % sf == 0
    got[...] = 0
    assert img.any()                                                    # a copy, as np.copy in the reference
    stack = np.stack([img, img[::-1]]) if img.ndim == 3 else None       # the loader's [N,H,W,C] stacks crop the same window
    if stack is not None:
        assert np.array_equal(drv.modcrop(stack, sf)[1], _reference_modcrop(img[::-1], sf))


def test_modcrop_rejects_other_ranks():
    with pytest.raises(ValueError):
        drv.modcrop(np.zeros(5), 2)


def test_synthetic_size_parsing():
    assert drv.parse_size("192x320") == (192, 320) and drv.parse_size("96X160") == (96, 160) and drv.parse_size("64") == (64, 64)
    for bad in ("", "x", "12x", "3x4x5", "-4x8", "0x16", "axb", "1.5x2"):
        with pytest.raises(argparse.ArgumentTypeError):
            drv.parse_size(bad)


class _Cfg(types.SimpleNamespace):
    def get(self, k, d=None):
        return getattr(self, k, d)


def test_load_images_synthetic_size_and_crop(tmp_path):
    cfg = _Cfg(cwd=str(tmp_path), testset_name="none", sf=3)
    imgs, names = drv.load_images(cfg, 2, (50, 64))
    assert imgs.shape == (2, 48, 63, 3) and imgs.dtype == np.uint8 and len(names) == 2
    full, _ = drv.load_images(_Cfg(cwd=str(tmp_path), testset_name="none", sf=1), 2, (50, 64))
    assert full.shape == (2, 50, 64, 3) and np.array_equal(full[:, :48, :63], imgs)
    assert drv.load_images(_Cfg(cwd=str(tmp_path), testset_name="none", sf=1), 1)[0].shape == (1, 256, 256, 3)      # the default stays 256 x 256
