"""YAML-driven batched driver with the reference's config surface (main_ddpir.py:127-169, 172-599), on the engine.

    python -m diffpir_amd.main_ddpir --opt <config.yaml> [--synthetic N] [--synthetic-size HxW] [--device 0] [--num-gpus G]

--num-gpus G (or the YAML key `num_gpus`) re-launches the driver as G processes, one per GPU (torch.distributed.run); every batch
is then block-partitioned over the ranks (dist.restore_sharded) and one all-gather of the uint8 results ends it.

Accepts the reference's configs/*.yaml unchanged.  What it keeps from the reference driver: the derived fields
(noise_level_img/255, sigma = max(0.001, .), kernel_std), the per-task lambda/zeta sweeps (main_ddpir.py:548-580),
the per-image degradation recipe (main_ddpir.py:46-117) and the batch PSNR log line.  What it does differently:
the loop body is one engine call (restore.restore_batch), images are read / written with PIL when available (cv2
is not installed here), LPIPS is computed by the engine (dpir_lpips) from the two weight files under <cwd>/model_zoo when `calc_LPIPS`
is set and they are there (one WARNING and no LPIPS otherwise: never a metric on synthetic weights), and the batch's LPIPS is the mean over
its images (the reference keeps image 0's score times the batch size, main_ddpir.py:491: the same thing at batch_size 1).  `calc_FID: true` (an engine
key: the reference leaves FID to pytorch-fid on the saved images) accumulates the FID Inception features of every restored batch and of the ground
truth (dpir_fid_features) and logs the Frechet distance per sweep point, when model_zoo holds pytorch-fid's weight file.  `calc_SSIM: true`
(an engine key, no weight file) adds the 8-bit protocol of the reference's standalone programs (dpir_metrics_u8): PSNR and SSIM of the uint8 result, RGB and
Y, with the border cropped first (sf for task sr, else 0; `metrics_border` overrides), per batch and per sweep point.
`engine_save_results: true` (an engine key, default false) makes the driver honour the reference's `save_E` / `save_L` / `save_LEH`: the restored
image, the measurement, the L / E / H strip and, for task deblur, the kernel picture are written under results/<result_name>/ with the reference's
file names (result_file_names; dpir_result_panels builds the L and LEH bytes), encoded by a small thread pool while the next batch runs.  With no
dataset / checkpoint on disk it falls back to synthetic ground truth and synthetic weights, saying so in the log.
"""
from __future__ import annotations

import argparse
import glob
import logging
import os
import queue
import threading
import time

import numpy as np
import yaml

from . import restore, synth, script_util, utils_model, weights, degrade as dgr, lpips as lpips_host, fid as fid_host
from .engine import Engine
from .utils_inpaint import mask_generator

log = logging.getLogger("diffpir_amd")


class Config:
    def __init__(self, dictionary):
        for k, v in dictionary.items():
            setattr(self, k, Config(v) if isinstance(v, dict) else v)

    def get(self, k, default=None):
        return getattr(self, k, default)


def parse_config(path):
    with open(path, "r") as f:
        config = Config(yaml.safe_load(f))
    config.opt = path
    config.noise_level_img = config.noise_level_img / 255.0              # main_ddpir.py:138
    config.noise_level_model = config.noise_level_img                    # :140
    config.sigma = max(0.001, config.noise_level_img)                    # :141
    if config.task == "deblur":
        config.kernel_std = 3.0 if config.blur_mode == "Gaussian" else 0.5   # :151
    if config.task == "inpaint":
        assert config.generate_mode in ["DiffPIR", "repaint", "vanilla"]
    for k, d in dict(sr_mode="blur", inIter=1, gamma=0.01, sf=1).items():
        if not hasattr(config, k):
            setattr(config, k, d)
    return config


def loop_config(config, lambda_, zeta) -> restore.LoopConfig:
    return restore.LoopConfig(task=config.task, iter_num=config.iter_num, noise_level_img=config.noise_level_img,
                              lambda_=lambda_, zeta=zeta, eta=config.eta, guidance_scale=config.guidance_scale,
                              sf=config.sf, sr_mode=config.sr_mode, inIter=config.inIter, gamma=config.gamma,
                              skip_type=config.skip_type, num_train_timesteps=config.num_train_timesteps,
                              beta_start=config.beta_start, beta_end=config.beta_end, generate_mode=config.generate_mode,
                              model_output_type=config.model_output_type, sub_1_analytic=config.sub_1_analytic,
                              ddim_sample=config.ddim_sample, iter_num_U=config.iter_num_U,
                              noise_init_img=config.get("noise_init_img", "max"),
                              skip_noise_model_t=bool(config.get("skip_noise_model_t", False)),
                              driver=config.get("driver", "main_ddpir"))


def sweeps(config):
    """main_ddpir.py:548-580."""
    if config.task == "sr":
        return [(config.lambda_ * i, config.zeta) for i in range(2, 13)]
    if config.task == "deblur":
        return [(config.lambda_ * 7, config.zeta * 3)]
    return [(config.lambda_ * 1, config.zeta * 1)]


def flatten_sweeps(n_points: int, n_images: int, batch_size: int):
    """`engine_batch_sweeps: true`: the (sweep point, image) pairs of the whole test set in the order the sequential driver visits them (point by
    point, main_ddpir.py:548-580; image by image inside a point), cut into batches of batch_size.  Returns a list of lists of (point, image)."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    pairs = [(s, g) for s in range(n_points) for g in range(n_images)]
    return [pairs[j:j + batch_size] for j in range(0, len(pairs), batch_size)]


def regroup_sweeps(batches, values, n_points: int, n_images: int):
    """The inverse of flatten_sweeps for per-pair results: values[b][j] belongs to pair batches[b][j]; returns [n_points][n_images], each point's
    values in image order."""
    out = [[None] * n_images for _ in range(n_points)]
    for pairs, vals in zip(batches, values):
        if len(pairs) != len(vals):
            raise ValueError(f"a batch of {len(pairs)} pairs came back with {len(vals)} values")
        for (s, g), v in zip(pairs, vals):
            out[s][g] = v
    if any(v is None for row in out for v in row):
        raise ValueError("regroup_sweeps: some (point, image) pair has no value")
    return out


def image_runs(images):
    """[(first image, count)] of the maximal runs of consecutive image numbers in `images` (distinct, in visiting order): each run is degraded by
    one dgr.degrade call with image_offset = its first image, exactly as a batch of the sequential driver is."""
    runs = []
    for g in images:
        if runs and runs[-1][0] + runs[-1][1] == g:
            runs[-1][1] += 1
        else:
            runs.append([g, 1])
    return [tuple(r) for r in runs]


def check_batch_sweeps(config):
    """What `engine_batch_sweeps: true` cannot do, refused before any work starts."""
    if config.get("engine_noise", "device") != "device":
        raise ValueError("engine_batch_sweeps needs engine_noise: device -- the reference's one global generator would have to be drawn for every "
                         "sweep point up front (about 8 GB for the super-resolution sweep)")
    if progress_options(config)[0]:
        raise ValueError("engine_batch_sweeps with save_progressive / log_process: the strips' file names carry one lambda, a batch holds several")
    if bool(config.get("calc_FID", False)):
        raise ValueError("engine_batch_sweeps with calc_FID: a batch mixes the images of several sweep points, FID is one number per point's whole set "
                         "(run the sweep point by point: engine_batch_sweeps: false)")
    restore.check_per_image(loop_config(config, *sweeps(config)[0]), restore.PerImage(lambda_=[], zeta=[]))


def setup_lpips(eng, config) -> bool:
    """calc_LPIPS (main_ddpir.py:542-545): load the VGG16 trunk and the LPIPS heads once.  False -- after ONE warning -- when the key is off
    or the weight files are not under <cwd>/model_zoo; the run then continues exactly as without the key."""
    if not bool(config.get("calc_LPIPS", False)):
        return False
    paths = lpips_host.find_weight_files(config)
    try:
        if not paths:
            raise FileNotFoundError("no weight file found")
        eng.load_lpips(lpips_host.load_weights(*paths))
    except (FileNotFoundError, KeyError) as ex:
        log.warning("calc_LPIPS: LPIPS is not computed -- %s.  It needs model_zoo/%s (torchvision's VGG16) and model_zoo/%s (the lpips package's "
                    "weights/v0.1/vgg.pth) under cwd=%r; see INTEGRATION.md", ex, config.get("lpips_vgg_path", "vgg16-397923af.pth"),
                    config.get("lpips_lin_path", "lpips_vgg.pth"), config.get("cwd", ""))
        return False
    return True


def setup_fid(eng, config, n_images) -> bool:
    """calc_FID: load the FID Inception-v3 once.  False -- after ONE warning -- when the weight file is not under <cwd>/model_zoo or the test
    set has fewer than 2 images (no covariance); False without a word when the key is off.  The run then continues exactly as without the key."""
    if not bool(config.get("calc_FID", False)):
        return False
    if n_images < 2:
        log.warning("calc_FID: FID is not computed -- the test set has %d image(s), a covariance needs at least 2", n_images)
        return False
    path = fid_host.find_weight_file(config)
    try:
        if not os.path.exists(path):
            raise FileNotFoundError("weight file not found")
        eng.load_fid(fid_host.load_weights(path))
    except (FileNotFoundError, KeyError) as ex:
        log.warning("calc_FID: FID is not computed -- %s.  It needs %s (pytorch-fid's FID Inception weights, YAML key fid_inception_path) under "
                    "cwd=%r; see INTEGRATION.md", ex, os.path.join("model_zoo", config.get("fid_inception_path", fid_host.DEFAULT_FILE)), config.get("cwd", ""))
        return False
    return True


def fid_rows(eng, img_u8_dev, n_local, n_b, ddist, rank, world):
    """float64 [n_b, 2048]: the FID Inception features of the batch's images (this rank's shard through dpir_fid_features, then gathered the way
    the metric rows are)."""
    local = dgr.fid_features(eng, img_u8_dev).astype(np.float64) if n_local else np.zeros((0, fid_host.FEATURES))
    return ddist.all_gather_results(local.reshape(-1, fid_host.FEATURES), n_b, rank, world, engine=eng)


def ssim_border(config):
    """calc_SSIM (an engine key): None when it is off, else the border the 8-bit metrics crop first -- the reference's rule, sf for task sr and 0
    otherwise (main_ddpir.py:552, 564, 573), unless the optional key metrics_border overrides it."""
    if not bool(config.get("calc_SSIM", False)):
        return None
    override = config.get("metrics_border", None)
    if override is not None:
        return int(override)
    return int(config.sf) if config.task == "sr" else 0


U8_NAMES = ("PSNR(8-bit RGB)", "PSNR(8-bit Y)", "SSIM(RGB)", "SSIM(Y)")
U8_UNITS = ("dB", "dB", "", "")


def metric_rows(eng, out_f32, gt_dev, with_lpips, border=None):
    """float64 [n, 2 or 3 (+ 4)]: per-image PSNR, PSNR-Y [, LPIPS] (dpir_metrics, dpir_lpips) and, with calc_SSIM (border not None), the four
    8-bit columns PSNR, PSNR-Y, SSIM, SSIM-Y of dpir_metrics_u8 behind them."""
    cols = list(dgr.metrics(eng, out_f32, gt_dev))
    if with_lpips:
        cols.append(dgr.lpips(eng, out_f32, gt_dev))
    if border is not None:
        cols.extend(dgr.metrics_u8(eng, out_f32, gt_dev, border))
    return np.stack(cols, 1).astype(np.float64)


def log_batch_u8(number, values):
    """calc_SSIM: the batch's means of the four 8-bit columns, one line each, behind the batch line."""
    for name, unit, v in zip(U8_NAMES, U8_UNITS, values):
        log.info("batch%4d--> %s: %.4f%s", number, name, v, unit)


def log_average_u8(config, sums, n):
    for name, unit, v in zip(U8_NAMES, U8_UNITS, sums):
        log.info("-----------> Average %s of (%s) scale factor: (%d), sigma: (%.3f): %.4f%s",
                 name, config.testset_name, config.sf, config.noise_level_model, v / n, " dB" if unit else "")


def run_batched_sweeps(eng, config, points, imgs, ddist, rank, world, use_graph, cache, with_lpips=False, border=None, names=None, rw=None):
    """The sweep loop of main() flattened into full batches (YAML `engine_batch_sweeps: true`): every batch holds batch_size (point, image) pairs
    and runs as ONE restore_batch call with per-image (lambda, zeta) and the images' global numbers as noise keys.  Each distinct image of a batch
    is degraded once, with the seed and image_offset the sequential driver uses, and its y / k / mask / ground-truth rows are gathered on the
    device.  Logs and returns what the sequential loop does: one average PSNR per point, in the same order.  rw (engine_save_results): one E file
    per (point, image) row -- the names carry lambda and zeta -- L and the kernel picture at each image's first point, the strip at its last."""
    n_img, bs = len(imgs), config.batch_size
    H, W = imgs.shape[1], imgs.shape[2]
    batches = flatten_sweeps(len(points), n_img, bs)
    cfg = loop_config(config, *points[0])
    values, t0 = [], time.time()
    ncol = (3 if with_lpips else 2) + (4 if border is not None else 0)

    def gather(parts, rows):
        """device rows: rows[j] = (part index, row inside it) -> one DeviceArray [len(rows), ...] (dpir_d2d per row), or None"""
        if parts[0] is None:
            return None
        out = eng.empty((len(rows),) + parts[0].shape[1:], parts[0].dtype)
        nb = out.nbytes // len(rows)
        for j, (q, r) in enumerate(rows):
            eng._check(eng.lib.dpir_d2d(eng.h, out.ptr + j * nb, parts[q].ptr + r * nb, nb))
        return out

    for pairs in batches:
        lo, hi = ddist.shard_range(len(pairs), rank, world)
        mine = pairs[lo:hi]
        wanted = {g for _, g in mine}
        u8_local = eng.empty((hi - lo, H, W, 3), np.uint8)
        per_img = np.zeros((0, ncol))
        where, ys, ks, ms, gts, khs = {}, [], [], [], [], []
        for g0, cnt in image_runs(list(dict.fromkeys(g for _, g in pairs))):
            k_all, mask_all = make_operators(config, cnt, g0, H, W)          # every rank draws every operator of the batch (seeded numpy)
            if not wanted & set(range(g0, g0 + cnt)):
                continue
            y, ops = dgr.degrade(eng, config.task, imgs[g0:g0 + cnt], k=k_all, mask=mask_all, noise_level_img=config.noise_level_img, sf=config.sf,
                                 sr_mode=config.sr_mode, seed=config.seed + 1, image_offset=g0)
            for r in range(cnt):
                where[g0 + r] = (len(ys), r)
            ys.append(y); ks.append(ops.get("k")); ms.append(ops.get("mask")); gts.append(ops["gt"]); khs.append(k_all)
        if mine:
            rows = [where[g] for _, g in mine]
            pi = restore.PerImage(lambda_=[points[s][0] for s, _ in mine], zeta=[points[s][1] for s, _ in mine], image_index=[g for _, g in mine])
            y_rows, gt_rows = gather(ys, rows), gather(gts, rows)
            out_f32 = restore.restore_batch(eng, cfg, y_rows, k=gather(ks, rows), mask=gather(ms, rows), noise_source="device",
                                            seed=config.seed, use_graph=use_graph, out_u8=u8_local, _cache=cache,
                                            skip_dead_final_eval=bool(config.get("engine_skip_dead_final_eval", False)), per_image=pi)
            per_img = metric_rows(eng, out_f32, gt_rows, with_lpips, border)
            if rw is not None:
                save_results(eng, config, rw, [names[g] for _, g in mine], pi.lambda_, pi.zeta, y_rows, u8_local, gt_rows,
                             None if khs[0] is None else np.stack([khs[q][r] for q, r in rows]),
                             first=[s == 0 for s, _ in mine], last=[s == len(points) - 1 for s, _ in mine])
        ddist.all_gather_results(u8_local, len(pairs), rank, world, engine=eng)           # the one collective of the path
        allm = ddist.all_gather_results(per_img.reshape(-1, ncol), len(pairs), rank, world, engine=eng)
        values.append([tuple(v) for v in allm])
    if rw is not None:
        rw.drain()                         # the images/s figure includes saving
    dt = time.time() - t0
    results = []
    for (lambda_, zeta), per_point in zip(points, regroup_sweeps(batches, values, len(points), n_img)):
        if rank == 0:
            log.info("eta:%s, zeta:%s, lambda:%s, guidance_scale:%s", config.eta, zeta, lambda_, config.guidance_scale)
        psnrs, psnrs_y, lps, u8s = [], [], [], np.zeros(4)
        for i0 in range(0, n_img, bs):             # the sequential driver's batches of this point: the same averages, the same log lines
            chunk = np.asarray(per_point[i0:i0 + bs], np.float64)
            p, p_y = float(np.mean(chunk[:, 0])), float(np.mean(chunk[:, 1]))
            psnrs.append(p * len(chunk))
            psnrs_y.append(p_y * len(chunk))
            if with_lpips:
                lps.append(float(np.mean(chunk[:, 2])) * len(chunk))
            if rank == 0:
                log_batch(i0 // bs + 1, p, lps[-1] / len(chunk) if with_lpips else None, sum(lps) / n_img)
            if border is not None:
                u8 = np.mean(chunk[:, -4:], axis=0)
                u8s += u8 * len(chunk)
                if rank == 0:
                    log_batch_u8(i0 // bs + 1, u8)
        if rank == 0:
            log.info("-----------> Average PSNR(RGB) of (%s) scale factor: (%d), sigma: (%.3f): %.4f dB  [%.2f images/s on %d GPU(s)]",
                     config.testset_name, config.sf, config.noise_level_model, sum(psnrs) / n_img, len(points) * n_img / dt, world)
            log.info("-----------> Average PSNR(Y) of (%s) scale factor: (%d), sigma: (%.3f): %.4f dB",
                     config.testset_name, config.sf, config.noise_level_model, sum(psnrs_y) / n_img)
            if with_lpips:
                log.info("-----------> Average LPIPS of (%s) scale factor: (%d), sigma: (%.3f): %.4f",
                         config.testset_name, config.sf, config.noise_level_model, sum(lps) / n_img)
            if border is not None:
                log_average_u8(config, u8s, n_img)
        results.append(sum(psnrs) / n_img)
    return results


def log_batch(number, psnr, lpips_score, ave_lpips):
    """The batch line of main_ddpir.py:493 / :495.  `ave LPIPS` is the running sum over the WHOLE test set's image count, as in the reference."""
    if lpips_score is None:
        log.info("batch%4d--> PSNR: %.4fdB", number, psnr)
    else:
        log.info("batch%4d--> PSNR: %.4fdB; LPIPS: %.4f; ave LPIPS: %.4f", number, psnr, lpips_score, ave_lpips)


def modcrop(img, sf):
    """util.modcrop (utils_image.py:538, main_ddpir.py:82): the top-left H - H % sf by W - W % sf of an image [H,W] or [H,W,C] (here also a
    stack [N,H,W,C]), copied."""
    a = np.asarray(img)
    if a.ndim not in (2, 3, 4):
        raise ValueError(f"Wrong img ndim: [{a.ndim}].")
    ax = 1 if a.ndim == 4 else 0
    H, W = a.shape[ax], a.shape[ax + 1]
    idx = [slice(None)] * a.ndim
    idx[ax], idx[ax + 1] = slice(0, H - H % sf), slice(0, W - W % sf)
    return np.copy(a[tuple(idx)])


def parse_size(text):
    """--synthetic-size: 'HxW' (or one number for a square) -> (H, W)"""
    parts = str(text).lower().split("x")
    if len(parts) not in (1, 2) or not all(p.strip().isdigit() for p in parts):
        raise argparse.ArgumentTypeError(f"expected HxW, e.g. 192x320 (got {text!r})")
    h, w = int(parts[0]), int(parts[-1])
    if h < 1 or w < 1:
        raise argparse.ArgumentTypeError(f"expected a positive HxW (got {text!r})")
    return h, w


def load_images(config, n_synth, synth_size=(256, 256)):
    """uint8 [N,H,W,3] (what util.imread_uint returns, main_ddpir.py:84) + names, each image cropped to a multiple of sf (util.modcrop,
    main_ddpir.py:82).  testsets/<testset_name>/*.png via PIL when present, else synthetic."""
    sf = int(config.get("sf", 1) or 1)
    d = os.path.join(config.get("cwd", "") or "", "testsets", config.testset_name)
    paths = sorted(glob.glob(os.path.join(d, "*.png")) + glob.glob(os.path.join(d, "*.jpg")))
    if paths and not n_synth:
        try:
            from PIL import Image
            imgs = [modcrop(np.asarray(Image.open(p).convert("RGB"), np.uint8), sf) for p in paths]
            return np.stack(imgs), [os.path.basename(p) for p in paths]
        except Exception as ex:   # pragma: no cover
            log.warning("cannot read %s (%s); using synthetic images", d, ex)
    n = n_synth or 16
    sh, sw = synth_size
    log.info("no dataset on disk: using %d synthetic %dx%d ground-truth images", n, sh, sw)
    f = synth.smooth_images(n, sh, sw, 42)
    return modcrop(np.ascontiguousarray((f * 255.0).round().astype(np.uint8).transpose(0, 2, 3, 1)), sf), [f"synth_{i:04d}.png" for i in range(n)]


_MAT_CACHE = {}


def load_reference_kernels(config, name):
    """kernels/<name>.mat of the reference tree (main_ddpir.py:54, 71: hdf5storage.loadmat(...)['kernels']) -> object array [1, n] of 2-D
    float arrays, or None when the file is not under <cwd>/kernels.  The two v5 files are read with scipy; Levin09.mat is v7.3 (HDF5):
    h5py if importable, else a `<name>.npz` beside it (tools/convert_mat_v73.py writes it under an interpreter that has h5py)."""
    path = os.path.join(config.get("cwd", "") or "", "kernels", name + ".mat")
    if path in _MAT_CACHE:
        return _MAT_CACHE[path]
    cell = None
    if os.path.exists(path):
        try:
            import scipy.io
            cell = scipy.io.loadmat(path)["kernels"]
        except NotImplementedError:
            try:
                import h5py
                with h5py.File(path, "r") as f:
                    refs = f["kernels"]
                    ks = [np.array(f[refs[i, 0]]).T for i in range(refs.shape[0])]     # MATLAB is column-major: h5py sees the transpose
            except ImportError:
                side = os.path.splitext(path)[0] + ".npz"
                if not os.path.exists(side):
                    raise RuntimeError(f"{path} is a MATLAB v7.3 (HDF5) file and h5py is not importable here: convert it once with "
                                       f"`<python with h5py> tools/convert_mat_v73.py {path}` (writes {side})")
                z = np.load(side)
                ks = [z[f"k{i}"] for i in range(len(z.files))]
            cell = np.empty((1, len(ks)), dtype=object)
            for i, kk in enumerate(ks):
                cell[0, i] = kk
    _MAT_CACHE[path] = cell
    return cell


def make_operators(config, n, idx0, H, W):
    """Per-image PSFs / masks of CustomDataset.__getitem__ (main_ddpir.py:52-110): a few hundred scalar operations per image
    under the numpy RNG, kept on the host so that they stay bit-identical to the reference's.  Returns (k, mask) numpy or None."""
    k = mask = None
    if config.task == "deblur" and not config.get("use_DIY_kernel", True):
        # main_ddpir.py:69-72: k_index = 0 of kernels/Levin09.mat, float32, the same PSF for every image
        cell = load_reference_kernels(config, "Levin09")
        if cell is None:
            raise FileNotFoundError("use_DIY_kernel: false needs kernels/Levin09.mat under `cwd` (main_ddpir.py:71); it is not there")
        k = np.broadcast_to(cell[0, 0].astype(np.float32), (n, 1) + cell[0, 0].shape).copy()
    elif config.task == "deblur":
        ks = []
        for b in range(n):
            np.random.seed(seed=(idx0 + b) * 10)                            # main_ddpir.py:59
            if config.blur_mode == "Gaussian":
                ks.append(synth.gaussian_psf(config.kernel_size, config.kernel_std * np.abs(np.random.rand() * 2 + 1)))
            else:
                ks.append(synth.motion_psf(config.kernel_size, seed=idx0 + b))
        k = np.stack(ks)[:, None].astype(np.float32)
    elif config.task == "sr":
        # main_ddpir.py:53-56: kernels_bicubicx234.mat[0, sf - 2] (index 2 for sf >= 5)
        cell = load_reference_kernels(config, "kernels_bicubicx234")
        if cell is not None:
            kk = cell[0, config.sf - 2 if config.sf < 5 else 2].astype(np.float64).astype(np.float32)
        else:
            if config.sf != 4:
                raise FileNotFoundError(f"task sr, sf = {config.sf}: kernels/kernels_bicubicx234.mat is not under `cwd` and the built-in stand-in exists for sf = 4 only")
            if not _MAT_CACHE.get("warned"):
                log.warning("kernels/kernels_bicubicx234.mat not found under cwd=%r: using the ANALYTIC x4 bicubic PSF stand-in (differs from the "
                            "reference's file by up to 1.9e-3 per tap, 3 %% of the peak) -- results will not match a reference run", config.get("cwd", ""))
                _MAT_CACHE["warned"] = True
            kk = synth.bicubic_psf_x4()
        k = np.broadcast_to(kk, (n, 1) + kk.shape).copy()
    elif config.get("load_mask", False):
        # main_ddpir.py:103-104: ONE mask image for every test image, `imread_uint(mask_path, n_channels).astype(bool)`
        mask = load_mask_image(config, H, W)
        mask = np.broadcast_to(mask, (n,) + mask.shape[1:]).copy()
    else:
        gen = mask_generator(config.mask_type, config.mask_len_range, config.mask_prob_range)
        mask = np.concatenate([gen((1, 3, H, W)) for _ in range(n)], 0)
    return k, mask


def load_mask_image(config, H, W):
    """`load_mask: true` (main_ddpir.py:103-104): util.imread_uint(mask_path, n_channels) -> astype(bool): any non-zero byte keeps the pixel.
    Returns uint8 {0, 1} [1, 3, H, W].  A relative mask_path is looked up under `cwd` like the reference's other inputs; a mask whose size differs
    from the images is an error (the reference would fail at `img_H * mask`)."""
    path = config.get("mask_path", "")
    if not path:
        raise ValueError("load_mask: true needs mask_path (main_ddpir.py:104)")
    if not os.path.isabs(path) and not os.path.exists(path):
        path = os.path.join(config.get("cwd", ""), path)
    if path.endswith(".npy"):
        m = np.load(path)
    else:
        from PIL import Image
        m = np.asarray(Image.open(path).convert("RGB"), np.uint8)          # imread_uint(n_channels=3): grey images are replicated (utils_image.py:190-199)
    if m.ndim == 2:
        m = np.repeat(m[:, :, None], 3, axis=2)
    if m.shape[:2] != (H, W) or m.shape[2] != 3:
        raise ValueError(f"mask {path}: shape {m.shape}, the test images are {H} x {W} x 3 (main_ddpir.py:109 multiplies them elementwise)")
    return np.ascontiguousarray((m != 0).astype(np.uint8).transpose(2, 0, 1)[None])


def progress_options(config):
    """(save_progressive, save_progressive_mask, log_process): the reference's three switches (main_ddpir_deblur.py:46, 53;
    main_ddpir_inpainting.py:48-49, 63), all off unless the YAML says otherwise.  log_process logs inside the `if save_progressive` block
    (main_ddpir_deblur.py:361-368), so it needs save_progressive; save_progressive_mask is read by the standalone inpainting program only, for
    generate_mode repaint and DiffPIR (main_ddpir_inpainting.py:352, 364, 370)."""
    save = bool(config.get("save_progressive", False))
    driver = config.get("driver", "main_ddpir")
    mask = save and bool(config.get("save_progressive_mask", False)) and driver == "main_ddpir_inpainting" and config.task == "inpaint" \
        and config.generate_mode in ("repaint", "DiffPIR")
    return save, mask, save and bool(config.get("log_process", False))


def result_dir(config):
    """E_path of main_ddpir.py:146-158: <results>/<result_name>, under `cwd`."""
    name = (f"{config.testset_name}_{config.task}_{config.generate_mode}_{config.model_name}_sigma{config.noise_level_img}_NFE{config.iter_num}"
            f"_eta{config.eta}_zeta{config.zeta}_lambda{config.lambda_}")
    if config.task == "sr":
        name += f"_{config.sr_mode}{config.sf}"
    elif config.task == "deblur":
        name += f"_blurmode_{config.blur_mode}"
    else:
        name += f"_mask_type_{config.get('mask_type', 'loaded')}"
    return os.path.join(config.get("cwd", "") or "", config.get("results", "results"), name)


def progress_file_names(config, img_name, ext, lambda_, current_time, psnr):
    """(process strip, masked process strip) file names: main_ddpir_inpainting.py:359, 371 under driver main_ddpir_inpainting,
    main_ddpir_deblur.py:406 (= main_ddpir_sisr.py:432) under the other two."""
    if config.get("driver", "main_ddpir") == "main_ddpir_inpainting":
        return (img_name + "_process_lambda_{:.3f}_{}{}".format(lambda_, current_time, ext),
                img_name + "_process_mask_lambda_{:.3f}_{}{}".format(lambda_, current_time, ext))
    return (img_name + "_sigma_{:.3f}_process_lambda_{:.3f}_{}_psnr_{:.4f}{}".format(config.noise_level_img, lambda_, current_time, psnr, ext), None)


def write_png(path, img_u8):
    """uint8 [H,W,3] (RGB) or [H,W] (mode L, one channel: the kernel picture) -> the image file `path` names through PIL (cv2, the reference's
    writer, is not a dependency).  The format follows the extension, as with cv2.imwrite: only a lossless one (.png) gives back the bytes."""
    from PIL import Image
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(np.ascontiguousarray(img_u8)).save(path)        # a 2-D uint8 array becomes mode L, [H,W,3] mode RGB


def result_options(config):
    """(save_E, save_L, save_LEH, kernel picture).  The engine key engine_save_results (default false) arms the reference's three switches
    (main_ddpir.py:497, 510; main_ddpir_deblur.py:43-45): with it off all four are off, whatever the YAML's save_* keys say.  The kernel picture
    (main_ddpir.py:299, main_ddpir_deblur.py:177) goes with task deblur whenever one of the three is on."""
    if not bool(config.get("engine_save_results", False)):
        return False, False, False, False
    e, l, leh = bool(config.get("save_E", False)), bool(config.get("save_L", False)), bool(config.get("save_LEH", False))
    return e, l, leh, config.task == "deblur" and (e or l or leh)


def result_file_names(config, full_name, lambda_, zeta):
    """(E, L, LEH, kernel picture) file names of one image, `full_name` being its file name with the extension; the kernel's is None unless the
    task is deblur.
      driver main_ddpir              main_ddpir.py:499, 511, 299 (imsave_batch puts its prefix in front of the whole file name, utils_image.py:168-173);
                                     that program has no save_LEH: the strip takes the standalone programs' names, main_ddpir_deblur.py:421 for
                                     deblur and sr, main_ddpir_inpainting.py:347 for inpaint
      driver main_ddpir_deblur       main_ddpir_deblur.py:398, 424, 421, 177
      driver main_ddpir_inpainting   main_ddpir_inpainting.py:341, 344, 347 (no underscore in front of the model name of the strip)"""
    img_name, ext = os.path.splitext(full_name)
    driver = config.get("driver", "main_ddpir")
    kernel = f"motion_kernel_{img_name}{ext}" if config.task == "deblur" else None
    if driver == "main_ddpir_inpainting" or (driver == "main_ddpir" and config.task == "inpaint"):
        leh = img_name + config.model_name + "_LEH" + ext
    else:
        leh = img_name + "_LEH" + ext
    if driver == "main_ddpir":
        return (f"{config.model_name}_x{config.sf}_lambda{lambda_:.4f}_zeta{zeta:.4f}_" + full_name, f"LR_x{config.sf}_" + full_name, leh, kernel)
    est = img_name + "_" + config.model_name + ext
    return est, img_name + ("_L" if driver == "main_ddpir_inpainting" else "_LR") + ext, leh, kernel


def kernel_picture(k):
    """uint8 [kh,kw]: what cv2.imwrite makes of the float array k * 255. * 200 (main_ddpir.py:299, main_ddpir_deblur.py:177) -- saturate to
    [0, 255], round half to even -- evaluated in float64 on the host.  One channel."""
    return np.rint(np.clip(np.asarray(k, np.float64) * 255. * 200, 0, 255)).astype(np.uint8)


class ResultWriter:
    """A bounded pool of threads around write_png: the files of one batch are encoded while the next batch's loop runs.  The worker count is
    fixed (at most 8, never derived from the machine's CPU count); the queue holds at most two batches of files and submit() blocks when it
    is full.  drain() waits until everything submitted is on disk and re-raises the first error a worker met; close() ends the threads."""
    MAX_WORKERS = 8

    def __init__(self, files_per_batch, workers=4, writer=write_png):
        self.writer = writer
        self.q = queue.Queue(maxsize=max(1, 2 * int(files_per_batch)))
        self.error, self.lock = None, threading.Lock()
        self.threads = [threading.Thread(target=self._work, name=f"result-writer-{i}", daemon=True)
                        for i in range(max(1, min(int(workers), self.MAX_WORKERS)))]
        for t in self.threads:
            t.start()

    def _work(self):
        while True:
            item = self.q.get()
            try:
                if item is None:
                    return
                self.writer(*item)
            except BaseException as ex:        # kept for drain(); the worker goes on so that the queue never stalls
                with self.lock:
                    if self.error is None:
                        self.error = ex
            finally:
                self.q.task_done()

    def submit(self, path, array):
        self.q.put((path, array))

    def drain(self):
        self.q.join()
        with self.lock:
            err, self.error = self.error, None
        if err is not None:
            self.close()
            raise err

    def close(self):
        for _ in self.threads:
            self.q.put(None)
        for t in self.threads:
            t.join()
        self.threads = []


def emit_results(config, names, lambdas, zetas, est_u8=None, L_u8=None, leh_u8=None, k=None, submit=write_png, first=None, last=None):
    """The files the reference saves after one batch (main_ddpir.py:299, 497-511; main_ddpir_deblur.py:177, 397-424;
    main_ddpir_inpainting.py:340-347), for the rows of the batch: est_u8 [n,H,W,3], L_u8 [n,h,w,3], leh_u8 [n,H,3W,3] (degrade.result_panels),
    k [n,1,kh,kw] host PSFs.  lambdas / zetas: one number, or one per row (engine_batch_sweeps).  first[j] / last[j] (default all true): row j is
    its image's first / last sweep point -- L and the kernel picture are written at the first, the strip, whose name carries no lambda, at the
    last, as the point-by-point driver leaves them.  Every file goes through submit(path, array).  Nothing is written, and submit is never
    called, unless engine_save_results is on.  Returns the paths."""
    save_E, save_L, save_LEH, save_k = result_options(config)
    if not (save_E or save_L or save_LEH):
        return []
    n = len(names)
    lambdas = [lambdas] * n if np.ndim(lambdas) == 0 else list(lambdas)
    zetas = [zetas] * n if np.ndim(zetas) == 0 else list(zetas)
    out_dir, paths = result_dir(config), []

    def put(name, array):
        paths.append(os.path.join(out_dir, name))
        submit(paths[-1], array)
    for j, full in enumerate(names):
        e_name, l_name, leh_name, k_name = result_file_names(config, full, lambdas[j], zetas[j])
        is_first, is_last = first is None or first[j], last is None or last[j]
        if save_k and k is not None and is_first:
            put(k_name, kernel_picture(np.asarray(k[j]).reshape(np.asarray(k[j]).shape[-2:])))
        if save_E:
            put(e_name, est_u8[j])
        if save_L and is_first:
            put(l_name, L_u8[j])
        if save_LEH and is_last:
            put(leh_name, leh_u8[j])
    return paths


def save_results(eng, config, rw, names, lambdas, zetas, y, est_u8_dev, gt_dev, k, first=None, last=None):
    """One batch's saved files from the device arrays of its loop: the L and LEH bytes through degrade.result_panels (dpir_result_panels) when
    asked for, E from the loop's out_u8, the kernel picture from the host PSFs; all handed to the writer pool."""
    save_E, save_L, save_LEH, _ = result_options(config)
    # L is used at an image's first sweep point only, the strip at its last: a batch of middle points computes and downloads neither
    want_L = save_L and (first is None or any(first))
    want_LEH = save_LEH and (last is None or any(last))
    L = leh = None
    if want_L or want_LEH:
        # the PSFs are the strip's inset: without the strip they are not passed, and an image smaller than 3 x the kernel still gets its L
        L, leh = dgr.result_panels(eng, y, est_u8_dev, gt_dev, k=k if want_LEH and config.task != "inpaint" else None, sf=config.sf,
                                   mode="inpaint" if config.task == "inpaint" else "kernel", want_L=want_L, want_LEH=want_LEH)
    return emit_results(config, names, lambdas, zetas, est_u8=est_u8_dev.numpy() if save_E else None, L_u8=L, leh_u8=leh, k=k, submit=rw.submit,
                        first=first, last=last)


def make_result_writer(config, H, W):
    """None unless engine_save_results arms one of the save_* keys; else the writer pool, after the one refusal that can be made ahead of all
    work: a strip whose x 3 kernel inset does not fit the image (the reference's slice assignment raises there, main_ddpir_deblur.py:418)."""
    opts = result_options(config)
    if not any(opts):
        return None
    if opts[2] and config.task in ("deblur", "sr"):
        state = np.random.get_state()          # the Gaussian PSF recipe seeds and draws from numpy's global generator
        k, _ = make_operators(config, 1, 0, H, W)
        np.random.set_state(state)
        if 3 * k.shape[2] > H or 3 * k.shape[3] > W:
            raise ValueError(f"save_LEH: the kernel inset is 3 x {k.shape[2]} by 3 x {k.shape[3]} pixels, the images are {H} x {W} "
                             "(main_ddpir_deblur.py:418 fails there too)")
    return ResultWriter(config.batch_size * sum(bool(o) for o in opts))


def emit_progress(config, pg, names, lambda_, psnrs, current_time=None, writer=write_png, logger=None):
    """What the reference does with progress_img after one image (main_ddpir_deblur.py:367-368, 400-406; main_ddpir_inpainting.py:310-311,
    349-371), for every image of a batch: the log_process lines, one "process" PNG and, when asked for, the masked one.  The strips are the
    engine's uint8 conversion (clamp, x 255, round half to even) of the float panels.  Returns the paths written."""
    save, mask, log_p = progress_options(config)
    logger = logger or log
    current_time = current_time or time.strftime("%Y_%m_%d_%H_%M_%S")
    out_dir, paths = result_dir(config), []
    for b, full in enumerate(names):
        img_name, ext = os.path.splitext(full)
        if log_p:
            for line in pg.log_lines(b):
                logger.info(line)
        if save:
            plain, masked = progress_file_names(config, img_name, ext, lambda_, current_time, float(psnrs[b]))
            paths.append(os.path.join(out_dir, plain))
            writer(paths[-1], pg.strip_u8[b])
            if mask:
                paths.append(os.path.join(out_dir, masked))
                writer(paths[-1], pg.masked_u8[b])
    return paths


def main(argv=None):
    import sys
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt", type=str, required=True, help="Path to option YAML file.")
    ap.add_argument("--synthetic", type=int, default=0, help="use N synthetic images instead of the testset")
    ap.add_argument("--synthetic-size", type=parse_size, default=(256, 256), metavar="HxW", help="size of the synthetic images (default 256x256)")
    ap.add_argument("--device", type=int, default=None, help="HIP ordinal (default: LOCAL_RANK, else 0)")
    ap.add_argument("--max-sweeps", type=int, default=0)
    ap.add_argument("--num-gpus", type=int, default=0, help="shard every batch over this many GPUs (one process per GPU)")
    ap.add_argument("--dist-backend", default="rccl", help="result collective: rccl (the C ABI's ncclAllGather binding, default) | nccl | gloo (torch.distributed)")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    config = parse_config(args.opt)
    batch_sweeps = bool(config.get("engine_batch_sweeps", False))
    if batch_sweeps:
        check_batch_sweeps(config)
    num_gpus = args.num_gpus or int(config.get("num_gpus", 1) or 1)
    if num_gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one process per GPU: re-launch under torch.distributed.run (rendezvous on 127.0.0.1)
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={num_gpus}", "--master-addr", "127.0.0.1",
               "--master-port", os.environ.get("MASTER_PORT", "29541"), "-m", "diffpir_amd.main_ddpir"] + list(argv if argv is not None else sys.argv[1:])
        return subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))
    from . import dist as ddist
    rank, local_rank, world = ddist.init(args.dist_backend)
    np.random.seed(config.seed)
    eng = Engine(args.device if args.device is not None else local_rank)
    eng.set_precision(str(config.get("engine_precision", "f16x3")))      # before load_state_dict: selects the weight packing
    if config.generate_mode == "DPS_y0":
        eng.enable_grad()                  # main_ddpir.py:236-239: DPS_y0 is the one mode that differentiates through the network
    ddist.attach(eng)                      # rccl: ncclCommInitRank on this engine's device

    model_config = dict(model_path=os.path.join(config.get("cwd", "") or "", "model_zoo", config.model_name + ".pt"),
                        num_channels=128, num_res_blocks=1, attention_resolutions="16") \
        if config.model_name == "diffusion_ffhq_10m" else \
        dict(model_path=os.path.join(config.get("cwd", "") or "", "model_zoo", config.model_name + ".pt"),
             num_channels=256, num_res_blocks=2, attention_resolutions="8,16,32")
    margs = utils_model.create_argparser(model_config).parse_args([])
    model, diffusion = script_util.create_model_and_diffusion(
        **script_util.args_to_dict(margs, script_util.model_and_diffusion_defaults().keys()), engine=eng)
    if os.path.exists(margs.model_path):
        model.load_state_dict(weights.load_checkpoint(margs.model_path))
    else:
        log.info("checkpoint %s not found: using synthetic weights (results are not meaningful images)", margs.model_path)
        model.load_state_dict(weights.synth_state_dict("ffhq" if config.model_name == "diffusion_ffhq_10m" else "imagenet256"))

    with_lpips = setup_lpips(eng, config)
    border = ssim_border(config)           # calc_SSIM: the 8-bit PSNR / SSIM columns (dpir_metrics_u8); None when off
    ncol = (3 if with_lpips else 2) + (4 if border is not None else 0)
    imgs, names = load_images(config, args.synthetic, args.synthetic_size)
    with_fid = setup_fid(eng, config, len(imgs))
    fid_gt, fids = {}, []                  # ground-truth feature rows per batch (computed at the first sweep point, reused by the others); FID per point
    use_graph = bool(config.get("engine_graph", True))
    noise = config.get("engine_noise", "device")
    host_gen = None
    if noise == "host":
        # ONE generator for the whole run, like the reference's global torch RNG (main_ddpir.py:131): successive batches
        # continue the stream instead of replaying it
        import torch
        host_gen = torch.Generator().manual_seed(config.seed)
    results = []
    cache = {}
    import torch
    # every batch's sharding is checked BEFORE any work starts (a ragged last batch smaller than the world used to raise after all earlier
    # batches had been computed, losing the run)
    for i0 in range(0, len(imgs), config.batch_size):
        ddist.check_dps_sharding(eng, loop_config(config, *sweeps(config)[0]), min(config.batch_size, len(imgs) - i0), world)
    points = sweeps(config)[:args.max_sweeps] if args.max_sweeps else sweeps(config)
    try:
        rw = make_result_writer(config, imgs.shape[1], imgs.shape[2])   # engine_save_results; None when off: nothing below touches a file
    except ValueError:
        ddist.shutdown()
        eng.close()
        raise
    if batch_sweeps:
        results = run_batched_sweeps(eng, config, points, imgs, ddist, rank, world, use_graph, cache, with_lpips, border, names=names, rw=rw)
        points = []
    for si, (lambda_, zeta) in enumerate(points):
        cfg = loop_config(config, lambda_, zeta)
        if rank == 0:
            log.info("eta:%s, zeta:%s, lambda:%s, guidance_scale:%s", config.eta, zeta, lambda_, config.guidance_scale)
        psnrs, psnrs_y, lps, t0, n = [], [], [], time.time(), 0
        u8s = np.zeros(4)
        fid_out = fid_host.FidStats()
        for i0 in range(0, len(imgs), config.batch_size):
            gt = imgs[i0:i0 + config.batch_size]                           # uint8 [n,H,W,3]
            n_b, H, W = gt.shape[0], gt.shape[1], gt.shape[2]
            k_all, mask_all = make_operators(config, n_b, i0, H, W)      # every rank draws the same operators (seeded numpy)
            lo, hi = ddist.shard_range(n_b, rank, world)                 # this rank's images of the batch
            per_img = np.zeros((0, ncol))
            u8_local = eng.empty((hi - lo, H, W, 3), np.uint8)          # engine-owned result buffer (send side of the all-gather)
            drawn = None
            dps_mode = cfg.generate_mode in ("DPS_y0", "DPS_yt")
            # driver: main_ddpir_deblur -- the standalone deblurring program's gradient modes pull their noise through noise_fn and run eagerly on one GPU
            deb_grad = cfg.driver == "main_ddpir_deblur" and (dps_mode or not cfg.sub_1_analytic)
            if deb_grad and world > 1:
                raise NotImplementedError("driver main_ddpir_deblur: the gradient modes are single-GPU")
            dps_mode = dps_mode or deb_grad
            ddist.check_dps_sharding(eng, cfg, n_b, world)
            dps_nf = None
            if noise == "host" and dps_mode:
                # the DPS modes draw in their own order (init, then per step the sampler's draw [and the y_t draw]); restore_batch pulls
                # them through noise_fn.  The GLOBAL batch's tensor is drawn every time and this rank keeps its image rows, so results do
                # not depend on the number of ranks; a rank with an empty shard still advances the shared generator.
                dps_nf = lambda shape: torch.randn((n_b,) + tuple(shape[1:]), generator=host_gen).numpy()[lo:hi]
                if hi == lo:
                    _, steps, _ = restore._steps(cfg)
                    for shp in restore.dps_host_noise_shapes(cfg, steps, 0, H, W):
                        dps_nf(shp)
            elif noise == "host" and cfg.driver == "main_ddpir_inpainting":
                # driver: main_ddpir_inpainting -- the standalone program's per-image draw order (restore.inpaint_host_noise_shapes); every rank
                # draws the global batch and keeps its images
                _, rows, _ = restore._inpaint_rows(cfg)
                nf = lambda shape: torch.randn(tuple(shape), generator=host_gen).numpy()
                full = restore.draw_inpaint_host_noise(nf, cfg, rows, n_b, H, W)
                drawn = {k_: None if a is None else np.ascontiguousarray(a[lo:hi] if a.ndim == 4 else a[:, lo:hi]) for k_, a in full.items()}
            elif noise == "host" and cfg.is_ancestral():
                # model_output_type: pred_x_prev -- init, then per step [the repaint draw] and the sampler's draw (restore.ancestral_host_noise_shapes),
                # batch-shaped; every rank draws the global batch and keeps its images
                _, rows, _ = restore._ancestral_rows(cfg)
                nf = lambda shape: torch.randn(tuple(shape), generator=host_gen).numpy()
                full = restore.draw_ancestral_host_noise(nf, cfg, rows, n_b, H, W)
                drawn = {k_: None if a is None else np.ascontiguousarray(a[lo:hi] if a.ndim == 4 else a[:, lo:hi]) for k_, a in full.items()}
            elif noise == "host":
                # EVERY rank draws the global batch's noise, also a rank whose shard is empty (ragged last batch with fewer images
                # than ranks): the shared generator must advance identically everywhere or later batches depend on the world size
                _, steps, _ = restore._steps(cfg)
                nf = lambda shape: torch.randn(tuple(shape), generator=host_gen).numpy()
                full = restore.draw_host_noise(nf, steps, (n_b, 3, H, W), cfg.eta != 0, repaint=cfg.generate_mode == "repaint")
                drawn = [None if a is None else (np.ascontiguousarray(a[lo:hi]) if a.ndim == 4 else np.ascontiguousarray(a[:, lo:hi])) for a in full]
            save_p, mask_p, _ = progress_options(config)
            if save_p and world > 1:
                raise NotImplementedError("save_progressive / log_process on several GPUs: the strips are not gathered across ranks (num_gpus: 1)")
            pg = restore.Progress(u8=True, masked=mask_p) if save_p else None
            if hi > lo:
                sl = slice(lo, hi)
                # degradation on the device (dpir_degrade): blur / down-sampling / masking + AWGN, device Philox noise keyed by the
                # global image index
                y, ops = dgr.degrade(eng, config.task, gt[sl], k=None if k_all is None else k_all[sl], mask=None if mask_all is None else mask_all[sl],
                                     noise_level_img=config.noise_level_img, sf=config.sf, sr_mode=config.sr_mode, seed=config.seed + 1,
                                     image_offset=i0 + lo)
                out_f32 = restore.restore_batch(eng, cfg, y, k=ops.get("k"), mask=None if dps_mode else ops.get("mask"), noise_source=noise,
                                                predrawn=drawn, noise_fn=dps_nf, seed=config.seed, image_offset=i0 + lo, use_graph=use_graph and not deb_grad, out_u8=u8_local, _cache=cache,
                                                skip_dead_final_eval=bool(config.get("engine_skip_dead_final_eval", False)), progress=pg)
                per_img = metric_rows(eng, out_f32, ops["gt"], with_lpips, border)     # dpir_metrics: per-image PSNR / PSNR-Y; dpir_lpips; dpir_metrics_u8
                if pg is not None:
                    emit_progress(config, pg, names[i0 + lo:i0 + hi], lambda_, per_img[:, 0].astype(np.float32))
                if rw is not None:         # this rank's shard: names are disjoint across ranks, no collective
                    save_results(eng, config, rw, names[i0 + lo:i0 + hi], lambda_, zeta, y, u8_local, ops["gt"], None if k_all is None else k_all[sl])
            if with_fid:
                if i0 not in fid_gt:
                    fid_gt[i0] = fid_rows(eng, ops["gt"] if hi > lo else None, hi - lo, n_b, ddist, rank, world)
                fid_out.add(fid_rows(eng, u8_local, hi - lo, n_b, ddist, rank, world))
            u8 = ddist.all_gather_results(u8_local, n_b, rank, world, engine=eng)           # the one collective of the path
            allm = ddist.all_gather_results(per_img.reshape(-1, ncol), n_b, rank, world, engine=eng)   # per-image PSNR [/ LPIPS] rows (host numpy)
            p, p_y = float(np.mean(allm[:, 0])), float(np.mean(allm[:, 1]))
            psnrs.append(p * n_b)
            psnrs_y.append(p_y * n_b)
            n += n_b
            if with_lpips:
                lps.append(float(np.mean(allm[:, 2])) * n_b)           # the mean over the batch's images (Q: the reference keeps image 0's)
            if rank == 0:
                log_batch(i0 // config.batch_size + 1, p, lps[-1] / n_b if with_lpips else None, sum(lps) / len(imgs))
            if border is not None:
                u8 = np.mean(allm[:, -4:], axis=0)
                u8s += u8 * n_b
                if rank == 0:
                    log_batch_u8(i0 // config.batch_size + 1, u8)
        if rw is not None:
            rw.drain()                     # the images/s line includes saving; a later sweep point may write the same path again
        dt = time.time() - t0
        if rank == 0:
            log.info("-----------> Average PSNR(RGB) of (%s) scale factor: (%d), sigma: (%.3f): %.4f dB  [%.2f images/s on %d GPU(s)]",
                     config.testset_name, config.sf, config.noise_level_model, sum(psnrs) / n, n / dt, world)
            log.info("-----------> Average PSNR(Y) of (%s) scale factor: (%d), sigma: (%.3f): %.4f dB",
                     config.testset_name, config.sf, config.noise_level_model, sum(psnrs_y) / n)
            if with_lpips:
                log.info("-----------> Average LPIPS of (%s) scale factor: (%d), sigma: (%.3f): %.4f",
                         config.testset_name, config.sf, config.noise_level_model, sum(lps) / n)
            if border is not None:
                log_average_u8(config, u8s, n)
        if with_fid:
            gt_stats = fid_host.FidStats()
            for key in sorted(fid_gt):
                gt_stats.add(fid_gt[key])
            fids.append(fid_host.frechet_distance(fid_out.mu, fid_out.sigma, gt_stats.mu, gt_stats.sigma))
            if rank == 0:
                log.info("-----------> FID of (%s) scale factor: (%d), sigma: (%.3f): %.4f",
                         config.testset_name, config.sf, config.noise_level_model, fids[-1])
        results.append(sum(psnrs) / n)
    if fids and rank == 0:
        log.info("-----------> Average FID of (%s) over %d sweep point(s): %.4f", config.testset_name, len(fids), sum(fids) / len(fids))
    if rw is not None:
        rw.close()
    ddist.shutdown()
    eng.close()
    return results


if __name__ == "__main__":
    main()
