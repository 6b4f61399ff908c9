"""CPU tests of the per-image (lambda, zeta, sigma) path: schedule.build_image_table against build_steps, the YAML driver's flattening of a
sweep into full batches and its regrouping, the refusals (raised before a device is touched) and the C ABI's new struct and entries."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import yaml

from diffpir_amd import _lib, restore, schedule
from diffpir_amd import main_ddpir as drv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (lambda, zeta, noise_level_img): zeta = 0, zeta = 1, a repeated triple, three noise levels (one below the 0.001 floor of sigma)
TRIPLES = [(7.0, 0.3, 12.75 / 255), (3.5, 0.0, 5.0 / 255), (11.0, 1.0, 0.0), (7.0, 0.3, 12.75 / 255), (2.0, 0.6, 20.0 / 255)]


@pytest.mark.parametrize("kw", [dict(iter_num=6, eta=0.0), dict(iter_num=5, eta=0.7), dict(iter_num=8, eta=0.3, skip_type="uniform"),
                                dict(iter_num=6, eta=0.0, generate_mode="repaint")], ids=["eta0", "eta07", "uniform", "repaint"])
def test_image_table_rows_equal_build_steps_exactly(kw):
    lam, zet, sig = [t[0] for t in TRIPLES], [t[1] for t in TRIPLES], [max(0.001, t[2]) for t in TRIPLES]
    (dt, steps, arr), table = schedule.build_image_table(lambda_=lam, zeta=zet, sigma=sig, **kw)
    assert table.dtype == np.float32 and table.shape == (len(steps), len(TRIPLES), 4)
    assert not table[:, :, 3].any()
    for b in range(len(TRIPLES)):
        _, s_b, a_b = schedule.build_steps(lambda_=lam[b], zeta=zet[b], sigma=sig[b], **kw)
        assert len(s_b) == len(steps)
        for i in range(len(steps)):
            for j, f in enumerate(("tau", "k1", "k2")):
                assert table[i, b, j] == np.float32(getattr(a_b[i], f)), (b, i, f)          # == on float32, no tolerance
    # the ordinary step table is image 0's
    _, _, a_0 = schedule.build_steps(lambda_=lam[0], zeta=zet[0], sigma=sig[0], **kw)
    assert bytes(arr) == bytes(a_0)
    # the three columns do differ between the images (the test would pass vacuously otherwise); zeta = 0 -> k2 = 0, k1 = 1; zeta = 1 -> k1 = 0
    assert len({float(v) for v in table[0, :, 0]}) == 4
    assert table[0, 1, 1] == 1.0 and table[0, 1, 2] == 0.0 and table[0, 2, 1] == 0.0


def test_image_table_refuses_a_difference_in_a_shared_field(monkeypatch):
    real = schedule.build_steps

    def doctored(**kw):
        dt, steps, arr = real(**kw)
        if kw["lambda_"] == 3.5:
            arr[2].sa_p = arr[2].sa_p + 1e-3          # a field that (lambda, zeta, sigma) cannot reach
        return dt, steps, arr
    monkeypatch.setattr(schedule, "build_steps", doctored)
    with pytest.raises(ValueError, match="sa_p"):
        schedule.build_image_table(lambda_=[7.0, 3.5], zeta=[0.3, 0.3], sigma=[0.05, 0.05], iter_num=6)
    schedule.build_image_table(lambda_=[7.0, 7.0], zeta=[0.3, 0.1], sigma=[0.05, 0.02], iter_num=6)      # the undoctored triples pass
    monkeypatch.setattr(schedule, "build_steps", real)
    with pytest.raises(ValueError, match="one length"):
        schedule.build_image_table(lambda_=[7.0, 3.5], zeta=[0.3], sigma=[0.05, 0.05], iter_num=6)


def test_restore_batch_builds_the_table_from_the_loop_config():
    cfg = restore.LoopConfig(task="deblur", iter_num=6, lambda_=7.0, zeta=0.3, eta=0.5)
    pi = restore.PerImage(lambda_=[7.0, 2.0], noise_level_img=[12.75 / 255, 0.0])
    (_, steps, _), table = restore._image_table(cfg, pi, 2)
    for b, (lam, nl) in enumerate(zip(pi.lambda_, pi.noise_level_img)):
        _, _, a_b = restore._steps(restore.LoopConfig(task="deblur", iter_num=6, lambda_=lam, zeta=0.3, eta=0.5, noise_level_img=nl))
        for i in range(len(steps)):
            assert tuple(table[i, b, :3]) == tuple(np.float32(getattr(a_b[i], f)) for f in ("tau", "k1", "k2"))
    with pytest.raises(ValueError, match="batch of 3"):
        pi.check(3)
    assert pi.rows(1, 2).lambda_ == [2.0] and pi.rows(1, 2).zeta is None


def test_driver_flattening_and_regrouping():
    batches = drv.flatten_sweeps(11, 5, 16)
    assert [len(b) for b in batches] == [16, 16, 16, 7]
    flat = [p for b in batches for p in b]
    assert flat == [(s, g) for s in range(11) for g in range(5)]           # sweep-major: the order the sequential driver visits
    values = [[100 * s + g for s, g in b] for b in batches]
    assert drv.regroup_sweeps(batches, values, 11, 5) == [[100 * s + g for g in range(5)] for s in range(11)]
    with pytest.raises(ValueError):
        drv.regroup_sweeps(batches[:-1], values[:-1], 11, 5)
    # a batch's distinct images, in visiting order, as runs of consecutive image numbers: one degrade call each
    assert drv.image_runs(list(dict.fromkeys(g for _, g in batches[0]))) == [(0, 5)]
    assert drv.image_runs(list(dict.fromkeys(g for _, g in batches[1]))) == [(1, 4), (0, 1)]
    assert drv.image_runs([3]) == [(3, 1)]


def _config(tmp_path, **kw):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "sweep_batch_example.yaml")))
    cfg.update(kw)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_driver_key_refusals(tmp_path):
    c = drv.parse_config(_config(tmp_path))
    assert c.engine_batch_sweeps is True and c.task == "sr" and len(drv.sweeps(c)) == 11
    drv.check_batch_sweeps(c)
    with pytest.raises(ValueError, match="engine_noise: device"):
        drv.main(["--opt", _config(tmp_path, engine_noise="host")])
    with pytest.raises(ValueError, match="save_progressive"):
        drv.main(["--opt", _config(tmp_path, save_progressive=True)])
    with pytest.raises(NotImplementedError):
        drv.main(["--opt", _config(tmp_path, sub_1_analytic=False)])
    # the default is off, and every shipped config leaves it off
    assert not drv.parse_config(os.path.join(ROOT, "configs", "engine_example.yaml")).get("engine_batch_sweeps", False)


@pytest.mark.parametrize("kw,pi", [
    (dict(task="sr", sf=4, sub_1_analytic=False), restore.PerImage(lambda_=[1.0])),
    (dict(task="sr", sf=4, generate_mode="DPS_yt"), restore.PerImage(zeta=[0.1])),
    (dict(task="sr", sf=4, generate_mode="DPS_y0"), restore.PerImage(image_index=[3])),
    (dict(task="deblur", driver="main_ddpir_deblur"), restore.PerImage(lambda_=[1.0])),
    (dict(task="inpaint", driver="main_ddpir_inpainting"), restore.PerImage(lambda_=[1.0])),
    (dict(task="deblur", skip_noise_model_t=True), restore.PerImage(noise_level_img=[0.05])),
], ids=["first_order", "dps_yt", "dps_y0", "deblur_program", "inpainting_program", "skip_noise_model_t"])
def test_restore_batch_refusals_need_no_device(kw, pi):
    """engine = None and y = None: anything that touched them would raise AttributeError, not NotImplementedError."""
    cfg = restore.LoopConfig(**kw)
    with pytest.raises(NotImplementedError):
        restore.restore_batch(None, cfg, None, per_image=pi)
    from diffpir_amd import dist as ddist
    with pytest.raises(NotImplementedError):
        ddist.restore_sharded(None, cfg, np.zeros((1, 3, 8, 8), np.float32), rank=0, world=1, per_image=pi)
    # skip_noise_model_t is refused only together with a per-image noise level
    if kw.get("skip_noise_model_t"):
        restore.check_per_image(cfg, restore.PerImage(lambda_=[1.0]))


def test_header_mirror_and_struct_size_agree():
    hdr = open(os.path.join(ROOT, "include", "diffpir_engine.h")).read()
    m = re.search(r"typedef struct dpir_image_step \{([^}]*)\} dpir_image_step;", hdr)
    assert m and [f.strip() for f in m.group(1).replace("float", "").strip(" ;").split(",")] == [f for f, _ in _lib.ImageStep._fields_]
    assert C.sizeof(_lib.ImageStep) == 16 and all(t is C.c_float for _, t in _lib.ImageStep._fields_)
    for name in ("dpir_run_loop_per_image", "dpir_randn_indexed"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "dpir_run_loop_per_image") and hasattr(lib, "dpir_randn_indexed")
    assert lib.dpir_version() == _lib.ABI_VERSION == 2 and _lib.LoopDesc.y_dev.offset == 48        # neither moved
    # argument counts of the mirror against the header's declarations
    for name in ("dpir_run_loop_per_image", "dpir_randn_indexed"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1])
    if shutil.which("gcc"):
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            src = os.path.join(td, "sz.c")
            open(src, "w").write('#include "diffpir_engine.h"\n#include <stdio.h>\nint main(void){printf("%zu\\n", sizeof(dpir_image_step));return 0;}\n')
            subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(td, "sz")], check=True)
            assert int(subprocess.run([os.path.join(td, "sz")], check=True, capture_output=True, text=True).stdout) == 16
