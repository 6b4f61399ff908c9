"""CPU tests of the progressive strip: which steps keep a panel (schedule.progress_panels) against a literal evaluation of the reference's
two progress_seq recipes and, where the reference tree is present, against its own statements; tests/golden/progress*.npz (the standalone
inpainting program's progress_img) against the CPU float32 statement tests/progress_ref.py; the driver's three YAML keys, file names and log
line; and what refuses a strip."""
import ast
import logging
import os

import numpy as np
import pytest

from diffpir_amd import dist, main_ddpir, restore, schedule
from oracle import unet_oracle as uo
from tests import inpaint_resample_ref as ref, progress_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000
PROGRAMS = ("main_ddpir", "main_ddpir_deblur", "main_ddpir_sisr", "main_ddpir_inpainting")


def literal_progress_seq(seq, program):
    """the two recipes of the reference programs, written out literally"""
    seq = list(seq)
    if program == "main_ddpir_inpainting":
        ps = seq[::(len(seq) // 10)]
        ps.append(seq[-1])
    else:
        ps = seq[::max(len(seq) // 10, 1)]
        if ps[-1] != seq[-1]:
            ps.append(seq[-1])
    return ps


def visited_of(seq, t_start):
    dt = schedule.DriverTables.make()
    t_list = [schedule.find_nearest(dt.reduced, dt.reduced[T - 1 - s]) for s in seq]
    return [i for i, t in enumerate(t_list) if t <= t_start], t_list


@pytest.mark.parametrize("iter_num", [10, 15, 20, 100, 1000])
@pytest.mark.parametrize("skip_type", ["quad", "uniform"])
@pytest.mark.parametrize("t_start", [T - 1, 400])
@pytest.mark.parametrize("program", PROGRAMS)
def test_progress_panels_are_the_literal_recipes(iter_num, skip_type, t_start, program):
    seq = schedule.make_seq(T, iter_num, skip_type)
    visited, _ = visited_of(seq, t_start)
    assert (len(visited) < len(seq)) == (t_start < T - 1)
    ps = literal_progress_seq(seq, program)
    assert schedule.progress_seq(seq, program) == ps
    got = schedule.progress_panels(seq, visited, program)
    keep = [seq[i] in ps for i in visited]                   # membership by value; a skipped step never reaches the block
    assert [p >= 0 for p in got] == keep
    assert [p for p in got if p >= 0] == list(range(sum(keep)))
    assert got[-1] == sum(keep) - 1                          # the final step always owns the last panel
    assert all(got[j] >= 0 for j, i in enumerate(visited) if seq[i] == seq[-1])


@pytest.mark.parametrize("program", PROGRAMS)
def test_panel_counts(program):
    """iter_num 10 -> 10 panels, 15 -> 15, 20 and 100 -> 11; quad skipping at 1000 -> 17 (250 seq values repeat and seq[-1] occurs twice)."""
    for iter_num, want in ((10, 10), (15, 15), (20, 11), (100, 11), (1000, 17)):
        seq = schedule.make_seq(T, iter_num, "quad")
        got = schedule.progress_panels(seq, range(len(seq)), program)
        assert sum(p >= 0 for p in got) == want, (iter_num, want)
    seq = schedule.make_seq(T, 1000, "quad")
    assert len(seq) - len(set(seq)) == 250 and seq.count(seq[-1]) == 2


def test_inpainting_recipe_keeps_its_refusal_of_short_schedules():
    with pytest.raises(ValueError, match=":227"):
        schedule.progress_seq(list(range(9)), "main_ddpir_inpainting")
    assert schedule.progress_seq(list(range(9)), "main_ddpir_deblur") == list(range(9))
    with pytest.raises(ValueError):
        schedule.progress_seq(list(range(20)), "nope")


@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("init", ["max", 120.0])
def test_progress_table_puts_a_groups_panel_on_its_last_row(U, init):
    cfg = restore.LoopConfig(task="inpaint", driver="main_ddpir_inpainting", iter_num=20, iter_num_U=U, noise_level_img=12.75 / 255, noise_init_img=init)
    _, rows, _ = restore._inpaint_rows(cfg)
    table, panels = restore.progress_table(cfg, rows)
    seq = schedule.make_seq(T, 20, "quad")
    ps = literal_progress_seq(seq, "main_ddpir_inpainting")
    assert len(table) == len(rows)
    for r, p in zip(rows, table):
        assert (p >= 0) == (r["u"] == U - 1 and r["seq"] in ps)
    assert panels == [(r["seq"], r["t"]) for r, p in zip(rows, table) if p >= 0]
    assert [p for p in table if p >= 0] == list(range(len(panels))) and panels[-1] == (999, 0)
    assert len(panels) == (11 if init == "max" else 5)      # a t_start below T - 1 drops the panels of the skipped steps
    # the default driver: one entry per step
    dcfg = restore.LoopConfig(task="inpaint", iter_num=20, noise_init_img=init)
    _, steps, _ = restore._steps(dcfg)
    dtable, dpanels = restore.progress_table(dcfg, steps)
    assert len(dtable) == len(steps) and dpanels == panels


def _program_statements(path, first_target):
    """the `progress_seq = ...` statement of a reference program and the one that follows it, as source"""
    with open(path) as f:
        tree = ast.parse(f.read())
    for node in ast.walk(tree):
        body = getattr(node, "body", None)
        if not isinstance(body, list):
            continue
        for i, n in enumerate(body):
            if isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == first_target for t in n.targets):
                return body[i:i + 2]
    raise AssertionError(f"no `{first_target} = ...` in {path}")


@pytest.mark.parametrize("program", PROGRAMS)
def test_recipes_are_the_reference_programs_own_statements(program):
    from oracle import ref_import
    path = os.path.join(ref_import.REF_ROOT, program + ".py")
    if not ref_import.available() or not os.path.exists(path):
        pytest.skip("reference tree absent")
    stmts = _program_statements(path, "progress_seq")
    code = compile(ast.Module(body=stmts, type_ignores=[]), path, "exec")
    for iter_num in (10, 15, 20, 100, 1000):
        for skip_type in ("quad", "uniform"):
            seq = schedule.make_seq(T, iter_num, skip_type)
            ns = dict(seq=list(seq), len=len, max=max)
            exec(code, ns)
            assert ns["progress_seq"] == schedule.progress_seq(seq, program), (program, iter_num, skip_type)


# ---------------------------------------------------------------- the fixture against its CPU float32 statement
@pytest.fixture(scope="module")
def fx(golden):
    g = pr.load(golden)
    assert sorted(str(c) for c in g["cases"]) == sorted(pr.CASES)
    return g


@pytest.mark.parametrize("name", pr.CASES)
def test_fixture_panels_match_the_cpu_float32_statement(fx, name):
    """Every panel: max|statement - program| <= 2e-3 max(1, max|panel of the program|).  Measured on the generating machine: at most
    1.3e-6 (both cases), against bounds of 2.0e-3 .. 6.3e-3."""
    hp = uo.tiny_hp()
    c = pr.case_config(fx, name)
    assert c["iter_num"] == 20 and c["iter_num_U"] == 2
    cfg = ref.loop_config(c)
    strip, panels = pr.panels_ref(uo.synth_state_dict(hp, 0), hp, cfg, fx["y"], fx["mask"], pr.seeded(c["seed"]))
    assert panels == list(zip(fx[name + ".panel_seq"].tolist(), fx[name + ".panel_t"].tolist()))
    assert fx[name + ".seq"].tolist() == schedule.make_seq(T, 20, "quad")
    want = pr.fixture_strip(fx, name)
    assert strip.shape == want.shape == (2, 3, 64, len(panels) * 64)
    errs = pr.per_panel_errors(strip, want, len(panels))
    print(f"{name}: per panel max|statement - program| " + " ".join(f"{a:.2e}" for a, _ in errs))
    assert all(a <= b for a, b in errs), errs
    assert len(panels) == (11 if name == "diffpir_u2" else 5)


def test_fixture_files_stay_under_the_size_limit():
    for n in ("progress",) + tuple("progress." + c for c in pr.CASES):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) <= 1 << 20


# ---------------------------------------------------------------- driver behaviour with a stub in place of the engine's strips
def _config(tmp_path, **over):
    d = dict(task="inpaint", driver="main_ddpir_inpainting", generate_mode="DiffPIR", testset_name="demo", model_name="m", noise_level_img=12.75 / 255,
             iter_num=20, eta=0.0, zeta=1.0, lambda_=1.0, mask_type="box", cwd=str(tmp_path), sf=1, sr_mode="blur", blur_mode="Gaussian")
    d.update(over)
    return main_ddpir.Config(d)


def _stub_progress(B=2, P=3, H=4, W=5):
    rng = np.random.default_rng(0)
    pg = restore.Progress(masked=True)
    pg.panels = [(0, 999), (458, 541), (999, 0)][:P]
    pg.strip_u8 = rng.integers(0, 255, (B, H, P * W, 3)).astype(np.uint8)
    pg.masked_u8 = rng.integers(0, 255, (B, H, P * W, 3)).astype(np.uint8)
    pg.minmax = np.array([[[3.25, -2.5], [1.0, 0.0]], [[1.5, -0.25], [1.0, 0.5]], [[1.00004, -0.00004], [0.75, 0.125]]], np.float32)[:P, :B]
    return pg


def test_the_three_keys_default_to_off_and_every_shipped_config_keeps_today_s_behaviour():
    import glob
    assert main_ddpir.progress_options(main_ddpir.Config(dict(task="deblur", generate_mode="DiffPIR"))) == (False, False, False)
    on = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml"))):
        opts = main_ddpir.progress_options(main_ddpir.parse_config(path))
        if os.path.basename(path) == "progress_example.yaml":
            assert opts == (True, True, True)
            on += 1
        else:
            assert opts == (False, False, False), path
    assert on == 1


def test_key_parsing():
    opt = lambda **kw: main_ddpir.progress_options(main_ddpir.Config(dict(dict(task="inpaint", generate_mode="DiffPIR", driver="main_ddpir_inpainting"), **kw)))   # noqa: E731
    assert opt(save_progressive=True) == (True, False, False)
    assert opt(save_progressive=True, log_process=True, save_progressive_mask=True) == (True, True, True)
    assert opt(log_process=True, save_progressive_mask=True) == (False, False, False)         # both live inside `if save_progressive`
    assert opt(save_progressive=True, save_progressive_mask=True, generate_mode="vanilla") == (True, False, False)
    assert opt(save_progressive=True, save_progressive_mask=True, generate_mode="repaint") == (True, True, False)
    for driver in ("main_ddpir", "main_ddpir_deblur"):
        assert opt(save_progressive=True, save_progressive_mask=True, log_process=True, driver=driver) == (True, False, True)


def test_file_names_and_log_lines(tmp_path, caplog):
    pg = _stub_progress()
    written = {}
    cfg = _config(tmp_path, save_progressive=True, save_progressive_mask=True, log_process=True)
    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        paths = main_ddpir.emit_progress(cfg, pg, ["a.png", "b.jpg"], 1.0, [30.0, 31.0], current_time="2026_01_02_03_04_05",
                                         writer=lambda p, a: written.__setitem__(p, a))
    d = main_ddpir.result_dir(cfg)
    assert d.startswith(str(tmp_path)) and "demo_inpaint_DiffPIR_m_sigma0.05_NFE20_eta0.0_zeta1.0_lambda1.0_mask_type_box" in d
    assert [os.path.relpath(p, d) for p in paths] == ["a_process_lambda_1.000_2026_01_02_03_04_05.png", "a_process_mask_lambda_1.000_2026_01_02_03_04_05.png",
                                                     "b_process_lambda_1.000_2026_01_02_03_04_05.jpg", "b_process_mask_lambda_1.000_2026_01_02_03_04_05.jpg"]
    assert written[paths[0]].tobytes() == pg.strip_u8[0].tobytes() and written[paths[3]].tobytes() == pg.masked_u8[1].tobytes()
    lines = [r.getMessage() for r in caplog.records]
    fmt = "{:>4d}, steps: {:>4d}, np.max(x_show): {:.4f}, np.min(x_show): {:.4f}"
    assert lines == [fmt.format(s, t, pg.minmax[p, b, 0], pg.minmax[p, b, 1]) for b in range(2) for p, (s, t) in enumerate(pg.panels)]
    assert lines[0] == "   0, steps:  999, np.max(x_show): 3.2500, np.min(x_show): -2.5000"
    assert lines[2] == " 999, steps:    0, np.max(x_show): 1.0000, np.min(x_show): -0.0000"
    # the deblurring / default drivers: the other name, no masked strip, nothing logged without log_process
    caplog.clear()
    cfg = _config(tmp_path, task="deblur", driver="main_ddpir_deblur", save_progressive=True, save_progressive_mask=True)
    with caplog.at_level(logging.INFO, logger="diffpir_amd"):
        paths = main_ddpir.emit_progress(cfg, pg, ["a.png"], 7.0, [29.123456], current_time="T", writer=lambda p, a: None)
    assert [os.path.basename(p) for p in paths] == ["a_sigma_0.050_process_lambda_7.000_T_psnr_29.1235.png"]
    assert not caplog.records
    assert main_ddpir.emit_progress(_config(tmp_path), pg, ["a.png"], 1.0, [0.0], writer=lambda p, a: pytest.fail("nothing is written by default")) == []


def test_png_writer_round_trips(tmp_path):
    from PIL import Image
    a = _stub_progress().strip_u8[0]
    path = str(tmp_path / "sub" / "strip.png")
    main_ddpir.write_png(path, a)
    assert np.array_equal(np.asarray(Image.open(path)), a)


def test_restore_sharded_refuses_a_strip():
    with pytest.raises(NotImplementedError, match="progress"):
        dist.restore_sharded(None, restore.LoopConfig(task="inpaint"), np.zeros((2, 3, 8, 8), np.float32), rank=0, world=2, progress=restore.Progress())


def test_progress_request_defaults():
    pg = restore.Progress()
    assert pg.u8 and not pg.masked and pg.panels is None and pg.strip_f32 is None


def test_progress_hip_is_built_without_fp_contraction_like_elem_hip():
    """x/2+.5 and the masked blend must round once per operation, as finalize_kernel's do (csrc/Makefile)."""
    mk = open(os.path.join(ROOT, "diffpir_amd", "csrc", "Makefile")).read()
    rule = lambda name: mk.split(f"$(OBJDIR)/{name}.o: {name}.hip $(HDRS)")[1].split("\n\n")[0].split("$(OBJDIR)/")[0]      # noqa: E731
    assert "-ffp-contract=off" in rule("progress") and rule("progress").strip() == rule("elem").strip()
    assert " progress.hip " in mk.split("SRCS =")[1].split("\n")[0] and " progress.h " in mk.split("HDRS =")[1].split("\n")[0]
