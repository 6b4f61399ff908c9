"""CPU: the host side of FID (diffpir_amd/fid.py: the network table, the BatchNorm fold, the key layouts, the Frechet distance; the driver's
calc_FID switch; the ABI table) and the float64 statement of tests/fid_f64.py against the table's checksums."""
import logging
import os
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diffpir_amd import _lib, fid as fd, main_ddpir as drv
from tests import fid_f64 as Fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diffpir_engine.h")


@pytest.fixture(scope="module")
def raw():
    return fd.synth_weights(3, raw=True)


def test_the_table_has_the_networks_checksums(raw):
    spec = fd.inception_spec()
    assert len(spec) == 94 and len({l.name for l in spec}) == 94
    weights = sum(l.cin * l.cout * l.kernel[0] * l.kernel[1] for l in spec)
    assert weights == 21_751_136
    # torchvision's inception_v3 without the auxiliary head has 23 834 568 parameters; its fc has 2 049 000
    assert weights + sum(2 * l.cout for l in spec) == 21_785_568 == 23_834_568 - 2_049_000
    # Multiply-accumulates: an output of K products takes K of them.  5 711 168 096 is torchvision's 5.71 G for inception_v3 (its table's "GFLOPS"
    # are multiply-accumulates) and TWICE the 2 855 584 048 this network's plan was first drawn up with, which had labelled the same 5.711 G as
    # FLOPs; the float64 statement's own conv2d calls are counted below and agree.
    assert fd.macs() == 2 * 2_855_584_048 == 5_711_168_096 and fd.flops() == 2.0 * fd.macs()
    ks = [l.cin * l.kernel[0] * l.kernel[1] for l in spec]
    assert min(ks) == 27 and max(ks) == 4032
    assert {32, 48, 80, 96, 160, 320, 448} <= {l.cout for l in spec}
    assert {l.out_hw for l in spec if l.stride == 2} == {(149, 149), (17, 17), (8, 8)}
    assert len(raw) == 94 * 5 and all(v.dtype == np.float32 for v in raw.values())
    again = fd.synth_weights(3, raw=True)
    assert all(np.array_equal(raw[k], again[k]) for k in raw)
    assert not np.array_equal(raw["Conv2d_1a_3x3.conv.weight"], fd.synth_weights(4, raw=True)["Conv2d_1a_3x3.conv.weight"])


def test_the_float64_statement_has_the_tap_shapes_and_reads_every_key(raw, monkeypatch):
    class Counting(dict):
        def __init__(self, d):
            super().__init__(d)
            self.read = set()

        def __getitem__(self, k):
            self.read.add(k)
            return super().__getitem__(k)
    sd = Counting(raw)
    real, count = F.conv2d, [0]

    def counting(x, w, b=None, **kw):
        y = real(x, w, b, **kw)
        count[0] += y[0].numel() * w.shape[1] * w.shape[2] * w.shape[3]
        return y
    monkeypatch.setattr(Fd.F, "conv2d", counting)
    taps = Fd.features(sd, Fd.make_images(40, 56, 1, as_u8=False))
    monkeypatch.undo()
    assert count[0] == fd.macs() == 5_711_168_096     # the statement's own convolutions, per image
    assert [t.shape for t in taps] == [(1, c, s, s) for c, s in fd.TAP_SHAPES] + [(1, 2048)]
    assert [t.shape[1:] for t in taps[:13]] == [(64, 73, 73), (192, 35, 35), (256, 35, 35), (288, 35, 35), (288, 35, 35)] + [(768, 17, 17)] * 5 + \
        [(1280, 8, 8), (2048, 8, 8), (2048, 8, 8)]
    assert sd.read == set(raw)                        # the statement, written out on its own, uses exactly the table's 94 layers
    assert all(t.dtype == np.float64 and np.isfinite(t).all() and t.max() > 0 for t in taps)


def test_canonical_takes_the_raw_and_the_folded_layout_and_names_what_is_wrong(raw):
    full = {k: torch.from_numpy(v) for k, v in raw.items()}
    full.update({"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008), "AuxLogits.conv0.conv.weight": torch.zeros(128, 768, 1, 1),
                 "Mixed_5b.branch1x1.bn.num_batches_tracked": torch.tensor(0)})
    sd = fd.canonical(full)
    spec = fd.inception_spec()
    assert list(sd) == [f"{l.name}.{leaf}" for l in spec for leaf in ("weight", "bias")]
    assert all(sd[f"{l.name}.weight"].shape == (l.cout, l.cin) + l.kernel and sd[f"{l.name}.bias"].shape == (l.cout,) for l in spec)
    assert all(v.dtype == np.float32 and v.flags["C_CONTIGUOUS"] for v in sd.values())
    again = fd.canonical(sd)                           # the folded layout passes through unchanged
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    assert all(np.array_equal(sd[k], v) for k, v in fd.synth_weights(3).items())
    with pytest.raises(KeyError, match=r"Mixed_6d\.branch7x7dbl_4\.bn\.running_var"):
        fd.canonical({k: v for k, v in full.items() if k != "Mixed_6d.branch7x7dbl_4.bn.running_var"})
    bad = dict(full)
    bad["Mixed_7c.branch3x3_2b.conv.weight"] = full["Mixed_7c.branch3x3_2b.conv.weight"].permute(0, 1, 3, 2).contiguous()     # (1,3) for (3,1)
    with pytest.raises(ValueError, match=r"Mixed_7c\.branch3x3_2b\.conv\.weight"):
        fd.canonical(bad)
    with pytest.raises(KeyError, match=r"Conv2d_1a_3x3\.conv\.weight"):
        fd.canonical({})


@pytest.mark.parametrize("name", ["Conv2d_1a_3x3", "Mixed_5b.branch5x5_2", "Mixed_6b.branch7x7_2", "Mixed_7c.branch3x3dbl_2"])
def test_fold_bn_is_the_layer_to_float32_rounding(raw, name):
    """The folded layer (w', b' rounded ONCE to float32, evaluated in float64) against float64 convolution + BatchNorm on random input.
    Rounding a weight costs its product at most u = 2^-24 relative, so |folded - reference| <= u (sum_k |w'_k| |x_k| + |b'|) at every output --
    at most u (Cin KH KW max|w'| max|x| + max|b'|), a few float32 ulps of the output scale."""
    l = next(x for x in fd.inception_spec() if x.name == name)
    g, b, m, v = (raw[f"{name}.bn.{leaf}"] for leaf in ("weight", "bias", "running_mean", "running_var"))
    wf, bf = fd.fold_bn(raw[f"{name}.conv.weight"], g, b, m, v)
    assert wf.dtype == bf.dtype == np.float32
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((1, l.cin, 12, 12)))
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ref = F.conv2d(x, t(raw[f"{name}.conv.weight"]), None, stride=l.stride, padding=l.padding)
    ref = (ref - t(m).view(1, -1, 1, 1)) / torch.sqrt(t(v).view(1, -1, 1, 1) + 1e-3) * t(g).view(1, -1, 1, 1) + t(b).view(1, -1, 1, 1)
    got = F.conv2d(x, t(wf), t(bf), stride=l.stride, padding=l.padding)
    u = 2.0 ** -24
    bound = u * (F.conv2d(x.abs(), t(wf).abs(), t(bf).abs(), stride=l.stride, padding=l.padding)) * 1.001
    err = (got - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    K = l.cin * l.kernel[0] * l.kernel[1]
    assert float(err.max()) <= u * (K * float(np.abs(wf).max()) * float(x.abs().max()) + float(np.abs(bf).max()))
    assert float(err.max()) > 0                        # it IS rounded: not the float64 fold


def _rand_cov(rng, d, n):
    x = rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, d)
    return np.mean(x, 0), np.cov(x, rowvar=False)


def test_frechet_distance_known_answers():
    rng = np.random.default_rng(0)
    mu, s = _rand_cov(rng, 24, 200)
    assert abs(fd.frechet_distance(mu, s, mu, s)) <= 1e-8 * np.trace(s)
    # commuting covariances Q diag(a) Q^T, Q diag(b) Q^T: |dmu|^2 + sum (sqrt a - sqrt b)^2
    q, _ = np.linalg.qr(rng.standard_normal((24, 24)))
    a, b = rng.uniform(0.1, 3.0, 24), rng.uniform(0.1, 3.0, 24)
    mu2 = mu + rng.standard_normal(24) * 0.3
    want = float(np.sum((mu - mu2) ** 2) + np.sum((np.sqrt(a) - np.sqrt(b)) ** 2))
    got = fd.frechet_distance(mu, (q * a) @ q.T, mu2, (q * b) @ q.T)
    assert abs(got - want) <= 1e-9 * want, (got, want)
    # rank-deficient: 16 rows at d = 64 (the paper's 100 images at d = 2048 are the same situation)
    x1, x2 = rng.standard_normal((16, 64)), rng.standard_normal((16, 64)) * 1.3 + 0.2
    st1, st2 = fd.FidStats(), fd.FidStats()
    st1.add(x1[:10]); st1.add(x1[10:]); st2.add(x2)
    assert len(st1) == 16 and np.linalg.matrix_rank(st1.sigma) == 15
    assert np.array_equal(st1.mu, np.mean(x1, 0)) and np.array_equal(st1.sigma, np.cov(x1, rowvar=False))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = fd.fid_from_features(x1, x2)
    ev = np.linalg.eigvals(st1.sigma @ st2.sigma)
    want = float(np.sum((st1.mu - st2.mu) ** 2) + np.trace(st1.sigma) + np.trace(st2.sigma) - 2 * np.sum(np.sqrt(np.clip(ev.real, 0, None))))
    assert np.isfinite(got) and abs(got - want) <= 1e-5 * want, (got, want)
    assert got == fd.frechet_distance(st1.mu, st1.sigma, st2.mu, st2.sigma)
    with pytest.raises(ValueError, match="at least 2 rows"):
        fd.fid_from_features(x1[:1], x2)
    with pytest.raises(ValueError, match="shapes differ"):
        fd.frechet_distance(mu, s, mu[:3], s[:3, :3])


def test_frechet_distance_non_finite_and_complex_branches(monkeypatch):
    from scipy import linalg
    calls = []
    real = linalg.sqrtm

    def recording(a, *args, **kw):
        calls.append(np.array(a))
        return real(a, *args, **kw)
    monkeypatch.setattr(linalg, "sqrtm", recording)
    z = np.zeros(2)
    # a nilpotent product has no square root: sqrtm returns non-finite values, and the eps I retry [[e,1],[0,e]] (1 + e) has one
    nil = np.array([[0.0, 1.0], [0.0, 0.0]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first = real(nil @ np.eye(2))
        first = first[0] if isinstance(first, tuple) else first
        got = fd.frechet_distance(z, nil, z, np.eye(2))
    if not np.isfinite(first).all():
        assert len(calls) == 2 and np.allclose(calls[1], (nil + 1e-6 * np.eye(2)) @ (np.eye(2) * (1 + 1e-6)))
        assert np.isfinite(got) and abs(got - (2.0 - 2 * 2 * np.sqrt(1e-6 * (1 + 1e-6)))) < 1e-9
    else:                                              # a scipy whose sqrtm copes with the nilpotent matrix: the retry is not needed, nor taken
        assert len(calls) == 1
    # the retry itself, whatever scipy does with the matrix above: a first answer with a NaN in it
    calls.clear()
    answers = iter([np.full((2, 2), np.nan), None])
    monkeypatch.setattr(linalg, "sqrtm", lambda a, *args, **kw: (calls.append(np.array(a)), next(answers))[1] if len(calls) == 0 else recording(a))
    got = fd.frechet_distance(z, np.eye(2), z, np.eye(2) * 4)
    assert len(calls) == 2 and np.allclose(calls[1], (1 + 1e-6) * (4 + 1e-6) * np.eye(2)) and abs(got - (2 + 8 - 2 * 2 * 2)) < 1e-5
    monkeypatch.setattr(linalg, "sqrtm", real)
    # complex: a (constructed, not PSD) covariance with a negative eigenvalue -- diagonal imaginary part 1e-4 is dropped, 1 is an error
    got = fd.frechet_distance(z, np.diag([1.0, -1e-8]), z, np.eye(2))
    assert isinstance(got, float) and abs(got - (1 - 1e-8 + 2 - 2 * 1)) < 1e-12
    with pytest.raises(ValueError, match="imaginary component"):
        fd.frechet_distance(z, np.diag([1.0, -1.0]), z, np.eye(2))


def test_header_carries_the_entries_and_their_citations_and_the_abi_stays_2():
    text = open(HEADER).read()
    for name in ("dpir_fid_load", "dpir_fid_features", "dpir_fid_keep_taps", "dpir_fid_read_tap"):
        assert re.search(rf"\bint {name}\(dpir_engine\* e\b", text), name
        assert name in _lib.SIGNATURES
    block = text[text.index("/* ---- FID"):text.index("int dpir_fid_read_tap")]
    assert "README.md:119-141" in block and "pytorch-fid" in block
    assert re.search(r"#define DPIR_ABI_VERSION 2\b", text)
    assert _lib.SIGNATURES["dpir_fid_features"][1][1:3] == _lib.SIGNATURES["dpir_lpips"][1][2:4]        # two device pointers, one of them given


def test_documents_say_what_the_agreement_rests_on():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("profiles", "fid", "README.md")):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert "not on a run of `pytorch-fid`, which has never been executed here" in text, doc


class _NoEngine:
    def load_fid(self, sd):
        raise AssertionError("must not be reached")


def test_driver_switch_without_the_weight_file_or_with_one_image(tmp_path, caplog):
    cfg = drv.parse_config(os.path.join(ROOT, "configs", "engine_example.yaml"))
    assert cfg.get("calc_FID", None) is False
    assert drv.setup_fid(_NoEngine(), cfg, 4) is False and not caplog.records               # key off: not a word
    cfg.calc_FID, cfg.cwd = True, str(tmp_path)
    assert fd.find_weight_file(cfg) == os.path.join(str(tmp_path), "model_zoo", "pt_inception-2015-12-05-6726825d.pth")
    with caplog.at_level(logging.WARNING, logger="diffpir_amd"):
        assert drv.setup_fid(_NoEngine(), cfg, 4) is False
    assert len(caplog.records) == 1 and "pt_inception-2015-12-05-6726825d.pth" in caplog.records[0].getMessage()
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="diffpir_amd"):
        assert drv.setup_fid(_NoEngine(), cfg, 1) is False
    assert len(caplog.records) == 1 and "at least 2" in caplog.records[0].getMessage()
    cfg.fid_inception_path = "other.pth"
    assert fd.find_weight_file(cfg).endswith(os.path.join("model_zoo", "other.pth"))


def test_batched_sweeps_refuse_fid():
    cfg = drv.parse_config(os.path.join(ROOT, "configs", "sweep_batch_example.yaml"))
    drv.check_batch_sweeps(cfg)
    cfg.calc_FID = True
    with pytest.raises(ValueError, match="calc_FID"):
        drv.check_batch_sweeps(cfg)
