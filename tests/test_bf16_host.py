"""CPU: what bf16-operand training (AZ_TRAIN_BF16, cfg.TRAIN.PRECISION = 'bf16') rests on, without a GPU.

1. ffi.bf16_round is torch's float32 -> bfloat16 conversion: random values over the whole range, every tie of one binade,
   zeros, infinities, overflow and NaN.
2. The conditions of tests/test_gpu_train_bf16.py, asserted here rather than assumed there: the integer cases stay below
   2^24; on every step case the float32 restatement of the bf16 model opens exactly the ReLU gates its float64 restatement
   opens; on the random cases the bf16 model is further than 1e-4 (relative) from the fp32 model, so a kernel that silently
   ran fp32 could not pass for it.
3. The front door: the config key, --bf16 on both tools' parsers, the ValueError, SolverWrapper -> trainer.set_precision."""
import importlib
import os
import sys

import numpy as np
import pytest

import bf16_ref as B
import det_step_ref as D
import train_step_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")


def to_bf16(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. the rounding -------------------------------------------------------------------------------------------------------
def test_bf16_round_equals_torch_on_random_values():
    from aznet_hip import ffi
    rng = np.random.Generator(np.random.PCG64(1))
    x = (10.0 ** rng.uniform(-30, 38, 100000) * rng.choice((-1.0, 1.0), 100000)).astype(np.float32)
    assert np.all(np.isfinite(x)) and np.abs(x).min() < 1e-29 and np.abs(x).max() > 1e37
    got = ffi.bf16_round(x)
    assert got.dtype == np.float32 and same_bits(got, to_bf16(x))
    assert (got != x).mean() > 0.9                                    # (it does round)
    y = rng.standard_normal((37, 5)).astype(np.float32)
    assert ffi.bf16_round(y).shape == (37, 5) and same_bits(ffi.bf16_round(y[:, ::2]), to_bf16(y[:, ::2]))


def test_bf16_round_ties_and_specials():
    from aznet_hip import ffi
    # one binade, [256, 512): bf16 keeps 8 bits, so the spacing is 2; every float32 whose dropped 16 bits are 0x8000 is a tie
    top = np.arange(0x4380, 0x4400, dtype=np.uint32)                  # all 128 kept patterns: odd and even kept mantissas
    for sign in (0, 0x80000000):
        ties = ((top << 16) | 0x8000 | sign).astype(np.uint32).view(np.float32)
        got = ffi.bf16_round(ties)
        assert same_bits(got, to_bf16(ties))
        up = (got.view(np.uint32) >> 16) != (top | (sign >> 16))
        assert np.array_equal(up, (top & 1) == 1)                    # odd kept mantissa: up to even; even: stays
        for low in (0x7FFF, 0x8001, 0x0001, 0xFFFF):                 # next to the tie, and the ends
            v = ((top << 16) | low | sign).astype(np.uint32).view(np.float32)
            assert same_bits(ffi.bf16_round(v), to_bf16(v))
    x = np.array([257, 259, -257, -259, 258, 3.4e38, -3.4e38, np.finfo(np.float32).max, 0.0, -0.0, np.inf, -np.inf], np.float32)
    want = np.array([256, 260, -256, -260, 258, np.inf, -np.inf, np.inf, 0.0, -0.0, np.inf, -np.inf], np.float32)
    assert same_bits(ffi.bf16_round(x), want) and same_bits(to_bf16(x), want)
    nan = np.array([np.nan, -np.nan, 1.0], np.float32)
    got = ffi.bf16_round(nan)
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 1.0
    assert same_bits(B.q(np.array([257.0, 259.0])), np.array([256.0, 260.0]))       # float64 in, float64 out


# ---- 2. the conditions of the GPU tests ----------------------------------------------------------------------------------------
def test_integer_cases_stay_below_2_24():
    worst = 0.0
    for form in (0, 1, 2):
        for M, N in B.INT_MN:
            for K in B.INT_K:
                rng = np.random.Generator(np.random.PCG64(1000 * form + K))
                a, b, want = B.gemm_operands(form, M, N, K, B.integer_draw(rng))
                assert same_bits(B.q(a), a) and same_bits(B.q(b), b)  # -8..8: exact in bf16
                worst = max(worst, B.gemm_abs_sum(form, B.q(a), B.q(b)))
    M, N, K = B.INT_BIG
    for form in (0, 1):
        a, b, _ = B.gemm_operands(form, M, N, K, B.integer_draw(np.random.Generator(np.random.PCG64(form))))
        worst = max(worst, B.gemm_abs_sum(form, B.q(a), B.q(b)))
    for M, N, K in B.ROUND_SHAPES:
        for form in (0, 1, 2):
            for draw in (B.tie_draw, B.mixed_draw):
                rng = np.random.Generator(np.random.PCG64(7 * form + K))
                a, b, _ = B.gemm_operands(form, M, N, K, draw(rng))
                assert K <= 16
                worst = max(worst, B.gemm_abs_sum(form, B.q(a), B.q(b)), B.gemm_abs_sum(form, a, b))
    print("largest sum of |a||b| over all exact cases: %.0f (2^24 = %d)" % (worst, 2 ** 24))
    assert worst < 2 ** 24


def test_rounding_cases_do_round():
    """The tie operands need rounding in both directions and both signs, and the rounded product is not the exact one."""
    for M, N, K in B.ROUND_SHAPES:
        for form in (0, 1, 2):
            rng = np.random.Generator(np.random.PCG64(7 * form + K))
            a, b, exact = B.gemm_operands(form, M, N, K, B.tie_draw(rng))
            if a.size >= 64:
                d = B.q(a) - a
                assert (d > 0).any() and (d < 0).any() and (a > 0).any() and (a < 0).any()
            assert not np.array_equal(B.rounded_product(form, a, b), exact)
            rng = np.random.Generator(np.random.PCG64(7 * form + K))
            a, b, exact = B.gemm_operands(form, M, N, K, B.mixed_draw(rng))
            assert same_bits(B.q(a), a) and not same_bits(B.q(b), b)
            assert not np.array_equal(B.rounded_product(form, a, b), exact)


def test_random_cases_tell_bf16_from_fp32():
    for M, N, K in B.RANDOM_SHAPES:
        for form in (0, 1, 2):
            rng = np.random.Generator(np.random.PCG64(100 * form + M))
            a, b, fp = B.gemm_operands(form, M, N, K, B.normal_draw(rng))
            gap = B.rel_err(B.rounded_product(form, a, b), fp)
            print("form %d %dx%dx%d: the bf16 model is %.2e (relative) from the fp32 model" % (form, M, N, K, gap))
            assert gap > 1e-4


def _gates_agree(r64, r32, keys):
    for k in keys:
        miss = B.gate_mismatch(r32[k], r64[k])
        print("  %s: %.2e of the float32 gates differ from float64" % (k, miss))
        assert miss == 0.0, k


@pytest.mark.parametrize("name", sorted(D.HEADS))
def test_det_cases_float32_gates_equal_float64(name):
    head, fmap, blobs = B.det_case(name)
    pool, _ = D.roi_pool(fmap, blobs["rois"])
    masks = D.step_masks(3, 0, pool.shape[0], head)
    r64 = B.det_step(head, pool, blobs, masks)
    r32 = B.det_step(head, pool, blobs, masks, dtype=np.float32)
    _gates_agree(r64, r32, ("pre6", "pre7"))
    fp = D.step(head, pool, blobs, masks)
    gap, flips = B.rel_err(r64["pre6"], fp["pre6"]), B.gate_mismatch(r64["pre6"], fp["pre6"])
    print("%s: the bf16 model's pre6 is %.2e (relative) from the fp32 model's; %.2e of its gates differ" % (name, gap, flips))
    assert gap > 1e-4 and np.all(np.isfinite(r64["losses"]))
    assert B.rel_err(r32["grads"]["W6"], r64["grads"]["W6"]) < 1e-3


@pytest.mark.parametrize("name", sorted(B.AZ_CASES))
def test_az_cases_float32_gates_equal_float64(name):
    from aznet_hip import ffi
    head, fmap, blobs = B.az_case(name)
    pool, _ = R.roi_pool(fmap, blobs["rois"])
    n = pool.shape[0]
    masks = {t: ffi.dropout_mask(3, 0, l, n * head[k].shape[0]).reshape(n, -1) for t, l, k in ((6, 0, "b6"), (71, 1, "b71"), (72, 2, "b72"))}
    r64 = B.az_step(head, pool, blobs, masks)
    r32 = B.az_step(head, pool, blobs, masks, dtype=np.float32)
    _gates_agree(r64, r32, ("pre6", "pre71", "pre72"))
    assert B.rel_err(r64["pre6"], R.step(head, pool, blobs, masks)["pre6"]) > 1e-4


def test_skip_case_float32_gates_equal_float64():
    import skip_train_ref as T
    head, front, maps, blobs = B.skip_case()
    pooled = T.pool_argmax(maps, blobs["rois"])
    masks = D.step_masks(3, 0, blobs["rois"].shape[0], head)
    r64 = B.skip_step(head, front, maps, blobs, masks, pooled=pooled)
    r32 = B.skip_step(head, front, maps, blobs, masks, dtype=np.float32, pooled=pooled)
    _gates_agree(r64, r32, ("pre_pool", "pre6", "pre7"))
    fp = T.step(head, front, maps, blobs, masks, pooled=pooled)
    assert B.rel_err(r64["pre_pool"], fp["pre_pool"]) > 1e-4
    assert np.array_equal(r64["cat"], fp["cat"])                      # GRN and scale stay as they are


def test_restatements_equal_the_fp32_ones_on_bf16_exact_operands():
    """With every operand already a bf16 value the rounding is the identity: the bf16 restatement of a product is the plain
    one (what ties bf16_ref's graphs to det_step_ref's)."""
    rng = np.random.Generator(np.random.PCG64(3))
    for form in (0, 1, 2):
        a, b, want = B.gemm_operands(form, 9, 11, 13, B.integer_draw(rng))
        assert np.array_equal(B.rounded_product(form, a, b), want)
    head = B.integer_det_head(5, 4, 8, 8, 2)
    pool = rng.integers(-2, 3, (3, 4 * 49)).astype(np.float32) * (rng.random((3, 196)) < 0.1)
    z = np.zeros((3, 8), np.float32)
    blobs = {"labels": np.array([0, 1, 0], np.float32), "bbox_targets": z, "bbox_loss_weights": z}
    a, b = B.det_step(head, pool, blobs, None), D.step(head, pool, blobs, None)
    assert np.array_equal(a["pre6"], b["pre6"]) and np.abs(b["pre6"]).max() > 0


# ---- 3. the front door -----------------------------------------------------------------------------------------------------------
def test_config_key_and_value_error(monkeypatch):
    from detect import config
    assert config.cfg.TRAIN.PRECISION == "fp32" and config.train_precision() == 0
    assert config.train_precision("bf16") == 1 and config.train_precision("fp32") == 0
    for bad in ("fp16", "BF16", "", 1, None):
        if bad is None:
            continue
        with pytest.raises(ValueError, match="PRECISION"):
            config.train_precision(bad)
    monkeypatch.setattr(config.cfg.TRAIN, "PRECISION", "bf16")
    assert config.train_precision() == 1
    monkeypatch.setattr(config.cfg.TRAIN, "PRECISION", "fp8")
    with pytest.raises(ValueError, match="fp8"):
        config.train_precision()
    src = open(os.path.join(REPO, "az-net_amd", "lib", "detect", "config.py")).read()
    line = [l for l in src.splitlines() if "PRECISION=" in l]
    assert len(line) == 1 and "(not in the reference)" in line[0]


def test_yaml_sets_the_key(tmp_path, monkeypatch):
    from detect import config
    monkeypatch.setattr(config.cfg.TRAIN, "PRECISION", "fp32")
    y = tmp_path / "bf16.yml"
    y.write_text("TRAIN:\n  PRECISION: bf16\n")
    config.cfg_from_file(str(y))
    assert config.cfg.TRAIN.PRECISION == "bf16" and config.train_precision() == 1


@pytest.mark.parametrize("tool", ["train_az_net", "train_det_net"])
def test_bf16_flag_on_the_parser(tool, monkeypatch):
    monkeypatch.syspath_prepend(TOOLS)
    mod = importlib.import_module(tool)
    cli = importlib.import_module("_cli")
    parser = cli.build_parser("x", [mod.COMMON, mod.FLAGS])
    assert parser.parse_args(["--bf16"]).bf16 is True and parser.parse_args(["--iters", "4"]).bf16 is False
    row = [r for r in mod.FLAGS if r[0] == "--bf16"]
    assert len(row) == 1 and row[0][2].startswith("(extension)")
    src = open(os.path.join(TOOLS, tool + ".py")).read()
    assert "cfg.TRAIN.PRECISION = 'bf16'" in src


class FakeTrainer(object):
    """What _configure needs of a trainer, recording the calls."""

    def __init__(self, with_precision=True):
        self.calls = []
        if with_precision:
            self.set_precision = lambda p: self.calls.append(("set_precision", p))

    def set_hyper(self, lr, dc, drop):
        self.calls.append(("set_hyper", len(list(lr))))

    def set_skip_hyper(self, lr, dc):
        self.calls.append(("set_skip_hyper",))


def _bare_wrapper(kind, tmp_path, trainer):
    """A SolverWrapper with just what _configure reads: the train net's table, the trainer, no backbone."""
    from detect import prototxt as P
    net = str(tmp_path / ("train_%s.prototxt" % kind))
    if kind == "az":
        from detect.train_az import SolverWrapper
        P.write_train_prototxt(net, P.layer_table())
        param = P.read_train_net(net)
    else:
        from detect.train_det import SolverWrapper
        P.write_train_prototxt(net, P.det_layer_table(), name="frcnn_train")
        param = P.read_det_train_net(net)
    sw = SolverWrapper.__new__(SolverWrapper)
    sw.net_param, sw.trainer, sw.backbone, sw.skip = param, trainer, None, None
    return sw


@pytest.mark.parametrize("kind", ["az", "det"])
def test_solver_wrapper_sets_the_trainer_precision(kind, tmp_path, monkeypatch):
    from detect.config import cfg
    monkeypatch.setattr(cfg.TRAIN, "PRECISION", "bf16")
    tr = FakeTrainer()
    _bare_wrapper(kind, tmp_path, tr)._configure()
    assert ("set_precision", 1) in tr.calls and tr.calls[0][0] == "set_hyper"
    monkeypatch.setattr(cfg.TRAIN, "PRECISION", "fp32")
    tr = FakeTrainer()
    _bare_wrapper(kind, tmp_path, tr)._configure()
    assert [c for c in tr.calls if c[0] == "set_precision"] in ([], [("set_precision", 0)])
    old = FakeTrainer(with_precision=False)                           # a trainer object from before the mode: fp32 asks nothing of it
    _bare_wrapper(kind, tmp_path, old)._configure()
    assert [c[0] for c in old.calls] == ["set_hyper"]
    monkeypatch.setattr(cfg.TRAIN, "PRECISION", "half")
    with pytest.raises(ValueError, match="PRECISION"):
        _bare_wrapper(kind, tmp_path, FakeTrainer())._configure()


def test_header_states_the_mode():
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    import re
    assert int(re.search(r"#define\s+AZ_TRAIN_FP32\s+(\d+)", src).group(1)) == 0
    assert int(re.search(r"#define\s+AZ_TRAIN_BF16\s+(\d+)", src).group(1)) == 1
    from aznet_hip import ffi
    assert (ffi.AZ_TRAIN_FP32, ffi.AZ_TRAIN_BF16) == (0, 1)
    for name in ("az_solver_set_precision", "az_det_solver_set_precision", "az_solver_gemm_unit_prec"):
        assert name in src and name in ffi.SYMBOLS
