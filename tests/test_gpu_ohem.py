"""GPU: online hard-example mining (csrc/az_det_mine.hip, AzDetSolver.mine / mine_skip, TRAIN.OHEM in detect.train_det) against
the NumPy restatement tests/ohem_ref.py.

Row losses: the box term and the final add bit for bit (the library is built without contraction, so NumPy float32 restates
them); the softmax term and the whole loss within the suite's 8x rule -- max|got - ref64| / max|ref64| against 8 x the same
quantity of the float32 restatement, floor 1e-6 (det_step_ref.bound).  Selection: exact, against the restatement applied to
the device's own losses, and on the planted case against the float64 restatement from the maps on.  Every figure is printed
before it is asserted (run with -s)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bf16_ref as B
import det_step_ref as D
import det_train_ref as DR
import ohem_ref as O
import skip_ref as S
import skip_train_ref as T

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g21_train_det.npz")
FP32, BF16 = 0, 1
SEL_NCLS = 5
SEL_MAX = 256 + 257 + 600


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check(name, got, r64, r32):
    e_dev, e_cpu = D.rel_err(got, r64), D.rel_err(r32, r64)
    b = D.bound(e_cpu)
    print("  %-22s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (name, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    return e_dev <= b


def make_solver(ctx, head, max_rois, prec=FP32):
    from aznet_hip import ffi
    n6, n7, ncls = head["W6"].shape[0], head["W7"].shape[0], head["Wc"].shape[0]
    sol = ffi.AzDetSolver(ctx, head["W6"].shape[1] // 49, n6, n7, ncls, max_rois=max_rois, seed=1, head=head)
    sol.set_precision(prec)
    return sol


def dev(fmap):
    import torch
    return torch.from_numpy(np.ascontiguousarray(fmap)).cuda()


def zero_blobs(n, nb):
    z = np.zeros((n, nb))
    return {"labels": np.zeros(n), "bbox_targets": z, "bbox_loss_weights": z}


def head_forward(head, pool, dtype, prec, pin=None):
    """(cls_score, bbox_pred, a6, a7) of the TEST-phase head on pooled rows in the trainer's precision model (fp32:
    det_step_ref; bf16: bf16_ref's, both operands of every product rounded to bfloat16).  pin = (a6, a7) of the device: the
    activations that the next layer rounds are the device's -- see check_rows."""
    if prec == FP32:
        r = D.step(head, pool, zero_blobs(pool.shape[0], head["bb"].size), None, dtype=dtype, want_dpool=False)
        return r["cls_score"], r["bbox_pred"], r["a6"], r["a7"]
    P = {k: np.asarray(head[k], dtype) for k in D.KEYS}
    a6 = np.maximum(B.mm(np.asarray(pool, dtype), P["W6"].T) + P["b6"], 0)
    x6 = a6 if pin is None else np.asarray(pin[0], dtype)
    a7 = np.maximum(B.mm(x6, P["W7"].T) + P["b7"], 0)
    x7 = a7 if pin is None else np.asarray(pin[1], dtype)
    return B.mm(x7, P["Wc"].T) + P["bc"], B.mm(x7, P["Wb"].T) + P["bb"], a6, a7


# ---- 1. row losses ---------------------------------------------------------------------------------------------------------
ROW_HEADS = ["voc", "coco", 2, 64, 65, 128, 129, 256]


def row_case(name):
    if isinstance(name, str):
        head, fmap, _ = D.case(name)
        return head, fmap
    head = O.synth_head(100 + name, name)
    return head, O.synth_map(100 + name, head["W6"].shape[1] // 49)


def check_rows(sol, head, conv, blobs, prec, what):
    ncls = head["Wc"].shape[0]
    sel, n_sel, loss = sol.mine(conv, blobs["rois"], blobs["labels"], blobs["targets"], 0.7, 4, want_losses=True)
    got, cls, box = sol.fetch("mine_loss"), sol.fetch("mine_loss_cls"), sol.fetch("mine_loss_bbox")
    s_dev, b_dev, pool = sol.fetch("cls_score"), sol.fetch("bbox_pred"), sol.fetch("pool5")
    assert same_bits(loss, got) and got.shape == (blobs["rois"].shape[0],)
    # the box term and the final add: NumPy float32 restates them
    assert same_bits(box, O.bbox_loss32(b_dev, blobs["labels"], blobs["targets"])), what + ": mine_loss_bbox"
    assert same_bits(got, (cls + box).astype(np.float32)), what + ": mine_loss is not float32(cls + bbox)"
    # the softmax term from the device's own scores
    c64, c32 = O.cls_loss(s_dev, blobs["labels"], np.float64), O.cls_loss(s_dev, blobs["labels"], np.float32)
    ok = check(what + " cls", cls, c64, c32)
    # the whole loss from pool5 on.  bf16 mode: rounding an activation to bfloat16 is a step function, so an a6 / a7 within
    # float32 rounding of a step rounds one way on the device and the other way in float64, 2^-9 of its value apart, which no
    # implementation can avoid.  As the fp32 step tests give the device's ReLU gates to the restatement, this one gives it
    # the device's a6 and a7 as the operands of the next layer, after holding each of them to the same 8x rule.
    pin = (sol.fetch("a6"), sol.fetch("a7")) if prec == BF16 else None
    s64, b64, a6_64, a7_64 = head_forward(head, pool, np.float64, prec, pin)
    s32, b32, a6_32, a7_32 = head_forward(head, pool, np.float32, prec, pin)
    if pin is not None:
        free = head_forward(head, pool, np.float64, prec)
        flips = [int((B.q(np.asarray(f, np.float32)) != B.q(d)).sum()) for f, d in zip(free[2:], pin)]
        print("  %s: %d of a6's and %d of a7's bfloat16 roundings differ from the unpinned float64 model's" % (what, flips[0], flips[1]))
        ok &= check(what + " a6", pin[0], a6_64, a6_32) & check(what + " a7", pin[1], a7_64, a7_32)
    l64 = O.row_losses(s64, b64, blobs["labels"], blobs["targets"])[0]
    l32 = O.row_losses(s32, b32, blobs["labels"], blobs["targets"], np.float32)[0]
    ok &= check(what + " loss", got, l64, l32)
    # the forward is forward_test's
    sol.forward_test(conv, blobs["rois"])
    assert same_bits(sol.fetch("cls_score"), s_dev) and same_bits(sol.fetch("bbox_pred"), b_dev), what + ": forward differs from forward_test's"
    labs = set(int(v) for v in blobs["labels"])
    assert blobs["rois"].shape[0] < 3 or {0, 1, ncls - 1} <= labs
    return ok


@pytest.mark.parametrize("prec", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ROW_HEADS)
def test_row_losses(ctx, name, prec):
    head, fmap = row_case(name)
    ncls = head["Wc"].shape[0]
    sol = make_solver(ctx, head, 257, prec)
    conv = dev(fmap)
    ok = True
    for R in (1, 63, 64, 65, 257):
        blobs = O.pool_blobs(R + ncls, (R // 2, R - R // 2), ncls)
        ok &= check_rows(sol, head, conv, blobs, prec, "%s R=%d" % (name, R))
    sol.close()
    assert ok, "a row loss exceeds 8 x the float32-CPU error"


def test_row_loss_clamp(ctx):
    """Logits scaled until p[label] underflows: the row's loss is -log(FLT_MIN), in float64 as on the device."""
    head, fmap = row_case("voc")
    head = dict(head, Wc=head["Wc"] * np.float32(3000), bc=head["bc"] * np.float32(3000))
    sol = make_solver(ctx, head, 65)
    blobs = O.pool_blobs(3, (30, 35), 21)
    conv = dev(fmap)
    assert check_rows(sol, head, conv, blobs, FP32, "clamp")
    s = sol.fetch("cls_score").astype(np.float64)
    e = np.exp(s - s.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True))[np.arange(65), blobs["labels"].astype(int)]
    n = int((p < O.TINY).sum())
    print("  %d of 65 rows have p[label] below FLT_MIN" % n)
    assert n >= 5
    cls = sol.fetch("mine_loss_cls")[p < O.TINY]
    assert np.all(np.abs(cls - (-np.log(np.float64(O.TINY)))) <= 1e-5 * 87.4) and np.all(np.isfinite(sol.fetch("mine_loss")))
    sol.close()


# ---- 2. selection, exact ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(ctx):
    head = O.synth_head(31, SEL_NCLS)
    sol = make_solver(ctx, head, SEL_MAX)
    conv = dev(O.synth_map(31, head["W6"].shape[1] // 49, N=3))
    yield sol, conv
    sol.close()


def mine_and_check(sol, conv, blobs, N, thresh, per_image, what=""):
    """One mining call against the restatement on the device's own losses; returns (sel, n_sel, keep lists, raw bytes)."""
    sel, n_sel, loss = sol.mine(conv[:N], blobs["rois"], blobs["labels"], blobs["targets"], thresh, per_image, want_losses=True)
    R = blobs["rois"].shape[0]
    keep, nkeep = sol.fetch("mine_keep"), sol.fetch("mine_nkeep")
    assert sel.dtype == np.int32 and n_sel.dtype == np.int32 and keep.dtype == np.int32 and keep.shape == (R,) and nkeep.shape == (N,)
    assert same_bits(loss, sol.fetch("mine_loss"))
    w_sel, w_n, w_keeps = O.select(blobs["rois"], loss, N, thresh, per_image)
    off = O.image_ranges(blobs["rois"], N)
    print("  %s N=%d rows %s thresh %g per_image %d: kept %s, selected %s" % (what, N, np.diff(off).tolist(), thresh, per_image, nkeep.tolist(), n_sel.tolist()))
    assert np.array_equal(n_sel, w_n) and np.array_equal(sel, w_sel), what
    assert np.array_equal(nkeep, [k.size for k in w_keeps]) and np.array_equal(keep, O.keep_array(w_keeps, off, R)), what
    return sel, n_sel, w_keeps, (sel.tobytes(), n_sel.tobytes(), keep.tobytes(), nkeep.tobytes(), loss.tobytes())


@pytest.mark.parametrize("counts", [(1,), (255,), (256,), (257,), (600,), (0, 40, 30), (40, 0, 30), (40, 30, 0), (257, 256), (256, 257, 600)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_selection_over_images_and_both_nms_paths(rig, counts):
    sol, conv = rig
    blobs = O.pool_blobs(sum(counts), counts, SEL_NCLS)
    assert sum(counts) <= sol.max_rois and (counts != (256, 257, 600) or sum(counts) == sol.max_rois)
    for thresh in (0.0, 0.7, 1.0):
        mine_and_check(sol, conv, blobs, len(counts), thresh, 64, "counts")


def test_selection_per_image_at_and_around_the_survivors(rig):
    sol, conv = rig
    blobs = O.pool_blobs(5, (300, 90), SEL_NCLS)
    _, _, keeps, _ = mine_and_check(sol, conv, blobs, 2, 0.7, 1, "per_image 1")
    n0, n1 = keeps[0].size, keeps[1].size
    assert 1 < n1 < 90 and 1 < n0 < 300
    for per in (n1, n1 + 1, n0, n0 + 7, 300):
        sel, n_sel, _, _ = mine_and_check(sol, conv, blobs, 2, 0.7, per, "per_image")
        assert n_sel.tolist() == [min(per, n0), min(per, n1)]


def test_selection_duplicates_and_identical_rows(rig):
    sol, conv = rig
    blobs = O.pool_blobs(8, (300, 120), SEL_NCLS, dup=60)
    same = np.flatnonzero(np.all(blobs["rois"][1:] == blobs["rois"][:-1], axis=1)) + 1
    assert same.size >= 40
    for thresh in (0.0, 0.7, 1.0):
        mine_and_check(sol, conv, blobs, 2, thresh, 64, "duplicates")
    loss = sol.fetch("mine_loss")
    assert same_bits(loss[same], loss[same - 1]), "exact duplicates must have equal loss bits"
    for n in (257, 64):                                                       # all rows one row: both NMS paths
        one = {k: np.repeat(v[:1], n, axis=0) for k, v in blobs.items()}
        sel, n_sel, _, _ = mine_and_check(sol, conv, one, 1, 0.7, 64, "identical")
        assert sel.tolist() == [n - 1] and n_sel.tolist() == [1]              # the highest index goes first, the rest overlap it
        sel, n_sel, _, _ = mine_and_check(sol, conv, one, 1, 1.5, 64, "identical, thresh above 1")
        assert sel.tolist() == list(range(n - 1, n - 65, -1))


def test_selection_repeats_and_survives_a_larger_call(rig):
    sol, conv = rig
    small = O.pool_blobs(12, (270, 33), SEL_NCLS)
    big = O.pool_blobs(13, (256, 257, 600), SEL_NCLS)
    a = mine_and_check(sol, conv, small, 2, 0.7, 64, "first")[3]
    b = mine_and_check(sol, conv, small, 2, 0.7, 64, "second")[3]
    assert a == b, "two calls in a row differ"
    mine_and_check(sol, conv, big, 3, 0.7, 64, "larger")
    c = mine_and_check(sol, conv, small, 2, 0.7, 64, "after the larger call")[3]
    assert a == c, "a call after a larger call differs (stale scratch)"


# ---- 3. the planted case against float64 -----------------------------------------------------------------------------------
def test_planted_case_selects_what_float64_selects(ctx):
    head, fmap, blobs, info = O.planted_case()
    P = O.PLANT
    sol = make_solver(ctx, head, blobs["rois"].shape[0])
    sel, n_sel, loss = sol.mine(dev(fmap), blobs["rois"], blobs["labels"], blobs["targets"], P["thresh"], P["per_image"], want_losses=True)
    assert check("planted loss", loss, info["loss64"], info["loss32"])
    w_sel, w_n, w_keeps = O.select(blobs["rois"], info["loss64"], 2, P["thresh"], P["per_image"])
    assert np.array_equal(sel, w_sel) and np.array_equal(n_sel, w_n)
    assert np.array_equal(sol.fetch("mine_keep"), O.keep_array(w_keeps, O.image_ranges(blobs["rois"], 2), blobs["rois"].shape[0]))
    sol.close()


# ---- 4. the skip front -----------------------------------------------------------------------------------------------------
def test_mine_skip(ctx):
    from aznet_hip import ffi, synth
    import torch
    head, front, maps, blobs = T.case("small")
    d = T.SMALL
    rois = blobs["rois"]
    R = rois.shape[0]
    rng = np.random.Generator(np.random.PCG64(2))
    targets = (rng.standard_normal((R, 4)) * 1.5).astype(np.float32)
    sol = make_solver(ctx, head, R)
    tmaps = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in maps]
    with pytest.raises(ffi.AzError) as e:
        sol.mine_skip(tmaps, rois, blobs["labels"], targets, 0.7, 16)
    assert e.value.code == ffi.AZ_ERR_STATE
    sol.attach_skip(d["Cs"], S.SCALES, gain=front["gain"], eps=front["eps"], seed=1, front=front)
    with pytest.raises(ffi.AzError) as e:
        sol.mine(torch.zeros(1, d["Cout"], 6, 8).cuda(), rois, blobs["labels"], targets, 0.7, 16)
    assert e.value.code == ffi.AZ_ERR_STATE
    for thresh, per in ((0.7, 16), (0.0, 3), (1.0, R)):
        sel, n_sel, loss = sol.mine_skip(tmaps, rois, blobs["labels"], targets, thresh, per, want_losses=True)
        w_sel, w_n, w_keeps = O.select(rois, loss, 1, thresh, per)
        assert np.array_equal(sel, w_sel) and np.array_equal(n_sel, w_n)
        assert np.array_equal(sol.fetch("mine_keep"), O.keep_array(w_keeps, [0, R], R))
    cat, s_dev, b_dev = sol.fetch("cat"), sol.fetch("cls_score"), sol.fetch("bbox_pred")
    assert same_bits(sol.fetch("mine_loss_bbox"), O.bbox_loss32(b_dev, blobs["labels"], targets))
    assert check("skip cls", sol.fetch("mine_loss_cls"), O.cls_loss(s_dev, blobs["labels"], np.float64), O.cls_loss(s_dev, blobs["labels"], np.float32))
    sol.forward_test_skip(tmaps, rois)
    assert same_bits(sol.fetch("cls_score"), s_dev) and same_bits(sol.fetch("bbox_pred"), b_dev) and same_bits(sol.fetch("cat"), cat)
    ictx = ffi.AzContext(0, max_regions=512)
    try:
        ictx.load_head(synth.make_head(seed=3, C=d["Cout"], n6=4, n71=4, n72=4))
        ictx.load_det_head(head)
        ictx.load_skip_front(dict(front, Cs=d["Cs"], scales=S.SCALES))
        ictx.set_skip_maps(tmaps)
        assert same_bits(cat, ictx.skip_pool(rois, normalise=True)), "cat after mining differs from az_skip_pool's bits"
    finally:
        ictx.close()
    sol.close()


# ---- 5. refusals and state -------------------------------------------------------------------------------------------------
def raw_mine(sol, conv, rois, labels, targets, thresh, per, sel, n_sel):
    import ctypes
    lead, _r, _ = sol._pass_args(conv, rois)
    f, i32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    return sol.L.az_det_solver_mine(sol.h, *(list(lead) + [p(labels, f), p(targets, f), float(thresh), int(per), p(sel, i32), p(n_sel, i32), None]))


def test_refusals_leave_the_outputs_and_the_trainer_alone(ctx):
    from aznet_hip import ffi
    head, fmap = row_case("voc")
    sol = make_solver(ctx, head, 64)
    conv = dev(fmap)
    blobs = O.pool_blobs(4, (30, 34), 21)
    rois, lab, tgt = blobs["rois"], blobs["labels"], blobs["targets"]
    good = sol.mine(conv, rois, lab, tgt, 0.7, 8, want_losses=True)
    sel, n_sel = np.full(16, -7, np.int32), np.full(2, -7, np.int32)
    swapped = rois.copy()
    swapped[[0, 40]] = swapped[[40, 0]]
    bad_lab = [lab.copy() for _ in range(3)]
    bad_lab[0][3], bad_lab[1][3], bad_lab[2][3] = 21, -1, 0.5
    more = np.vstack([rois, rois[:1]])
    cases = [("null labels", (rois, None, tgt, 0.7, 8, sel, n_sel)), ("null sel_out", (rois, lab, tgt, 0.7, 8, None, n_sel)),
             ("null n_sel_out", (rois, lab, tgt, 0.7, 8, sel, None)), ("per_image 0", (rois, lab, tgt, 0.7, 0, sel, n_sel)),
             ("thresh < 0", (rois, lab, tgt, -0.1, 8, sel, n_sel)), ("thresh nan", (rois, lab, tgt, float("nan"), 8, sel, n_sel)),
             ("thresh inf", (rois, lab, tgt, float("inf"), 8, sel, n_sel)), ("decreasing image index", (swapped, lab, tgt, 0.7, 8, sel, n_sel)),
             ("R above max_rois", (more, np.append(lab, 0).astype(np.float32), np.vstack([tgt, tgt[:1]]), 0.7, 8, sel, n_sel))]
    cases += [("label %r" % float(b[3]), (rois, b, tgt, 0.7, 8, sel, n_sel)) for b in bad_lab]
    for what, args in cases:
        rc = raw_mine(sol, conv, *args)
        print("  %-24s -> %d  %s" % (what, rc, ctx.last_error() if hasattr(ctx, "last_error") else ""))
        assert rc == ffi.AZ_ERR_INVALID, what
        assert np.all(sel == -7) and np.all(n_sel == -7), what
    again = sol.mine(conv, rois, lab, tgt, 0.7, 8, want_losses=True)
    assert all(same_bits(a, b) for a, b in zip(good, again)), "the trainer is not usable as before"
    # without targets there is no box term
    _, _, no_box = sol.mine(conv, rois, lab, None, 0.7, 8, want_losses=True)
    assert same_bits(no_box, sol.fetch("mine_loss_cls")) and not np.any(sol.fetch("mine_loss_bbox"))
    # a NaN bias: found through the flag after the pass, nothing handed over
    sol.load({"bc": np.where(np.arange(21) == 0, np.nan, head["bc"]).astype(np.float32)})
    rc = raw_mine(sol, conv, rois, lab, tgt, 0.7, 8, sel, n_sel)
    assert rc == ffi.AZ_ERR_INVALID and np.all(sel == -7) and np.all(n_sel == -7)
    assert np.isnan(sol.fetch("cls_score")).any()
    sol.load({"bc": head["bc"]})
    again = sol.mine(conv, rois, lab, tgt, 0.7, 8, want_losses=True)
    assert all(same_bits(a, b) for a, b in zip(good, again))
    # an update straight after a mining pass has no gradients to apply
    with pytest.raises(ffi.AzError):
        sol.update(0.01, 0.9, 0.0005, 1.0)
    sol.close()


def test_mining_leaves_gradients_history_and_the_accumulate_flag_alone(ctx):
    head, fmap, mb = D.case("voc")
    conv = dev(fmap)
    pool = O.pool_blobs(6, (20, 17), 21)
    step = lambda s, it: s.step(conv, mb["rois"], mb["labels"], mb["bbox_targets"], mb["bbox_loss_weights"], 5, it)
    grads = lambda s: [s.fetch("g_" + k) for k in D.KEYS]
    a, b = make_solver(ctx, head, 64), make_solver(ctx, head, 64)
    # a plain step gives the bits it gives without a mining pass before it
    b.mine(conv, pool["rois"], pool["labels"], pool["targets"], 0.7, 8)
    la, lb = step(a, 0), step(b, 0)
    assert same_bits(la[0], lb[0]) and la[1] == lb[1] and all(same_bits(x, y) for x, y in zip(grads(a), grads(b)))
    for s in (a, b):
        s.update(0.01, 0.9, 0.0005, 1.0)
    # step; mine; step accumulates what step; step accumulates
    for s in (a, b):
        s.set_accumulate(0)
        step(s, 1)
        s.set_accumulate(1)
    b.mine(conv, pool["rois"], pool["labels"], pool["targets"], 0.7, 8)
    la, lb = step(a, 2), step(b, 2)
    assert same_bits(la[0], lb[0]) and la[1] == lb[1] and all(same_bits(x, y) for x, y in zip(grads(a), grads(b)))
    for s in (a, b):
        s.update(0.01, 0.9, 0.0005, 0.5)
    pa, pb, ha, hb = a.read(), b.read(), a.read_history(), b.read_history()
    assert all(same_bits(pa[k], pb[k]) and same_bits(ha[k], hb[k]) for k in D.KEYS) and all(np.any(ha[k]) for k in D.KEYS)
    a.close()
    b.close()


# ---- 6. through SolverWrapper ------------------------------------------------------------------------------------------------
OHEM_CFG = dict(OHEM=True, OHEM_NMS=0.7, OHEM_POOL=160)


def ohem_wrapper(ctx, g, tmp, monkeypatch, name, iter_size=1):
    """detect.train_det.SolverWrapper under TRAIN.OHEM on det_step_ref.TRAJ's rig (width-reduced frozen backbone, reduced head,
    synthetic_375x500_8 with the golden's proposals), built and seeded the same way at every call."""
    from aznet_hip import ffi
    from detect import prototxt as P
    from detect.config import cfg
    from detect.train_det import SolverWrapper
    from roi_data_layer import roidb as rdl
    for k, v in OHEM_CFG.items():
        monkeypatch.setattr(cfg.TRAIN, k, v)
    sub = tmp / name
    sub.mkdir()
    ffi.set_default_context(ctx)
    imdb, _, _ = DR.synthetic_roidb(rdl, g, sub, monkeypatch)
    np.random.seed(D.TRAJ["np_seed"])
    sol = D.traj_solver_files(str(sub))
    if iter_size != 1:
        P.write_solver_prototxt(sol, P.read_solver(sol)["train_net"], **dict(D.TRAJ["solver"], iter_size=iter_size))
    sw = SolverWrapper(sol, imdb, str(sub / "out"), backbone=D.traj_backbone("cuda:0"), ctx=ctx,
                       dims=dict(n6=D.TRAJ["n6"], n7=D.TRAJ["n7"]), seed=D.TRAJ["solver_seed"])
    assert sw.trainer.max_rois == 2 * OHEM_CFG["OHEM_POOL"] and sw.iter_size == iter_size
    return sw


def test_solver_wrapper_mines_every_iteration(ctx, g, tmp_path, monkeypatch):
    from roi_data_layer.minibatch import _get_bbox_regression_labels
    sw = ohem_wrapper(ctx, g, tmp_path, monkeypatch, "w")
    pools = []
    forward = sw.layer.forward

    def recording():
        pools.append(forward())
        return pools[-1]
    monkeypatch.setattr(sw.layer, "forward", recording)
    # a fixed probe minibatch: the pool of the first two entries on the current backbone
    probe = sw.layer.get_ohem_minibatch([sw.layer._roidb[0], sw.layer._roidb[1]], sw.num_classes, ctx)
    probe = {k: np.asarray(v).astype(np.float32) for k, v in probe.items()}
    state = np.random.get_state()

    def probe_loss():
        conv = sw.backbone.forward_train(probe["data"]).detach()
        return float(np.mean(sw.trainer.mine(conv, probe["rois"], probe["labels"], probe["targets"], 0.7, 64, want_losses=True)[2], dtype=np.float64))
    before = probe_loss()
    np.random.set_state(state)
    for it in range(D.TRAJ["steps"]):
        sw.step()
        pool, mb, sel = pools[-1], sw.last_blobs, sw.last_sel
        R = pool["rois"].shape[0]
        assert R <= 2 * OHEM_CFG["OHEM_POOL"] and sorted(pool) == ["data", "labels", "rois", "targets"]
        loss = sw.trainer.fetch("mine_loss")
        assert loss.shape == (R,)
        w_sel, w_n, w_keeps = O.select(pool["rois"], loss, 2, 0.7, 64)
        assert np.array_equal(sel, w_sel), "iteration %d: the selection is not the restatement's on the device's losses" % it
        bt, bw = _get_bbox_regression_labels(np.hstack((pool["labels"][sel, None], pool["targets"][sel])), sw.num_classes)
        assert same_bits(mb["rois"], pool["rois"][sel]) and same_bits(mb["labels"], pool["labels"][sel])
        assert same_bits(mb["bbox_targets"], bt) and same_bits(mb["bbox_loss_weights"], bw) and mb["data"] is pool["data"]
        m = sw.last_mining
        assert m["pool"] == R and m["selected"] == w_n.tolist() and m["kept"] == [k.size for k in w_keeps]
        assert m["fg"] == int((pool["labels"][sel] > 0).sum())
        assert m["pool_loss"] == float(np.mean(loss, dtype=np.float64)) and m["mined_loss"] == float(np.mean(loss[sel], dtype=np.float64))
        assert sw.trainer.last_rows == sel.size
        if it % 5 == 0:
            print("  iteration %2d: %s" % (it, sw._display_extra()))
    after = probe_loss()
    print("  mean pool loss of the probe minibatch: %.4f before, %.4f after %d iterations" % (before, after, D.TRAJ["steps"]))
    assert after < before
    sw.trainer.close()


def test_solver_wrapper_resume_is_exact_under_mining(ctx, g, tmp_path, monkeypatch):
    """fp32, iter_size 2: 3 iterations + save_state + restore into a fresh wrapper + 3 iterations equal 6 straight."""
    def state(sw):
        w, h = sw._trainer_state()
        st = np.random.get_state()
        return ({k: v.tobytes() for k, v in w.items()}, {k: v.tobytes() for k, v in h.items()}, st[1].tobytes(), st[2], sw.iter,
                sw.layer._perm.tobytes(), int(sw.layer._cur), sw.last_mining, [l.tobytes() for l in sw.losses[-3:]])
    a = ohem_wrapper(ctx, g, tmp_path, monkeypatch, "a", iter_size=2)
    for _ in range(6):
        a.step()
    end_a = state(a)
    a.trainer.close()
    b = ohem_wrapper(ctx, g, tmp_path, monkeypatch, "b", iter_size=2)
    for _ in range(3):
        b.step()
    path = b.save_state()
    b.trainer.close()
    c = ohem_wrapper(ctx, g, tmp_path, monkeypatch, "c", iter_size=2)
    np.random.seed(4711)
    assert c.restore(path) == 3 and c.last_mining is None
    for _ in range(3):
        c.step()
    end_c = state(c)
    assert len(end_a) == len(end_c)
    for i, (x, y) in enumerate(zip(end_a, end_c)):
        assert x == y, "part %d of the state differs" % i
    c.trainer.close()


# ---- 7. the tool -----------------------------------------------------------------------------------------------------------
def test_train_det_tool_with_ohem_then_test_det_net_loads_it():
    import shutil
    tools = os.path.join(REPO, "az-net_amd", "tools")
    exp = "train_det_ohem_tool_test_%d" % os.getpid()
    out_dir = os.path.join(REPO, "az-net_amd", "output", exp)
    try:
        out = subprocess.run([sys.executable, os.path.join(tools, "train_det_net.py"), "--ohem", "--net", "synthetic:8", "--imdb",
                              "synthetic_375x500_8", "--iters", "4", "--exp", exp], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:], out.stderr[-3000:])
        assert out.returncode == 0
        snap = os.path.join(out_dir, "synthetic_375x500_8", "vgg16_frcnn_iter_4.caffemodel")
        assert os.path.exists(snap) and "Iteration 0, loss" in out.stdout and "mining: pool = " in out.stdout
        sys.path.insert(0, tools)
        try:
            import test_det_net
        finally:
            sys.path.remove(tools)
        net = test_det_net.load_frcnn_net(snap, 0)
        assert net.name == "vgg16_frcnn_iter_4" and net.ctx.det_dims["ncls"] == 21 and net.ctx.det_dims["n6"] == 4096 // 8
        net.ctx.close()
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
