#!/usr/bin/env python3
"""Times the full-size detection-net head training step (C = 512, n6 = n7 = 4096, ncls = 21, R = 128 rows over two 38 x 63
maps; forward + backward + update, conv5_3 resident): the HIP trainer (az_det_solver_step + az_det_solver_update) and, in the
same process on the same card, a torch-ROCm statement of the same step (torch.addmm, autograd, the same update).  Prints both
(warm-up, then the median of --reps), the per-kernel table (az_set_profiling), every GEMM against the fp32-MFMA rate and the
update against the copy rate az_measure_box reports on this card; then add_bbox_regression_targets on synthetic_600x1000_64
with flips (seeded proposals) against the NumPy restatement.  Not collected by pytest; it lives under tests/ because it uses
the tests' case builders.

  python tests/perf_det_train_step.py [--reps 20] [--warmup 3] [--no-targets]"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "az-net_amd", "lib"), REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FULL = dict(C=512, n6=4096, n7=4096, ncls=21)


def torch_step(P, H, conv, blobs, masks, geom, rate, mom, wd, clip_at):
    """The same step in torch-ROCm: RoIPool by indexing with a precomputed arg-max (a gather; its backward an index_add),
    torch.addmm layers, cross_entropy and SmoothL1, autograd, then the update on every blob."""
    import torch
    flat = conv.reshape(conv.shape[0] * conv.shape[1], -1)
    x = torch.where(geom["ok"], flat.reshape(-1)[geom["idx"]], torch.zeros((), device=conv.device))
    a6 = torch.relu(torch.addmm(P["b6"], x, P["W6"].t())) * masks[0]
    a7 = torch.relu(torch.addmm(P["b7"], a6, P["W7"].t())) * masks[1]
    n = x.shape[0]
    loss = torch.nn.functional.cross_entropy(torch.addmm(P["bc"], a7, P["Wc"].t()), blobs["labels"], reduction="sum") / n
    d = blobs["bbox_loss_weights"] * (torch.addmm(P["bb"], a7, P["Wb"].t()) - blobs["bbox_targets"])
    loss = loss + torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).sum() / n
    for p in P.values():
        p.grad = None
    conv.grad = None
    loss.backward()
    with torch.no_grad():
        norm = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in P.values()))
        clip = torch.clamp(clip_at / norm, max=1.0).float()
        for k, p in P.items():
            bias = k.startswith("b")
            g = p.grad * clip + (0.0 if bias else wd) * p
            H[k].mul_(mom).add_(g, alpha=rate * (2.0 if bias else 1.0))
            p.sub_(H[k])
    return loss


def median_ms(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out))


def seeded_proposals(gt_roidb, w, h, per_image=300):
    rng = np.random.RandomState(7)
    out = []
    for e in gt_roidb:
        gt = e["boxes"].astype(np.float64)
        near = np.repeat(gt, 20, axis=0) + rng.uniform(-25, 25, (20 * gt.shape[0], 4))
        x = np.sort(rng.uniform(0, w - 1, (per_image, 2)), axis=1)
        y = np.sort(rng.uniform(0, h - 1, (per_image, 2)), axis=1)
        b = np.vstack((near, np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1)))
        b[:, 0::2] = np.clip(b[:, 0::2], 0, w - 1)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, h - 1)
        out.append(np.stack([np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 0], b[:, 2]),
                             np.maximum(b[:, 1], b[:, 3])], 1).astype(np.float32))
    return out


def time_targets(ctx):
    import tempfile
    import pickle
    import det_train_ref as DR
    from datasets.synthetic import SyntheticImdb
    from detect import config
    from detect.train_det import get_training_roidb
    from roi_data_layer import roidb as rdl
    tmp = tempfile.mkdtemp()
    config.cfg.ROOT_DIR, config.cfg.EXP_DIR = tmp, "perf"
    imdb = SyntheticImdb(600, 1000, 64)
    net = DR.FakeNet()
    out = config.get_output_dir(imdb, net)
    os.makedirs(out)
    with open(os.path.join(out, "proposals.pkl"), "wb") as f:
        pickle.dump(seeded_proposals(imdb.gt_roidb(), 1000, 600), f, pickle.HIGHEST_PROTOCOL)
    get_training_roidb(imdb, net)
    boxes = sum(e["ex_boxes"].shape[0] for e in imdb.roidb)
    res = {}
    for name, backend in (("HIP (az_det_targets + az_det_target_stats)", None), ("NumPy restatement", DR.RefBackend())):
        rdl.set_backend(backend)
        best = []
        for _ in range(3 if backend is None else 1):
            t0 = time.perf_counter()
            res[name] = rdl.add_bbox_regression_targets(imdb.roidb, imdb.num_classes)
            best.append((time.perf_counter() - t0) * 1e3)
        print("add_bbox_regression_targets, %d images, %d example boxes, %s: best %.1f ms of %d" % (len(imdb.roidb), boxes, name, min(best), len(best)))
    rdl.set_backend(None)
    a, b = list(res.values())
    print("  means agree to %.2e, stds to %.2e" % (np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-targets", action="store_true")
    args = ap.parse_args()
    import torch
    import det_step_ref as D
    import train_step_ref as R
    from aznet_hip import ffi, synth
    ctx = ffi.AzContext(0)
    ffi.set_default_context(ctx)
    mfma, copy = ctx.measure_box()
    print("this card: %.1f TFLOP/s fp32 MFMA (register loop), %.2f TB/s float4 copy (read + written)" % (mfma, copy))
    d = FULL
    Rn, K6, nb = 128, d["C"] * 49, 4 * d["ncls"]
    head = D.filler_head(5, **d)
    fmap = np.concatenate([synth.make_feature_map(s, 512, 38, 63) for s in (31, 32)], axis=0)
    blobs = D.random_blobs(11, Rn, 2, 38, 63, d["ncls"])
    sol = ffi.AzDetSolver(ctx, d["C"], d["n6"], d["n7"], d["ncls"], max_rois=Rn, head=head)
    conv = torch.from_numpy(fmap).cuda()
    dmap = torch.empty_like(conv)
    it = [0]

    def hip_step():
        _, sq = sol.step(conv, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"], 3, it[0], dmap=dmap)
        sol.update(0.001, 0.9, 0.0005, R.clip_scale(sq, 20.0))
        it[0] += 1
    hip_med, hip_min = median_ms(hip_step, args.reps, args.warmup, lambda: None)       # (both calls are synchronous)
    print("HIP trainer, full-size detection head step (forward + backward with d conv5_3 + update): median %.3f ms, best %.3f ms of %d"
          % (hip_med, hip_min, args.reps))
    ctx.set_profiling(2 | 4)
    hip_step()
    times = ctx.last_kernel_times()
    ctx.set_profiling(0)
    f6, f7 = 2.0 * Rn * K6 * d["n6"], 2.0 * Rn * d["n6"] * d["n7"]
    fc, fb = 2.0 * Rn * d["n7"] * d["ncls"], 2.0 * Rn * d["n7"] * nb
    flops = {"fc6_fwd": f6, "fc6_dx": f6, "fc6_dw": f6, "fc7_fwd": f7, "fc7_dx": f7, "fc7_dw": f7,
             "cls_score_fwd": fc, "cls_score_dx": fc, "cls_score_dw": fc, "bbox_pred_fwd": fb, "bbox_pred_dx": fb, "bbox_pred_dw": fb}
    nparam = sum(int(np.prod(v.shape)) for v in head.values())
    agg, order = {}, []
    for name, _, ms in times:
        if name not in agg:
            agg[name] = [0, 0.0]
            order.append(name)
        agg[name][0] += 1
        agg[name][1] += ms
    print("per launch group (HIP events on the trainer's stream, one step):")
    for name in order:
        n, ms = agg[name]
        note = ""
        if name in flops:
            tf = flops[name] / (ms * 1e-3) / 1e12
            note = "%6.1f TFLOP/s = %4.1f %% of the card's fp32-MFMA rate" % (tf, 100.0 * tf / mfma)
            if name.startswith("fc6"):
                note += "; %s %.0f MB = %.2f TB/s" % ("writes" if name == "fc6_dw" else "streams", 4e-6 * K6 * d["n6"],
                                                      4.0 * K6 * d["n6"] / (ms * 1e-3) / 1e12)
        if name == "sgd_update":
            tb = 5.0 * 4.0 * nparam / (ms * 1e-3) / 1e12          # reads w, g, hist; writes w, hist
            note = "%.2f TB/s = %4.1f %% of the card's copy rate" % (tb, 100.0 * tb / copy)
        print("  %-16s x%-2d %9.3f ms  %s" % (name, n, ms, note))
    print("  sum %.3f ms in %d launch groups" % (sum(v[1] for v in agg.values()), sum(v[0] for v in agg.values())))
    sol.close()
    del sol

    # ---- the torch-ROCm statement of the same step -------------------------------------------------------------------
    dev = conv.device
    P = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in head.items()}
    Hh = {k: torch.zeros_like(v) for k, v in P.items()}
    pool, arg = R.roi_pool(fmap, blobs["rois"])
    C, HW = fmap.shape[1], fmap.shape[2] * fmap.shape[3]
    rows = (blobs["rois"][:, 0].astype(np.int64)[:, None] * C + np.repeat(np.arange(C), 49)[None, :]) * HW
    geom = {"idx": torch.from_numpy(rows + np.maximum(arg, 0)).to(dev), "ok": torch.from_numpy(arg >= 0).to(dev)}
    tb = {k: torch.from_numpy(v).to(dev) for k, v in blobs.items() if k != "rois"}
    tb["labels"] = tb["labels"].long()
    masks = [torch.from_numpy(ffi.dropout_mask(3, 0, l, Rn * n).reshape(Rn, n).astype(np.float32) * 2).to(dev)
             for l, n in ((0, d["n6"]), (1, d["n7"]))]
    tconv = conv.clone().requires_grad_(True)
    t_med, t_min = median_ms(lambda: torch_step(P, Hh, tconv, tb, masks, geom, 0.001, 0.9, 0.0005, 20.0), args.reps, args.warmup,
                             torch.cuda.synchronize)
    print("torch-ROCm statement of the same step (addmm, autograd, same update; dropout masks and arg-max given): median %.3f ms, "
          "best %.3f ms of %d" % (t_med, t_min, args.reps))
    print("HIP / torch = %.2f" % (hip_med / t_med))
    del P, Hh
    torch.cuda.empty_cache()
    if not args.no_targets:
        time_targets(ctx)


if __name__ == "__main__":
    main()
