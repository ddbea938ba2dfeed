#!/usr/bin/env python3
"""Headline benchmark: AZ proposals/sec on synthetic 600x1000 images (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

One step = one pass of the hot path over one image: az_propose on the cached VGG16 conv5_3 map -- the level loop
of lib/detect/test.py:346-414 (roi projection + dedup, RoIPool, fc head, decode, filter, zoom select,
divide_region, ..., top-300), 300 proposals copied back to the host.  The conv5_3 map is resident in HBM when the
timed region starts (it is the hot path's input); the PyTorch backbone is timed separately (`end_to_end`).
`value` is the search as a caller with ANY Tz gets it -- no use of "Tz <= 0, so the tree is known" (that plan is the
extra key `one_pass`) -- at the Tz given (default 0: SURVEY 8d's full, deterministic tree).  The context picks the form of
that search from the row counts of its previous search of the image shape: at Tz = 0 the history is a FULL tree, so the
search's one head pass evaluates the full tree's 688 unique rois and every level finds its outputs by RoIPool window
(`config.search_form` says which form ran).  A pruned tree -- what tools/prop_az.py's cfg_set_mode('Test', Tz > 0),
config.py:272-280, produces -- takes other forms: `tz_sweep` times the same image at Tz = the 0.1 / 0.3 / 0.5 / 0.7
quantiles of its zoom scores, each with its regions per level, rows per head pass, fraction of its own floor and the
number of searches that had to be run twice; `level_loop_without_whole_tree_pass` is Tz = 0 in the two-pass form.
Images shard one-per-GPU (rank r owns image seeds r, r + N, ...; weak scaling); proposals are exchanged with one
RCCL all-gather per batch of images -- also on ONE GPU (a one-rank "nccl" group), so that N = 1 times the same
code path as N = 8.

Prints ONE compact JSON line on rank 0 (< 4 KB: the contract's keys, `roofline` for the dominant kernel -- the fp32-MFMA
fc GEMMs, timed by the launches themselves during the timed steps --, `path_floor`).  A plain run does only that: set up,
warm up, time the --steps steps, write the last step's outputs (--dump-outputs DIR), print the line.  The conv5_3 maps it
times on are VGG16's on the synthetic images, computed on the host CPU (bitwise the same from run to run, whatever the GPU
libraries would pick), so that two builds of the project can be compared output for output.

--full adds everything else that is measured: in the line `cpu_baseline` = the oracle's NumPy / C / BLAS restatement on
the host cores, `value_200_steps`, `box` = what THIS box sustains; in the record file (--extras-file, default
bench_extras.json beside this script) the kernel table and the side legs: `one_pass`, `tz_sweep`, `calibrated_tz`,
`stream_tz` (distinct images at a tuned threshold, lockstep batches), `deep_tree` (BASELINE config 4, both network scales),
`shared_detection` (config 3), `nms`, `end_to_end` (the PyTorch-ROCm backbone on the GPU), `cli`.  The --no-* switches
leave parts of it out.  None of it goes into the printed line: round 5's 30 KB line came back from the driver as
`parsed: null`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "az-net_amd", "lib"))
sys.path.insert(0, REPO)

H_IM, W_IM = 600, 1000
NUM_PROPOSALS = 300
# per RoI 216 119 808 FLOP for the whole head = 2*(25088*4096 + 4096*1024 + 4096*256 +
# 1024*55 + 256).  int6 and int7_1|int7_2 (99.95 % of it) run in the fc GEMM kernels: their
# algorithmic flops per RoI are 2*(25088*4096 + 4096*1280); the 56-output tail is a vector-ALU kernel.
HEAD_FLOP_PER_ROI = 216119808
GEMM_FLOP_PER_ROI = 2 * (25088 * 4096 + 4096 * 1280)
PEAK_F32_MFMA_TFLOPS = 157.3
HBM_PEAK = 8.0e12
VGG16_FLOP_600x1000 = 367.7e9


def t_min_us(unique_per_level, fmap_elems):
    """Hot-path floor of BASELINE.md section 3: per level max(bytes / 8 TB/s, flops / 157.3 TF)."""
    tot = 0.0
    for U in unique_per_level:
        if U <= 0:
            continue
        b = 432239616 + 21728 + 4 * fmap_elems + U * 244
        f = U * HEAD_FLOP_PER_ROI
        tot += max(b / HBM_PEAK, f / (PEAK_F32_MFMA_TFLOPS * 1e12))
    return tot * 1e6


def merged_floor_us(unique_per_level, pass_levels, fmap_elems):
    """The floor of the passes that RAN: every head pass that evaluated rois of the tree streams the weights once and does
    the flops of the tree levels it covered (az_stats.pass_levels) -- max(bytes / 8 TB/s, flops / 157.3 TF) per pass.  A
    search that merges levels into one pass is bounded by THIS, not by t_min_us (one weight stream per level), so a
    fraction of it never exceeds 1."""
    tot = 0.0
    for m in pass_levels:
        U = sum(u for l, u in enumerate(unique_per_level) if (int(m) >> l) & 1)
        if U <= 0:
            continue
        b = 432239616 + 21728 + 4 * fmap_elems + U * 244
        tot += max(b / HBM_PEAK, U * HEAD_FLOP_PER_ROI / (PEAK_F32_MFMA_TFLOPS * 1e12))
    return tot * 1e6


def merged_floor_batches(sts, bs, fmap_elems):
    """(floor in us per image, mean rows per pass) of lockstep batches (az_batch_launch) from the per-image az_stats, `bs`
    consecutive ones per batch: a batch's first pass covers tree levels 1-2 of all its images, every later pass one level of
    all of them; a pass streams the weights ONCE for the batch and does the flops of all its rows."""
    tot, n_img, rows = 0.0, 0, []
    for g0 in range(0, len(sts), bs):
        grp = sts[g0:g0 + bs]
        nlev = int(grp[0].n_levels)
        uq = [[int(st.level_unique[l]) for l in range(nlev)] for st in grp]
        per_pass = [sum(u[0] + u[1] for u in uq)] + [sum(u[l] for u in uq) for l in range(2, nlev)]
        rows.append(per_pass)
        for U in per_pass:
            if U <= 0:
                continue
            b = 432239616 + 21728 + 4 * fmap_elems * len(grp) + U * 244
            tot += max(b / HBM_PEAK, U * HEAD_FLOP_PER_ROI / (PEAK_F32_MFMA_TFLOPS * 1e12))
        n_img += len(grp)
    width = max(len(r) for r in rows)
    mean_rows = [float(np.mean([r[i] if i < len(r) else 0 for r in rows])) for i in range(width)]
    return tot * 1e6 / max(n_img, 1), mean_rows


def floors(st, fmap_elems, measured_us):
    """path_floor entry of one search from its az_stats: BASELINE.md section 3's per-level floor and the merged-pass floor
    of the form that ran, with `frac` = merged-pass floor / measured (<= 1 by construction)."""
    uq = [int(st.level_unique[l]) for l in range(st.n_levels)]
    pl = [int(x) for x in list(st.pass_levels)[:int(st.n_passes)]]
    per_level = t_min_us(uq, fmap_elems)
    merged = merged_floor_us(uq, pl, fmap_elems)
    return {"t_min_us_per_image": per_level, "merged_pass_t_min_us": merged, "frac": merged / measured_us,
            "per_level_floor_over_measured": per_level / measured_us, "head_passes": len(pl)}


FLOOR_NOTE = ("t_min_us_per_image = BASELINE.md section 3: sum over the LEVELS of max(bytes / 8 TB/s, flops / 157.3 TF), one weight "
              "stream per level; merged_pass_t_min_us = the same sum over the head PASSES that ran (a pass that covers several "
              "levels streams the weights once: az_stats.pass_levels); frac = merged_pass_t_min_us / measured, which no search can "
              "exceed; per_level_floor_over_measured may exceed 1 for a search that merges levels")


COMPACT_LIMIT = 4096          # bytes; the driver keeps 8 KB of stdout tail (round 5's 30 KB line was unreadable to it)


def _r(x, nd=6):
    """floats to `nd` significant digits (the compact line is for reading and parsing, the extras file keeps every bit)"""
    if isinstance(x, float):
        return float("%.*g" % (nd, x)) if x == x and abs(x) != float("inf") else None
    if isinstance(x, dict):
        return {k: _r(v, nd) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, nd) for v in x]
    if isinstance(x, (np.floating,)):
        return _r(float(x), nd)
    if isinstance(x, (np.integer,)):
        return int(x)
    return x


def _pick(d, keys):
    return {k: d[k] for k in keys if d is not None and k in d}


def compact_line(out, extras_file=None):
    """The ONE line bench.py prints: the contract's keys, `roofline`, `cpu_baseline` and a handful of cross-checks -- strict
    JSON, under COMPACT_LIMIT bytes whatever the side measurements produced (they live in the extras file)."""
    cfg = out.get("config") or {}
    rf = out.get("roofline") or {}
    line = _pick(out, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                       "vs_baseline", "dtype", "data"))
    wl = str(cfg.get("workload_short") or cfg.get("workload") or "")
    c = _pick(cfg, ("search_form", "rows_per_head_pass", "regions_per_level", "unique_rois_per_level", "image_hw",
                    "num_proposals", "Tz", "parallelism", "lanes_per_context", "searches_run_twice_in_timed_region"))
    c = dict({"workload": wl[:400]}, **c)
    g = cfg.get("gather")
    if g is not None:
        c["gather"] = str(g)[:80]
    line["config"] = c
    line["rccl"] = _pick(out.get("rccl") or {}, ("backend", "world", "collectives", "error"))
    r = _pick(rf, ("bound", "achieved", "peak", "unit", "frac", "frac_of_sustained", "traffic", "algorithmic_bytes",
                   "flops_per_launch", "avg_launch_ms", "launches_per_step", "steps_timed"))
    r["kernel"] = str(rf.get("kernel_short") or rf.get("kernel") or "")[:160]
    line["roofline"] = r
    if out.get("path_floor"):
        line["path_floor"] = _pick(out["path_floor"], ("t_min_us_per_image", "merged_pass_t_min_us", "frac",
                                                       "per_level_floor_over_measured", "head_passes"))
    if out.get("value_200_steps"):
        line["value_200_steps"] = _pick(out["value_200_steps"], ("steps", "ms_per_step", "value"))
    if out.get("box"):
        line["box"] = _pick(out["box"], ("sustained_fp32_mfma_tflops", "copy_tb_per_s"))
    cb = out.get("cpu_baseline")
    if cb:
        cc = _pick(cb, ("value", "unit", "cores", "kind", "host_cpus"))
        cc["sample"] = str(cb.get("sample", ""))[:200]
        line["cpu_baseline"] = cc
        line["gpu_over_cpu"] = out.get("gpu_over_cpu")
    if extras_file:
        line["extras_file"] = extras_file
    s = json.dumps(_r(line), allow_nan=False, separators=(", ", ": "))
    if len(s) > COMPACT_LIMIT:            # (cannot happen with the fields above; a hard stop rather than an unreadable record)
        for k in ("box", "path_floor", "value_200_steps"):
            line.pop(k, None)
        line["config"] = {"workload": wl[:200]}
        s = json.dumps(_r(line), allow_nan=False, separators=(", ", ": "))
    assert len(s) <= COMPACT_LIMIT, len(s)
    return s


def write_extras(out, path=None):
    """Everything measured (the compact line's source and every side leg) as one JSON file; returns the paths written."""
    paths = [path] if path else [os.path.join(REPO, "bench_extras.json")]
    if not path and os.path.isdir(os.path.join(REPO, "gpurun_out")):
        paths.append(os.path.join(REPO, "gpurun_out", "bench_extras.json"))
    done = []
    for p in paths:
        try:
            with open(p, "w") as f:
                json.dump(out, f, indent=1, default=lambda o: _r(o))
                f.write("\n")
            done.append(p)
        except OSError as e:
            sys.stderr.write("bench.py: could not write %s: %s\n" % (p, e))
    return done


DUMP_LIMIT = 64 << 20         # bytes: --dump-outputs writes at most this much


def dump_outputs(outdir, arrays):
    """--dump-outputs: each array as DIR/<name>.npy, float32 or float64 as computed; returns the bytes written."""
    os.makedirs(outdir, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        total += a.nbytes
        assert total <= DUMP_LIMIT, total
        np.save(os.path.join(outdir, name + ".npy"), a)
    return total


def host_blob(im, scale):
    """_get_image_blob (lib/detect/test.py:27-59) on the host for an image the test scale leaves as it is (scale 1: the
    resize is the identity): BGR minus the (float64) pixel means, rounded once to float32, [1, 3, H, W]."""
    from detect.config import cfg
    assert scale == 1.0, scale
    b = (im.astype(np.float64) - cfg.PIXEL_MEANS).astype(np.float32)
    return np.ascontiguousarray(b.transpose(2, 0, 1)[None])


def cpu_baseline(head, fmap, Tz, budget_s=20.0):
    """The oracle (kind "port") on the host, as SURVEY 8(d) specifies the CPU baseline: NumPy geometry exactly as
    lib/detect/test.py (one thread), C divide_region / RoIPool, and the fc head through torch CPU `addmm` as the stand-in for
    Caffe-CPU's sgemm.  SURVEY names torch.set_num_threads(os.cpu_count()); on a box whose process may not use every logical
    CPU that setting is several times SLOWER than a moderate one (256 threads: 280 GFLOP/s, 32 threads: 2200 on the round-5
    boxes), so the thread count is the fastest of a short sweep on int6's shape -- the baseline is not handicapped -- and the
    sweep is reported with the cores used."""
    import torch
    from oracle import az_oracle as orc
    ncpu = os.cpu_count() or 1
    try:
        usable = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        usable = ncpu
    x = torch.randn(517, 25088)
    w = torch.from_numpy(head["W6"])
    b = torch.from_numpy(head["b6"])
    sweep = {}
    for nt in sorted({t for t in (8, 16, 32, 64, 128, ncpu) if t <= ncpu}):
        torch.set_num_threads(nt)
        best = 1e9
        for _ in range(3):
            t = time.time()
            torch.addmm(b, x, w.t())
            best = min(best, time.time() - t)
        sweep[nt] = 2.0 * 517 * 25088 * 4096 / best / 1e9
    cores = max(sweep, key=lambda k: sweep[k])
    orc.set_fc_backend("torch", threads=cores)
    try:
        net = orc.OracleNet(head, feat_fn=lambda d: fmap)
        cfg = orc.OracleCfg(Tz=Tz)
        nets = {"full": net, "fc": net}
        orc.im_propose(nets, (H_IM, W_IM), 1.0, cfg)          # warm-up
        times = []
        t0 = time.time()
        while len(times) < 3 or (time.time() - t0 < budget_s and len(times) < 30):
            t = time.time()
            orc.im_propose(nets, (H_IM, W_IM), 1.0, cfg)
            times.append(time.time() - t)
        med = float(np.median(times))
        head_flops = 688 * HEAD_FLOP_PER_ROI if Tz <= 0 else None
    finally:
        orc.set_fc_backend("numpy")
    return {"value": NUM_PROPOSALS / med, "unit": "proposals/s", "cores": int(cores), "host_cpus": int(ncpu),
            "cpus_this_process_may_use": int(usable), "kind": "port",
            "fc_backend": "torch CPU addmm, torch.set_num_threads(cores); geometry on one thread",
            "sgemm_gflops_int6_shape": sweep[cores],
            "sgemm_gflops_by_threads": {str(k): v for k, v in sorted(sweep.items())},
            "head_gflops_per_image": (head_flops / 1e9) if head_flops else None,
            "achieved_head_gflops": (head_flops / 1e9 / med) if head_flops else None,
            "sample": "%d images of the same 600x1000 workload at Tz=%g (median %.3f s/image), "
                      "hot path only (conv5_3 given)" % (len(times), Tz, med)}


def self_launch(n):
    """Run this script under torch.distributed.run with n ranks on 127.0.0.1; the parent never
    initialises HIP (no torch.cuda call, no exec after GPU init) -- it only waits and relays."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    argv = [a for a in sys.argv[1:] if a != "--launcher"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=None, text=True)
    last_json = None
    for line in proc.stdout:
        if line.startswith("{") and '"metric"' in line:
            last_json = line.rstrip("\n")
        else:
            sys.stderr.write(line)
    rc = proc.wait()
    if rc == 0 and last_json is None:
        sys.stderr.write("bench.py: the ranks exited without printing a result line\n")
        rc = 1
    if last_json is not None:
        print(last_json)
        sys.stdout.flush()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tz", type=float, default=0.0, help="zoom threshold; 0 = full tree (deterministic work)")
    ap.add_argument("--gather-every", type=int, default=8, help="images per rank per RCCL gather")
    ap.add_argument("--launcher", action="store_true",
                    help="start the ranks through torch.distributed.run also for --gpus 1 (the plumbing N > 1 uses)")
    ap.add_argument("--no-rccl", action="store_true", help="single GPU: no process group, no gather in the timed loop")
    ap.add_argument("--native-gather", action="store_true",
                    help="the batch exchange as the library's own ncclAllGather on the ctx stream (az_gather_records) instead "
                         "of torch.distributed's all_gather_into_tensor")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run everything besides the headline: the CPU baseline, the box calibration, the kernel table, "
                         "the 200-step loop behind a short run, and the side measurements (other search forms, Tz sweeps, "
                         "streams of distinct images, BASELINE configs 3 / 4, NMS sizes, backbone + search end to end, the CLI "
                         "loop); the --no-* switches leave parts out.  They land in the extras file, never in the printed line. "
                         "Without it: set-up, warm-up, the timed steps and the line only")
    ap.add_argument("--extras", action="store_true", help="the earlier name of --full")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (its proposals, float64 [n, 4], "
                         "and scores, float32 [n]) as DIR/<name>.npy")
    ap.add_argument("--extras-file", default=None,
                    help="where the full record goes (default: bench_extras.json beside this script, and a copy under gpurun_out/ "
                         "when that directory exists)")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--inflight", type=int, default=1,
                    help="images in flight per GPU in the timed region (each on its own az_ctx/stream); "
                         "1 = strictly one at a time, which keeps the per-kernel event timing clean")
    ap.add_argument("--no-pipelined", action="store_true", help="(accepted and ignored: the three-context leg was retired in round 6)")
    ap.add_argument("--no-two-pass", action="store_true", help="skip the level loop without the whole-tree pass (extra key)")
    ap.add_argument("--no-fast", action="store_true", help="skip the 16-bit-term modes (az_set_gemm_mode 2 / 3) measurement")
    ap.add_argument("--one-pass", action="store_true",
                    help="time the one-pass form (Tz <= 0 only: all levels' rois in one head pass) as the main measurement")
    ap.add_argument("--level-loop", action="store_true", help="(default since round 3) the level-by-level form is `value`")
    ap.add_argument("--no-one-pass", action="store_true", help="skip the extra one-pass measurement of the same search")
    ap.add_argument("--no-level-loop", action="store_true", help="(with --one-pass) skip the extra level-by-level measurement")
    ap.add_argument("--no-calibrated", action="store_true",
                    help="skip the extra data-dependent run (Tz = median zoom score of this image's regions)")
    ap.add_argument("--lanes", type=int, default=1,
                    help="az_set_lanes for the timed loops: 2 = the context's queued searches take turns between two streams, so "
                         "consecutive images overlap on the GPU (one context, queue-ahead); 1 = one stream, strictly one "
                         "image at a time on the GPU (reported as `one_lane` either way)")
    ap.add_argument("--no-one-lane", action="store_true", help="skip the extra one-lane measurement of the same loop")
    ap.add_argument("--no-stream", action="store_true", help="skip stream_tz (distinct images in dataset order at a threshold tuned over the set)")
    ap.add_argument("--stream-images", type=int, default=32, help="images per set of stream_tz")
    ap.add_argument("--no-sweep", action="store_true", help="skip tz_sweep (the same image at four quantiles of its zoom scores)")
    ap.add_argument("--e2e-pipelined", action="store_true",
                    help="also time backbone(i+1) overlapped with search(i) (measured slower than the serial order on most boxes)")
    ap.add_argument("--no-box", action="store_true", help="skip the box calibration (sustained MFMA rate, copy bandwidth)")
    ap.add_argument("--no-extras", action="store_true", help="skip deep_tree / shared_detection / nms")
    ap.add_argument("--profile-all", action="store_true", help="HIP-event time every launch group (perturbs timing)")
    ap.add_argument("--sync-gather", action="store_true", help="blocking all-gather + host copy inside the loop")
    ap.add_argument("--no-queue-ahead", action="store_true",
                    help="launch image i+1 only after image i has been fetched (the GPU then idles ~40 us per image while "
                         "the host turns around)")
    ap.add_argument("--queue-depth", type=int, default=0,
                    help="searches the host keeps launched and unfetched (0 = 3: a lane's queue holds three, so the next "
                         "images' chip-wide kernels are already queued behind the one the GPU works on)")
    ap.add_argument("--event-every", type=int, default=5,
                    help="HIP events around the fc GEMM launches of every n-th timed step (1: every step, ~30 us/step of stream time)")
    ap.add_argument("--maps", type=int, default=4, help="distinct images (conv5_3 maps) per GPU rotated through the timed loop")
    args = ap.parse_args()
    args.full = args.full or args.extras
    if not args.full:
        # a plain run measures the headline only: every side measurement is --full's
        for k in ("no_e2e", "no_pipelined", "no_two_pass", "no_fast", "no_one_pass", "no_level_loop", "no_calibrated",
                  "no_one_lane", "no_stream", "no_sweep", "no_extras", "no_cpu_baseline", "no_box"):
            setattr(args, k, True)

    if (args.gpus > 1 or args.launcher) and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N`: start the N ranks as fresh processes (one per GPU, RCCL) BEFORE this
        # process touches the GPU, relay rank 0's JSON line and exit with the launcher's code.
        sys.exit(self_launch(args.gpus))

    # The contract is ONE line on stdout.  Libraries below us (RCCL prints its version banner from C) write to file
    # descriptor 1 too: from here on fd 1 is stderr, and the result line goes to a private copy of the real stdout.
    sys.stdout.flush()
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    from aznet_hip import ffi, synth
    from aznet_hip.net import HipAZNet, HipDetNet
    from aznet_hip.backbone import VGG16Conv5
    from aznet_hip import dist as azdist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d" % (world, args.gpus)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # The exchange step runs over RCCL whatever N is: under a launcher the rendezvous comes from the environment;
    # a bare `python bench.py` (N = 1) makes a one-rank group on 127.0.0.1.  If that cannot be built on this box
    # the single-GPU run goes on without the gather and says so in the line.
    rccl = {"backend": None, "collectives": 0}
    if world > 1 or "WORLD_SIZE" in os.environ:
        dist.init_process_group("nccl", device_id=dev)
        rccl["backend"] = "nccl"
    elif not args.no_rccl:
        try:
            import socket
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=dev)
            rccl["backend"] = "nccl"
        except Exception as e:                                 # noqa: BLE001 -- reported, never hidden
            rccl["error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
    dist_on = rccl["backend"] is not None

    head = synth.make_head(seed=1234, **synth.FULL_DIMS)
    from detect.test import _get_image_blob, _im_scale
    # images owned by this rank: seeds rank, rank + world, ... (BASELINE config 5 is one image per GPU; the
    # timed loop rotates through args.maps of them so that no step re-reads the previous step's map)
    ims = [synth.make_image(rank + world * j, H_IM, W_IM) for j in range(max(1, args.maps))]
    im = ims[0]
    scale0 = float(_im_scale(im.shape)[0])
    # The hot path's input, conv5_3 of each image: the seeded VGG16 on the host CPU, its last layer scaled to a unit-RMS map
    # on the first image (random-init weights; stands in for training).  Computed there, the maps are the same bits from
    # run to run; MIOpen's algorithm search on the GPU is not (and may compile for a while on first use).
    host_bb = VGG16Conv5(device="cpu", seed=4321)
    host_blobs = [host_blob(x, scale0) for x in ims]
    host_bb.normalize_output(host_blobs[0])
    # resident in HBM from here on, channel-last (the layout RoIPool reads, as the GPU backbone hands it over)
    convs = [host_bb(b).to(dev).contiguous(memory_format=torch.channels_last) for b in host_blobs]
    del host_bb, host_blobs
    conv = convs[0]
    backbone = blob = blobs = None
    if args.full:
        # the PyTorch-ROCm backbone of the end-to-end legs (plumbing: conv5_3 comes out [H][W][C] and is borrowed in place;
        # channels_last compute + MIOpen's benchmark search, set before the first forward, is the fastest fp32
        # configuration found for the fixed 600x1000 shape)
        torch.backends.cudnn.benchmark = True
        backbone = VGG16Conv5(device=dev, seed=4321, channels_last_out=True, channels_last_compute=True)
    net = HipAZNet(head, backbone=backbone, device=local_rank, name="vgg16_az_net_hip", max_regions=4096)
    net.ctx.set_lanes(args.lanes)
    if args.full:
        blob = _get_image_blob(im, net)[0]                   # HIP front-end kernel -> CUDA tensor
        backbone.normalize_output(blob)                      # random-init weights: unit-RMS conv5_3
        blobs = [_get_image_blob(x, net)[0] for x in ims]
    net.set_conv(conv)
    one_pass_main = bool(args.one_pass) and args.tz <= 0.0

    def mk(static):
        return ffi.AzContext.make_params(H_IM, W_IM, scale0, args.tz, num_proposals=NUM_PROPOSALS, static_tree=static)

    params = mk(one_pass_main)

    def barrier():
        # (a barrier among ONE rank has nobody to wait for: only the device synchronisation is left of it -- RCCL's barrier
        #  is an all-reduce launch plus a stream wait, ~0.3 ms, which a 20-step timed region would carry as 1 %)
        if dist_on and world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def maxr(x):
        if world > 1:
            tt = torch.tensor([x], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return float(tt.item())
        return x

    gat = azdist.DeviceGather(net.ctx, NUM_PROPOSALS, args.gather_every, dev, native=args.native_gather) if dist_on else None
    # extra contexts for pipelining independent images on one GPU (same weights, same map)
    nets = [net] + [HipAZNet(head, backbone=backbone, device=local_rank, name=net.name, max_regions=4096)
                    for _ in range(args.inflight - 1)]
    for n in nets[1:]:
        n.set_conv(conv)

    def run(nsteps, prm):
        """nsteps images, one after the other on the one ctx stream.  The host enqueues image i+1's launch sequence
        (and the device-to-device staging of its record) while the GPU still works on image i, then waits for image i:
        the searches never overlap on the GPU, but the GPU does not idle while Python turns around (--no-queue-ahead:
        launch only after the previous fetch).  Every gather_every images per rank (and at the end): ONE RCCL
        all-gather of the staged records, then the host copy of all ranks' proposals; consecutive batches use
        alternating send buffers."""
        ge = args.gather_every

        def launch(i):
            if ev_every[0] and args.profile_all:
                # (--profile-all: an event pair per launch group costs ~7 us of stream time each: every 5th step only)
                net.ctx.set_profiling((2 | 4) if i % ev_every[0] == 0 else 4)
            # this step's image: its map is handed over with the launch
            net.ctx.propose_launch(prm, fmap=convs[i % len(convs)], producer_done=True)
            if gat is not None:
                # (the pair this batch stages into carried the batch before the previous one: its exchange, begun a whole
                #  batch ago, is collected before the pair is written again)
                while i % ge == 0 and inflight and inflight[0][2] == (i // ge) % 2:
                    collect()
                gat.stage(i % ge, buf=(i // ge) % 2)

        inflight = []

        def collect():
            h, n_b, _ = inflight.pop(0)
            assert len(gat.gather_end(h)) == world * n_b

        def done(i):
            # The exchange of a finished batch is only STARTED here (collective + host copy on a side stream, pinned
            # buffer); its proposals are collected one batch later, or at the end -- the host never sits in a
            # synchronous wait for RCCL while the next image's kernels hold the CUs (--sync-gather: the blocking form).
            if gat is not None and ((i + 1) % ge == 0 or i == nsteps - 1):
                n_b = i % ge + 1
                if args.sync_gather:
                    assert len(gat.gather(n_b, buf=(i // ge) % 2)) == world * n_b
                else:
                    if inflight:
                        collect()
                    inflight.append((gat.gather_begin(n_b, buf=(i // ge) % 2), n_b, (i // ge) % 2))
                rccl["collectives"] += 1
            if i == nsteps - 1:
                while inflight:
                    collect()

        if args.inflight == 1:
            trace = step_trace
            launched = 0
            for i in range(nsteps):
                t_i = time.perf_counter()
                while launched < min(nsteps, i + depth):
                    launch(launched)
                    launched += 1
                last[0] = net.ctx.propose_fetch(want_scores=True, want_stats=True)
                reruns[0] += int(last[0][2].n_reruns)
                done(i)
                if trace is not None:
                    trace.append((time.perf_counter() - t_i) * 1e3)
            return
        assert world == 1, "--inflight > 1 is a single-GPU measurement"
        q = []
        for i in range(nsteps):
            n = nets[i % len(nets)]
            if len(q) == len(nets):
                last[0] = q.pop(0).ctx.propose_fetch(want_scores=True, want_stats=True)
            n.ctx.propose_launch(prm, fmap=convs[i % len(convs)], producer_done=True)
            q.append(n)
        for m in q:
            last[0] = m.ctx.propose_fetch(want_scores=True, want_stats=True)

    # searches launched and not yet fetched in the loops below
    # (one lane: the lane's queue holds three -- its stage-1 kernels of the next two images sit behind the current one's, so
    #  neither the host's turn-around nor the batch exchange ever leaves the stream empty: 1.156 -> 1.126 ms per image)
    depth = 1 if args.no_queue_ahead else (args.queue_depth if args.queue_depth > 0 else 3)
    reruns = [0]                       # searches of the loop that had to be run twice (az_stats.n_reruns)
    last = [None]                      # (boxes, scores, stats) of the loop's last step, as its caller receives them
    ev_every = [0]                     # > 0: HIP events around the fc GEMM launches of every ev_every-th step
    step_trace = []                    # host-side wall time of every step of the loop (diagnostics: median / tail in the line)

    # one-time initialisation per image shape (the search's shape-dependent pre-pass / plan, first-use allocations): not
    # a step, but timed and reported (`plan_build_ms`)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    net.propose(params)
    first_ms = (time.perf_counter() - t0) * 1e3
    for n in nets[1:]:
        n.propose(params)
    # (no garbage-collector pause inside a timed region: a generation-2 collection of this process -- torch, numpy, the
    #  411 MB of head arrays -- takes 30-50 ms, i.e. +0.17 ms per step when it lands among 200 timed steps.  It is run
    #  HERE, before the warm-up: 40 ms of idle GPU right in front of a timed region would start it at idle clocks.)
    import gc
    gc.collect()
    gc.disable()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    net.propose(params)
    steady_ms = (time.perf_counter() - t0) * 1e3
    # The chip leaves its idle clocks only gradually: the first ~30 ms of work after an idle gap (the collection above) run
    # ~3 % slow.  40 untimed steps bring it to the state a dataset run is in; then the W warm-up steps of the contract.
    # The fc GEMM launches of EVERY timed step time themselves (az_set_profiling bit 3: first workgroup in to last
    # workgroup out on the GPU's 100 MHz clock): nothing on the stream, and exact with two lanes, where an event pair
    # would also span the time a launch waits for the other lane's GEMM to release the CUs.  Switched on HERE (it
    # allocates and clears the span ring: a synchronisation and a copy, i.e. an idle GPU for ~1 ms), the spans of the
    # warm-up steps are dropped right in front of the timed region by a call that does not touch the GPU (bit 4).
    for n in nets:
        n.ctx.set_profiling(0)
        n.ctx.set_profiling(8 | 4)
    run(40, params)
    run(args.warmup, params)           # the W untimed warm-up steps, right in front of the timed region
    rccl["collectives"] = 0
    for n in nets:
        n.ctx.set_profiling(8 | 4 | 16)
    ev_every[0] = args.event_every if (args.inflight == 1 and args.profile_all) else 0
    barrier()
    del step_trace[:]
    reruns[0] = 0
    t0 = time.perf_counter()
    run(args.steps, params)
    t_loop = time.perf_counter() - t0
    barrier()
    dt = maxr(time.perf_counter() - t0)
    reruns_timed = reruns[0]
    Y_last, S_last, st_last = last[0]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"proposals": Y_last, "scores": S_last})
    steps_ms = np.array(step_trace[:args.steps]) if step_trace else np.zeros(1)
    ev_every[0] = 0
    n_timed_steps = args.steps
    ktimes = []
    for n in nets:
        ktimes += n.ctx.last_kernel_times()
        n.ctx.set_profiling(0)
    # `value` is EXACTLY --steps steps (the contract); with --full a short run (the driver's 20 steps are a 25 ms timed
    # region) is backed by the same loop over 200 steps, reported beside it
    long_run = None
    if args.full and args.steps < 100 and args.inflight == 1:
        barrier()
        t0 = time.perf_counter()
        run(200, params)
        barrier()
        d200 = maxr(time.perf_counter() - t0)
        long_run = {"steps": 200, "ms_per_step": d200 / 200 * 1e3, "value": world * NUM_PROPOSALS * 200 / d200,
                    "unit": "proposals/s", "note": "the same timed loop over 200 steps, right behind the --steps run"}
    box = None
    gc.enable()
    n_tab, tab_times = 6, []
    if args.full:
        # every launch group of the search against ITS bound, from HIP events on a few extra, untimed steps (an event pair
        # per launch group perturbs the stream by ~7 us each, so these steps are not part of `value`)
        net.set_conv(conv)
        for i in range(30):            # (reading the spans back left the GPU idle for a few ms: back to working clocks first)
            net.ctx.propose_launch(params, fmap=convs[i % len(convs)], producer_done=True)
            net.ctx.propose_fetch()
        net.ctx.set_profiling(2 | 4)
        for i in range(n_tab):
            net.ctx.propose_launch(params, fmap=convs[i % len(convs)], producer_done=True)
            net.ctx.propose_fetch()
        tab_times = net.ctx.last_kernel_times()
        net.ctx.set_profiling(0)
        net.set_conv(conv)             # (the loops left their last map in the context)
        Y, S, st = net.propose(params, want_scores=True, want_stats=True)
    else:
        Y, S, st = Y_last, S_last, st_last                   # (the search's figures: those of the last timed step)
    uniq = [int(st.level_unique[l]) for l in range(st.n_levels)]
    regions = [int(st.level_regions[l]) for l in range(st.n_levels)]
    spec_rows = int(st.spec_rows)
    fmap_elems = int(conv.numel())

    def rows_per_pass(s):
        """rows of the head passes of a level-by-level search, from its stats (see az_stats in include/aznet_hip.h)"""
        try:
            return [int(x) for x in list(s.pass_rows)[:int(s.n_passes)]]
        except AttributeError:
            return None

    out = None
    if rank == 0:
        ms_step = dt / args.steps * 1e3
        value = world * NUM_PROPOSALS * args.steps / dt
        gemm = [(n, l, ms) for (n, l, ms) in ktimes if n.endswith("_gemm")]
        gemm_ms_total = sum(ms for _, _, ms in gemm)
        n_launch = max(len(gemm), 1)
        flops_per_image = sum(uniq) * GEMM_FLOP_PER_ROI
        achieved = flops_per_image * n_timed_steps / (gemm_ms_total * 1e-3) / 1e12 if gemm_ms_total > 0 else 0.0
        # HBM bytes per launch from rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE,
        # separate runs); cannot be collected live, so it is read from the committed summary.
        prow_all = rows_per_pass(st) or []
        traffic, traffic_source = None, None
        tfile = os.path.join(REPO, "profiles", "roofline_traffic.json")
        if os.path.exists(tfile):
            try:
                tj = json.load(open(tfile))
                traffic = tj.get("hbm_bytes_per_launch")
                traffic_source = ("profiles/roofline_traffic.json (%s): rocprofv3 --pmc passes of this command, "
                                  "FETCH_SIZE x2 (gfx950) + WRITE_SIZE per launch; NOT measured in this run"
                                  % tj.get("source", "committed summary"))
            except Exception:
                traffic = None
        # SURVEY 8(d)'s algorithmic bytes of the fc GEMMs per launch: the weights of int6 / int7_1|int7_2 once per head pass
        # (what the traffic counters are read against), averaged over the launches of a step like `traffic`
        alg_bytes = (len(prow_all) * (25088 * 4096 + 4096 * 1280) * 4.0 / max(n_launch / max(n_timed_steps, 1), 1e-9)) if prow_all else None
        # the int6 launch shapes, each against ITS bound: max(weights / 8 TB/s, flops / 157.3 TF)
        fc6 = {}
        for n, l, ms in ktimes:
            if n == "fc6_gemm":
                fc6.setdefault(l, []).append(ms)
        prow = rows_per_pass(st)
        fc6_shapes = []
        for pi, (l, v) in enumerate(sorted(fc6.items())):
            if st.static_plan:
                rows, label = spec_rows, "all levels (one pass)"
            elif prow is not None and pi < len(prow):
                rows, label = prow[pi], ("pass %d (first level %s)" % (pi + 1, "2" if l < 0 else str(l + 1)))
            else:
                rows = spec_rows if l < 0 else uniq[l] + (1 if (st.root_deferred and l == 3) else 0)
                label = "speculative 1-3" if l < 0 else l + 1
            t_us = float(np.mean(v)) * 1e3
            if not t_us > 0:                 # (a launch that found no rows -- an empty level -- records no span)
                continue
            fl = rows * 2.0 * 25088 * 4096
            tmin = max(25088 * 4096 * 4 / HBM_PEAK, fl / (PEAK_F32_MFMA_TFLOPS * 1e12)) * 1e6
            fc6_shapes.append({"level": label, "rows": int(rows), "avg_us": t_us,
                               "tflops": fl / t_us / 1e6, "t_min_us": tmin, "frac": tmin / t_us})
        per_level = {}
        for n, l, ms in ktimes:
            per_level.setdefault("%s@L%d" % (n, l + 1), []).append(ms)
        # per launch group and pass: time, algorithmic bytes / flops (SURVEY 8d's units), fraction of its bound
        ktab = {}
        for n, l, ms in tab_times:
            ktab.setdefault((n, l), []).append(ms)
        pass_rows_now = rows_per_pass(st) or []
        pass_levels = sorted({l for (n, l) in ktab if n == "fc6_gemm"})
        kernel_table = []
        for (n, l), v in sorted(ktab.items(), key=lambda kv: (kv[0][1], kv[0][0])):
            us = float(np.mean(v)) * 1e3
            if not us > 0:                   # (as above: launches of an empty level)
                continue
            rows = pass_rows_now[pass_levels.index(l)] if (l in pass_levels and pass_levels.index(l) < len(pass_rows_now)) else None
            ent = {"kernel": n, "first_level": ("2" if l < 0 else str(l + 1)), "avg_us": us}
            if rows is not None and not st.static_plan:
                if n == "fc6_gemm":
                    fl = rows * 2.0 * 25088 * 4096
                    bound = max(25088 * 4096 * 4 / HBM_PEAK, fl / (PEAK_F32_MFMA_TFLOPS * 1e12)) * 1e6
                    ent.update(rows=rows, bound="max(weights / 8 TB/s, flops / 157.3 TF)", t_min_us=bound, frac=bound / us)
                elif n == "fc7_gemm":
                    fl = rows * 2.0 * 4096 * 1280
                    bound = max(4096 * 1280 * 4 / HBM_PEAK, fl / (PEAK_F32_MFMA_TFLOPS * 1e12)) * 1e6
                    ent.update(rows=rows, bound="max(weights / 8 TB/s, flops / 157.3 TF)", t_min_us=bound, frac=bound / us)
                elif n == "fc6_reduce":
                    by = rows * 4096 * 4 * 17.0                     # 16 slabs read, one row of int6 written
                    ent.update(rows=rows, bound="hbm", bytes=by, gb_per_s=by / us / 1e3, frac=by / HBM_PEAK * 1e6 / us)
                elif n == "roi_pool":
                    by = rows * 100352.0 + 4.0 * fmap_elems         # pool5 written, the map read once
                    ent.update(rows=rows, bound="hbm", bytes=by, gb_per_s=by / us / 1e3, frac=by / HBM_PEAK * 1e6 / us)
                elif n == "tail":
                    by = rows * (8 * 1280 * 4 + 56 * 4 + 44 * 8) + 1280 * 64 * 4.0
                    ent.update(rows=rows, bound="hbm (latency-bound in practice)", bytes=by, gb_per_s=by / us / 1e3,
                               frac=by / HBM_PEAK * 1e6 / us)
            kernel_table.append(ent)
        floor_us = t_min_us(uniq, fmap_elems)
        form_name = ffi.SEARCH_FORMS.get(int(st.search_form), "?")
        form = {
            "one_pass_plan": "Tz <= 0, every zoom test passes: the %d RoIs of all levels in ONE head pass" % spec_rows,
            "whole_tree_pass": "search for any Tz; this context's previous search of the shape walked the FULL tree, so ONE head "
                               "pass evaluates the full tree's unique rois and every level finds its outputs by RoIPool window -- "
                               "zoom selection, divide_region, _sift_dup, dedup all run level by level; a pruned tree does not "
                               "take this form (see tz_sweep): head passes of %s rows" % (prow if prow else "?"),
            "closure_pass": "search for any Tz; ONE head pass over the closure rows (every region any pruning of the shape's tree "
                            "can produce), every level finds its outputs by RoIPool window: head passes of %s rows" % (prow if prow else "?"),
            "pair_speculation": "level by level, some head passes also carrying the next level's rows: head passes of %s rows"
                                % (prow if prow else "?"),
            "level_loop": "level by level: head passes of %s rows" % (prow if prow else "?"),
        }.get(form_name, "?")
        out = {
            "metric": "AZ proposals/sec (600x1000 img)", "value": value, "unit": "proposals/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": "VGG16 AZ proposal hot path, 600x1000 image (scale 1.0), batch=1 per GPU, "
                                   "Tz=%g, regions/level %s, unique RoIs/level %s (%s), top-%d of %d candidates; "
                                   "conv5_3 %s resident in HBM, %d distinct images rotated" %
                                   (args.tz, regions, uniq, form, NUM_PROPOSALS, st.n_candidates,
                                    [int(x) for x in conv.shape], len(convs)),
                       "workload_short": "BASELINE config 2: VGG16 AZ proposal hot path, synthetic 600x1000 image (scale 1.0), "
                                         "batch=1 per GPU, Tz=%g, top-%d of %d candidates; conv5_3 %s resident in HBM, %d images "
                                         "rotated" % (args.tz, NUM_PROPOSALS, st.n_candidates, [int(x) for x in conv.shape], len(convs)),
                       "regions_per_level": regions, "unique_rois_per_level": uniq,
                       "search_form": form_name, "rows_per_head_pass": prow,
                       "searches_run_twice_in_timed_region": reruns_timed,
                       "image_hw": [H_IM, W_IM], "num_proposals": NUM_PROPOSALS, "Tz": args.tz,
                       "parallelism": "image-shard x%d" % world, "images_in_flight_per_gpu": args.inflight,
                       "host_queue_ahead": (0 if args.no_queue_ahead else 1), "searches_launched_and_unfetched": depth,
                       "lanes_per_context": args.lanes,
                       "images_overlapping_on_the_gpu": (2 if (args.lanes == 2 and not args.no_queue_ahead) else 1) * args.inflight,
                       "gather": ("RCCL all_gather every %d images/rank (in the timed loop)" % args.gather_every)
                                 if gat is not None else "none"},
            "rccl": dict(rccl, world=world, native_gather=bool(args.native_gather),
                         note="one process per GPU; a one-rank group still builds an RCCL communicator and runs the "
                              "all-gather on the GPU, so N = 1 times the code path of N = 8"),
            "roofline": {"bound": "mfma",
                         "kernel": "fc GEMMs of the head passes: k_fc_splitk12 (int6 at >= 161 / 257 rows) and k_fc_splitk "
                                   "(int6 below, int7_1|int7_2); v_mfma_f32_32x32x2_f32",
                         "kernel_short": "fc GEMMs of the head pass (k_fc_splitk12 int6 + k_fc_splitk int7), v_mfma_f32_32x32x2_f32",
                         "algorithmic_bytes": alg_bytes,
                         "achieved": achieved, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_F32_MFMA_TFLOPS,
                         "frac_of_sustained": (achieved / box["sustained_fp32_mfma_tflops"]) if box else None,
                         "flops_per_launch": flops_per_image / (n_launch / max(n_timed_steps, 1)),
                         "avg_launch_ms": gemm_ms_total / n_launch,
                         "launches_per_step": n_launch / max(n_timed_steps, 1),
                         "steps_timed": n_timed_steps, "traffic": traffic,
                         "timing": "every fc GEMM launch of the timed region times itself: first workgroup in to last workgroup "
                                   "out on the GPU's constant 100 MHz clock (az_set_profiling bit 3), which is what rocprofv3's "
                                   "kernel trace reports as the kernel's duration; no event pair on the stream",
                         "traffic_source": traffic_source, "int6_launch_shapes": fc6_shapes,
                         "note": "achieved = ALGORITHMIC flops (unique RoIs of the tree x 216 006 656) / time inside the "
                                 "fc GEMM launches; speculative rows that the tree did not need are work done but not counted"},
            "path_floor": dict(floors(st, fmap_elems, ms_step * 1e3), measured_us_per_image=ms_step * 1e3, note=FLOOR_NOTE),
            "timed_region_ms": {"total": dt * 1e3, "loop_of_this_rank": t_loop * 1e3, "closing_barrier": (dt - t_loop) * 1e3},
            "value_200_steps": long_run,
            "box": box,
            "head_pass_costs_us": {"table": [list(x) for x in net.ctx.pass_costs()],
                                   "note": "one head pass (RoIPool + int6 + reduce + int7 + heads) at these row counts, measured by "
                                           "the context on this device at its first launch: what it chooses the search form by"},
            "plan_build_ms": {"first_call_ms": first_ms, "steady_call_ms": steady_ms, "one_time_ms": max(first_ms - steady_ms, 0.0),
                              "note": "one-time work per image shape (shape-dependent pre-pass / plan, first-use allocations), "
                                      "done before the warm-up and not part of `value`"},
            "kernel_ms_per_step": {k: float(np.sum(v)) / n_timed_steps for k, v in sorted(per_level.items())},
            "kernel_table": {"rows": kernel_table, "sum_us": float(sum(e["avg_us"] for e in kernel_table)),
                             "note": "every launch group of one search (HIP events on the ctx stream, %d untimed steps right "
                                     "behind the timed region): the geometry kernels (spec_levels, level_geom, final_select) "
                                     "move a few hundred KB each and are latency chains of one workgroup -- no bandwidth "
                                     "figure is given for them" % n_tab},
            "step_ms": {"median": float(np.median(steps_ms)), "p95": float(np.percentile(steps_ms, 95)),
                        "max": float(steps_ms.max()), "over_1.5x_median": int((steps_ms > 1.5 * np.median(steps_ms)).sum()),
                        "note": "host-side wall time per step of the timed loop (a step whose batch exchange is collected "
                                "waits for the next image's kernels, so every gather_every-th step is long and the next short)"},
        }

    def timed_loop(fn, n, warm=10):
        gc.collect()                   # (before the warm-up: see the main loop)
        gc.disable()
        fn(warm)
        barrier()
        t = time.perf_counter()
        fn(n)
        barrier()
        d_ = maxr(time.perf_counter() - t)
        gc.enable()
        return d_

    def simple_run(prm, ctxnet=None):
        cn = ctxnet or net

        def f(k):
            # (same host pattern as the main loop: `depth` searches launched and unfetched; a context on one lane queues two)
            dd = min(depth, 3 * int(getattr(cn.ctx, "lanes", 1)))
            launched = 0
            for i in range(k):
                while launched < min(k, i + dd):
                    cn.ctx.propose_launch(prm, fmap=convs[launched % len(convs)], producer_done=True)
                    launched += 1
                cn.ctx.propose_fetch(want_scores=True)
        return f

    # ---- the same loop on ONE lane: strictly one image at a time on the GPU (the host still queues one ahead) -----------
    if args.lanes == 2 and args.inflight == 1 and not args.no_one_lane:
        net.ctx.set_lanes(1)
        n_1 = max(100, args.steps // 2)
        d_1 = timed_loop(simple_run(params), n_1)
        net.set_conv(conv)
        Y1, S1 = net.propose(params, want_scores=True)
        assert np.array_equal(Y1, Y) and np.array_equal(S1, S), "one lane and two lanes disagree"
        net.ctx.set_lanes(2)
        for _ in range(4):
            net.propose(params)
        if rank == 0:
            out["one_lane"] = {"value": world * NUM_PROPOSALS * n_1 / d_1, "unit": "proposals/s", "ms_per_image": d_1 / n_1 * 1e3,
                               "path_floor": floors(st, fmap_elems, d_1 / n_1 * 1e6),
                               "path_floor_frac": floors(st, fmap_elems, d_1 / n_1 * 1e6)["frac"],
                               "note": "az_set_lanes(1): the context's searches run one after the other on one stream -- nothing of "
                                       "image i+1 starts on the GPU before image i's last kernel (rounds 1-3's `value`).  With two "
                                       "lanes (`value`) image i+1's RoIPool + int6 run beside image i's single-workgroup geometry "
                                       "kernels and vice versa; same bits"}
    # ---- the same search in its other form (bit-identical results are asserted) ------------------------------------
    other_wanted = (args.tz <= 0.0) and not (args.no_level_loop if one_pass_main else args.no_one_pass)
    if other_wanted:
        po = mk(not one_pass_main)
        n_o = max(100, args.steps // 2)
        net.propose(po)
        d_o = timed_loop(simple_run(po), n_o)
        net.set_conv(conv)
        Yo, So, sto = net.propose(po, want_scores=True, want_stats=True)
        assert np.array_equal(Yo, Y) and np.array_equal(So, S), "level loop and one-pass plan disagree"
        if rank == 0:
            uo = [int(sto.level_unique[l]) for l in range(sto.n_levels)]
            if one_pass_main:
                out["level_loop"] = {"value": world * NUM_PROPOSALS * n_o / d_o, "unit": "proposals/s",
                                     "ms_per_image": d_o / n_o * 1e3, "rows_per_pass": rows_per_pass(sto),
                                     "path_floor": floors(sto, fmap_elems, d_o / n_o * 1e6),
                                     "path_floor_frac": floors(sto, fmap_elems, d_o / n_o * 1e6)["frac"],
                                     "note": "same image, same Tz, walked level by level; bit-identical to `value`'s"}
            else:
                out["one_pass"] = {"value": world * NUM_PROPOSALS * n_o / d_o, "unit": "proposals/s",
                                   "ms_per_image": d_o / n_o * 1e3, "rows": int(sto.spec_rows),
                                   "path_floor": floors(sto, fmap_elems, d_o / n_o * 1e6),
                                   "path_floor_frac": floors(sto, fmap_elems, d_o / n_o * 1e6)["frac"],
                                   "one_pass_t_min_us": t_min_us([sum(uo)], fmap_elems),
                                   "note": "Tz <= 0 ONLY (the reference's TRAIN-phase setting, config.py:275): every zoom test "
                                           "passes, the tree is a function of the image shape, all levels' rois go through "
                                           "ONE head pass (az_static.hip); proposals and scores bit-identical to `value`'s. "
                                           "No Tz > 0 search can take this form."}
    # ---- the level loop WITHOUT the whole-tree pass (two head passes: speculative rows, then level 4 + pair rows) ------
    if (not one_pass_main and not args.no_level_loop and not args.no_two_pass and st.n_passes == 1 and
            int(st.pass_rows[0]) > int(st.spec_rows) + 1):
        pw = ffi.AzContext.make_params(H_IM, W_IM, scale0, args.tz, num_proposals=NUM_PROPOSALS, static_tree=False,
                                       full_spec=False)
        n_w = max(100, args.steps // 2)
        net.propose(pw)
        d_w = timed_loop(simple_run(pw), n_w)
        net.set_conv(conv)
        Yw, Sw, stw = net.propose(pw, want_scores=True, want_stats=True)
        assert np.array_equal(Yw, Y) and np.array_equal(Sw, S), "the forms of the level loop disagree"
        if rank == 0:
            out["level_loop_without_whole_tree_pass"] = {
                "value": world * NUM_PROPOSALS * n_w / d_w, "unit": "proposals/s", "ms_per_image": d_w / n_w * 1e3,
                "rows_per_pass": rows_per_pass(stw),
                "path_floor": floors(stw, fmap_elems, d_w / n_w * 1e6),
                "path_floor_frac": floors(stw, fmap_elems, d_w / n_w * 1e6)["frac"],
                "search_form": ffi.SEARCH_FORMS.get(int(stw.search_form), "?"),
                "note": "Tz = 0 without the whole-tree pass: speculative rows, then level 4 + all children of level 4 -- the "
                        "form a dense pruned tree takes; bit-identical results"}
    # ---- opt-in: int6 on the 16-bit matrix cores, fp32 operands as two fp16 / three bf16 terms (az_set_gemm_mode) -----
    if not args.no_fast and net.ctx.gemm_mode == 0:
        # error of the head's outputs against an f64 evaluation of the same head (numpy; pool5 from the RoIPool kernel,
        # which is bit-exact), mode 0 beside the others: what the 16-bit-term modes give up, if anything
        rng = np.random.RandomState(5)
        nr = 32
        x1 = rng.uniform(0, 900, nr); y1 = rng.uniform(0, 500, nr)
        rr = np.stack([np.zeros(nr), x1, y1, x1 + rng.uniform(16, 300, nr), y1 + rng.uniform(16, 300, nr)], 1).astype(np.float32)
        net.set_conv(conv)
        p5 = net.ctx.roi_pool(rr).astype(np.float64)

        def f64_fc(x, W, b, relu):
            y = x @ W.astype(np.float64).T + b.astype(np.float64)
            return np.maximum(y, 0) if relu else y
        h6 = f64_fc(p5, head["W6"], head["b6"], True)
        h71 = f64_fc(h6, head["W71"], head["b71"], True)
        h72 = f64_fc(h6, head["W72"], head["b72"], True)
        truth = (1 / (1 + np.exp(-f64_fc(h72, head["Wz"], head["bz"], False))),
                 1 / (1 + np.exp(-f64_fc(h71, head["Was"], head["bas"], False))), f64_fc(h71, head["Wab"], head["bab"], False))
        del p5, h6

        def err_vs_f64(n_):
            n_.set_conv(conv)
            o = n_.ctx.head_forward(rr)
            return {k: float(np.abs(a - t).max()) for k, a, t in zip(("zoom_prob", "adj_prob", "adj_bbox"), o, truth)}
        e0 = err_vs_f64(net)
        modes = {}
        for gm, label in ((2, "f16x3: int6 operands as two fp16 terms of x * 2^k (22 mantissa bits), 3 fp16 MFMAs per product, "
                              "fp32 accumulate"),
                          (3, "bf16x6: int6 operands as three bf16 terms (all 24 mantissa bits), 6 bf16 MFMAs per product, "
                              "fp32 accumulate")):
            nf = HipAZNet(head, backbone=backbone, device=local_rank, name=net.name, max_regions=4096, gemm_mode=gm)
            nf.set_conv(conv)
            ent = {"dtype": label, "max_abs_err_vs_f64": err_vs_f64(nf), "fp32_mfma_path_err_vs_f64": e0}
            n_f = max(60, args.steps // 2)
            for key, prm in (("level_loop", mk(False)), ("one_pass", mk(True))):
                if args.tz > 0 and key == "one_pass":
                    continue
                nf.set_conv(conv)
                Yf, Sf, stf = nf.propose(prm, want_scores=True, want_stats=True)
                d1 = timed_loop(simple_run(prm, nf), n_f)
                nf.set_conv(conv)
                stf = nf.propose(prm, want_stats=True)[1]
                ent[key] = {"value": world * NUM_PROPOSALS * n_f / d1, "unit": "proposals/s", "ms_per_image": d1 / n_f * 1e3,
                            "rows_per_pass": rows_per_pass(stf),
                            "max_score_diff_vs_fp32_path": float(np.abs(Sf - S).max()) if Sf.shape == S.shape else None}
            # the int6 kernel of the one-pass form against the 16-bit MFMA peak (HIP events around the launch group)
            if args.tz <= 0:
                nf.set_conv(conv)
                nf.ctx.set_profiling(2 | 4)
                for _ in range(6):
                    nf.propose(mk(True))
                t6 = [ms for n_, l_, ms in nf.ctx.last_kernel_times() if n_ == "fc6_gemm"]
                nf.ctx.set_profiling(0)
                if t6:
                    rows6 = int(rows_per_pass(stf)[0]) if rows_per_pass(stf) else sum(st.level_unique[:st.n_levels])
                    us6 = float(np.mean(t6)) * 1e3 * (len(t6) / 6.0)      # (both shapes of the kernel are launched: sum per search)
                    mf = {2: 3, 3: 6}[gm]
                    padded = ((rows6 + 31) // 32) * 32
                    ex = padded * 2.0 * 25088 * 4096 * mf
                    ent["int6_kernel"] = {"rows": rows6, "avg_us": us6, "mfmas_per_product": mf,
                                          "executed_tflops": ex / us6 / 1e6, "peak_tflops": 2500.0,
                                          "frac": ex / us6 / 1e6 / 2500.0,
                                          "fp32_equivalent_tflops": rows6 * 2.0 * 25088 * 4096 / us6 / 1e6,
                                          "note": "peak = dense fp16 / bf16 MFMA at 2.4 GHz; under these MFMAs the chip sustains "
                                                  "1.77-1.80 GHz (profiles/r03_mode*_pmc_2.csv: GRBM_GUI_ACTIVE), where the "
                                                  "matrix pipe is 71-77 % busy"}
            # config 3 in this mode: the detection head's fc6 runs on the same kernel as int6
            if not args.no_extras and args.tz <= 0:
                import time as _t
                nf.set_conv(conv)
                pdet = mk(False)
                Ypd = nf.propose(pdet)
                detm = HipDetNet(synth.make_det_head(seed=99), nf)
                for _ in range(3):
                    scm, bxm = detm.detect(Ypd, 1.0, (H_IM, W_IM), 1. / 16., 10000, 1e-14)
                torch.cuda.synchronize()
                t0 = _t.perf_counter()
                for _ in range(20):
                    nf.propose(pdet)
                t1 = _t.perf_counter()
                for _ in range(20):
                    detm.detect(Ypd, 1.0, (H_IM, W_IM), 1. / 16., 10000, 1e-14)
                t2 = _t.perf_counter()
                ent["shared_detection"] = {"az_propose_ms": (t1 - t0) / 20 * 1e3, "az_detect_ms": (t2 - t1) / 20 * 1e3,
                                           "note": "config 3's two GPU parts in this mode (per-class NMS as in `shared_detection`)"}
                del detm
            ent["note"] = ("opt-in (az_set_gemm_mode %d), not `value`: int6 leaves the fp32-input MFMA; everything else is "
                           "unchanged.  The error columns are the head's outputs against an f64 evaluation on %d rois" % (gm, nr))
            modes["gemm_mode_%d" % gm] = ent
            del nf
        if rank == 0:
            out["int6_on_16bit_matrix_cores"] = modes
            m3 = modes.get("gemm_mode_3", {})
            if "level_loop" in m3:
                k3 = m3.get("int6_kernel", {})
                out["value_exact_split"] = {
                    "value": m3["level_loop"]["value"], "unit": "proposals/s", "ms_per_image": m3["level_loop"]["ms_per_image"],
                    "dtype": "f32 operands as three bf16 terms (8 + 8 + 8 mantissa bits: every fp32 value exactly), six bf16 "
                             "MFMAs per product (all cross terms of order <= 2), fp32 accumulation",
                    "rows_per_pass": m3["level_loop"]["rows_per_pass"],
                    "max_score_diff_vs_value": m3["level_loop"]["max_score_diff_vs_fp32_path"],
                    "max_abs_err_vs_f64": m3["max_abs_err_vs_f64"], "fp32_mfma_path_err_vs_f64": m3["fp32_mfma_path_err_vs_f64"],
                    "roofline": {"bound": "mfma", "kernel": "k_fc_terms (int6, v_mfma_f32_32x32x16_bf16)",
                                 "achieved": k3.get("executed_tflops"), "peak": 2500.0, "unit": "TFLOP/s",
                                 "frac": k3.get("frac"), "fp32_equivalent_tflops": k3.get("fp32_equivalent_tflops"),
                                 "note": "achieved = executed bf16 flops (6 MFMAs per fp32 product) / kernel time; the chip "
                                         "holds 1.77-1.80 GHz under these MFMAs (power), i.e. ~1.85 PFLOP/s is what it "
                                         "sustains of the 2.5 PFLOP/s data-sheet figure"},
                    "note": "the same search as `value` (same trees, scores within 2.4e-7 of it) with int6 on the 16-bit matrix "
                            "cores in the exact split (az_set_gemm_mode 3); opt-in, NOT `value`: the judge of whether an "
                            "exact operand split with dropped third-order terms stands for fp32 is the reader.  The full-head "
                            "parity tests run in this mode too (tests/conftest.py: gemm_mode)"}
    # ---- a data-dependent tree: Tz = the median zoom score over the full tree's regions ----------
    if not args.no_calibrated:
        net.set_conv(conv)
        net.propose(ffi.AzContext.make_params(H_IM, W_IM, scale0, 0.0, num_proposals=NUM_PROPOSALS, tune=True))
        zz = net.ctx.last_anchors()[1].astype(np.float64)
        full_regions = regions if args.tz <= 0 else [1, 8, 32]
        n3 = int(sum(full_regions[:3]))                 # root + its children + their children
        tz_c = float(np.quantile(zz[1:n3], 0.5))        # (untrained weights: scores drift with region size,
                                                        #  so the threshold is set where the tree branches)
        pc = ffi.AzContext.make_params(H_IM, W_IM, scale0, tz_c, num_proposals=NUM_PROPOSALS)
        Yc, stc = net.propose(pc, want_stats=True)

        n_c = max(100, args.steps // 2)
        # (the calibrated threshold belongs to convs[0]'s image: that map only)
        convs_keep = convs[:]
        del convs[1:]
        dc = timed_loop(simple_run(pc), n_c, warm=5)
        convs[:] = convs_keep
        if rank == 0:
            uc = [int(stc.level_unique[l]) for l in range(stc.n_levels)]
            out["calibrated_tz"] = {
                "Tz": tz_c, "value": world * Yc.shape[0] * n_c / dc, "unit": "proposals/s",
                "ms_per_image": dc / n_c * 1e3,
                "regions_per_level": [int(stc.level_regions[l]) for l in range(stc.n_levels)],
                "unique_per_level": uc, "rows_per_pass": rows_per_pass(stc),
                "search_form": ffi.SEARCH_FORMS.get(int(stc.search_form), "?"),
                "path_floor": floors(stc, fmap_elems, dc / n_c * 1e6),
                "note": "HISTORY-PRIMED (one image replayed; a stream of different images is `stream_tz`): same image and "
                        "weights, zoom threshold at the median zoom score of the regions of levels 2-3: a partially expanded, "
                        "data-dependent tree"}
    # ---- the searches a tuned Tz > 0 produces: the same image at four quantiles of its own zoom scores ----------------
    if not args.no_sweep:
        net.set_conv(conv)
        net.propose(ffi.AzContext.make_params(H_IM, W_IM, scale0, 0.0, num_proposals=NUM_PROPOSALS, tune=True))
        zz = np.sort(net.ctx.last_anchors()[1].astype(np.float64)[1:])        # every region of the full tree but the root
        convs_keep = convs[:]
        del convs[1:]                                    # (the thresholds belong to convs[0]'s image)
        n_s = max(100, args.steps // 2)
        pts = []
        for q in (0.1, 0.3, 0.5, 0.7):
            tz_q = float(np.quantile(zz, q))
            pq = ffi.AzContext.make_params(H_IM, W_IM, scale0, tz_q, num_proposals=NUM_PROPOSALS)
            net.set_conv(conv)
            for _ in range(3):                           # (the context's history of this shape now is THIS tree)
                net.propose(pq)
            cnt_r = [0]

            def fq(k, pq=pq):
                launched = 0
                for i in range(k):
                    while launched < min(k, i + depth):
                        net.ctx.propose_launch(pq, fmap=convs[0], producer_done=True)
                        launched += 1
                    cnt_r[0] += int(net.ctx.propose_fetch(want_stats=True)[1].n_reruns)
            gc.collect(); gc.disable()
            fq(12)                                       # (both lanes' histories: a form may need several searches of a kind)
            cnt_r[0] = 0
            barrier()
            t = time.perf_counter()
            fq(n_s)
            barrier()
            dq = maxr(time.perf_counter() - t)
            gc.enable()
            net.set_conv(conv)
            Yq, stq = net.propose(pq, want_stats=True)
            uq = [int(stq.level_unique[l]) for l in range(stq.n_levels)]
            pts.append({"quantile": q, "Tz": tz_q, "ms_per_image": dq / n_s * 1e3,
                        "value": world * Yq.shape[0] * n_s / dq, "unit": "proposals/s",
                        "regions_per_level": [int(stq.level_regions[l]) for l in range(stq.n_levels)],
                        "zoomed_per_level": [int(stq.level_zoomed[l]) for l in range(stq.n_levels)],
                        "unique_per_level": uq, "rows_per_pass": rows_per_pass(stq),
                        "search_form": ffi.SEARCH_FORMS.get(int(stq.search_form), "?"),
                        "path_floor": floors(stq, fmap_elems, dq / n_s * 1e6),
                        "searches_run_twice": cnt_r[0], "timed_images": n_s})
        convs[:] = convs_keep
        net.set_conv(conv)
        for _ in range(3):
            net.propose(params)                          # (back to `value`'s tree as the shape's history)
        if rank == 0:
            out["tz_sweep"] = {"points": pts,
                               "note": "HISTORY-PRIMED (each point replays ONE image; a stream of different images is `stream_tz`): "
                                       "convs[0]'s image, Tz at quantiles of the zoom scores of ALL regions of its full tree (untrained "
                                       "weights: the scores drift with region size, so a quantile can empty the deep levels). Each "
                                       "point: 3 + 12 untimed searches (the context's history -- both lanes' -- becomes this tree), then "
                                       "timed_images searches, queue-ahead, one image at a time.  path_floor = BASELINE.md section "
                                       "3's per-level floor for THIS tree (every level one weight stream at 8 TB/s or its flops at "
                                       "157.3 TF): a tree of a few dozen rois per level is five 54.6 us weight streams there, "
                                       "which two head passes replace"}
    # ---- the reference's operating point: ONE threshold tuned over a set, a stream of DIFFERENT images in dataset order ------
    if not args.no_stream and rank == 0 and args.inflight == 1:
        from bench_legs import stream_tz
        out["stream_tz"] = stream_tz(net, head, backbone, convs, ffi, synth, HipAZNet, torch, _get_image_blob, args, depth,
                                     local_rank)
        # the leg's headline, where a reader of the line finds it: proposals per second at the tuned threshold of the
        # planted-object set, one image per search and in lockstep batches (every image's result identical in both)
        try:
            po = out["stream_tz"]["points"][0]
            best = min(po["lockstep_batches"].items(), key=lambda kv: kv[1]["ms_per_image"])
            out["tuned_threshold_stream"] = {
                "set": "objects (32 planted-object maps, Tz tuned over the set at %d anchors per image)" % po["anchors_per_img"],
                "one_image_per_search": {"ms_per_image": po["ms_per_image"], "proposals_per_s": po["value"]},
                "lockstep_batches": {"images_per_batch": int(best[0]), "ms_per_image": best[1]["ms_per_image"],
                                     "proposals_per_s": best[1]["value"], "vs_one_image_per_search": best[1]["vs_one_image_at_a_time"]},
                "unit": "proposals/s", "note": "details and the two other sets: stream_tz"}
        except (KeyError, IndexError, ValueError):
            pass
        net.set_conv(conv)
        for _ in range(3):
            net.propose(params)                          # (back to `value`'s tree as the shape's history)
    # ---- BASELINE configs 3 and 4 and the NMS kernel under this run's clock (kernel time from HIP events) -----------
    if not args.no_extras and rank == 0:
        from bench_legs import extras
        out.update(extras(net, head, ffi, synth, HipDetNet, torch, args))
        net.set_conv(conv)
    # ---- backbone + hot path, for context (not `value`) -----------------------------------
    if not args.no_e2e:
        net.set_conv(conv)
        for _ in range(3):
            net.compute_conv(blob)
        barrier()
        n_e2e = max(5, min(50, args.steps // 4))
        t0 = time.perf_counter()
        for _ in range(n_e2e):
            net.compute_conv(blob)
            net.propose(params)
        barrier()
        de = maxr(time.perf_counter() - t0)
        # ... and from the uint8 host image: PCIe upload + the HIP front-end kernel (mean, resize, CHW)
        t0 = time.perf_counter()
        for _ in range(n_e2e):
            b2, _ = _get_image_blob(im, net)
            net.compute_conv(b2)
            net.propose(params)
        barrier()
        di = maxr(time.perf_counter() - t0)
        # backbone alone
        t0 = time.perf_counter()
        for _ in range(n_e2e):
            backbone(blob)
        barrier()
        db = maxr(time.perf_counter() - t0)
        # ... and overlapped: image i+1's backbone on torch's stream while image i's search runs on the ctx stream,
        # ordered on the device by an event (no host synchronisation between the two)
        bb_cl = backbone

        def run_e2e_pipe(k):
            nxt = bb_cl(blobs[0])
            ev = torch.cuda.Event()
            ev.record()
            for i in range(k):
                cur, evc = nxt, ev
                net.ctx.propose_launch(params, fmap=cur, producer_event=evc)
                nxt = bb_cl(blobs[(i + 1) % len(blobs)])          # enqueued while the search runs
                ev = torch.cuda.Event()
                ev.record()
                net.ctx.propose_fetch(want_scores=True)
            torch.cuda.synchronize()
        dpp = timed_loop(run_e2e_pipe, n_e2e, warm=3) if args.e2e_pipelined else None
        if rank == 0:
            out["end_to_end"] = {"value": world * NUM_PROPOSALS * n_e2e / de, "unit": "proposals/s",
                                 "ms_per_image": de / n_e2e * 1e3,
                                 "from_host_image_value": world * NUM_PROPOSALS * n_e2e / di,
                                 "from_host_image_ms": di / n_e2e * 1e3,
                                 "backbone_ms": db / n_e2e * 1e3,
                                 "backbone_tflops": VGG16_FLOP_600x1000 / (db / n_e2e) / 1e12,
                                 "note": "adds the fp32 PyTorch-ROCm VGG16 conv1_1..conv5_3 forward (367.7 GFLOP, channels_last "
                                         "weights and activations; its channels_last conv5_3 is borrowed in place); "
                                         "from_host_image also uploads the uint8 image over PCIe and runs the "
                                         "front-end kernel (az_image_blob_dev)"}
            if dpp is not None:
              out["end_to_end_pipelined"] = {
                "value": world * NUM_PROPOSALS * n_e2e / dpp, "unit": "proposals/s", "ms_per_image": dpp / n_e2e * 1e3,
                "vs_serial": (de / n_e2e) / (dpp / n_e2e),
                "note": "backbone of image i+1 (torch stream, channels-last output borrowed in place) enqueued while the "
                        "search of image i runs (ctx stream); the hand-over is an event wait on the device.  Measured for the "
                        "record: both saturate the GPU, and the search's persistent one-workgroup-per-CU GEMM shares the "
                        "CUs badly with MIOpen's kernels -- vs_serial < 1 means the serial order (end_to_end) is the faster one"}
    # ---- the CLI's loop: detect.test.test_proposals over a synthetic imdb (what tools/prop_az.py runs) ----------------
    if not args.no_e2e and rank == 0:
        import contextlib
        import io as _io
        import pickle as _pickle
        from datasets.factory import get_imdb
        from detect import config as dcfg
        from detect import test as dtest
        dcfg.cfg_set_mode("Test", args.tz)
        dcfg.cfg.EXP_DIR = "bench_cli_%d" % os.getpid()
        imdb_cli = get_imdb("synthetic_%dx%d_64" % (H_IM, W_IM))
        for i in range(len(imdb_cli.image_index)):
            imdb_cli.image_at(i)                         # (generated once; a dataset's files would be in the page cache)
        times = []
        for rep in range(2):                             # (the first pass of a shape builds its plan: not counted)
            with contextlib.redirect_stdout(_io.StringIO()):
                pf = dtest.test_proposals({"full": net, "fc": net}, imdb_cli)
            with open(pf, "rb") as f:
                times.append(float(_pickle.load(f)["time"]))
        try:
            os.remove(pf)
        except OSError:
            pass
        out["cli"] = {"ms_per_image": times[-1] * 1e3, "proposals_per_s": NUM_PROPOSALS / times[-1],
                      "first_pass_ms_per_image": times[0] * 1e3, "images": len(imdb_cli.image_index),
                      "vs_end_to_end": (out["end_to_end"]["from_host_image_ms"] / (times[-1] * 1e3)) if "end_to_end" in out else None,
                      "note": "seconds per image as detect.test.test_proposals reports them (proposals.pkl['time']) over "
                              "synthetic_600x1000_64: image from the imdb (read ahead by a worker thread), PCIe upload + "
                              "front-end kernel + VGG16 + search enqueued one image ahead of the GPU, boxes to the host, the "
                              "reference's per-image print lines.  vs_end_to_end = end_to_end.from_host_image_ms over this "
                              "(> 1: the harness loop is faster than the one-image-at-a-time sequence timed there).  The backbone "
                              "is this run's (channels_last + MIOpen's benchmark search: tools/prop_az.py --tune-backbone; the "
                              "tool's default backbone layout is ~0.45 ms per image slower)"}
        net.set_conv(conv)
    # what this box holds under the matrix pipe and through HBM (register-only MFMA loop, float4 copy);
    # measured LAST: 40 ms of a saturated matrix pipe and HBM leave the chip ~8 % slower for the next tens of ms
    if not args.no_box:
        mf, cp = net.ctx.measure_box()
        box = {"sustained_fp32_mfma_tflops": mf, "copy_tb_per_s": cp,
               "data_sheet_fp32_mfma_tflops": PEAK_F32_MFMA_TFLOPS, "data_sheet_hbm_tb_per_s": HBM_PEAK / 1e12,
               "note": "az_measure_box: ~3 ms register-only v_mfma_f32_32x32x2_f32 loops on all SIMDs, pseudo-random "
                       "operands (median of 7); best median of three float4-copy launch shapes over 1 GiB, bytes read + "
                       "written.  frac_of_sustained = roofline.achieved over the MFMA figure"}
    if rank == 0 and box is not None:
        out["box"] = box
        out["roofline"]["frac_of_sustained"] = out["roofline"]["achieved"] / box["sustained_fp32_mfma_tflops"]
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # (N = 1 only: at N > 1 the other ranks would sit in the closing barrier while rank 0 holds the host's cores)
        fm = conv.detach().cpu().numpy()
        out["cpu_baseline"] = cpu_baseline(head, fm, args.tz)
        out["gpu_over_cpu"] = out["value"] / world / out["cpu_baseline"]["value"]
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        paths = write_extras(out, args.extras_file) if args.full else []
        real_stdout.write(compact_line(out, extras_file=(os.path.relpath(paths[0], REPO) if paths else None)) + "\n")
        real_stdout.flush()


if __name__ == "__main__":
    main()
