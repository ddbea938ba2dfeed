"""Command-line plumbing shared by the tools: the reference's flags (tools/prop_az.py:30-54,
tools/set_thresh.py:26-52, tools/test_shared.py) declared as tables, plus the common start-up steps."""
import argparse
import os
import pprint
import sys
import time

# flag, dest, help, default, type   (type None = store_true)
COMMON = [
    ("--gpu", "gpu_id", "GPU id to use", 0, int),
    ("--cfg", "cfg_file", "optional config file", None, str),
    ("--wait", "wait", "wait until the weights file exists", True, bool),
    ("--exp", "exp_dir", "experiment path", None, str),
    # (extension) the backbone in channels_last memory with MIOpen's benchmark search: ~12 % faster convolutions once a shape
    # is tuned, seconds of search the first time a shape is seen -- pays for datasets of few image shapes
    ("--tune-backbone", "tune_backbone", "channels_last VGG16 + MIOpen benchmark search per image shape", None, None),
]
THRESH = [
    ("--thresh", "thresh_file", "file that stores the zoom threshold (pickle)", None, str),
    ("--tz", "tz", "zoom threshold given directly (instead of --thresh)", None, float),
]
# tools/train_az_net.py and tools/train_det_net.py: the reference's flags of both, and (behind each tool's own) the extensions of both
TRAIN = [
    ("--solver", "solver", "solver prototxt", None, str),
    ("--iters", "max_iters", "number of iterations to train", 40000, int),
    ("--weights", "pretrained_model", "initialize with pretrained model weights", None, str),
    ("--imdb", "imdb_name", "dataset to train on", "voc_2007_trainval", str),
    ("--rand", "randomize", "randomize (do not use a fixed seed)", None, None),
    ("--norm", "normalize", "to un-normalize (use when pre-trained model is normalized)", None, None),
]
TRAIN_EXT = [
    ("--base-lr", "base_lr", "(extension, without --solver) base_lr of the written solver", 0.001, float),
    ("--bf16", "bf16", "(extension) bf16 operands in the trainer's matrix products (cfg.TRAIN.PRECISION = 'bf16')", None, None),
    ("--snapshot-state", "snapshot_state", "(extension) write a .solverstate beside every snapshot (cfg.TRAIN.SNAPSHOT_STATE)", None, None),
    ("--restore", "restore", "(extension) continue from this .solverstate; --iters stays the total", None, str),
]
# what happens to the detections before evaluation (type a tuple = one of these values).  Every tool that evaluates
# detections takes them: build_parser adds the table wherever a tool declares --comp, the competition-mode flag of
# imdb.evaluate_detections (tools/test_det_net.py, tools/test_shared.py), and parse hands the values to cfg.TEST;
# tools/eval_det.py, which has a parser of its own, adds and applies it itself.
POSTPROC = [
    ("--soft-nms", "soft_nms", "(extension) Soft-NMS instead of NMS at cfg.TEST.NMS (cfg.TEST.NMS_METHOD)", None, ("linear", "gaussian")),
    ("--bbox-vote", "bbox_vote", "(extension) box voting on the kept detections (cfg.TEST.BBOX_VOTE)", None, None),
]


# iterative box localisation in the detection pass itself (cfg.TEST.ITER_LOC*): the tools that run a detection net take them
# (build_parser adds the table beside POSTPROC); tools/eval_det.py, which re-scores saved detections and has no net, does not
ITER_LOC = [
    ("--iter-loc", "iter_loc", "(extension) rounds of iterative box localisation, 1 = one pass (cfg.TEST.ITER_LOC)", None, int),
    ("--iter-loc-score", "iter_loc_score", "(extension) a class box is fed back at this score or above (cfg.TEST.ITER_LOC_SCORE)", None, float),
    ("--iter-loc-max", "iter_loc_max", "(extension) boxes fed back per round at most (cfg.TEST.ITER_LOC_MAX)", None, int),
]


def add_flags(parser, tables):
    for table in tables:
        for flag, dest, text, default, typ in table:
            if typ is None:
                parser.add_argument(flag, dest=dest, help=text, action="store_true")
            elif isinstance(typ, tuple):
                parser.add_argument(flag, dest=dest, help=text, default=default, choices=typ)
            else:
                parser.add_argument(flag, dest=dest, help=text, default=default, type=typ)
    return parser


def build_parser(description, tables):
    tables = list(tables)
    if POSTPROC not in tables and any(row[0] == "--comp" for table in tables for row in table):
        tables.append(POSTPROC)
        tables.append(ITER_LOC)
    return add_flags(argparse.ArgumentParser(description=description), tables)


def set_postproc(args):
    """--soft-nms / --bbox-vote into cfg.TEST: a flag wins over a --cfg file read before or after (cfg_set_cli), no flag
    leaves the file's value."""
    from detect.config import cfg_set_cli
    if getattr(args, "soft_nms", None):
        cfg_set_cli("TEST", "NMS_METHOD", args.soft_nms)
    if getattr(args, "bbox_vote", False):
        cfg_set_cli("TEST", "BBOX_VOTE", True)


def set_iter_loc(args):
    """--iter-loc / --iter-loc-score / --iter-loc-max into cfg.TEST, as set_postproc does it; a value the keys do not take is
    a ValueError here (detect.config.iter_loc)."""
    from detect.config import cfg_set_cli, iter_loc
    given = {k: getattr(args, k, None) for k in ("iter_loc", "iter_loc_score", "iter_loc_max")}
    if all(v is None for v in given.values()):
        return
    iter_loc(given["iter_loc"], given["iter_loc_score"], given["iter_loc_max"])
    for k, v in given.items():
        if v is not None:
            cfg_set_cli("TEST", k.upper(), v)


def parse(description, tables):
    parser = build_parser(description, tables)
    if len(sys.argv) == 1:
        parser.print_help()
        sys.exit(1)
    args = parser.parse_args()
    print("Called with args:")
    print(args)
    set_postproc(args)
    set_iter_loc(args)
    return args


def wait_for(path, wait):
    while not os.path.exists(path) and wait:
        print("Waiting for {} to exist...".format(path))
        time.sleep(10)


def setup_cfg(args, mode):
    """cfg_from_file / cfg_set_path / cfg_set_mode in the reference's order; mode 'Test' reads the zoom
    threshold from --tz or the --thresh pickle."""
    from detect.config import cfg, cfg_from_file, cfg_set_mode, cfg_load_thresh, cfg_set_path
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    cfg_set_path(args.exp_dir)
    if mode == "Test":
        if getattr(args, "tz", None) is not None:
            thresh = args.tz
        else:
            if getattr(args, "thresh_file", None) is None:
                print("error: one of --thresh / --tz is required in Test mode", file=sys.stderr)
                sys.exit(2)
            wait_for(args.thresh_file, args.wait)
            thresh = cfg_load_thresh(args.thresh_file)
        cfg_set_mode("Test", thresh)
    else:
        cfg_set_mode(mode)
    print("Using config:")
    pprint.pprint(cfg)
    return cfg


def train_seed(args):
    """What both training tools do behind setup_cfg(args, "Train"): the seed of the dropout / filler generator -- a fresh one
    under --rand, else cfg.RNG_SEED, which then seeds numpy as well -- and cfg.TRAIN.UN_NORMALIZE from --norm."""
    import numpy as np
    from detect.config import cfg
    seed = cfg.RNG_SEED
    if args.randomize:
        seed = int.from_bytes(os.urandom(4), "little")
    else:
        np.random.seed(cfg.RNG_SEED)          # fix the random seeds (numpy and the dropout / filler generator)
    cfg.TRAIN.UN_NORMALIZE = bool(args.normalize)
    return seed


def reduced_net(device, seed, div, full_dims, keys):
    """(backbone, dims) of a --net synthetic[:width_div] run: a seeded VGG16Conv5 1 / div as wide, its output normalised on
    an image of ones, and the head's sizes `keys` of `full_dims` divided alike (at least 4)."""
    import numpy as np
    from aznet_hip.backbone import VGG16Conv5
    backbone = VGG16Conv5(device="cuda:%d" % device, seed=seed, width_div=div)
    backbone.normalize_output(np.ones((1, 3, 600, 1000), dtype=np.float32))
    return backbone, {k: max(4, full_dims[k] // div) for k in keys}


def ranks():
    """(world, rank, device) from the torch.distributed.run environment, or the single-process default."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    return world, rank
