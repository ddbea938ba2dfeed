#!/usr/bin/env python3
"""Use AZ-Net to generate object proposals on an image database in diagnostic mode -- the MI355X counterpart of the
reference's tools/diagnose_prop.py (same flags; writes <output_dir>/AZ_results.mat as lib/detect/tune.py:368-419 does).
The reference stopped there and left the analysis to MATLAB; this tool also runs it (detect.diagnose: zoom precision /
recall per search level, recall by proposal budget and object size, the missed objects split into never reached / reached
but not hit), prints the tables and writes <output_dir>/diagnosis.pkl.  --net / --imdb / --tz as in tools/prop_az.py.
One process: the analysis needs the whole image set."""
import _init_paths  # noqa: F401
import os
import pickle
import sys

import _cli

FLAGS = [
    ("--def", "prototxt", "(ignored) prototxt of the full net", None, str),
    ("--def_fc", "prototxt_fc", "(ignored) prototxt of the fc layers", None, str),
    ("--net", "caffemodel", "AZ-Net weights (.caffemodel / .npz) or synthetic[:seed]", "synthetic", str),
    ("--imdb", "imdb_name", "dataset to test", "voc_2007_test", str),
]


def parser():
    return _cli.build_parser("Use AZ-Net to generate proposals (diagnostic mode)", [_cli.COMMON, _cli.THRESH, FLAGS])


def main():
    args = _cli.parse("Use AZ-Net to generate proposals (diagnostic mode)", [_cli.COMMON, _cli.THRESH, FLAGS])
    world, _ = _cli.ranks()
    if world > 1:
        print("error: tools/diagnose_prop.py runs as one process (WORLD_SIZE is %d): the diagnosis is computed over the "
              "whole image set in one call" % world, file=sys.stderr)
        sys.exit(2)
    _cli.setup_cfg(args, "Test")
    if not args.caffemodel.startswith("synthetic"):
        _cli.wait_for(args.caffemodel, args.wait)
    import torch
    torch.cuda.set_device(args.gpu_id)
    from prop_az import load_net
    from datasets.factory import get_imdb
    from detect.config import get_output_dir
    from detect.tune import test_proposals
    from detect.diagnose import diagnose, summary_lines
    net = load_net(args.caffemodel, args.gpu_id, tuned=bool(getattr(args, "tune_backbone", False)))
    imdb = get_imdb(args.imdb_name)
    results = test_proposals({"full": net, "fc": net}, imdb)
    d = diagnose(results, imdb, ctx=net.ctx)
    for line in summary_lines(d):
        print(line)
    out = os.path.join(get_output_dir(imdb, net), "diagnosis.pkl")
    with open(out, "wb") as f:
        pickle.dump(d, f, pickle.HIGHEST_PROTOCOL)
    print("wrote", out)


if __name__ == "__main__":
    main()
