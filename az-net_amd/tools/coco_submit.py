#!/usr/bin/env python3
"""Convert a saved detections.pkl (test_net's all_boxes) into COCO submission file(s) -- the reference's
tools/coco_submit.py, same flags: instances_<split><year>_results_<k>.json next to the pkl, a new file every
--size images (coco.write_coco_multiple_files)."""
import _init_paths  # noqa: F401
import argparse
import os
import pickle
import sys


def parse_args():
    parser = argparse.ArgumentParser(description="Convert results in to COCO submission file")
    parser.add_argument("--size", dest="max_size", help="Max size of each file (in number of images)",
                        default=30000, type=int)
    parser.add_argument("--file", dest="filename", help="filename for detection file", default="detections.pkl",
                        type=str)
    parser.add_argument("--split", dest="split", help="split of the dataset", default="test", type=str)
    parser.add_argument("--year", dest="year", help="year of the dataset", default="2015", type=str)
    if len(sys.argv) == 1:
        parser.print_help()
        sys.exit(1)
    return parser.parse_args()


def main():
    args = parse_args()
    print("Called with args:")
    print(args)
    with open(args.filename, "rb") as f:
        all_boxes = pickle.load(f)
    output_dir = os.path.dirname(args.filename)
    from datasets.coco import coco
    coco(args.split, args.year).write_coco_multiple_files(all_boxes, args.max_size, output_dir)


if __name__ == "__main__":
    main()
