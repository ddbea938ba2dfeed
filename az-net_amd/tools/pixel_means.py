#!/usr/bin/env python3
"""Compute the pixel means of a dataset -- the counterpart of the reference's tools/pixel_means.py (same flag, same
progress line; exact integer sums divided once instead of a running mean).  --imdb takes the values tools/prop_az.py does."""
import _init_paths  # noqa: F401

import _cli

FLAGS = [
    ("--imdb", "imdb_name", "dataset to average", "voc_2007_trainval", str),
]


def parser():
    return _cli.build_parser("Compute pixel means of imdb", [FLAGS])


def main():
    args = _cli.parse("Compute pixel means of imdb", [FLAGS])
    from datasets.factory import get_imdb
    from datasets.pixel_means import pixel_means
    means = pixel_means(get_imdb(args.imdb_name))
    print("PIXEL_MEANS (BGR): [{:.4f}, {:.4f}, {:.4f}]".format(*means))


if __name__ == "__main__":
    main()
