"""Zoom-threshold tuning of the reference's `detect.tune` (lib/detect/tune.py) on the MI355X path.

    im_propose(net, im)       tune.py:256-316   -> ([Y | score] [n,5], Bhis [m,5])
    tune_thresh(net, imdb)    tune.py:318-366   -> writes thresh.pkl, returns the threshold
    test_proposals(net, imdb) tune.py:368-419   -> writes AZ_results.mat, returns what it holds (detect.diagnose reads it)

The tuner's search differs from lib/detect/test.py's: it walks K levels (not K-1), compares the
zoom scores of the first level against 0 and of later levels against cfg.SEAR.Tz (0 in 'Train'
mode, tools/set_thresh.py:70), never forces the root, and remembers every anchor region with its
zoom score (Bhis).  It is one az_propose call with the tuner flag.  tune_thresh then needs the
(num_images * cfg.TRAIN.ANCHORS_PER_IMG)-th largest zoom score of the whole set: the scores never
leave HBM (az_tune_begin / az_tune_kth_largest) instead of feeding a Python heap.
"""
import os
import pickle

import numpy as np

from detect.config import cfg, get_output_dir
from detect.test import _im_scale, _get_image_blob, _as_uint8
from utils.timer import Timer
from aznet_hip import ffi


def _tune_params(im_shape, scale):
    return ffi.AzContext.make_params(
        im_shape[0], im_shape[1], scale, cfg.SEAR.Tz, num_proposals=cfg.SEAR.NUM_PROPOSALS, fixed_num=True,
        Tc=cfg.SEAR.Tc, dedup=cfg.DEDUP_BOXES, eps=cfg.EPS, min_side=cfg.SEAR.MIN_SIDE,
        batch_size=cfg.SEAR.BATCH_SIZE, tune=True)


def _search(hnet, im, conv=None):
    scales = _im_scale(im.shape)
    if len(scales) > 1:
        # an image pyramid (several cfg.TEST.SCALES): its padded maps and az_propose_pyramid with the tuner flag
        if conv is None:
            hnet.compute_pyramid(_as_uint8(im), cfg.PIXEL_MEANS, scales)
        else:
            hnet.set_pyramid(conv[cfg.SEAR.AZ_CONV[0]])
        return hnet.propose_pyramid(_tune_params(im.shape, scales[0]), scales, want_scores=True, want_stats=True)
    if conv is None:
        blob, _ = _get_image_blob(im, hnet)
        hnet.compute_conv(blob)
    else:
        hnet.set_conv(conv[cfg.SEAR.AZ_CONV[0]])
    return hnet.propose(_tune_params(im.shape, scales[0]), want_scores=True, want_stats=True)


def im_propose(net, im, conv=None):
    """tune.py:256-316.  Returns (hstack(Y, scores) [n,5] float64, Bhis [m,5] float64 =
    anchor regions with their zoom scores, level-major)."""
    Y5, Bhis, _ = _im_propose_stats(net, im, conv)
    return Y5, Bhis


def _im_propose_stats(net, im, conv=None):
    """im_propose plus the search's statistics (level_regions: the anchors of each level, Bhis being level-major)."""
    hnet = net["full"] if isinstance(net, dict) else net
    Y, S, st = _search(hnet, im, conv)
    regions, zoom = hnet.ctx.last_anchors()
    print('{0} proposals, evaluate {1} regions, reaches depth {2}.'.format(Y.shape[0], st.num_eval, st.depth))
    return (np.hstack((Y, S.astype(np.float64)[:, np.newaxis])),
            np.hstack((regions, zoom.astype(np.float64)[:, np.newaxis])), st)


def tune_thresh(net, imdb, gather=None):
    """Zoom threshold such that on average cfg.TRAIN.ANCHORS_PER_IMG anchors per image score above
    it (tune.py:318-366).  Writes <output_dir>/thresh.pkl (a pickled float, what
    cfg_load_thresh reads) and returns the value.
    gather (multi-GPU): callable(list of float32 arrays) -> list over ranks; each rank tunes its
    shard of the imdb and rank 0 merges the per-rank top scores."""
    hnet = net["full"] if isinstance(net, dict) else net
    num_images = len(imdb.image_index)
    max_per_set = num_images * cfg.TRAIN.ANCHORS_PER_IMG
    output_dir = get_output_dir(imdb, hnet)
    if not os.path.exists(output_dir):
        os.makedirs(output_dir)
    _t = {'im_prop': Timer()}
    mine = getattr(imdb, "shard", None) or range(num_images)
    ctx = hnet.ctx
    ctx.tune_begin(max(1, len(mine)) * 2 * ctx.max_regions)
    # (images read ahead by a worker thread, as in detect.test.test_proposals: reading / decoding an image takes about as long
    #  as the GPU needs for one)
    from detect.test import _prefetched
    images = _prefetched(imdb, list(mine), depth=int(cfg.TEST.get("PREFETCH", 2)))
    for n, i in enumerate(mine):
        im = next(images)
        _t['im_prop'].tic()
        _search(hnet, im)
        _t['im_prop'].toc()
        print('im_tune: {:d}/{:d} {:.3f}s'.format(n + 1, len(mine), _t['im_prop'].average_time))
    if gather is not None:
        tops = gather(ctx.tune_top(max_per_set))
        ctx.tune_begin(max(1, sum(t.size for t in tops)))
        for t in tops:
            ctx.tune_push(t)
    thresh, _ = ctx.tune_kth_largest(max_per_set)
    ctx.tune_end()
    thresh = -np.inf if thresh == float("-inf") else np.float64(thresh)
    print('the threshold is set to {0}'.format(thresh))
    with open(os.path.join(output_dir, 'thresh.pkl'), 'wb') as f:
        pickle.dump(thresh, f, pickle.HIGHEST_PROTOCOL)
    return thresh


AZ_RESULTS_KEYS = ("prop_boxes", "anchor_boxes", "gt_boxes", "fn", "Tz", "num_proposals", "im_shapes")


def write_az_results(path, results):
    """AZ_results.mat as tune.py:412-419 writes it: the seven keys, the per-image ones as object arrays of
    num_images cells built as tune.py:375-379 builds them."""
    import scipy.io as sio
    n = len(results["fn"])
    out = {}
    for key in ("prop_boxes", "anchor_boxes", "gt_boxes", "fn", "im_shapes"):
        cells = np.zeros((n,), dtype=object)
        for i in range(n):
            cells[i] = results[key][i]
        out[key] = cells
    sio.savemat(path, dict(prop_boxes=out["prop_boxes"], anchor_boxes=out["anchor_boxes"], gt_boxes=out["gt_boxes"],
                           fn=out["fn"], Tz=results["Tz"], num_proposals=results["num_proposals"],
                           im_shapes=out["im_shapes"]))


def test_proposals(net, imdb):
    """Record everything a fine-grained analysis of a proposal run needs -- proposals, every anchor region with its
    zoom score, ground truth, file names, image shapes (tune.py:368-419) -- with the tuner-variant search in whatever
    mode cfg is in.  Writes <output_dir>/AZ_results.mat and returns its contents as a dict, plus `level_regions` (the
    anchors of each search level per image: anchor_boxes is level-major) for detect.diagnose."""
    hnet = net["full"] if isinstance(net, dict) else net
    num_images = len(imdb.image_index)
    prop_boxes, anchor_boxes, gt_boxes = [None] * num_images, [None] * num_images, [None] * num_images
    fn, im_shapes, level_regions = [None] * num_images, [None] * num_images, [None] * num_images
    output_dir = get_output_dir(imdb, hnet)
    if not os.path.exists(output_dir):
        os.makedirs(output_dir)
    _t = {'im_prop': Timer()}
    gt_roidb = imdb.gt_roidb()
    from detect.test import _prefetched
    images = _prefetched(imdb, list(range(num_images)), depth=int(cfg.TEST.get("PREFETCH", 2)))
    for i in range(num_images):
        im = next(images)
        im_shapes[i] = tuple(int(d) for d in im.shape)
        _t['im_prop'].tic()
        prop_boxes[i], anchor_boxes[i], st = _im_propose_stats(net, im)
        _t['im_prop'].toc()
        level_regions[i] = np.array(st.level_regions[:st.n_levels], dtype=np.int32)
        gt_boxes[i] = gt_roidb[i]['boxes']
        fn[i] = os.path.basename(imdb.image_path_at(i))
        print('im_prop: {:d}/{:d} {:.3f}s'.format(i + 1, num_images, _t['im_prop'].average_time))
    results = dict(prop_boxes=prop_boxes, anchor_boxes=anchor_boxes, gt_boxes=gt_boxes, fn=fn, Tz=cfg.SEAR.Tz,
                   num_proposals=cfg.SEAR.NUM_PROPOSALS, im_shapes=im_shapes)
    write_az_results(os.path.join(output_dir, 'AZ_results.mat'), results)
    results["level_regions"] = level_regions
    return results
