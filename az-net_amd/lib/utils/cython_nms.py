"""Drop-in for the reference's Cython module `utils.cython_nms`
(lib/utils/nms.pyx:17-68), backed by the HIP NMS kernels behind az_nms; soft_nms and box_vote (not in the
reference) are backed by az_soft_nms_batched and az_box_vote_batched."""
import numpy as np

from aznet_hip import ffi


def _check(dets):
    if not isinstance(dets, np.ndarray) or dets.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2)")
    if dets.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t' but got '%s'" % dets.dtype)


def nms(dets, thresh):
    """dets float32 [N,5] (x1,y1,x2,y2,score) -> list of kept original indices in
    descending-score order; suppression when IoU >= thresh."""
    _check(dets)
    return [int(i) for i in ffi.default_context().nms(dets, float(thresh))]


def soft_nms(dets, method='linear', thresh=0.3, sigma=0.5, min_score=0.001):
    """Soft-NMS (Bodla et al., ICCV 2017) of dets float32 [N,5]: (keep, scores) -- the picked original indices in pick order
    (a list) and their decayed scores at the moment they were picked (float32 [nk]).  method 'hard', 'linear' or
    'gaussian'; the decay applies when IoU >= thresh (linear, hard) or always (gaussian, by sigma); a box whose score falls
    below min_score is dropped."""
    _check(dets)
    keep, scores = ffi.default_context().soft_nms_batched([dets], method, float(thresh), float(sigma), float(min_score))[0]
    return [int(i) for i in keep], scores


def box_vote(dets, keep, vote_thresh=0.8):
    """Box voting (Gidaris & Komodakis, ICCV 2015): for every index in `keep`, the mean of the rows of dets float32 [N,5]
    whose IoU with it is >= vote_thresh, weighted by their scores -> float32 [len(keep), 4]."""
    _check(dets)
    return ffi.default_context().box_vote_batched([dets], [np.asarray(keep, dtype=np.int64)], float(vote_thresh))[0]
