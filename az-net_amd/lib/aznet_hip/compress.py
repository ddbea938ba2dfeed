"""Truncated-SVD compression of the detection head's fc layers and of the AZ head's int6 (Fast R-CNN, section 4.4; the
paper's compress_net tool).

A layer y = relu(W x + b), W [out, in], becomes t = L x (no bias, no ReLU: fc*_L) and y = relu(U t + b) (fc*_U) with
    U_, s, Vt = svd(W);  L = diag(s[:r]) Vt[:r]  [r, in];  U = U_[:, :r]  [out, r].
U L is the best rank-r approximation of W in the Frobenius norm, with error sqrt(sum_{i >= r} s_i^2) (Eckart-Young).
The SVD runs in float64 -- on the GPU through torch when one is there, in NumPy otherwise -- and the factors are cast to
float32 once, at the end.  Inference only: AzContext.load_det_head_lowrank / load_head_lowrank run such a head; the
trainers keep full weights."""
import numpy as np


def _svd64(W):
    """(U, s, Vt) of W in float64, thin."""
    W = np.asarray(W, dtype=np.float64)
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        gpu = False
    if gpu:
        import torch
        U, s, Vt = torch.linalg.svd(torch.from_numpy(np.ascontiguousarray(W)).cuda(), full_matrices=False)
        return U.cpu().numpy(), s.cpu().numpy(), Vt.cpu().numpy()
    return np.linalg.svd(W, full_matrices=False)


def compress_layer(W, r):
    """(L [r, in], U [out, r]) float32 of W [out, in] at rank r, 1 <= r <= min(out, in).  The factors are unique only up
    to the signs (and, for equal singular values, rotations) of the singular vectors: compare products U L, not factors."""
    W = np.asarray(W)
    if W.ndim != 2:
        raise ValueError("compress_layer takes a matrix [out, in], got shape %s" % (W.shape,))
    r = int(r)
    if not 1 <= r <= min(W.shape):
        raise ValueError("rank %d outside [1, min(out, in) = %d]" % (r, min(W.shape)))
    U, s, Vt = _svd64(W)
    L = s[:r, None] * Vt[:r]
    return np.ascontiguousarray(L, dtype=np.float32), np.ascontiguousarray(U[:, :r], dtype=np.float32)


def rel_error(W, L, U):
    """||W - U L||_F / ||W||_F in float64."""
    W = np.asarray(W, dtype=np.float64)
    return float(np.linalg.norm(W - np.asarray(U, np.float64) @ np.asarray(L, np.float64)) / max(np.linalg.norm(W), 1e-300))


def compress_det_head(head, r6=1024, r7=256):
    """The detection-head dict (W6, b6, W7, b7, Wc, bc, Wb, bb [, skip_front]) with fc6 at rank r6 and fc7 at rank r7
    (0 or None: that layer stays as it is): W6 -> L6, U6 and W7 -> L7, U7; biases, cls_score, bbox_pred and a skip front
    are passed through.  The dict AzContext.load_det_head / HipDetNet / HipFrcnnNet take."""
    out = {k: v for k, v in head.items() if k not in ("W6", "W7")}
    for i, r in ((6, r6), (7, r7)):
        if r:
            out["L%d" % i], out["U%d" % i] = compress_layer(head["W%d" % i], r)
        else:
            out["W%d" % i] = head["W%d" % i]
    return out


def compress_az_head(head, r6=1024):
    """The AZ-head dict (W6, b6, W71, b71, W72, b72, Was, bas, Wab, bab, Wz, bz) with int6 at rank r6: W6 -> L6 [r6, C*49],
    U6 [n6, r6]; b6 and every other layer are passed through.  -> (the dict AzContext.load_head / HipAZNet take, the
    relative error ||W6 - U6 L6||_F / ||W6||_F).  A different model from the full head: thresholds tuned on the full net
    have to be tuned again."""
    out = {k: v for k, v in head.items() if k != "W6"}
    out["L6"], out["U6"] = compress_layer(head["W6"], r6)
    return out, rel_error(head["W6"], out["L6"], out["U6"])


__all__ = ["compress_layer", "compress_det_head", "compress_az_head", "rel_error"]
