"""Planted zoom trees for the search forms' table limits (tests/test_search_limits_host.py, tests/test_gpu_search_limits.py).

With a head from synth.make_object_head(noise=0, beta=0, gamma steep) and a map whose zoom channel is a 0/1 mask, a region
zooms exactly when its RoIPool window holds a planted cell: the populations of every level of the search are then integer
functions of (H, W, scale, mask), computed here on the CPU with the oracle's geometry.  `populations` is that function,
`search` and `twin` the seeded search and the single-cell pass that found the frozen cases of tests/search_limits_cases.py
(RECIPES records the calls; never run by a test: the tests recompute the populations of every frozen case and assert what
the table claims), `case_inputs` the head / map / parameters of a case.

The limits (az-net_amd/csrc): k_spec_levels owns levels 0-2 and hands level 3 over (FL_R = 256 regions, FL_C = 2048
children, SPEC_PRE = 64 staged rows); k_level_geom owns levels 3 .. nlev-2 (LV_R = 1024, LV_C = 4096); both give a level
whose regions exceed batch_size to the chunked multi-launch dedup.  Levels are numbered from 0 (the root) as in az_stats.
"""
import numpy as np

from oracle import az_oracle as orc

LV_R, LV_C = 1024, 4096
FL_R, FL_C = 256, 2048
SPEC_PRE = 64
TZ = 0.5
HEAD_KW = dict(seed=4321, zoom_channel=0, gamma=40.0, beta=0.0, delta=10.0, noise=0.0, clip=0.5)
MAP_SEED = 11


def map_size(H, W, scale):
    from aznet_hip import synth
    return synth.conv_out_size(int(round(H * scale))), synth.conv_out_size(int(round(W * scale)))


def default_scale(H, W):
    """cfg.TEST.SCALES = (600,), MAX_SIZE = 1000 (lib/detect/test.py:27-59)."""
    scale = 600.0 / min(H, W)
    if np.round(scale * max(H, W)) > 1000:
        scale = 1000.0 / max(H, W)
    return float(scale)


def _cround(v):
    """C roundf of f32 values (half away from zero), as integers."""
    v = v.astype(np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def roi_windows(boxes, scale, fh, fw, spatial_scale=0.0625, pooled=7):
    """The map cells RoIPool reads for each box (ROIPooling of test_fc.prototxt:14-25, as oracle/c restates it): the union
    of the 7x7 bins, clipped to the map -- half-open [h0, h1) x [w0, w1), empty where h1 <= h0 or w1 <= w0."""
    rois = orc.get_rois_blob(np.asarray(boxes, dtype=np.float64), scale)[:, 1:]            # f32(box * scale)
    q = _cround(rois * np.float32(spatial_scale))
    sw, sh, ew, eh = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    out = []
    for s, e, lim in ((sh, eh, fh), (sw, ew, fw)):
        n = np.maximum(e - s + 1, 1)
        binsz = n.astype(np.float32) / np.float32(pooled)
        span = np.ceil(np.float32(pooled) * binsz).astype(np.int64)                      # end of the last bin
        out.append(np.clip(s, 0, lim))
        out.append(np.clip(s + span, 0, lim))
    return out[0], out[1], out[2], out[3]


def zoom_predicate(boxes, scale, mask):
    """True where the box's RoIPool window holds a planted cell of `mask` ([fh, fw] bool)."""
    fh, fw = mask.shape
    h0, h1, w0, w1 = roi_windows(boxes, scale, fh, fw)
    sat = np.zeros((fh + 1, fw + 1), dtype=np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(mask.astype(np.int64), axis=0), axis=1)
    h1 = np.maximum(h1, h0)
    w1 = np.maximum(w1, w0)
    return (sat[h1, w1] - sat[h0, w1] - sat[h1, w0] + sat[h0, w0]) > 0


def unique_rois(boxes, scale, batch, dedup=1. / 16.):
    """U of a level: test.py:202-218, one np.unique per chunk of `batch` regions."""
    U = 0
    for s in range(0, boxes.shape[0], batch):
        index, _ = orc.roi_dedup(orc.get_rois_blob(boxes[s:s + batch], scale), dedup)
        U += len(index)
    return U


def populations(H, W, scale, min_side, batch, mask, Tz=TZ, want_regions=False):
    """Every level's populations for the planted tree: a dict of lists indexed by level -- P regions, U unique rois, PZ
    zoomed regions, CH children before _sift_dup, Pn regions of the next level (CH and Pn are -1 at the last level, which
    the search never divides) -- plus P1 / CH1 / spec_rows of the speculative pass (root, its children B1, ALL children
    of B1: a function of the shape only)."""
    B = np.array([[0, 0, W - 1.0, H - 1.0]])
    nlev = orc.num_levels(H, W, min_side) - 1
    out = {k: [0] * nlev for k in ("P", "U", "PZ", "CH", "Pn")}
    regions = []
    for l in range(nlev):
        P = B.shape[0]
        z = zoom_predicate(B, scale, mask)
        if l == 0:
            z[0] = 1.0 >= Tz                                       # test.py:383-384
        out["P"][l], out["U"][l], out["PZ"][l] = P, unique_rois(B, scale, batch), int(z.sum())
        regions.append((B, z))
        if l + 1 == nlev:
            out["CH"][l] = out["Pn"][l] = -1
            break
        ch = orc.divide_children(B[z])
        B = orc.sift_dup(ch, float(min_side)) if ch.shape[0] else np.zeros((0, 4))
        out["CH"][l], out["Pn"][l] = ch.shape[0], B.shape[0]
        if B.shape[0] == 0:
            break
    root = np.array([[0, 0, W - 1.0, H - 1.0]])
    B1 = orc.divide_region(root, min_side)
    out["P1"] = B1.shape[0]
    out["CH1"] = orc.divide_children(B1).shape[0]
    out["spec_rows"] = 1 + out["P1"] + out["CH1"]
    out["nlev"] = nlev
    if want_regions:
        out["regions"] = regions
    return out


def level_multiplicity(parents, min_side=10):
    """The largest number of children of `parents` that share one _sift_dup hash (0 without children): the level keeps at
    least CH / that many regions."""
    ch = orc.divide_children(parents)
    if ch.shape[0] == 0:
        return 0
    h = np.round(ch / float(min_side)).dot(np.array([1, 1e3, 1e6, 1e9]))
    return int(np.unique(h, return_counts=True)[1].max())


def max_multiplicity(H, W, min_side=10):
    """Over the FULL tree of a shape: per dividing level, the largest number of children that share one _sift_dup hash.
    (A pruned tree may keep another first occurrence of a hash, hence other regions below it: this measures the full
    tree only; level_multiplicity measures any level.)"""
    B = np.array([[0, 0, W - 1.0, H - 1.0]])
    out = []
    for _ in range(orc.num_levels(H, W, min_side) - 2):
        ch = orc.divide_children(B)
        h = np.round(ch / float(min_side)).dot(np.array([1, 1e3, 1e6, 1e9]))
        out.append(int(np.unique(h, return_counts=True)[1].max()))
        B = orc.sift_dup(ch, float(min_side))
    return out


# ---------------------------------------------------------------------------------------------------------------------
def runs_of(mask):
    """Planted cells as row runs (row, first column, one past the last)."""
    runs = []
    for r in range(mask.shape[0]):
        c = 0
        row = mask[r]
        while c < row.size:
            if row[c]:
                e = c
                while e < row.size and row[e]:
                    e += 1
                runs.append((r, c, e))
                c = e
            else:
                c += 1
    return runs


def mask_of(runs, fh, fw):
    m = np.zeros((fh, fw), dtype=bool)
    for r, c, e in runs:
        m[r, c:e] = True
    return m


def search(H, W, level, key, targets, seed=0, iters=4000, jitter=2, fill="raster", keep=None, batch=10000):
    """Seeded search for masks (and shapes within `jitter` pixels of H x W) whose populations()[key][level] equals each
    value of `targets` (a dict name -> predicate on the value, or an int): raster fill up to the crossing of the smallest
    target, then single-cell toggles -- a cell next to planted ones moves few regions (adjacent parents share children), an
    isolated one moves a whole parent's worth --, and one-pixel changes of H and W, which re-place every hash.  `keep`
    (populations -> bool) rejects states that break another limit.  Returns {name: (H, W, scale, runs, value)}."""
    rng = np.random.RandomState(seed)
    preds = {n: (t if callable(t) else (lambda v, t=t: v == t)) for n, t in targets.items()}
    lo = min(t for t in targets.values() if not callable(t))
    found = {}

    def val(h, w, m):
        p = populations(h, w, default_scale(h, w), 10, batch, m)
        ok = keep is None or keep(p)
        return (p[key][level] if level < p["nlev"] else 0), ok

    def note(h, w, m, v, ok):
        if not ok:
            return
        for n, pr in preds.items():
            if pr(v) and (n not in found or abs(v - lo) < abs(found[n][4] - lo)):
                found[n] = (h, w, default_scale(h, w), runs_of(m), v)

    h, w = H, W
    fh, fw = map_size(h, w, default_scale(h, w))
    order = np.arange(fh * fw) if fill == "raster" else rng.permutation(fh * fw)
    a, b = 0, fh * fw
    while a < b:                               # smallest fill whose value reaches the smallest target
        mid = (a + b) // 2
        m = np.zeros(fh * fw, dtype=bool)
        m[order[:mid]] = True
        if val(h, w, m.reshape(fh, fw))[0] >= lo:
            b = mid
        else:
            a = mid + 1
    m = np.zeros(fh * fw, dtype=bool)
    m[order[:a]] = True
    m = m.reshape(fh, fw)
    v, ok = val(h, w, m)
    note(h, w, m, v, ok)
    for _ in range(iters):
        if len(found) == len(preds) and all(not callable(t) or found[n][4] == lo + 1 for n, t in targets.items()):
            break
        kind = rng.randint(10)
        h2, w2, m2 = h, w, m.copy()
        if kind == 0 and jitter:
            h2 = int(np.clip(h + rng.randint(-1, 2), H - jitter, H + jitter))
            w2 = int(np.clip(w + rng.randint(-1, 2), W - jitter, W + jitter))
            if map_size(h2, w2, default_scale(h2, w2)) != m.shape:
                continue
        else:
            r, c = rng.randint(m.shape[0]), rng.randint(m.shape[1])
            m2[r, c] = not m2[r, c]
        v2, ok2 = val(h2, w2, m2)
        note(h2, w2, m2, v2, ok2)
        if ok2 and (abs(v2 - lo) <= abs(v - lo) or rng.rand() < 0.05):
            h, w, m, v = h2, w2, m2, v2
    return found


def twin(found, level, limit, batch=10000):
    """Every single-cell toggle of an at-limit state `found` (as search returns it): the smallest Pn[level] in
    limit + 1 .. limit + 8 among the toggles that leave P and U up to `level` and PZ above it unchanged -- the past-limit
    twin with the same tree above the limited level.  Returns a state like search's, or None."""
    h, w, sc, runs, _ = found
    fh, fw = map_size(h, w, sc)
    m = mask_of(runs, fh, fw)
    p0 = populations(h, w, sc, 10, batch, m)
    best = None
    for r in range(fh):
        for c in range(fw):
            m2 = m.copy()
            m2[r, c] = not m2[r, c]
            p = populations(h, w, sc, 10, batch, m2)
            if (p["P"][:level + 1], p["U"][:level + 1], p["PZ"][:level]) != (p0["P"][:level + 1], p0["U"][:level + 1], p0["PZ"][:level]):
                continue
            x = p["Pn"][level]
            if limit < x <= limit + 8 and (best is None or x < best[4]):
                best = (h, w, sc, runs_of(m2), x)
    return best


def keep_lv(p):
    """nothing but the level under test over a table: levels 1-3 within FL_R, level 4 within LV_R"""
    return all(x <= FL_R for x in p["P"][:4]) and p["P"][4] <= LV_R


def keep_fl(p):
    return all(x <= FL_R for x in p["P"][:3])


# How each frozen pair was found: at = search(H, W, level, "Pn", {"at": limit}, seed=seed, iters=3000, keep=keep)["at"], the
# first seed (counting from 1) whose at-limit state has a twin(at, level, limit); past = that twin.  The other cases are
# written down directly: a lattice (a * row + b * col) % mod == 0 over the first `frac` of the columns, or single cells.
RECIPES = {
    "lv_r": dict(H=800, W=1200, level=4, limit=LV_R, seed=1, keep=keep_lv),
    "fl_r": dict(H=320, W=1600, level=2, limit=FL_R, seed=5, keep=keep_fl),
    "fl_r_last": dict(H=300, W=1500, level=2, limit=FL_R, seed=2, keep=keep_fl),
    "pre_49": dict(H=600, W=1000, lattice=(3, 5, 29)), "pre_67": dict(H=400, W=900, lattice=(3, 5, 29)),
    "cap": dict(H=375, W=500, lattice=(3, 5, 13), frac=0.6), "batch_fused": dict(H=375, W=500, cells=[(19, 25)]),
    "p1_254": dict(H=320, W=13600, cells=[(0, 10), (1, 40)]), "p1_257": dict(H=320, W=13760, cells=[(0, 10), (1, 40)]),
}


def regenerate(name):
    """{"at": state, "past": state} of a searched pair of RECIPES, or the mask of a written-down case."""
    r = RECIPES[name]
    if "level" in r:
        at = search(r["H"], r["W"], r["level"], "Pn", {"at": r["limit"]}, seed=r["seed"], iters=3000, keep=r["keep"])["at"]
        return {"at": at, "past": twin(at, r["level"], r["limit"])}
    fh, fw = map_size(r["H"], r["W"], default_scale(r["H"], r["W"]))
    m = np.zeros((fh, fw), dtype=bool)
    if "cells" in r:
        for y, x in r["cells"]:
            m[y, x] = True
    else:
        a, b, mod = r["lattice"]
        rr, cc = np.mgrid[0:fh, 0:fw]
        m = ((a * rr + b * cc) % mod == 0) & (cc < r.get("frac", 1.0) * fw)
    return m


# ---------------------------------------------------------------------------------------------------------------------
def case_inputs(case):
    """(head, fmap [1,C,fh,fw], mask) of a frozen case: make_object_head(noise=0) on SMALL_DIMS, make_feature_map with the
    zoom channel replaced by the 0/1 mask."""
    from aznet_hip import synth
    H, W, scale = case["H"], case["W"], case["scale"]
    fh, fw = map_size(H, W, scale)
    mask = mask_of(case["runs"], fh, fw)
    dims = dict(synth.SMALL_DIMS)
    kw = dict(HEAD_KW)
    kw.update(dims)
    head = synth.make_object_head(**kw)
    fmap = synth.make_feature_map(MAP_SEED, dims["C"], fh, fw)
    fmap[0, HEAD_KW["zoom_channel"]] = mask.astype(np.float32)
    return head, fmap, mask


def load_cases():
    """The frozen cases (tests/search_limits_cases.py, literals)."""
    import search_limits_cases
    return search_limits_cases.CASES


def case_populations(case, batch=10000):
    fh, fw = map_size(case["H"], case["W"], case["scale"])
    return populations(case["H"], case["W"], case["scale"], 10, batch, mask_of(case["runs"], fh, fw))
