"""The cases of the AZ training data layer's edge tests (tests/test_train_edges_host.py on the CPU, tests/test_gpu_train_edges.py
on the device, tests/gen_golden_train_edges.py for what the REFERENCE records of them in tests/golden/g23_train_roidb_edges.npz),
as plain data plus small builders, deterministic from fixed seeds; and the comparison helpers of tests/test_gpu_train.py.

Bounds (derived in tests/test_gpu_train.py's docstring, unchanged here).  Integer / boolean / index outputs, ex_boxes, the noise
consumed, row order, dx, dy and the IoU column: bit-exact.  dw, dh: 4 ulp (f64).  means: 1e-12 relative-or-absolute; stds:
1e-12 * max(1, E[x^2] / var); normalised targets: what those two imply for (x - mean) / std.

  A  LEVEL_CASES    one image each whose levels outgrow the chain kernel's 1024 threads (or its 4096-child level, or the dedup
                    hash's range): (size, gt, seed, TrainCfg keywords, what the device must answer)
  B  param_cases()  az_train_params off its defaults and image sizes at the MIN_SIDE edges, small enough to record in full
  C  match_case()   hand-made example regions over N objects: the S x N match matrix beyond one wave and beyond 64 KB of LDS
  D  stats_*()      rows for az_train_target_stats: exact in any summation order, hostile classes, every chunk edge
The noise of a case is np.random.RandomState(seed).random_sample(n): the doubles np.random.random draws after np.random.seed(seed),
which is what the reference consumes in the generator."""
import hashlib

import numpy as np

import train_ref as tr

NT, LV_C, LDS_MAX, ST_CHUNK = 1024, 4096, 128 * 1024, 4096     # csrc/az_train.hip: NT, LV_C, azk_adj_lds_max(), ST_CHUNK

SUB16 = tr.SUBREGION + [[0.25, 0.25, 0.75, 0.75], [0, 0, 0.5, 0.5], [0.5, 0.5, 1, 1], [-0.25, -0.25, 0.75, 0.75],
                        [0.25, 0.25, 1.25, 1.25]]
ADD16 = tr.ADDREGIONS + [[a, b, a + 0.6, b + 0.6] for a in (0, 0.2, 0.4) for b in (0, 0.2, 0.4)] + [[0, 0, 0.5, 1], [0.5, 0, 1, 1]]
assert len(SUB16) == 16 and len(ADD16) == 16


# ---- the comparison helpers of tests/test_gpu_train.py -----------------------------------------------------------------------
def ulp_diff(a, b):
    """Distance in units of the last place of b (f64), elementwise."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.finfo(np.float64).tiny))


def check_targets(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.shape[0] == 0:
        return 0.0
    for col in (4, 5, 0, 1, 6):
        assert np.array_equal(got[:, col], ref[:, col]), (what, "column", col)
    u = float(ulp_diff(got[:, 2:4], ref[:, 2:4]).max())
    assert u <= 4.0, (what, "dw/dh ulp", u)
    return u


def stat_bounds(means, stds):
    """Per-entry absolute bounds of means and stds from the golden's own values."""
    dm = 1e-12 * np.maximum(1.0, np.abs(means))
    var = stds ** 2
    amp = np.where(var > 0, (var + means ** 2) / np.where(var > 0, var, 1.0), 1.0)
    ds = 1e-12 * np.maximum(1.0, amp) * np.maximum(1.0, np.abs(stds))
    return dm, ds


def check_stats(m, s, t, means, stds, t_raw, t_norm, in_err=0.0):
    """Device means / stds / normalised rows against the golden's, within the bounds the module docstring derives.
    in_err: absolute error bound of the raw dw / dh the device summed (0 when it was handed the golden's own rows; 4 ulp of
    the largest |x| when it computed them with its own log).  It moves a mean by <= in_err, E[x^2] - mean^2 by
    <= 4 max|x| in_err, hence a std by <= 2 max|x| in_err / std, and a normalised value by the usual quotient rule."""
    dm, ds = stat_bounds(means, stds)
    xmax = float(np.abs(t_raw[:, :4]).max()) if t_raw.shape[0] else 0.0
    dm = dm + in_err
    ds = ds + np.where(stds > 0, 2.0 * xmax * in_err / np.where(stds > 0, stds, 1.0), 0.0)
    print("max |dmean| %.3e (bound %.1e), max |dstd| / bound %.3e" % (np.abs(m - means).max(), dm.min(),
                                                                     (np.abs(s - stds) / ds).max()))
    assert np.all(np.abs(m - means) <= dm)
    assert np.all(np.abs(s - stds) <= ds)
    cls = t_raw[:, 5].astype(int)
    tol = (dm[cls] + in_err + np.abs(t_raw[:, :4] - means[cls]) * ds[cls] / stds[cls]) / stds[cls] \
        + 8 * np.spacing(np.abs(t_norm[:, :4]))
    assert np.all(np.abs(t[:, :4] - t_norm[:, :4]) <= tol)
    assert np.array_equal(t[:, 4:], t_norm[:, 4:])


# ---- shared ------------------------------------------------------------------------------------------------------------------
def cfg_of(kw):
    return tr.TrainCfg(**kw)


def tp_of(kw):
    return dict(cfg_of(kw).__dict__)


def noise_of(seed, n):
    return np.random.RandomState(int(seed)).random_sample(int(n))


def sha(a):
    """SHA-256 of an array's dtype, shape and bytes."""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def level_summary(stats):
    """What a case's preconditions are asserted on: the (P, PZ, CH) of every zoomed level and their maxima."""
    lv = stats.get("levels", [])
    return dict(levels=np.array(lv, dtype=np.int64).reshape(-1, 3), max_P=max([l[0] for l in lv] or [0]),
                max_PZ=max([l[1] for l in lv] or [0]), max_CH=max([l[2] for l in lv] or [0]),
                max_parent=int(stats.get("max_parent", 0)))


def small_objects(seed, h, w, n, lo=0.01, hi=0.06):
    """n small objects with a duplicate, a 1-px object and a 1-px-wide one (as random_image of tests/test_gpu_train.py)."""
    rng = np.random.RandomState(seed)
    bw, bh = rng.uniform(lo, hi, n) * w, rng.uniform(lo, hi, n) * h
    x1, y1 = rng.uniform(0, w - 1 - bw), rng.uniform(0, h - 1 - bh)
    gt = np.floor(np.stack([x1, y1, x1 + bw, y1 + bh], 1)).reshape(-1, 4)
    if n >= 4:
        gt[n - 1] = gt[0]
        gt[n - 2, 2:] = gt[n - 2, :2]
        gt[n - 3, 2] = gt[n - 3, 0]
    return gt


NO_GT = np.zeros((0, 4))
ONE_ROOT = [[0, 0, 1, 1]]

# ---- A. levels larger than the workgroup ---------------------------------------------------------------------------------------
# name: (size, gt, seed, TrainCfg keywords, answer).  answer: "ok", "capacity" (a level past LV_C: AZ_ERR_CAPACITY, needed_out
# both zero) or "invalid" (the dedup hash leaves [0, 2^40): AZ_ERR_INVALID).  The reference and train_ref know neither limit:
# they give regions for all of them.
LEVEL_CASES = {
    # 1. one to four passes over the children, parents within one pass
    "children_passes": ((320, 400), NO_GT, 1, dict(zoom_err_prob=0.7, train_rep=1), "ok"),
    # 2. more than 1024 parents: two passes of the label / noise / append loop, zoomed regions on both sides of index 1024
    "parent_passes": ((800, 1200), NO_GT, 2, dict(zoom_err_prob=0.5, train_rep=1), "ok"),
    # 3. every region zoomed: the fullest level that fits (children come in fives here, 4095 = 5 * 819) and a neighbour past it
    "level_full": ((215, 220), NO_GT, 1, dict(zoom_err_prob=1.0, train_rep=1), "ok"),
    "level_over": ((215, 221), NO_GT, 1, dict(zoom_err_prob=1.0, train_rep=1), "capacity"),
    # 4. one parent with more than 1024 children; a thin image whose first level overflows
    "thin_parent": ((12, 2100), NO_GT, 1, dict(zoom_err_prob=1.0, train_rep=1, addregions=ONE_ROOT), "ok"),
    "thin_over": ((12, 4000), NO_GT, 1, dict(zoom_err_prob=1.0, train_rep=1), "capacity"),
    # 5. more than 1024 super-regions
    "objects_94": ((800, 800), small_objects(94, 800, 800, 94), 94, dict(train_rep=1), "ok"),
    "objects_120": ((800, 800), small_objects(120, 800, 800, 120), 120, dict(train_rep=1), "ok"),
    "objects_64_s16": ((800, 800), small_objects(64, 800, 800, 64), 64, dict(train_rep=1, subregion=SUB16), "ok"),
    "objects_65_s16": ((800, 800), small_objects(65, 800, 800, 65), 65, dict(train_rep=1, subregion=SUB16), "ok"),
    # 7. MIN_SIDE 1 on an image 1200 px high: the children's y2 / MIN_SIDE reaches 1100, the key 1.1e12 > 2^40
    "hash_range": ((1200, 4), NO_GT, 1, dict(zoom_err_prob=1.0, train_rep=1, min_side=1, addregions=ONE_ROOT), "invalid"),
}
# 6. several such images in one call on one stream: a case-2 image, a case-5 image, an image without levels, an ordinary one
SHARED_STREAM = dict(kw=dict(zoom_err_prob=0.5, train_rep=1), seed=2,
                     images=[((800, 1200), NO_GT), ((800, 800), small_objects(120, 800, 800, 120)),
                             ((8, 300), np.array([[10., 1., 60., 6.]])), ((375, 500), small_objects(7, 375, 500, 6, 0.1, 0.4))])


def run_level_case(name, stats=None):
    """train_ref on a case of group A -> (boxes f64, labels, used)."""
    size, gt, seed, kw, _ = LEVEL_CASES[name]
    return tr.compute_ex_rois(size, gt, noise_of(seed, 60000), cfg_of(kw), stats)


def level_digests(size, gt, ex, zl, used, targets, levels):
    """What g23 records of a large case: counts and SHA-256s."""
    return dict(E=np.array(ex.shape[0]), used=np.array(used), n_zoom=np.array(int(np.sum(zl))),
                T=np.array(targets.shape[0]), levels=np.asarray(levels, dtype=np.int64).reshape(-1, 3),
                sha_ex64=np.array(sha(np.asarray(ex, dtype=np.float64))), sha_ex32=np.array(sha(np.asarray(ex, dtype=np.float32))),
                sha_zoom=np.array(sha(np.asarray(zl).astype(bool))), sha_targets=np.array(sha(np.asarray(targets, dtype=np.float64))),
                sha_levels=np.array(sha(np.asarray(levels, dtype=np.int64).reshape(-1, 3))))


# ---- B. az_train_params off its defaults ---------------------------------------------------------------------------------------
B_SIZE = (150, 200)


def b_objects():
    gt = small_objects(23, 150, 200, 14, 0.08, 0.45)
    return gt


def param_cases():
    """(name, size, gt, seed, TrainCfg keywords).  train_rep 2 unless it is the subject, to keep the recorded arrays small."""
    gt = b_objects()
    out = []

    def add(name, kw, size=B_SIZE, g=gt):
        k = dict(train_rep=2)
        k.update(kw)
        out.append((name, size, g, 100 + len(out), k))
    for r in (0, 1, 3):
        add("rep%d" % r, dict(train_rep=r))
    add("add1", dict(addregions=ONE_ROOT))
    add("add16", dict(addregions=ADD16, train_rep=1))
    for s in (1, 5, 16):
        add("sub%d" % s, dict(subregion=SUB16[:s]))
    add("ms5", dict(min_side=5, train_rep=1))
    add("ms16", dict(min_side=16))
    add("ms12_5", dict(min_side=12.5))
    add("zep0", dict(zoom_err_prob=0.0))
    add("zep1", dict(zoom_err_prob=1.0, train_rep=1))
    add("emb_01_09", dict(emb_reg_thresh=0.1, emb_obj_thresh=0.9))
    add("emb_10_00", dict(emb_reg_thresh=1.0, emb_obj_thresh=0.0))
    add("adj0", dict(adj_thresh=0.0, train_rep=1))
    add("adj05", dict(adj_thresh=0.5))
    add("adj1", dict(adj_thresh=1.0))
    add("eps14", dict(eps=1e-14))
    add("eps6", dict(eps=1e-6))
    thin = np.array([[10., 1., 60., 6.], [100., 0., 140., 7.]])
    add("side_below", dict(), (8, 300), thin)                       # K = 0 and every super-region too low: E = 0
    add("side_min", dict(), (10, 64), np.array([[3., 0., 40., 9.], [20., 2., 30., 8.]]))
    add("side_2min", dict(), (20, 90), np.array([[3., 1., 40., 14.], [50., 2., 80., 19.]]))      # int(log2(2) + 1) = 2
    add("wide", dict(), (90, 260), small_objects(5, 90, 260, 6, 0.1, 0.5))
    add("tall", dict(), (260, 90), small_objects(6, 260, 90, 6, 0.1, 0.5))
    return out


# a batch whose first, a middle and the last image have no example regions (repeated values in ex_off)
EMPTY_BATCH = dict(kw=dict(train_rep=2), seed=321, names=["side_below", "wide", "side_below", "tall", "side_below"])


def empty_batch_images():
    by = {c[0]: c for c in param_cases()}
    return [(by[n][1], by[n][2]) for n in EMPTY_BATCH["names"]]


# ---- C. the match matrix ---------------------------------------------------------------------------------------------------------
MATCH_SIZES = [(63, 11), (64, 11), (65, 11), (129, 11), (744, 11), (745, 11), (746, 11), (1489, 11), (1024, 16)]
MATCH_OVER = [(1490, 11), (1025, 16)]


def match_case(N, S):
    """Example regions ex f32 [K,4] and objects gt f32 [N,4] for one image: region k's sub-region s is itself an object, at a
    column chosen so that the flat indices s * N + column visit every group of 64 entries of the matrix and every lane (the first
    at column 0, the last at N - 1): round s of region k finds its first maximum 1.0 there; every sixth region has objects for its first five sub-regions only (its later
    rounds, at ADJ_THRESH 0, are won at overlap 0); from N = 129 on, some objects have an identical twin 70 columns later
    (a tie between lanes, the earlier column wins).  Everything else is far away.  All coordinates are exact in float32."""
    sub = np.array(SUB16[:S], dtype=np.float64)
    K = min(36, N // S)
    col, used = {(0, 0): 0, (K - 1, S - 1): N - 1}, {0, N - 1}
    for s in range(S):                                              # row s of the matrix holds the groups lo .. hi of 64 entries
        lo, hi = (s * N) // 64, (s * N + N - 1) // 64
        for i, k in enumerate(k for k in range(K) if not (k % 6 == 2 and s >= 5)):
            if (k, s) in col:
                continue
            n = 64 * (lo + i % (hi - lo + 1)) + (11 * k + 5 * s + k // 7) % 64 - s * N
            n = min(max(n, 0), N - 1)
            while n in used:
                n = (n + 1) % N
            col[(k, s)] = n
            used.add(n)
    ex = np.zeros((K, 4))
    gt = np.zeros((N, 4))
    gt[:, 0] = 100000.0 + 50.0 * np.arange(N)                       # far away, all distinct
    gt[:, 1] = 7.0
    gt[:, 2] = gt[:, 0] + 20.0 + (np.arange(N) % 7)
    gt[:, 3] = 30.0
    planted = {}
    for k in range(K):
        x0, y0 = 200.0 + 400.0 * (k % 8), 200.0 + 300.0 * (k // 8)
        re = np.array([x0, y0, x0 + 64.0 + 8 * (k % 3), y0 + 48.0 + 4 * (k % 5)])
        ex[k] = re
        L = np.array([re[2] - re[0], re[3] - re[1], re[2] - re[0], re[3] - re[1]])
        d = np.array([re[0], re[1], re[0], re[1]])
        for s in range(S):
            if k % 6 == 2 and s >= 5:
                continue
            gt[col[(k, s)]] = L * sub[s] + d
            planted[col[(k, s)]] = (k, s)
    twins = 0
    if N >= 129:
        free = set(range(N)) - set(planted)
        for c in sorted(planted):
            if c + 70 in free and twins < 8:
                gt[c + 70] = gt[c]
                free.discard(c + 70)
                twins += 1
    assert np.array_equal(gt.astype(np.float32).astype(np.float64), gt) and np.array_equal(ex.astype(np.float32), ex)
    return ex.astype(np.float32), gt.astype(np.float32), twins


def match_kw(S, adj_thresh=0.1):
    return dict(subregion=SUB16[:S], adj_thresh=adj_thresh)


# ---- D. target statistics --------------------------------------------------------------------------------------------------------
STATS_NSUB = [1, 2, 11, 15, 16]
STATS_T = [0, 1, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 1]
HOSTILE = [-1.0, None, 1e9, 2.5, -0.5]          # None: n_sub itself


def stats_exact_rows(n_sub, T, seed):
    """[T,7] rows whose statistics are exact in any summation order: the four deltas are multiples of 2^-8 in [-4, 4], every
    class in [0, n_sub) has 2^p rows (the largest p with n_sub * 2^p <= T; with T < n_sub, one row each for the first T
    classes and none for the rest), the remaining rows carry classes no statistic counts (-1, n_sub, 1e9, 2.5, -0.5), and the
    rows are shuffled over all chunks.  Class 0's rows are all identical when it has more than one (std exactly 0)."""
    rng = np.random.RandomState(seed)
    t = np.zeros((T, 7))
    t[:, :4] = rng.randint(-1024, 1025, (T, 4)) / 256.0
    t[:, 4] = rng.randint(0, 50, T)
    t[:, 6] = rng.randint(0, 257, T) / 256.0
    per = 0
    if T >= n_sub:
        per = 1
        while n_sub * per * 2 <= T:
            per *= 2
    cls = np.repeat(np.arange(n_sub), per) if per else np.arange(T)
    rest = T - cls.size
    host = [float(n_sub) if v is None else v for v in HOSTILE]
    cls = np.concatenate([cls.astype(np.float64), np.array([host[i % len(host)] for i in range(rest)], dtype=np.float64)])
    t[:, 5] = cls
    if per > 1:
        t[cls == 0, :4] = t[np.where(cls == 0)[0][0], :4]
    return np.ascontiguousarray(t[rng.permutation(T)])


def stats_random_rows(n_sub, T, seed):
    rng = np.random.RandomState(seed)
    t = np.zeros((T, 7))
    t[:, :2] = rng.uniform(-3, 3, (T, 2))
    t[:, 2:4] = np.log(rng.uniform(0.1, 8, (T, 2)))
    t[:, 4] = rng.randint(0, 900, T)
    t[:, 5] = rng.randint(0, n_sub, T)
    t[:, 6] = rng.uniform(0.1, 1, T)
    return t


def stats_reference(t, n_sub, eps, normalise=True):
    """The reference's statistics (roidb.py:110-134, train_ref.target_stats) of one table -> (means, stds, normalised copy)."""
    c = tr.TrainCfg(eps=eps, subregion=SUB16[:n_sub])
    tn = t.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        m, s = tr.target_stats([tn], c, normalise)
    return m, s, tn


# ---- E. the host layer -----------------------------------------------------------------------------------------------------------
class FakeImdb(object):
    """What az_data_layer.roidb reads of an imdb."""

    def __init__(self, images, name="edges"):
        self.name, self.cache_path = name, "."
        self.sizes = [s for s, _ in images]
        self.roidb = [{"boxes": np.asarray(g, dtype=np.float64).reshape(-1, 4)} for _, g in images]
        self.image_index = list(range(len(images)))

    def image_path_at(self, i):
        return "fake://%d" % i

    def image_size(self, i):
        return self.sizes[i]


class patched_cfg(object):
    """detect.config.cfg with the keys of TrainCfg keywords `kw` edited, restored on exit."""
    KEYS = dict(min_side=("SEAR", "MIN_SIDE"), train_rep=("SEAR", "TRAIN_REP"), zoom_err_prob=("SEAR", "ZOOM_ERR_PROB"),
                emb_obj_thresh=("SEAR", "EMB_OBJ_THRESH"), emb_reg_thresh=("SEAR", "EMB_REG_THRESH"),
                adj_thresh=("SEAR", "ADJ_THRESH"), addregions=("TRAIN", "ADDREGIONS"), subregion=("SEAR", "SUBREGION"))

    def __init__(self, cfg, kw):
        self.cfg, self.kw, self.old = cfg, dict(kw), []

    def __enter__(self):
        for k, v in self.kw.items():
            if k == "eps":
                self.old.append((self.cfg, "EPS", self.cfg.EPS))
                self.cfg.EPS = v
                continue
            sec, key = self.KEYS[k]
            node = getattr(self.cfg, sec)
            self.old.append((node, key, getattr(node, key)))
            setattr(node, key, v)
            if k == "subregion":
                self.old.append((node, "NUM_SUBREG", node.NUM_SUBREG))
                node.NUM_SUBREG = len(v)
        return self.cfg

    def __exit__(self, *a):
        for node, key, v in reversed(self.old):
            setattr(node, key, v)


def host_overflow(rdl):
    """prepare_roidb on the image whose level overflows: the error surfaces, np.random stays where it was."""
    from aznet_hip import ffi
    from detect.config import cfg
    size, gt, seed, kw, _ = LEVEL_CASES["level_over"]
    imdb = FakeImdb([((150, 200), b_objects()), (size, gt)])
    with patched_cfg(cfg, kw):
        np.random.seed(11)
        before = np.random.get_state()
        err = None
        try:
            rdl.prepare_roidb(imdb)
        except ffi.AzError as e:
            err = e
        after = np.random.get_state()
    assert err is not None and err.code == ffi.AZ_ERR_CAPACITY and not hasattr(err, "needed") and not hasattr(err, "needed_cap")
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]


def host_mixed(rdl, monkeypatch):
    """prepare_roidb + add_adjacent_prediction_targets over a case-2 image, a case-5 image and an image without regions, two
    images per device call -> (roidb, np.random state, means, stds)."""
    from detect.config import cfg
    S = SHARED_STREAM
    monkeypatch.setattr(rdl, "CHUNK", 2)
    imdb = FakeImdb(S["images"][:3])
    with patched_cfg(cfg, S["kw"]):
        np.random.seed(S["seed"])
        rdl.prepare_roidb(imdb)
        state = np.random.get_state()
        means, stds = rdl.add_adjacent_prediction_targets(imdb)
    return imdb.roidb, state, means, stds


def mixed_expectation():
    """The same by train_ref walking np.random's stream itself -> (per image boxes f32 / labels / raw targets, state)."""
    S = SHARED_STREAM
    c = cfg_of(S["kw"])
    np.random.seed(S["seed"])
    out = []
    for size, gt in S["images"][:3]:
        st = np.random.get_state()
        noise = np.random.random(8000)
        np.random.set_state(st)
        b, z, u = tr.compute_ex_rois(size, gt, noise, c)
        if u:
            np.random.random(u)
        out.append((b.astype(np.float32), z, tr.compute_targets(gt, b.astype(np.float32), c)))
    return out, np.random.get_state()


def check_mixed(roidb, state, means, stds, in_err_ulps):
    exp, exp_state = mixed_expectation()
    assert np.array_equal(state[1], exp_state[1]) and state[2] == exp_state[2]
    for e, (b, z, t) in zip(roidb, exp):
        assert e["ex_boxes"].dtype == np.float32 and np.array_equal(e["ex_boxes"], b) and np.array_equal(e["zoom_gt"], z)
        assert e["bbox_targets"].shape == t.shape
    raw = np.vstack([t for _, _, t in exp])
    rm, rs, rn = stats_reference(raw, 11, 1e-14)
    got = np.vstack([e["bbox_targets"] for e in roidb])
    in_err = in_err_ulps * np.finfo(np.float64).eps * max(1.0, float(np.abs(raw[:, 2:4]).max()))
    check_stats(means.reshape(11, 4), stds.reshape(11, 4), got, rm, rs, raw, rn, in_err)
    assert roidb[2]["ex_boxes"].shape == (0, 4) and roidb[2]["bbox_targets"].shape == (0, 7)
