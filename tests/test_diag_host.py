"""CPU: the proposal diagnosis off the device -- the NumPy restatement's own conditions on the shared cases
(tests/diag_ref.py), AZ_results.mat against the reference's own file (golden g24, tests/gen_golden_diag.py), pixel means,
the summary on degenerate tables, the two command lines."""
import os
import sys

import numpy as np
import pytest

import diag_ref as R
import train_ref
from helpers import GOLDEN
from oracle import az_oracle as orc

TOOLS = os.path.join(os.path.dirname(GOLDEN), os.pardir, "az-net_amd", "tools")


# ------------------------------------------------------------------------------------------ the restatement's conditions
def _cases():
    return {"offsets": R.offsets_case(), "wave": R.wave_case()[0], "levels": R.levels_case()[0],
            "thresholds": R.threshold_case(), "random": R.random_case(n_images=16)}


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_best_iou_per_image_equals_the_set(cases):
    for name, case in cases.items():
        ref = R.diag_eval(case, R.TZ_EXACT)
        whole = R.best_iou_on_set(case)
        assert np.array_equal(ref["best_iou"].view(np.uint64), whole.view(np.uint64)), name


def test_offsets_case_has_its_empty_images():
    case = R.offsets_case()
    got = [(a.shape[0], g.shape[0], p.shape[0]) for a, g, p in zip(case["anchors"], case["gt"], case["props"])]
    assert got == R.OFFSET_COUNTS
    assert got[0][1:] == (0, 0) and got[2][:2] == (0, 0) and got[-1] == (0, 0, 0)
    ref = R.diag_eval(case, 0.5)
    assert ref["recall_table"][-1, 0] == sum(c[1] for c in R.OFFSET_COUNTS)
    assert ref["level_table"][:, 0].sum() == sum(c[0] for c in R.OFFSET_COUNTS)
    # image 1 has objects and no proposals
    assert np.array_equal(ref["best_rank"][:2], [-1, -1]) and np.array_equal(ref["best_iou"][:2], [0.0, 0.0])


def test_wave_case_has_its_ties():
    case, want = R.wave_case()
    assert [p.shape[0] for p in case["props"]] == list(R.WAVE_COUNTS) + [300] * len(R.WAVE_TIES)
    for k, (r0, r1) in enumerate(R.WAVE_TIES):
        p = case["props"][len(R.WAVE_COUNTS) + k]
        assert np.array_equal(p[r0], p[r1])
        ov = orc.bbox_overlaps(p, case["gt"][0])[:, 0]
        assert ov[r0] == ov[r1] == ov.max() and (ov == ov.max()).sum() == 2
    ref = R.diag_eval(case, 0.5)
    assert np.array_equal(ref["best_rank"], want) and np.array_equal(ref["first_hit"], want)


def test_levels_case_has_every_level_and_an_unheld_object():
    case, want = R.levels_case()
    lv = case["level"][0]
    assert sorted(lv.tolist()) == list(range(R.AZ_MAX_LEVELS)) and lv[0] == R.AZ_MAX_LEVELS - 1
    h = R.holds(case["anchors"][0], case["gt"][0], R.EMB_OBJ)
    assert h[:, 0].all() and not h[:, 2].any()
    # object 1: the deepest holder (level 2) sits BEFORE the shallower ones in memory
    idx = np.nonzero(h[:, 1])[0]
    assert lv[idx].tolist() == [2, 1, 0]
    ref = R.diag_eval(case, 0.5)
    assert np.array_equal(ref["deepest_level"], want)
    assert np.array_equal(ref["level_table"][:, 0], np.ones(R.AZ_MAX_LEVELS))


def test_threshold_case_has_its_exact_pairs():
    case = R.threshold_case()
    up = np.nextafter(0.5, 1.0)
    ref, ref_up = R.diag_eval(case, R.TZ_EXACT), R.diag_eval(case, R.TZ_EXACT, iou_thresh=up)
    off = np.cumsum([0] + [g.shape[0] for g in case["gt"]])
    # 0: IoU exactly 0.5
    assert orc.bbox_overlaps(case["props"][0], case["gt"][0])[0, 0] == 0.5
    assert ref["first_hit"][0] == 0 and ref_up["first_hit"][0] == -1 and ref["best_iou"][0] == 0.5
    # 1: first_hit at cuts[0] - 1 and at cuts[0]
    assert ref["first_hit"][off[1]:off[2]].tolist() == [R.CUTS[0] - 1, R.CUTS[0]]
    only1 = R.diag_eval(R.sub_case(case, 1), R.TZ_EXACT)["recall_table"]
    assert only1[0, 0] == 1 and only1[1, 0] == 2 and only1[-1, 0] == 2
    # 2: areas on the edges
    g = case["gt"][2]
    assert ((g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)).tolist() == [1024.0, 1023.0, 9216.0, 9215.0]
    only2 = R.diag_eval(R.sub_case(case, 2), R.TZ_EXACT)["recall_table"]
    assert only2[-1].tolist() == [4, 1, 2, 1]
    # 3: zoom == tz at level 1, below it at level 1, below it at level 0
    z, lv = case["zoom"][3], case["level"][3]
    assert float(z[1]) == R.TZ_EXACT and float(z[2]) < R.TZ_EXACT and float(z[0]) < R.TZ_EXACT and lv.tolist() == [0, 1, 1]
    only3 = R.diag_eval(R.sub_case(case, 3), R.TZ_EXACT)["level_table"]
    assert only3[0, :2].tolist() == [1, 1] and only3[1, :2].tolist() == [2, 1]
    # 4: coverage exactly EMB_OBJ and area ratio exactly EMB_REG
    a, g = case["anchors"][4], case["gt"][4]
    ga = (g[0, 2] - g[0, 0] + 1) * (g[0, 3] - g[0, 1] + 1)
    aa = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    iw = min(a[0, 2], g[0, 2]) - max(a[0, 0], g[0, 0]) + 1
    ih = min(a[0, 3], g[0, 3]) - max(a[0, 1], g[0, 1]) + 1
    assert iw * ih / (ga + 1e-14) == R.EMB_OBJ and (ga / (aa + 1e-14) == R.EMB_REG).all()
    only4 = R.diag_eval(R.sub_case(case, 4), R.TZ_EXACT)
    assert only4["anchor_label"].tolist() == [1, 1] and only4["deepest_level"].tolist() == [2]
    # just past either threshold the label is gone
    assert not train_ref.zoom_labels(a[:1], g, R.EMB_REG, np.nextafter(R.EMB_OBJ, 1.0)).any()
    assert not train_ref.zoom_labels(a, g, np.nextafter(R.EMB_REG, 0.0), R.EMB_OBJ).any()


def test_random_case_per_image_rows_add_up(cases):
    case = cases["random"]
    whole = R.diag_eval(case, R.TZ_EXACT)
    lt, rt = np.zeros_like(whole["level_table"]), np.zeros_like(whole["recall_table"])
    for i in range(len(case["gt"])):
        one = R.diag_eval(R.sub_case(case, i), R.TZ_EXACT)
        lt += one["level_table"]
        rt += one["recall_table"]
    assert np.array_equal(lt, whole["level_table"]) and np.array_equal(rt, whole["recall_table"])
    assert (whole["first_hit"] >= 0).any() and (whole["first_hit"] < 0).any()
    assert whole["anchor_label"].any() and not whole["anchor_label"].all()


# ------------------------------------------------------------------------------------------------------ AZ_results.mat
def _cells_equal(a, b, what):
    assert type(a) is type(b), what
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == object:
        for idx in np.ndindex(a.shape):
            _cells_equal(a[idx], b[idx], "%s%r" % (what, idx))
    else:
        assert np.array_equal(a, b), what


def test_write_az_results_matches_the_reference_file(tmp_path):
    import scipy.io as sio
    from detect import tune
    gold = sio.loadmat(os.path.join(GOLDEN, "g24_az_results.mat"))
    keys = [k for k in gold if not k.startswith("__")]
    assert sorted(keys) == sorted(tune.AZ_RESULTS_KEYS)
    n = gold["fn"].shape[1]
    assert n == 3
    # what test_proposals collects, rebuilt from the file: arrays per image, str file names, shape tuples, scalars
    results = {
        "prop_boxes": [gold["prop_boxes"][0, i] for i in range(n)],
        "anchor_boxes": [gold["anchor_boxes"][0, i] for i in range(n)],
        "gt_boxes": [gold["gt_boxes"][0, i] for i in range(n)],
        "fn": [str(gold["fn"][0, i][0]) for i in range(n)],
        "im_shapes": [tuple(int(v) for v in gold["im_shapes"][0, i].ravel()) for i in range(n)],
        "Tz": float(gold["Tz"][0, 0]), "num_proposals": int(gold["num_proposals"][0, 0]),
    }
    assert results["gt_boxes"][0].dtype == np.uint16 and results["gt_boxes"][1].shape == (0, 4)
    assert results["im_shapes"] == [(100, 64, 3), (64, 100, 3), (120, 160, 3)] and results["num_proposals"] == 50
    path = str(tmp_path / "AZ_results.mat")
    tune.write_az_results(path, results)
    mine = sio.loadmat(path)
    assert [k for k in mine if not k.startswith("__")] == keys
    for k in keys:
        _cells_equal(mine[k], gold[k], k)


# ---------------------------------------------------------------------------------------------------------- pixel means
class _StubImdb(object):
    name = "stub"

    def __init__(self, images):
        self.images = images
        self.image_index = list(range(len(images)))

    def image_at(self, i):
        return self.images[i]

    def image_path_at(self, i):
        return "stub://%d" % i


def _running_mean(images):
    """tools/pixel_means.py:49-58 of the reference."""
    means = np.zeros((3,))
    num_pixels = 0.0
    for im in images:
        im_means = im.mean(axis=(0, 1))
        im_num_pixels = float(im.shape[0] * im.shape[1])
        means = means * num_pixels / (num_pixels + im_num_pixels) + im_means * im_num_pixels / (num_pixels + im_num_pixels)
        num_pixels = num_pixels + im_num_pixels
    return means


def _images(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]


@pytest.mark.parametrize("shapes", [[(1, 1)], [(1, 5)], [(7, 11)], [(97, 131)],
                                    [(1, 1), (1, 5), (7, 11), (97, 131), (64, 100), (100, 64), (33, 2), (120, 160)]],
                         ids=["1x1", "1x5", "7x11", "97x131", "eight_mixed"])
def test_pixel_means_exact_sums_and_the_running_mean(shapes, capsys):
    from datasets.pixel_means import pixel_means, channel_sums
    images = _images(shapes, 5 + len(shapes))
    db = _StubImdb(images)
    sums, npix = channel_sums(db)
    want = sum(np.sum(im.reshape(-1, 3), axis=0, dtype=np.uint64) for im in images)
    assert sums.dtype == np.uint64 and np.array_equal(sums, want) and npix == sum(h * w for h, w in shapes)
    capsys.readouterr()
    means = pixel_means(db)
    out = capsys.readouterr().out
    N = len(images)
    assert "Processing 0/%d, the mean is (" % N in out and "Processing %d/%d, the mean is (" % (N - 1, N) in out
    assert means.dtype == np.float64 and np.array_equal(means, want / float(npix))
    # about six roundings per image on values <= 255 in the running mean; the exact sum has one
    bound = 8 * N * 2.0 ** -53 * 255
    assert np.abs(means - _running_mean(images)).max() <= bound


def test_pixel_means_refuses_other_layouts():
    from datasets.pixel_means import pixel_means
    with pytest.raises(ValueError):
        pixel_means(_StubImdb([np.zeros((4, 4), np.uint8)]))
    assert np.array_equal(pixel_means(_StubImdb([])), np.zeros(3))


# -------------------------------------------------------------------------------------------------------------- summary
def test_summary_lines_on_empty_tables():
    from detect.diagnose import summary_lines
    empty = {"level_table": np.zeros((R.AZ_MAX_LEVELS, 4), np.int64), "recall_table": np.zeros((len(R.CUTS) + 1, 4), np.int64),
             "cuts": np.array(R.CUTS), "first_hit": np.zeros(0, np.int32), "deepest_level": np.zeros(0, np.int32),
             "best_iou": np.zeros(0), "best_rank": np.zeros(0, np.int32), "gt_off": np.zeros(1, np.int32)}
    with np.errstate(all="raise"):
        lines = summary_lines(empty)
    assert any("no anchors" in l for l in lines) and any("n/a" in l for l in lines)
    # levels 0 and 3 in use, 1-2 empty; a level with anchors none of which is zoomed or labelled
    lt = np.zeros((R.AZ_MAX_LEVELS, 4), np.int64)
    lt[0] = [2, 2, 1, 1]
    lt[3] = [5, 0, 0, 0]
    case, _ = R.levels_case()
    d = R.diag_eval(case, 0.5)
    d.update(level_table=lt, cuts=np.array(R.CUTS), gt_off=np.array([0, 3], np.int32), Tz=0.5,
             need_level=np.array([3, 3, 3], np.int32), gt_image=np.zeros(3, np.int32), gt_area=np.full(3, 400.0))
    with np.errstate(all="raise"):
        lines = summary_lines(d)
    text = "\n".join(lines)
    assert "never reached" in text and "reached but not hit" in text
    first = next(i for i, l in enumerate(lines) if l.startswith("Recall at"))
    assert [l.split()[0] for l in lines[2:first]] == ["0", "3"]              # the level rows: empty levels are left out
    assert "n/a" in lines[3]                                                  # level 3: nothing zoomed, nothing labelled
    # objects 1 (deepest 2 < need 3) and 2 (held by no anchor) were never reached; none was reached and missed
    assert "their size): 2" in text and "failed):          0" in text


def test_need_level():
    from detect.diagnose import _need_level
    # root 500x375; an object of a quarter of its area is asked for at level 0 only (ratio 0.25 <= 0.25): sits at level 1
    root = np.full(3, 500.0 * 375.0)
    got = _need_level(root, np.array([500.0 * 375.0, 500.0 * 375.0 / 4, 500.0 * 375.0 / 64]), 0.25)
    assert got.tolist() == [0, 1, 3]
    assert _need_level(np.zeros(1), np.array([100.0]), 0.25).tolist() == [0]


# ------------------------------------------------------------------------------------------------------------------ CLI
def _tool(name):
    sys.path.insert(0, os.path.abspath(TOOLS))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_cli_parsers_accept_the_reference_flags():
    d = _tool("diagnose_prop").parser().parse_args(
        ["--gpu", "1", "--def", "a.prototxt", "--def_fc", "b.prototxt", "--net", "w.caffemodel", "--cfg", "c.yml", "--wait", "1",
         "--imdb", "voc_2007_test", "--thresh", "thresh.pkl", "--exp", "e"])
    assert (d.gpu_id, d.prototxt, d.prototxt_fc, d.caffemodel, d.cfg_file, d.imdb_name, d.thresh_file, d.exp_dir) == \
        (1, "a.prototxt", "b.prototxt", "w.caffemodel", "c.yml", "voc_2007_test", "thresh.pkl", "e")
    d = _tool("diagnose_prop").parser().parse_args(["--tz", "0.5"])
    assert d.tz == 0.5 and d.imdb_name == "voc_2007_test" and d.caffemodel == "synthetic"
    p = _tool("pixel_means").parser()
    assert p.parse_args(["--imdb", "voc_2012_trainval"]).imdb_name == "voc_2012_trainval"
    assert p.parse_args([]).imdb_name == "voc_2007_trainval"


def test_diagnose_prop_refuses_several_ranks():
    import subprocess
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "diagnose_prop.py"), "--tz", "0.5", "--imdb", "synthetic_64x64_1"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "one process" in r.stderr
