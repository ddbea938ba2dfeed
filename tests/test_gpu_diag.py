"""GPU: az_diag_eval against its NumPy restatement (tests/diag_ref.py) -- integer tables, labels, ranks and levels
exactly, best_iou bit for bit -- at the offsets, wave edges, exact thresholds and levels at which the two kernels can go
wrong; its error returns; and the front door: detect.tune.test_proposals, detect.diagnose and tools/diagnose_prop.py."""
import io
import os
import pickle
import shutil
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import diag_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    from aznet_hip import synth
    from aznet_hip.net import HipAZNet
    return HipAZNet(synth.make_head(seed=77, **synth.SMALL_DIMS), name="small_diag")


@pytest.fixture(scope="module")
def ctx(small):
    return small.ctx


def run(ctx, case, tz, iou_thresh=0.5, cuts=R.CUTS, edges=R.EDGES):
    return ctx.diag_eval(case["anchors"], case["zoom"], case["level"], case["gt"], case["props"], tz, R.EMB_REG, R.EMB_OBJ,
                         iou_thresh=iou_thresh, cuts=cuts, area_edges=edges)


def test_offsets_joint_and_alone(ctx):
    case = R.offsets_case()
    want = R.diag_eval(case, R.TZ_EXACT)
    got = run(ctx, case, R.TZ_EXACT)
    R.assert_same(got, want, "joint")
    a0, g0 = got["anc_off"], got["gt_off"]
    assert a0.tolist() == np.cumsum([0] + [c[0] for c in R.OFFSET_COUNTS]).tolist()
    lt, rt = np.zeros_like(got["level_table"]), np.zeros_like(got["recall_table"])
    for i in range(len(R.OFFSET_COUNTS)):
        one = run(ctx, R.sub_case(case, i), R.TZ_EXACT)
        R.assert_same(one, R.diag_eval(R.sub_case(case, i), R.TZ_EXACT), "image %d alone" % i)
        assert np.array_equal(one["anchor_label"], got["anchor_label"][a0[i]:a0[i + 1]])
        for k in ("best_iou", "best_rank", "first_hit", "deepest_level"):
            assert np.array_equal(one[k], got[k][g0[i]:g0[i + 1]]), (i, k)
        lt += one["level_table"]
        rt += one["recall_table"]
    assert np.array_equal(lt, got["level_table"]) and np.array_equal(rt, got["recall_table"])


def test_wave_edges_first_maximum_wins(ctx):
    case, want_rank = R.wave_case()
    got = run(ctx, case, 0.5)
    R.assert_same(got, R.diag_eval(case, 0.5), "wave")
    assert np.array_equal(got["best_rank"], want_rank) and np.array_equal(got["first_hit"], want_rank)


def test_exact_thresholds(ctx):
    case = R.threshold_case()
    up = float(np.nextafter(0.5, 1.0))
    got, got_up = run(ctx, case, R.TZ_EXACT), run(ctx, case, R.TZ_EXACT, iou_thresh=up)
    R.assert_same(got, R.diag_eval(case, R.TZ_EXACT), "thresholds")
    R.assert_same(got_up, R.diag_eval(case, R.TZ_EXACT, iou_thresh=up), "thresholds, next double up")
    off = got["gt_off"]
    assert got["best_iou"][0] == 0.5 and got["first_hit"][0] == 0 and got_up["first_hit"][0] == -1
    assert got["first_hit"][off[1]:off[2]].tolist() == [R.CUTS[0] - 1, R.CUTS[0]]
    one = run(ctx, R.sub_case(case, 1), R.TZ_EXACT)["recall_table"]
    assert one[0, 0] == 1 and one[1, 0] == 2
    assert run(ctx, R.sub_case(case, 2), R.TZ_EXACT)["recall_table"][-1].tolist() == [4, 1, 2, 1]
    lt = run(ctx, R.sub_case(case, 3), R.TZ_EXACT)["level_table"]
    assert lt[0, :2].tolist() == [1, 1] and lt[1, :2].tolist() == [2, 1]
    four = run(ctx, R.sub_case(case, 4), R.TZ_EXACT)
    assert four["anchor_label"].tolist() == [1, 1] and four["deepest_level"].tolist() == [2]
    # one step past either threshold and the label / the holder is gone
    past = ctx.diag_eval(case["anchors"][4:], case["zoom"][4:], case["level"][4:], case["gt"][4:], case["props"][4:], R.TZ_EXACT,
                         float(np.nextafter(R.EMB_REG, 0.0)), R.EMB_OBJ)
    assert past["anchor_label"].tolist() == [0, 0] and past["deepest_level"].tolist() == [2]
    past = ctx.diag_eval(case["anchors"][4:], case["zoom"][4:], case["level"][4:], case["gt"][4:], case["props"][4:], R.TZ_EXACT,
                         R.EMB_REG, float(np.nextafter(R.EMB_OBJ, 1.0)))
    assert past["anchor_label"].tolist() == [0, 1] and past["deepest_level"].tolist() == [2]
    # the second anchor alone gone too: the object is held by the first only at exactly 0.5
    only_a = R.make_case([case["anchors"][4][:1]], [case["zoom"][4][:1]], [case["level"][4][:1]], case["gt"][4:], case["props"][4:])
    assert run(ctx, only_a, R.TZ_EXACT)["deepest_level"].tolist() == [1]


def test_levels(ctx):
    case, want = R.levels_case()
    got = run(ctx, case, 0.5)
    R.assert_same(got, R.diag_eval(case, 0.5), "levels")
    assert np.array_equal(got["deepest_level"], want)
    assert np.array_equal(got["level_table"][:, 0], np.ones(R.AZ_MAX_LEVELS))


def test_random_set(ctx):
    case = R.random_case()
    for tz, cuts in ((R.TZ_EXACT, R.CUTS), (0.7, (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 400, 401, 100000))):
        got = run(ctx, case, tz, cuts=cuts)
        R.assert_same(got, R.diag_eval(case, tz, cuts=cuts), "random tz=%g" % tz)
    assert got["recall_table"].shape == (17, 4)
    none = run(ctx, case, tz, cuts=())
    assert none["recall_table"].shape == (1, 4) and np.array_equal(none["recall_table"][0], got["recall_table"][-1])


def test_errors_leave_the_outputs_alone(ctx):
    from aznet_hip import ffi
    case = R.case_from_counts([(4, 2, 3), (3, 1, 2), (5, 2, 4)], 11)
    a, g, p = (np.vstack(case[k]) for k in ("anchors", "gt", "props"))
    z, lv = np.concatenate(case["zoom"]), np.concatenate(case["level"])
    aoff, goff, poff = np.array([0, 4, 7, 12]), np.array([0, 2, 3, 5]), np.array([0, 3, 5, 9])

    def call(expect, anc_off=aoff, gt_off=goff, prop_off=poff, level=lv, cuts=R.CUTS, counts=None):
        out = {"anchor_label": np.full(12, 7, np.uint8), "level_table": np.full((R.AZ_MAX_LEVELS, 4), -5, np.int64),
               "best_iou": np.full(5, -3.0), "best_rank": np.full(5, -9, np.int32), "first_hit": np.full(5, -9, np.int32),
               "deepest_level": np.full(5, -9, np.int32), "recall_table": np.full((17, 4), -5, np.int64)}
        keep = {k: v.copy() for k, v in out.items()}
        if expect is None:
            ctx.diag_eval_packed(a, z, level, anc_off, g, gt_off, p, prop_off, 0.5, R.EMB_REG, R.EMB_OBJ, 0.5, cuts, R.EDGES,
                                 counts=counts, out=out)
            return out
        with pytest.raises(ffi.AzError) as e:
            ctx.diag_eval_packed(a, z, level, anc_off, g, gt_off, p, prop_off, 0.5, R.EMB_REG, R.EMB_OBJ, 0.5, cuts, R.EDGES,
                                 counts=counts, out=out)
        assert e.value.code == expect, (e.value.code, expect)
        for k in out:
            assert np.array_equal(out[k], keep[k]), k

    INV, CAP = ffi.AZ_ERR_INVALID, ffi.AZ_ERR_CAPACITY
    call(INV, anc_off=np.array([0, 7, 4, 12]))                 # not non-decreasing
    call(INV, gt_off=np.array([0, 3, 2, 5]))
    call(INV, prop_off=np.array([0, 5, 3, 9]))
    call(INV, gt_off=np.array([0, -1, 3, 5]))                  # negative
    call(INV, anc_off=np.array([-1, 4, 7, 12]))
    call(INV, prop_off=np.array([0, 3, 5, 8]))                 # the last entry and the count disagree
    call(INV, counts=(13, 5, 9))
    call(INV, counts=(12, 4, 9))
    lbad = lv.copy(); lbad[5] = R.AZ_MAX_LEVELS
    call(INV, level=lbad)
    lbad[5] = -1
    call(INV, level=lbad)
    call(INV, cuts=(10, 50, 49))                               # unsorted budgets
    call(INV, cuts=tuple(range(1, 18)))                        # 17 budgets
    call(CAP, counts=(2 ** 31, 5, 9))                          # totals past int32
    call(CAP, counts=(12, 2 ** 31, 9))
    call(CAP, counts=(12, 5, 2 ** 32 + 9))
    # and the same arrays, well-formed, are answered
    ok = call(None)
    want = R.diag_eval(case, 0.5)
    for k in R.KEYS:
        n = want[k].shape[0]
        assert np.array_equal(ok[k][:n], want[k]), k
    assert (ok["recall_table"][len(R.CUTS) + 1:] == -5).all()


# ----------------------------------------------------------------------------------------------------------- front door
class _Backbone(object):
    """conv5_3 as a function of the image blob: a seeded map per distinct blob (four images of one shape get four maps)."""
    device = "cuda:0"

    def __init__(self):
        self.maps = {}

    def __call__(self, blob):
        import torch
        from aznet_hip import synth
        host = blob.detach().cpu().numpy() if hasattr(blob, "detach") else np.asarray(blob)
        key = tuple(host.shape[2:]) + (float(host.astype(np.float64).sum()),)
        if key not in self.maps:
            self.maps[key] = synth.make_feature_map(60 + len(self.maps), synth.SMALL_DIMS["C"], synth.conv_out_size(key[0]),
                                                    synth.conv_out_size(key[1]))
        return torch.from_numpy(self.maps[key]).to("cuda:0")


def test_front_door_test_proposals_and_diagnose(small, tmp_path):
    import scipy.io as sio
    from detect import tune as U
    from detect import diagnose as D
    from detect.config import cfg, cfg_set_mode, cfg_set_path
    import detect.config as C
    from datasets.factory import get_imdb
    net = small
    old_tz, old_np, old_root, old_max = cfg.SEAR.get("Tz", 0.0), cfg.SEAR.get("NUM_PROPOSALS", 300), cfg.ROOT_DIR, cfg.TEST.MAX_SIZE
    cfg_set_path("pytest_diag")
    cfg.ROOT_DIR = str(tmp_path)
    cfg.TEST.MAX_SIZE = 1000
    try:
        db = get_imdb("synthetic_375x500_4")
        net.backbone = _Backbone()
        nets = {"full": net, "fc": net}
        sink = io.StringIO()
        cfg_set_mode("Train")                                   # Tz = 0: every zoom score of the first image
        with redirect_stdout(sink):
            _, Bhis = U.im_propose(nets, db.image_at(0))
        tz = float(np.quantile(Bhis[:, 4], 0.6))
        cfg_set_mode("Test", tz)
        with redirect_stdout(sink):
            res = U.test_proposals(nets, db)
            alone = [U.im_propose(nets, db.image_at(i)) for i in range(4)]
        assert len(net.backbone.maps) == 4
        gt = db.gt_roidb()
        assert res["Tz"] == tz and res["num_proposals"] == cfg.TEST.NUM_PROPOSALS
        for i in range(4):
            assert np.array_equal(res["prop_boxes"][i], alone[i][0]) and np.array_equal(res["anchor_boxes"][i], alone[i][1])
            assert np.array_equal(res["gt_boxes"][i], gt[i]["boxes"]) and res["im_shapes"][i] == (375, 500, 3)
            assert res["fn"][i] == os.path.basename(db.image_path_at(i))
            assert int(res["level_regions"][i].sum()) == res["anchor_boxes"][i].shape[0] and res["level_regions"][i][0] == 1
        assert [l for l in sink.getvalue().splitlines() if l.startswith("im_prop: ")][-1].startswith("im_prop: 4/4 ")
        mat = sio.loadmat(os.path.join(C.get_output_dir(db, net), "AZ_results.mat"))
        assert sorted(k for k in mat if not k.startswith("__")) == sorted(U.AZ_RESULTS_KEYS)
        assert np.array_equal(mat["anchor_boxes"][0, 3], res["anchor_boxes"][3]) and mat["gt_boxes"][0, 0].dtype == np.uint16
        # the diagnosis of the set against the restatement on the same arrays
        levels = D.anchor_levels(res)
        case = R.make_case([b[:, :4] for b in res["anchor_boxes"]], [b[:, 4] for b in res["anchor_boxes"]], levels,
                           res["gt_boxes"], [b[:, :4] for b in res["prop_boxes"]])
        d = D.diagnose(res, db, ctx=net.ctx)
        R.assert_same(d, R.diag_eval(case, tz, emb_reg=cfg.SEAR.EMB_REG_THRESH, emb_obj=cfg.SEAR.EMB_OBJ_THRESH), "front door")
        assert d["level_table"][0].tolist()[:2] == [4, 4] and d["recall_table"][-1, 0] == sum(g["boxes"].shape[0] for g in gt)
        for i in range(4):
            one = D.diagnose({k: ([v[i]] if isinstance(v, list) else v) for k, v in res.items()}, ctx=net.ctx)
            assert one["level_table"][0, 0] == 1
        assert d["need_level"].shape == d["first_hit"].shape and len(D.summary_lines(d)) > 8
    finally:
        net.backbone = None
        cfg.ROOT_DIR, cfg.TEST.MAX_SIZE = old_root, old_max
        cfg.SEAR.Tz, cfg.SEAR.NUM_PROPOSALS = old_tz, old_np
        cfg_set_path(None)


def test_diagnose_prop_tool():
    """The command line in a fresh child process under its own time limit: the tables on stdout, both files on disk."""
    import scipy.io as sio
    tools = os.path.join(REPO, "az-net_amd", "tools")
    exp = "diagnose_prop_test_%d" % os.getpid()
    out_dir = os.path.join(REPO, "az-net_amd", "output", exp)
    try:
        out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(tools, "diagnose_prop.py"), "--net",
                              "synthetic", "--imdb", "synthetic_375x500_4", "--tz", "0.5", "--exp", exp],
                             capture_output=True, text=True)
        print(out.stdout[-3000:], out.stderr[-3000:])
        assert out.returncode == 0
        where = os.path.join(out_dir, "synthetic_375x500_4", "vgg16_az_net_synthetic_1234")
        for text in ("im_prop: 4/4", "Zoom indicator by search level", "Recall at IoU >= 0.5", "Missed objects"):
            assert text in out.stdout, text
        mat = sio.loadmat(os.path.join(where, "AZ_results.mat"))
        assert mat["prop_boxes"].shape == (1, 4) and float(mat["Tz"][0, 0]) == 0.5
        with open(os.path.join(where, "diagnosis.pkl"), "rb") as f:
            d = pickle.load(f)
        assert d["level_table"][0, 0] == 4 and d["num_images"] == 4 and d["Tz"] == 0.5
        assert d["level_table"][:, 0].sum() == sum(mat["anchor_boxes"][0, i].shape[0] for i in range(4))
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
