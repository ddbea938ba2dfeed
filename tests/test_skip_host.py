"""CPU: the host side of the skip-connection detector -- the NumPy restatement against the oracle's RoIPool, the
conv_pool5 reader, the skip configuration, the refusals of detect.test, the backbone's taps and the tools' loaders."""
import copy
import os
import re
import sys

import numpy as np
import pytest

import skip_ref as S
import train_step_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
SKIP_YML = os.path.join(REPO, "tests", "golden", "voc_skip.yml")


@pytest.fixture
def cfg():
    from detect import config as C
    saved = copy.deepcopy(dict(C.cfg))
    yield C.cfg
    S.restore_tree(C.cfg, saved)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_ref_pools_like_the_oracle_at_one_sixteenth():
    from oracle import az_oracle as orc
    rois = np.concatenate([S.hostile_rois(), S.random_rois(60)], 0)
    for C in (12, 36):
        fmap = S.make_maps(3, (C, C, C))[2]
        want = orc.roi_pool(fmap[0], rois).reshape(rois.shape[0], C, 49).transpose(0, 2, 1)
        assert np.array_equal(S.roi_pool(fmap, rois, 0.0625), want)
    # the hostile set at the other two scales: nothing outside the map is read, empty bins give 0
    maps = S.make_maps(4, S.SMALL_CS)
    cat = S.cat_raw(maps, rois)
    assert cat.shape == (rois.shape[0] * 49, sum(S.SMALL_CS)) and np.isfinite(cat).all() and (cat >= 0).all()
    assert not cat[:2 * 49].any()                                      # the two rois outside the map
    whole = cat[5 * 49:6 * 49]                                         # the whole-map roi: its 49 bins tile every map
    for (lo, hi), m in zip(((0, 20), (20, 56), (56, 68)), maps):
        assert np.array_equal(whole[:, lo:hi].max(axis=0), m[0].reshape(m.shape[1], -1).max(axis=1))


def test_ref_grn_and_conv():
    x = np.array([[3.0, 0.0, 4.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 2.5, 0.0, 0.0]])
    for dt in (np.float64, np.float32):
        y = S.grn(x, 1e-10, dt)
        assert y.dtype == dt and np.isfinite(y).all()
        np.testing.assert_allclose(y[0], [0.6, 0, 0.8, 0], rtol=1e-6)
        assert not y[1].any() and abs(y[2, 1] - 1.0) < 1e-6      # (eps: 1 - 8e-12 in float64)
    maps, rois = S.make_maps(5, S.SMALL_CS), S.random_rois(6)
    c64 = S.cat_norm(maps, rois)
    o = 0
    for C in S.SMALL_CS:                                               # every non-zero block has norm `gain`
        n = np.sqrt((c64[:, o:o + C] ** 2).sum(axis=1))
        assert np.all((np.abs(n - 1000.0) < 1e-6) | (n == 0))
        o += C
    from aznet_hip import synth
    front = synth.make_skip_front(seed=1, Cs=S.SMALL_CS, Cout=12)
    assert front["Wp"].shape == (12, 68) and front["scales"] == S.SCALES and front["names"] == S.NAMES
    p64, p32 = S.pool5(front, maps, rois, np.float64), S.pool5(front, maps, rois, np.float32)
    assert p64.shape == (6, 12 * 49) and 0.2 < (p64 > 0).mean() < 0.8
    assert R.rel_err(p32, p64) < 1e-5
    # Caffe's flattening: column c * 49 + p is output channel c of bin p
    y = S.conv1x1(c64, front["Wp"], front["bp"], np.float64)
    assert p64[2, 5 * 49 + 11] == y[2 * 49 + 11, 5]


# ---- the conv_pool5 reader --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v1", [False, True])
def test_caffemodel_round_trip_of_conv_pool5(tmp_path, v1):
    from aznet_hip import caffemodel as cm
    from aznet_hip import synth
    front = synth.make_skip_front(seed=5, Cs=(256, 512, 512), Cout=512)
    dhead = synth.make_det_head(seed=6, C=4, n6=8, n7=8, ncls=3)
    layers = {"conv1_1": [np.ones((4, 3, 3, 3), np.float32), np.zeros(4, np.float32)],
              "conv_pool5": [front["Wp"].reshape(512, 1280, 1, 1), front["bp"]],
              "fc6": [dhead["W6"], dhead["b6"]], "fc7": [dhead["W7"], dhead["b7"]],
              "cls_score": [dhead["Wc"], dhead["bc"]], "bbox_pred": [dhead["Wb"], dhead["bb"]]}
    path = str(tmp_path / "skip.caffemodel")
    cm.write_caffemodel(path, layers, v1=v1)
    back = cm.load_caffemodel(path)
    assert back["conv_pool5"][0].shape == (512, 1280, 1, 1)
    got = cm.skip_front_from_layers(back)
    assert np.array_equal(got["Wp"], front["Wp"]) and np.array_equal(got["bp"], front["bp"])
    assert got["Wp"].shape == (512, 1280) and got["Cs"] == (256, 512, 512) and got["scales"] == (0.25, 0.125, 0.0625)
    assert got["names"] == ("conv3_3", "conv4_3", "conv5_3") and got["gain"] == 1000.0 and got["eps"] == 1e-10
    assert "conv_pool5" not in cm.backbone_from_layers(back) and "conv1_1" in cm.backbone_from_layers(back)
    head = cm.det_head_from_layers(back)
    assert sorted(head) == sorted(list(dhead) + ["skip_front"]) and np.array_equal(head["skip_front"]["Wp"], front["Wp"])
    for k, v in dhead.items():
        assert np.array_equal(head[k], v), k
    # the plain Fast R-CNN net has no such layer
    del layers["conv_pool5"]
    cm.write_caffemodel(path, layers, v1=v1)
    assert cm.skip_front_from_layers(cm.load_caffemodel(path)) is None
    assert sorted(cm.det_head_from_layers(cm.load_caffemodel(path))) == sorted(dhead)
    # a layer of another shape is refused, not reshaped
    with pytest.raises(ValueError):
        cm.skip_front_from_layers({"conv_pool5": [np.zeros((512, 1024, 1, 1), np.float32), np.zeros(512, np.float32)]})
    with pytest.raises(ValueError):
        cm.skip_front_from_layers({"conv_pool5": [np.zeros((64, 1280, 3, 3), np.float32), np.zeros(64 * 9, np.float32)]})
    with pytest.raises(ValueError):
        cm.skip_front_from_layers({"conv_pool5": [np.zeros((512, 1280, 1, 1), np.float32)]})


def test_tools_find_the_front(tmp_path):
    """A reduced skip model as a .caffemodel: the two detection tools' own loaders hand its front on with the head (the
    channel counts come from the file's conv layers)."""
    from aznet_hip import caffemodel as cm
    path = str(tmp_path / "skip16.caffemodel")
    sys.path[:0] = [TOOLS]
    try:
        import test_shared
        layers = S.skip_model_layers(seed=7, width_div=16, n6=8, n7=12, num_classes=3)
        cm.write_caffemodel(path, layers)
        head, name = test_shared.load_det_head(path)
    finally:
        sys.path.remove(TOOLS)
    front = head["skip_front"]
    assert name == "skip16" and front["Cs"] == (16, 32, 32) and front["names"] == S.NAMES and front["scales"] == S.SCALES
    assert np.array_equal(front["Wp"], layers["conv_pool5"][0].reshape(32, 80)) and np.array_equal(front["bp"], layers["conv_pool5"][1])
    assert head["W6"].shape == (8, 32 * 49) and head["Wc"].shape == (3, 12)
    bb = cm.backbone_from_layers(cm.load_caffemodel(path))
    assert len(bb) == 13 and bb["conv3_3"][0].shape[0] == 16 and "conv_pool5" not in bb


# ---- the configuration ------------------------------------------------------------------------------------------------------------
def test_cfg_from_the_skip_settings(cfg):
    from detect import config as C
    from detect import test as T
    assert list(cfg.SEAR.FRCNN_CONV) == ["conv5_3"] and not T._skip_mode()
    C.cfg_from_file(SKIP_YML)
    assert list(cfg.SEAR.FRCNN_CONV) == ["conv3_3", "conv4_3", "conv5_3"] and list(cfg.SEAR.AZ_CONV) == ["conv5_3"]
    assert cfg.DEDUP_BOXES == 0.5 and cfg.SEAR.BATCH_SIZE == 1000 and cfg.TEST.MAX_SIZE == 800
    assert cfg.SEAR.FIXED_PROPOSAL_NUM is True
    assert T._skip_mode()


class _FakeNet(object):
    """What detect.test looks at before it touches a GPU."""
    num_classes = 21

    def __init__(self, names=None, name="fake"):
        self.name = name
        self.skip_front = None if names is None else {"Cs": (4,) * len(names)}
        self.skip_names = names


def test_mismatched_net_and_configuration_are_value_errors(cfg, capsys, monkeypatch):
    from detect import config as C
    from detect import test as T
    im, boxes = np.zeros((96, 128, 3), np.uint8), np.array([[1.0, 2.0, 30.0, 40.0]])
    plain, skipn = _FakeNet(), _FakeNet(S.NAMES)
    # a net with a front under the plain configuration: shared ('fc') and full nets alike
    for net in ({"fc": skipn}, {"full": skipn}):
        with pytest.raises(ValueError, match="skip front"):
            T._frcnn_forward(net, im, boxes, 21, conv=None)
    C.cfg_from_file(SKIP_YML)
    # the skip configuration with a net that has no front: never on conv5_3 alone
    for net in ({"fc": plain}, {"full": plain}):
        with pytest.raises(ValueError, match="no skip front"):
            T._frcnn_forward(net, im, boxes, 21, conv={n: None for n in S.NAMES})
    with pytest.raises(ValueError, match="no skip front"):
        T.im_detect({"full": plain}, im, boxes, 21)
    # a front over other maps than the configuration names
    with pytest.raises(ValueError, match="reads"):
        T._skip_mode(_FakeNet(("conv4_3", "conv5_3")))
    assert T._skip_mode(skipn) is True
    # the maps the backbone returned must cover the names
    with pytest.raises(ValueError, match="also names"):
        T._conv_dict({"conv5_3": 1, "conv4_3": 2})
    assert T._conv_dict({"conv3_3": 3, "conv5_3": 1, "conv4_3": 2, "x": 0}) == {"conv3_3": 3, "conv4_3": 2, "conv5_3": 1}
    # several test scales with skip
    cfg.TEST.SCALES = (480, 600)
    with pytest.raises(ValueError, match="one test scale"):
        T._skip_mode(skipn)
    with pytest.raises(ValueError, match="one test scale"):
        T._frcnn_forward({"full": skipn}, im, boxes, 21)
    cfg.TEST.SCALES = (600,)
    # cfg.TEST.BATCH_IMAGES > 1: one line under AZ_FULL_DEBUG, none without
    cfg.TEST.BATCH_IMAGES = 4
    monkeypatch.delenv("AZ_FULL_DEBUG", raising=False)
    T._skip_note("test_net")
    assert capsys.readouterr().out == ""
    monkeypatch.setenv("AZ_FULL_DEBUG", "1")
    T._skip_note("test_net")
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1 and "image by image" in out[0] and "test_net" in out[0]
    cfg.TEST.BATCH_IMAGES = 1
    T._skip_note("test_net")
    assert capsys.readouterr().out == ""


class _FakeSynthetic(_FakeNet):
    class ctx(object):
        det_dims = {"C": 512}

    def attach_skip_front(self, front):
        self.skip_front, self.skip_names = front, tuple(front["names"])


def test_the_tools_synthetic_nets_get_a_synthetic_front(cfg):
    """tools/test_det_net.py and tools/test_shared.py name their `--net synthetic:<seed>` nets vgg16_frcnn_synthetic_<seed>:
    under a skip configuration such a net gets the seeded front; a net of any other name never does."""
    from aznet_hip import synth
    from detect import config as C
    from detect import test as T
    syn, real = _FakeSynthetic(name="vgg16_frcnn_synthetic_7"), _FakeSynthetic(name="VGG16_frcnn_iter_80000")
    T._synthetic_skip_front(syn)
    assert syn.skip_front is None                                       # the plain configuration: nothing happens
    C.cfg_from_file(SKIP_YML)
    T._synthetic_skip_front(syn)
    T._synthetic_skip_front(real)
    want = synth.make_skip_front(seed=9)
    assert syn.skip_names == S.NAMES and np.array_equal(syn.skip_front["Wp"], want["Wp"]) and T._skip_mode(syn)
    assert real.skip_front is None
    with pytest.raises(ValueError, match="no skip front"):
        T._skip_mode(real)
    front = syn.skip_front
    T._synthetic_skip_front(syn)
    assert syn.skip_front is front                                      # once


def test_nets_refuse_before_the_gpu():
    from aznet_hip import net as N
    with pytest.raises(ValueError):
        N._skip_names({"Cs": (4, 4), "names": ("conv5_3",)})
    assert N._skip_names({"Cs": (4, 4)}) == ("conv4_3", "conv5_3")
    assert N._skip_names({"Cs": (4, 4, 4), "names": None}) == S.NAMES


# ---- the backbone's taps ----------------------------------------------------------------------------------------------------------
def test_backbone_taps_on_the_cpu():
    import torch
    import torch.nn.functional as F
    from aznet_hip.backbone import VGG16Conv5
    bk = VGG16Conv5(device="cpu", seed=3, width_div=16)
    blob = torch.randn(1, 3, 100, 130, generator=torch.Generator().manual_seed(1))
    # what forward(blob) computed before it knew of taps: the plain layer stack
    x, plain = blob, {}
    for layer in bk.layers:
        if layer is None:
            x = F.max_pool2d(x, kernel_size=2, stride=2, ceil_mode=True)
            continue
        x = F.relu(F.conv2d(x, layer[1], layer[2], padding=1))
        plain[layer[0]] = x
    whole = bk.forward(blob)
    assert torch.equal(whole, plain["conv5_3"]) and whole.is_contiguous() and torch.equal(bk(blob), whole)
    assert torch.equal(bk.forward(blob, taps=None), whole) and torch.equal(bk.forward(blob, taps=()), whole)
    out = bk(blob, taps=("conv3_3", "conv4_3"))
    assert list(out) == ["conv3_3", "conv4_3", "conv5_3"]
    # ceil-mode sizes of a 100 x 130 blob: 50 x 65, 25 x 33, 13 x 17, 7 x 9
    assert tuple(out["conv3_3"].shape) == (1, 16, 25, 33)
    assert tuple(out["conv4_3"].shape) == (1, 32, 13, 17)
    assert tuple(out["conv5_3"].shape) == (1, 32, 7, 9)
    for name, t in out.items():
        assert torch.equal(t, plain[name]), name
        assert t.permute(0, 2, 3, 1).is_contiguous(), name                # [H][W][C] in memory: what RoIPool reads
    assert torch.equal(bk.forward(blob), whole)                             # (the taps left nothing behind)
    only4 = bk.forward(blob, taps=("conv4_3",))
    assert list(only4) == ["conv4_3", "conv5_3"] and torch.equal(only4["conv4_3"], plain["conv4_3"])
    with pytest.raises(ValueError):
        bk.forward(blob, taps=("conv6_1",))


# ---- the binding --------------------------------------------------------------------------------------------------------------------
def test_binding_restates_the_header():
    from aznet_hip import ffi
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    assert int(re.search(r"#define\s+AZ_SKIP_CHUNK\s+(\d+)", src).group(1)) == ffi.AZ_SKIP_CHUNK
    assert int(re.search(r"#define\s+AZ_SKIP_MAX_SRC\s+(\d+)", src).group(1)) == ffi.AZ_SKIP_MAX_SRC
    for name in ("az_load_skip_front", "az_set_skip_maps_dev_nhwc", "az_detect_skip", "az_det_forward_skip", "az_skip_pool",
                 "az_skip_conv"):
        assert name in ffi.SYMBOLS and ("int %s(" % name) in src
    for m in ("load_skip_front", "set_skip_maps", "detect_skip", "det_forward_skip", "skip_pool", "skip_conv"):
        assert callable(getattr(ffi.AzContext, m))
