"""CPU: the VOC results writer against the reference's own (g17), the XML reader, the NumPy restatement of
VOCevaldet / xVOCap on hand cases, and voc_eval.m's print format."""
import math
import os

import numpy as np
import pytest

from voc_cases import CASES
import voc_eval_ref as R


def _devkit(tmp, image_index, year="2007", image_set="test"):
    d = os.path.join(str(tmp), "VOCdevkit" + year)
    m = os.path.join(d, "VOC" + year, "ImageSets", "Main")
    os.makedirs(m)
    open(os.path.join(m, image_set + ".txt"), "w").write("\n".join(image_index) + "\n")
    os.makedirs(os.path.join(d, "VOC" + year, "Annotations"))
    return d


def _g17_boxes(z, n_classes, n_images):
    out = []
    for j in range(n_classes):
        out.append([z["boxes_%d_%d" % (j, i)] if int(z["kind_%d_%d" % (j, i)]) else [] for i in range(n_images)])
    return out


def test_results_writer_matches_the_reference_bytes(golden_dir, tmp_path, capsys):
    from datasets.pascal_voc import pascal_voc
    z = np.load(os.path.join(golden_dir, "g17_voc_results.npz"))
    index = [str(s) for s in z["image_index"]]
    d = pascal_voc("test", "2007", _devkit(tmp_path, index))
    assert list(d.classes) == [str(s) for s in z["classes"]]
    all_boxes = _g17_boxes(z, d.num_classes, len(index))
    d.competition_mode(True)
    comp = d._write_voc_results_file(all_boxes)
    assert comp == "comp4"
    res = os.path.join(d._devkit_path, "results", "VOC2007", "Main")
    names = sorted(os.listdir(res))
    assert names == [str(s) for s in z["names"]]
    for k, n in enumerate(names):
        assert open(os.path.join(res, n), "rb").read() == bytes(z["body_%d" % k]), n
    out = capsys.readouterr().out
    assert out.splitlines()[0] == "Writing aeroplane VOC results file" and len(out.splitlines()) == 20
    # salted names carry the pid, as the reference's do
    d.competition_mode(False)
    comp = d._write_voc_results_file(all_boxes)
    assert comp == "comp4-%d" % os.getpid()
    assert os.path.exists(os.path.join(res, str(z["salted"]).replace("{pid}", str(os.getpid()))))
    assert d.config == {"cleanup": True, "use_salt": True}
    d.competition_mode(True)
    assert d.config == {"cleanup": False, "use_salt": False}


def test_results_reader_round_trip(tmp_path):
    from datasets import voc_eval
    p = tmp_path / "r.txt"
    p.write_text("000005 0.500 1.0 2.0 3.5 4.0\n000001 0.125 10.1 20.0 30.0 40.0\n000005 -0.000 1.0 1.0 1.0 1.0\n")
    img, conf, box = voc_eval.read_results_file(str(p), ["000001", "000005"])
    assert img.tolist() == [1, 0, 1]
    assert conf.tolist() == [0.5, 0.125, 0.0]
    assert box.tolist() == [[1.0, 2.0, 3.5, 4.0], [10.1, 20.0, 30.0, 40.0], [1.0, 1.0, 1.0, 1.0]]
    p.write_text("")
    img, conf, box = voc_eval.read_results_file(str(p), ["000001"])
    assert img.size == 0 and box.shape == (0, 4)
    p.write_text("000009 0.5 1 1 2 2\n")
    with pytest.raises(ValueError, match="unrecognized image"):
        voc_eval.read_results_file(str(p), ["000001"])


def test_xml_reader_difficult_and_missing_tag(tmp_path):
    from datasets import voc_eval
    x = tmp_path / "a.xml"
    x.write_text("<annotation><object><name>dog</name><difficult>1</difficult><bndbox><xmin>5</xmin><ymin>6</ymin>"
                 "<xmax>50</xmax><ymax>60</ymax></bndbox></object><object><name> cat </name><bndbox><xmin>1</xmin>"
                 "<ymin>2</ymin><xmax>3</xmax><ymax>4</ymax></bndbox></object></annotation>")
    assert voc_eval.read_record(str(x)) == [("dog", [5.0, 6.0, 50.0, 60.0], 1), ("cat", [1.0, 2.0, 3.0, 4.0], 0)]
    gb, gd, goff = voc_eval.gt_segments(["cat", "dog"], [voc_eval.read_record(str(x))])
    assert goff.tolist() == [0, 1, 2] and gd.tolist() == [0, 1] and gb[1].tolist() == [5.0, 6.0, 50.0, 60.0]


def _run_case(gts, dets, metric_07=True):
    gb = [np.array([g[0] for g in im], np.float64).reshape(-1, 4) for im in gts]
    gd = [np.array([g[1] for g in im], bool) for im in gts]
    img = np.array([d[0] for d in dets], np.int64)
    conf = np.array([d[1] for d in dets], np.float64)
    box = np.array([d[2] for d in dets], np.float64).reshape(-1, 4)
    return R.evaldet(img, conf, box, gb, gd, 0.5, metric_07)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_hand_cases(case):
    name, gts, dets, want = case
    r = _run_case(gts, dets)
    assert r["match"].tolist() == want["match"]
    assert r["npos"] == want["npos"]
    assert r["ap"] == want["ap"]
    if math.isnan(want["ap_auc"]):
        assert math.isnan(r["ap_auc"])
    else:
        assert r["ap_auc"] == pytest.approx(want["ap_auc"], rel=1e-15)


def test_colon_thresholds_are_matlabs():
    t = R.colon_thresholds()
    assert t[6] == 0.6 and t[7] == 1 - 0.30000000000000004 and t[7] == 0.7
    ar = np.arange(0, 1.1, 0.1)
    assert ar[6] > 0.6 and ar[7] > 0.7                  # the convention the restatement must not use
    assert t[3] == 3 * 0.1 and t[5] == 0.5 and t[10] == 1.0


def test_print_format_is_voc_eval_m():
    from datasets import voc_eval
    lines, tail = voc_eval.report(["a", "b"], np.array([0.5, float("nan")]), np.array([0.25, float("nan")]))
    assert lines == ["!!! a : 0.5000 0.2500", "!!! b : NaN NaN"]
    assert tail == ["", "~~~~~~~~~~~~~~~~~~~~", "Results:", "50.0", "NaN", "NaN", "~~~~~~~~~~~~~~~~~~~~"]
    lines, tail = voc_eval.report(["a", "b"], np.array([0.5, 0.25]), np.array([0.0, 0.0]))
    assert tail[3:6] == ["50.0", "25.0", "37.5"]


def test_2012_test_set_is_not_evaluated(tmp_path, capsys):
    """voc_eval.m's do_eval is false for VOC2012 test: 0.0000 0.0000 per class, empty curves, no device call."""
    import scipy.io as sio
    from datasets.pascal_voc import pascal_voc
    d = pascal_voc("test", "2012", _devkit(tmp_path, ["a", "b"], year="2012"))
    all_boxes = [[[] for _ in range(2)] for _ in range(d.num_classes)]
    all_boxes[1][0] = np.array([[1, 1, 5, 5, 0.9]], np.float32)
    out_dir = str(tmp_path / "out")
    aps, aucs = d.evaluate_detections(all_boxes, out_dir, ctx=object())
    out = capsys.readouterr().out
    assert "!!! aeroplane : 0.0000 0.0000" in out and "!!! tvmonitor : 0.0000 0.0000" in out
    m = sio.loadmat(os.path.join(out_dir, "aeroplane_pr.mat"))
    assert m["recall"].size == 0 and float(m["ap"].ravel()[0]) == 0.0
    assert not os.listdir(os.path.join(d._devkit_path, "results", "VOC2012", "Main"))     # cleanup
