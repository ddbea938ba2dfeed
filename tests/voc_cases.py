"""Hand-made VOC evaluation cases shared by the host and GPU tests (not collected).
Each case: (name, gt per image [(box 1-based, difficult)], dets in file order [(image, conf, box)], expected)."""


def _sum11(vals):
    ap = 0.0
    for v in vals:
        ap = ap + v / 11
    return ap


SQ = [1.0, 1.0, 10.0, 10.0]

CASES = [
    ("duplicate", [[(SQ, 0)]], [(0, 0.9, SQ), (0, 0.8, SQ)],
     {"match": [1, -1], "npos": 1, "ap": _sum11([1.0] * 11), "ap_auc": 1.0}),
    ("difficult", [[(SQ, 1), ([50.0, 50.0, 60.0, 60.0], 0)]], [(0, 0.9, SQ), (0, 0.8, [50.0, 50.0, 60.0, 60.0])],
     {"match": [0, 1], "npos": 1, "ap": _sum11([1.0] * 11), "ap_auc": 1.0}),
    ("iou_exactly_half", [[(SQ, 0)]], [(0, 0.9, [1.0, 1.0, 10.0, 5.0])],
     {"match": [1], "npos": 1, "ap": _sum11([1.0] * 11), "ap_auc": 1.0}),
    ("iou_tie_first_box", [[(SQ, 0), (SQ, 0)]], [(0, 0.9, SQ), (0, 0.8, SQ)],
     {"match": [1, -1], "npos": 2, "ap": _sum11([1.0] * 6 + [0.0] * 5), "ap_auc": 0.5}),
    ("tie_across_images", [[], [(SQ, 0)]], [(0, 0.5, SQ), (1, 0.5, SQ)],
     {"match": [-1, 1], "npos": 1, "ap": _sum11([0.5] * 11), "ap_auc": 0.5}),
    ("tie_within_image", [[(SQ, 0)]], [(0, 0.5, [100.0, 100.0, 110.0, 110.0]), (0, 0.5, SQ)],
     {"match": [-1, 1], "npos": 1, "ap": _sum11([0.5] * 11), "ap_auc": 0.5}),
    # recall exactly 3/5: 0:0.1:1's t6 is 0.6 (NumPy's arange gives 0.6000000000000001 and would drop it)
    ("recall_0.6", [[([10.0 * k + 1, 1.0, 10.0 * k + 9, 9.0], 0) for k in range(5)]],
     [(0, 0.9 - 0.1 * k, [10.0 * k + 1, 1.0, 10.0 * k + 9, 9.0]) for k in range(3)],
     {"match": [1, 1, 1], "npos": 5, "ap": _sum11([1.0] * 7 + [0.0] * 4), "ap_auc": 0.6}),
    # recall exactly 7/10: t7 = 1 - 0.30000000000000004 = 0.7
    ("recall_0.7", [[([10.0 * k + 1, 1.0, 10.0 * k + 9, 9.0], 0) for k in range(10)]],
     [(0, 0.9 - 0.05 * k, [10.0 * k + 1, 1.0, 10.0 * k + 9, 9.0]) for k in range(7)],
     {"match": [1] * 7, "npos": 10, "ap": _sum11([1.0] * 8 + [0.0] * 3), "ap_auc": 0.7}),
    ("npos_zero", [[(SQ, 1)]], [(0, 0.9, [100.0, 100.0, 110.0, 110.0])],
     {"match": [-1], "npos": 0, "ap": 0.0, "ap_auc": float("nan")}),
    ("no_detections", [[(SQ, 0)]], [],
     {"match": [], "npos": 1, "ap": 0.0, "ap_auc": 0.0}),
]
