"""Frozen planted trees for the tuner's anchor history (capHis = 2 * max_regions rows on a context of 64 regions): image
shape, scale, planted cells of the zoom channel as row runs (row, first column, one past the last), and the populations
of the TUNER's loop at Tz = 0.5 that tests/test_tune_edges_host.py recomputes (tune_edges_ref.tuner_populations).  Found
by a seeded walk of single-cell toggles from the empty 38 x 50 mask towards a history of 128 rows with every level within
64 regions and 256 children; `past` is the single-cell toggle of `at` with the smallest history above 128."""

CASES = {
    "his_at": dict(H=375, W=500, scale=1.6, note="history exactly at capHis = 128: the search is right",
                   P=[1, 5, 10, 24, 38, 50], PZ=[1, 2, 5, 8, 12, 19], CH=[5, 10, 25, 40, 60], his=128,
                   runs=[(0, 16, 17), (3, 0, 1), (9, 11, 12), (11, 7, 8), (12, 8, 9), (37, 43, 44)]),
    "his_past": dict(H=375, W=500, scale=1.6, note="his_at with one more planted cell: 129 rows, err bit 16",
                     P=[1, 5, 10, 24, 38, 51], PZ=[1, 2, 5, 8, 13, 22], CH=[5, 10, 25, 40, 65], his=129,
                     runs=[(0, 16, 17), (3, 0, 1), (9, 11, 12), (10, 11, 12), (11, 7, 8), (12, 8, 9), (37, 43, 44)]),
}
