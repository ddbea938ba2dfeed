"""GPU: the launch sequence of one head pass in every form an fc layer is stored in -- full rank on the fp32 GEMM, a truncated
SVD (L stage, linear slab sum, U stage), the 16-bit-term modes -- for the AZ head (az_head_forward) and the detection head
(az_det_forward), as az_last_kernel_times names it under profiling mode 2; and the hand-over of int6 to the second lane.
The stage lists are written out here: bench.py and the tools' perf scripts key on these names."""
import numpy as np
import pytest

import head_sizes_ref as H
import lowrank_ref as LR

pytestmark = pytest.mark.gpu

AZ_FULL = ["roi_pool", "fc6_gemm", "fc6_reduce", "fc7_gemm", "tail"]
AZ_LOW = ["roi_pool", "fc6_L", "fc6_L_reduce", "fc6_U", "fc7_gemm", "tail"]
DET6 = {False: ["det_fc6_gemm", "det_fc6_reduce"], True: ["det_fc6_L", "det_fc6_L_reduce", "det_fc6_U"]}
DET7 = {False: ["det_fc7_gemm", "det_fc7_reduce"], True: ["det_fc7_L", "det_fc7_L_reduce", "det_fc7_U"]}


def det_stages(low6, low7):
    return ["det_roi_pool"] + DET6[low6] + DET7[low7] + ["det_tail_gemm", "det_epilogue"]


@pytest.fixture(scope="module")
def world():
    from aznet_hip import synth

    class World(object):
        pass

    w = World()
    w.fmap = synth.make_feature_map(11, synth.SMALL_DIMS["C"], 38, 63)
    w.rois = H.rois300()[:48]
    w.az = synth.make_head(seed=77, **synth.SMALL_DIMS)
    w.az_low = {k: v for k, v in w.az.items() if k != "W6"}
    w.az_low["L6"], w.az_low["U6"] = LR.compress_layer(w.az["W6"], 36)
    w.det = synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS)
    w.L6, w.U6 = LR.compress_layer(w.det["W6"], 36)
    w.L7, w.U7 = LR.compress_layer(w.det["W7"], 20)
    return w


def det_head(w, low6, low7):
    head = dict(w.det)
    if low6:
        del head["W6"]
        head["L6"], head["U6"] = w.L6, w.U6
    if low7:
        del head["W7"]
        head["L7"], head["U7"] = w.L7, w.U7
    return head


def stages(ctx, forward, rois):
    ctx.set_profiling(2)
    try:
        forward(rois)
        return [n for n, _, _ in ctx.last_kernel_times()]
    finally:
        ctx.set_profiling(0)


@pytest.mark.parametrize("tag,mode,want", [("full", 0, AZ_FULL), ("rank36", 0, AZ_LOW), ("mode2", 2, AZ_FULL), ("mode3", 3, AZ_FULL)])
def test_az_head_pass_launch_sequence(world, tag, mode, want):
    from aznet_hip import ffi
    ctx = ffi.AzContext(0, max_regions=512, gemm_mode=mode)
    try:
        ctx.load_head(world.az_low if tag == "rank36" else world.az)
        ctx.set_feature_map(world.fmap)
        assert stages(ctx, ctx.head_forward, world.rois) == want
    finally:
        ctx.close()


@pytest.mark.parametrize("low6,low7", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["full", "fc6_r36", "fc7_r20", "both"])
def test_detection_head_pass_launch_sequence(world, low6, low7):
    from aznet_hip import ffi
    ctx = ffi.AzContext(0, max_regions=512, gemm_mode=0)
    try:
        ctx.load_head(world.az)                   # (set_feature_map takes the map's channel count from the AZ head)
        ctx.load_det_head(det_head(world, low6, low7))
        ctx.set_feature_map(world.fmap)
        assert stages(ctx, ctx.det_forward, world.rois) == det_stages(low6, low7)
    finally:
        ctx.close()


def test_detection_head_pass_launch_sequence_with_term_planes_on_fc6(world):
    """gemm mode 3 with an AZ head loaded: fc6 of the full-rank detection head takes the 16-bit-term GEMM, under the same names."""
    from aznet_hip import ffi
    ctx = ffi.AzContext(0, max_regions=512, gemm_mode=3)
    try:
        ctx.load_head(world.az)
        ctx.load_det_head(world.det)
        ctx.set_feature_map(world.fmap)
        assert stages(ctx, ctx.det_forward, world.rois) == det_stages(False, False)
        assert stages(ctx, ctx.head_forward, world.rois) == AZ_FULL
    finally:
        ctx.close()


@pytest.mark.parametrize("tag,mode", [("rank36", 0), ("mode3", 3)])
def test_the_second_lane_reads_the_first_lanes_int6(world, tag, mode):
    """After set_lanes(2) two consecutive searches of one map -- the second runs on the twin, which took int6 from the
    context -- give the boxes and scores of one lane."""
    from aznet_hip import ffi
    from aznet_hip.net import HipAZNet
    net = HipAZNet(world.az_low if tag == "rank36" else world.az, name="fc_lane_" + tag, gemm_mode=mode)
    try:
        p = ffi.AzContext.make_params(600, 1000, 1.0, 0.2, static_tree=False)
        net.set_conv(world.fmap)
        Y, S = net.propose(p, want_scores=True)
        net.ctx.set_lanes(2)
        for turn in range(2):
            net.ctx.propose_launch(p)
            Y2, S2 = net.ctx.propose_fetch(want_scores=True)
            assert np.array_equal(Y2, Y) and np.array_equal(S2, S), (tag, turn)
    finally:
        net.ctx.close()
