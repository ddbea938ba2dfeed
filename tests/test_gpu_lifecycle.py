"""GPU: a context taken through everything that allocates -- head, geometry buffers, plans and pre-pass entries, stage
streams, the second lane, a lockstep batch, the detection head, the skip front, NMS / tuner / overlap scratch, the upload
ring, a trainer, a second head of other layer sizes -- four times over, each time from az_create to az_destroy.
(A fifth cycle runs first and is not measured: the HIP runtime itself takes 216 MiB more, once, during the second cycle
a process runs -- free memory after cycles 1 to 4 of a run without it, on the MI355X: 308096794624, 307870302208,
307870302208, 307870302208 B -- which is no leak of the library's: the figure does not move again.)

  * every answer of cycle 4 equals cycle 1's bit for bit (the same code on the same input: no tolerance), and the search
    after the second load_head equals a fresh context's with that head and map;
  * device memory in use after cycle 4 has not grown over cycle 1's end by as much as the smaller of pool5 and h6
    (16.8 MB at these dims): one head-sized buffer leaked per cycle would show three times over.

What is smaller than that -- an event, a pinned block, a few KB of scratch -- cannot be seen in the device's free memory;
the exactly-once release of every kind of handle is what tests/test_res_host.py checks on a counting fake of the runtime."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = dict(C=64, n6=2048, n71=256, n72=64)
DIMS2 = dict(C=64, n6=1024, n71=128, n72=32)          # the second head: other layer sizes, the same maps
R = 2048
H, W, MH, MW = 600, 1000, 38, 63
SKIP_CS = (16, 32, 64)
SKIP_HW = ((150, 250), (75, 125), (MH, MW))


@pytest.fixture(scope="module")
def data():
    import torch
    from aznet_hip import ffi, synth
    rng = np.random.RandomState(5)

    def boxes(n):
        x, y = rng.uniform(0, W - 40, n), rng.uniform(0, H - 40, n)
        return np.stack([x, y, x + rng.uniform(8, 300, n), y + rng.uniform(8, 300, n)], 1).clip(0, [W - 1, H - 1, W - 1, H - 1])

    d = dict(torch=torch, ffi=ffi, synth=synth)
    d["head"], d["head2"] = synth.make_head(seed=77, **DIMS), synth.make_head(seed=78, **DIMS2)
    d["det"] = synth.make_det_head(seed=9, C=DIMS["C"], n6=256, n7=128, ncls=21)
    d["front"] = synth.make_skip_front(seed=3, Cs=SKIP_CS, Cout=DIMS["C"])
    d["fmaps"] = [synth.make_scene_map(j, DIMS["C"], MH, MW) for j in range(3)]
    d["tmaps"] = [torch.from_numpy(f).cuda() for f in d["fmaps"]]
    d["cl"] = [t.contiguous(memory_format=torch.channels_last) for t in d["tmaps"]]          # ([1, C, H, W] maps)
    d["skip_maps"] = [torch.from_numpy(synth.make_scene_map(10 + i, c, h, w)).cuda() for i, (c, (h, w)) in enumerate(zip(SKIP_CS, SKIP_HW))]
    d["boxes"] = boxes(200)
    d["dets"] = np.concatenate([boxes(5000), rng.uniform(0, 1, (5000, 1))], 1).astype(np.float32)
    d["scores"] = rng.standard_normal(3000).astype(np.float32)
    d["images"] = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((120, 160), (375, 500))]
    # the fresh context the search after the second load_head is held against
    ctx = ffi.AzContext(0, max_regions=R)
    try:
        ctx.load_head(d["head2"])
        ctx.set_feature_map(d["fmaps"][1])
        d["fresh"] = ctx.propose(ffi.AzContext.make_params(H, W, 1.0, 0.5), want_scores=True)
    finally:
        ctx.close()
    return d


def _cycle(d):
    """One context from az_create to az_destroy; every answer by name."""
    torch, ffi = d["torch"], d["ffi"]
    P = ffi.AzContext.make_params
    out = {}

    def keep(name, *arrays):
        for i, a in enumerate(arrays):
            out["%s/%d" % (name, i)] = np.array(a)

    ctx = ffi.AzContext(0, max_regions=R)
    try:
        ctx.load_head(d["head"])
        ctx.set_feature_map(d["fmaps"][0])                      # (a host map: staging buffer and channel-last copies)
        keep("static", *ctx.propose(P(H, W, 1.0, 0.0), want_scores=True))
        keep("levels", *ctx.propose(P(H, W, 1.0, 0.5), want_scores=True))
        ctx.set_lanes(2)
        for t in d["tmaps"][1:]:
            ctx.propose_launch(P(H, W, 1.0, 0.5), t)
        for lane in range(2):
            keep("lane%d" % lane, *ctx.propose_fetch(want_scores=True))
        ctx.batch_launch(P(H, W, 1.0, 0.0), d["cl"])
        for i, r in enumerate(ctx.batch_fetch_all(want_scores=True)):
            keep("batch%d" % i, *r)
        ctx.set_lanes(1)
        ctx.load_det_head(d["det"])
        ctx.set_feature_map(d["fmaps"][0])
        keep("detect", *ctx.detect(d["boxes"], 1.0, H, W))
        ctx.load_skip_front(d["front"])
        ctx.set_skip_maps(d["skip_maps"])
        keep("detect_skip", *ctx.detect_skip(d["boxes"], 1.0, H, W))
        for j, n in enumerate((100, 3000, 100, 5000)):           # (small form, general form, small again, a regrow)
            keep("nms%d" % j, ctx.nms(d["dets"][:n], 0.5))
        keep("nms_batched", *ctx.nms_batched([d["dets"][i * 90:(i + 1) * 90] for i in range(20)], 0.3))
        for j, cap in enumerate((1000, 5000)):
            ctx.tune_begin(cap)
            ctx.tune_push(d["scores"][:cap - 200])
            keep("tune%d" % j, ctx.tune_kth_largest(40))
        keep("overlaps0", ctx.bbox_overlaps(d["boxes"][:10], d["boxes"][10:20]))
        keep("overlaps1", ctx.bbox_overlaps(d["dets"][:2000, :4], d["boxes"][:50]))
        for j, im in enumerate(d["images"]):
            keep("blob%d" % j, ctx.image_blob(im, (102.98, 115.95, 122.77), 1.5))
            oh, ow = ctx.image_blob_size(im.shape[0], im.shape[1], 1.5)
            dev = torch.empty((1, 3, oh, ow), dtype=torch.float32, device="cuda")
            ctx.image_blob(im, (102.98, 115.95, 122.77), 1.5, out=dev, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            keep("blob_dev%d" % j, dev.cpu().numpy())
        ffi.AzDetSolver(ctx, DIMS["C"], 64, 32, 21, max_rois=8, seed=1).close()
        ctx.load_head(d["head2"])                               # (drops the lanes, the batch slots and the spare set)
        ctx.set_feature_map(d["fmaps"][1])
        keep("reloaded", *ctx.propose(P(H, W, 1.0, 0.5), want_scores=True))
    finally:
        ctx.close()
    torch.cuda.synchronize()
    return out


def test_four_lifecycles_answer_alike_and_give_their_memory_back(data):
    torch = data["torch"]
    K6, n6 = DIMS["C"] * 49, DIMS["n6"]
    bound = min(4 * R * K6, 4 * R * n6)                          # the smaller of pool5 and h6, in bytes
    warm = _cycle(data)
    first = _cycle(data)
    free1 = torch.cuda.mem_get_info()[0]
    for name, want in zip(("reloaded/0", "reloaded/1"), data["fresh"]):
        assert np.array_equal(first[name], want), name
    last, free = first, [free1]
    for _ in range(3):
        last = _cycle(data)
        free.append(torch.cuda.mem_get_info()[0])
    grown = free1 - min(free)
    print("answers per cycle: %d; free device memory after each cycle: %s; in use grew by at most %d B over three cycles (bound %d B)"
          % (len(first), free, grown, bound))
    assert sorted(first) == sorted(last) == sorted(warm)
    for name in sorted(first):
        for other in (last, warm):
            assert first[name].shape == other[name].shape and np.array_equal(first[name], other[name]), name
    assert first["static/0"].shape == (300, 4) and len(first["nms1/0"]) > 0 and first["overlaps1/0"].shape == (2000, 50)
    assert grown < bound, (grown, bound)
