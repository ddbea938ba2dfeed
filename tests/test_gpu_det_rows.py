"""GPU: the detection head on the many-row GEMM (k_fc_splitk12, az_head12.hip) across row counts (cases and premises:
tests/det_rows_ref.py, tests/test_det_rows_host.py).

What forks on the detection head's row count, and where it is visited (launch_det_head, az_detect.hip: it
takes the pass's DetPass record -- projection, pool source, image sizes --, the row-count pointer and the host's row bound; the
choice of kernel: fc_gemm_fp32, az_ctx.hip):
  A  integer-exact heads, FULL and SHORT, GEMM mode 0: det_forward of rois[:n] and rois[2048 - n:] at every n of
     det_rows_ref.ROWS_A -- k_fc_splitk below 161 rows, the switch, the half strip (M & 31 in 1..16), the full but masked
     last strip (17..31), a multiple of 32, the m-tile seams 384 | 385, 768 | 769, six m-tiles, M = the context's capacity.
     fc6 AND fc7 run the many-row kernel (fc7: 16 resp. 8 K-steps per work item, A = dh6).  bbox_pred bit for bit,
     cls_prob within train_step_ref.bound of the float32 softmax restatement's own error on the same rows.
  B  random FULL head: every n >= 161, both windows, bit for bit the rows of 160-row launches (k_fc_splitk); the 2048-row
     launch within 8 x the float32-CPU head's error against float64.
  C  az_detect: P >= 161 boxes of which u are distinct -- the launch is chosen by P, the device finds M = u -- bit for bit
     az_detect of the u distinct boxes alone (k_fc_splitk).
  D  az_detect_batch: the rows of several images in one many-row launch, mixed inside an m-tile, and a pass split at the
     region capacity, bit for bit az_detect per image.
  E  GEMM modes 2 and 3 (fc6 on k_fc_terms' 256-row tiles, fc7 still on the many-row fp32 kernel): prefixes of the 1000-row
     launch around 256 and 512 rows bit for bit, the integer head exact, the random head within the 8 x rule.

Every context loads a tiny AZ head of the same C first (az_set_feature_map needs one; in modes 2 / 3 it is also what
sends the detection fc6 down the 16-bit-term path).  Contexts, heads and references are made once per module, on first
use.  Every tolerance-based figure is printed before it is asserted (run with -s)."""
import functools

import numpy as np
import pytest

import det_rows_ref as D
import head_sizes_ref as H
import train_step_ref as R

pytestmark = pytest.mark.gpu


class Env(object):
    """The module's contexts, made on first use; each remembers which head it holds."""
    SPEC = {"big": (D.NROIS, 0), "cap": (D.CAP_SMALL, 0), "m2": (D.CAP_TERMS, 2), "m3": (D.CAP_TERMS, 3)}

    def __init__(self):
        self.ctxs, self.loaded = {}, {}

    def ctx(self, kind, case_key):
        from aznet_hip import ffi
        if kind not in self.ctxs:
            cap, mode = self.SPEC[kind]
            self.ctxs[kind] = ffi.AzContext(0, max_regions=cap, gemm_mode=mode)
            self.ctxs[kind].load_head(D.tiny_az_head())
        c = self.ctxs[kind]
        if self.loaded.get(kind) != case_key:
            c.load_det_head(get_case(case_key)["head"])
            self.loaded[kind] = case_key
        return c

    def close(self):
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()
    get_case.cache_clear()
    chunked_reference.cache_clear()


@functools.lru_cache(maxsize=None)
def get_case(key):
    """"FULL" / "SHORT": the integer-exact head; "random": the random FULL head with its float64 / float32-CPU evaluations."""
    from oracle import az_oracle as orc
    if key == "random":
        return D.random_case(orc)
    return D.int_case(key, pool=lambda f, r: orc.roi_pool(f[0], r))


def check(tag, got, r64, r32):
    e_dev, e_cpu = R.rel_err(got, r64), R.rel_err(r32, r64)
    b = R.bound(e_cpu)
    print("  %-40s device %.3e   float32-CPU %.3e   bound %.3e   ratio %.3f   %s"
          % (tag, e_dev, e_cpu, b, e_dev / e_cpu if e_cpu else 0.0, "ok" if e_dev <= b else "EXCEEDS"))
    return e_dev <= b


def check_prob(tag, e, tol):
    print("  %-40s device %.3e   bound %.3e   %s" % (tag, e, tol, "ok" if e <= tol else "EXCEEDS"))
    return e <= tol


def _integer_rows(ctx, c, rows, tag):
    """det_forward of a window of an integer case: bbox_pred exact, cls_prob within the window's own tolerance."""
    p, b = ctx.det_forward(c["rois"][rows])
    assert np.array_equal(b, c["bbox"][rows]), "bbox_pred, %s" % tag
    return p, b, check_prob("cls_prob %s" % tag, R.rel_err(p, c["p64"]["cls"][rows]), D.prob_tol(c, rows))


# ---- A. integer-exact heads across row counts -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.ROWS_A)
@pytest.mark.parametrize("name", ("FULL", "SHORT"))
def test_integer_head_bit_for_bit_at_every_row_count(env, name, n):
    c = get_case(name)
    ctx = env.ctx("big", name)
    ctx.set_feature_map(c["fmap"])
    ok = True
    for back in (False, True):
        ok &= _integer_rows(ctx, c, D.window(n, back), "%s %d rows %s" % (name, n, "back" if back else "front"))[2]
    assert ok, "cls_prob exceeds 8 x the float32 restatement's error"


# ---- B. row independence on a random head ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunked_reference(ctx):
    """(cls_prob, bbox_pred) of all 2048 rois of the random head from launches of 160 rows: k_fc_splitk."""
    c = get_case("random")
    outs = [ctx.det_forward(c["rois"][i:i + D.CHUNK_B]) for i in range(0, D.NROIS, D.CHUNK_B)]
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def _random_on_big(env):
    c = get_case("random")
    ctx = env.ctx("big", "random")
    ctx.set_feature_map(c["fmap"])
    return c, ctx


@pytest.mark.parametrize("n", D.ROWS_B)
def test_random_head_same_bits_as_the_tile_gemm(env, n):
    c, ctx = _random_on_big(env)
    ref = chunked_reference(ctx)
    for back in (False, True):
        rows = D.window(n, back)
        got = ctx.det_forward(c["rois"][rows])
        for name, g, r in zip(("cls_prob", "bbox_pred"), got, ref):
            assert np.array_equal(g, r[rows]), "%s, %d rows, %s window" % (name, n, "back" if back else "front")


def test_random_head_accuracy_at_2048_rows(env):
    c, ctx = _random_on_big(env)
    got, ok = ctx.det_forward(c["rois"]), True
    for name, g, r64, r32 in zip(("cls_prob", "bbox_pred"), got, c["r64"], c["r32"]):
        ok &= check("%s mode 0, 2048 rows" % name, g, r64, r32)
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


# ---- C. few unique rows under a large bound -------------------------------------------------------------------------------
@pytest.mark.parametrize("P,u", D.FEW_CASES, ids=lambda v: str(v))
def test_few_unique_rows_under_a_large_bound(env, P, u):
    _, ctx = _random_on_big(env)
    boxes, distinct, rep = D.few_unique(P, u)
    s, b = ctx.detect(boxes, 1.0, H.IM_H, H.IM_W)
    if u < D.GEMM12_MIN:
        sr, br = ctx.detect(distinct, 1.0, H.IM_H, H.IM_W)                      # u rows under a bound of u: k_fc_splitk
    else:                                                                       # (u >= 161: in pieces that stay on it)
        parts = [ctx.detect(distinct[i:i + D.CHUNK_B], 1.0, H.IM_H, H.IM_W) for i in range(0, u, D.CHUNK_B)]
        sr, br = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    assert s.shape == (P, D.FULL[3]) and b.shape == (P, 4 * D.FULL[3])
    assert np.array_equal(s, sr[rep]) and np.array_equal(b, br[rep])


# ---- D. several images in one launch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(D.BATCH_CASES))
def test_rows_of_several_images_in_one_launch(env, key):
    counts, cap = D.BATCH_CASES[key]
    ctx = env.ctx("big" if cap == D.NROIS else "cap", "random")
    maps, boxes = D.batch_maps(len(counts)), D.batch_boxes(counts)
    hw = [(H.IM_H, H.IM_W)] * len(counts)
    got = ctx.detect_batch(maps, boxes, [1.0] * len(counts), hw)
    for i, (m, bx) in enumerate(zip(maps, boxes)):
        ctx.set_feature_map(m)
        if len(bx) < D.GEMM12_MIN:
            sr, br = ctx.detect(bx, 1.0, H.IM_H, H.IM_W)
        else:                                                                   # (the reference stays on k_fc_splitk)
            parts = [ctx.detect(bx[j:j + D.CHUNK_B], 1.0, H.IM_H, H.IM_W) for j in range(0, len(bx), D.CHUNK_B)]
            sr, br = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
        assert np.array_equal(got[i][0], sr) and np.array_equal(got[i][1], br), "image %d of %s" % (i, key)
        s1, b1 = ctx.detect(bx, 1.0, H.IM_H, H.IM_W)                            # ... and the image alone in one call
        assert np.array_equal(got[i][0], s1) and np.array_equal(got[i][1], b1), "image %d of %s alone" % (i, key)


# ---- E. the 16-bit-term modes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", D.TERM_MODES)
def test_integer_head_in_the_16_bit_term_modes(env, mode):
    c = get_case("FULL")
    ctx = env.ctx("m%d" % mode, "FULL")
    ctx.set_feature_map(c["fmap"])
    top = max(D.ROWS_E)
    ref = _integer_rows(ctx, c, slice(0, top), "mode %d, %d rows" % (mode, top))
    ok = ref[2]
    for n in D.ROWS_E:
        p, b, good = _integer_rows(ctx, c, slice(0, n), "mode %d, %d rows" % (mode, n))
        ok &= good
        assert np.array_equal(p, ref[0][:n]) and np.array_equal(b, ref[1][:n]), "prefix of the %d-row launch, mode %d, %d rows" % (top, mode, n)
    assert ok, "cls_prob exceeds 8 x the float32 restatement's error"


@pytest.mark.parametrize("mode", D.TERM_MODES)
def test_random_head_in_the_16_bit_term_modes(env, mode):
    c = get_case("random")
    ctx = env.ctx("m%d" % mode, "random")
    ctx.set_feature_map(c["fmap"])
    top, ok = max(D.ROWS_E), True
    ref = ctx.det_forward(c["rois"][:top])
    for name, g, r64, r32 in zip(("cls_prob", "bbox_pred"), ref, c["r64"], c["r32"]):
        ok &= check("%s mode %d, %d rows" % (name, mode, top), g, r64[:top], r32[:top])
    for n in D.ROWS_E:
        for name, g, r in zip(("cls_prob", "bbox_pred"), ctx.det_forward(c["rois"][:n]), ref):
            assert np.array_equal(g, r[:n]), "%s: prefix of the %d-row launch, mode %d, %d rows" % (name, top, mode, n)
    assert ok, "a tensor exceeds 8 x the float32-CPU error"
