"""The search forms at their table limits, on planted zoom trees (tests/search_limits_ref.py: a region zooms exactly when
its RoIPool window holds a planted cell, so every level's population is known on the CPU; the frozen cases put a level at
exactly a limit of a single-workgroup kernel and a few regions past it).  Every form gives the plain level loop's bits;
the plain level loop gives the oracle's search and the generator's populations; the forms that own the limited level
run it without a rerun at the limit, and past it hand over ONCE, remember the shape, and leave other shapes alone."""
import numpy as np
import pytest

import search_limits_ref as R

pytestmark = pytest.mark.gpu

CASES = R.load_cases()
PLAIN = dict(speculate=False, fused=False, fused_levels=False, static_tree=False, pair_spec=False, full_spec=False,
             early_end=False)
FORMS = {"default": {}, "fused_only": dict(fused=True, fused_levels=False), "levels_only": dict(fused=False, fused_levels=True),
         "pair": dict(pair_spec=True), "full": dict(full_spec=True), "closure": dict(full_spec="closure")}


@pytest.fixture(scope="module")
def mods():
    from aznet_hip import ffi, synth
    from aznet_hip.net import HipAZNet
    from oracle import az_oracle as orc
    return ffi, synth, HipAZNet, orc


@pytest.fixture(scope="module")
def world(mods):
    """Per case: head (one for all), map, populations; the plain level loop's result per (case, batch), computed once on a
    context of its own (that form takes no decision from history)."""
    ffi, synth, HipAZNet, orc = mods
    inp = {k: R.case_inputs(c) for k, c in CASES.items()}
    head = inp["cap"][0]
    plain_net = HipAZNet(head, name="limits_plain")
    cache = {}

    class World(object):
        pass

    w = World()
    w.head = head
    w.fmap = {k: v[1] for k, v in inp.items()}
    w.pops = {}

    def pops(name, batch=10000):
        if (name, batch) not in w.pops:
            w.pops[(name, batch)] = R.case_populations(CASES[name], batch)
        return w.pops[(name, batch)]

    def plain(name, batch=10000):
        if (name, batch) not in cache:
            plain_net.set_conv(w.fmap[name])
            cache[(name, batch)] = run(ffi, plain_net, name, batch, **PLAIN)
        return cache[(name, batch)]

    w.populations, w.plain, w.plain_net = pops, plain, plain_net
    return w


def params(ffi, name, batch=10000, **kw):
    c = CASES[name]
    return ffi.AzContext.make_params(c["H"], c["W"], c["scale"], R.TZ, batch_size=batch, **kw)


def run(ffi, net, name, batch=10000, **kw):
    Y, S, st = net.propose(params(ffi, name, batch, **kw), want_scores=True, want_stats=True)
    Ya, Sa = net.ctx.last_candidates()
    return dict(Y=Y, S=S, Ya=Ya, Sa=Sa, st=st)


def fresh(mods, world, name, tag="x", **kw):
    ffi, synth, HipAZNet, orc = mods
    net = HipAZNet(world.head, name="limits_%s_%s" % (name, tag), **kw)
    pin_costs(ffi, net)
    net.set_conv(world.fmap[name])
    return net


def pin_costs(ffi, net):
    """The form a search takes "by history" is decided from head-pass costs the context measures on its device; with this
    small head a pass costs next to nothing per row and a second search of a shape goes to the closure pass.  The tests
    that assert a form pin the table to the full head's figures, as tests/test_gpu_full.py does."""
    net.ctx.set_pass_costs(ffi.AzContext.REFERENCE_PASS_COSTS)


def same(a, b, what=""):
    for k in ("Y", "S", "Ya", "Sa"):
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), (what, k)
    for f in ("n_proposals", "num_eval", "depth", "n_levels", "n_candidates"):
        assert getattr(a["st"], f) == getattr(b["st"], f), (what, f)
    for f in ("level_regions", "level_unique", "level_zoomed"):
        assert list(getattr(a["st"], f)) == list(getattr(b["st"], f)), (what, f)


def passes(st, below=None):
    """[(levels mask, rows)] of a search's head passes (those of levels < `below` only)."""
    out = [(int(st.pass_levels[i]), int(st.pass_rows[i])) for i in range(st.n_passes)]
    return [p for p in out if below is None or p[0] < (1 << below)]


def overflows(p, batch):
    """Does the default form of a first search hand this tree over?  (az_fused.hip / az_level.hip: a level of levels 1-3
    past FL_R; level 3 past batch_size at the hand-over; a level k_level_geom produces past LV_R or batch_size.)"""
    nlev = p["nlev"]
    if nlev < 3:
        return False
    if any(p["P"][l] > R.FL_R for l in range(1, min(nlev, 4))):
        return True
    if nlev > 3 and p["P"][3] > batch:
        return True
    return any(p["P"][l + 1] > R.LV_R or p["P"][l + 1] > batch for l in range(3, nlev - 1))


# ------------------------------------------------------------------------------------------------ the reference of the rest
@pytest.mark.parametrize("name", sorted(CASES))
def test_plain_level_loop_is_the_oracles_search_and_the_planted_tree(mods, world, name):
    ffi, synth, HipAZNet, orc = mods
    c, p = CASES[name], world.populations(name)
    got = world.plain(name)
    st = got["st"]
    assert st.n_reruns == 0 and st.search_form == 0 and st.n_levels == p["nlev"]
    for l in range(p["nlev"]):
        assert (st.level_regions[l], st.level_unique[l], st.level_zoomed[l]) == (p["P"][l], p["U"][l], p["PZ"][l]), (name, l)
    net, fmap = world.plain_net, world.fmap[name]

    class Injected(object):      # pycaffe-shaped view of the HIP head
        name = "inj"
        blobs = net.blobs

        def forward(self, blobs=None, **kw):
            kw.pop("data", None)
            kw["conv5_3"] = fmap
            return net.forward(blobs=blobs, **kw)

    inj = Injected()
    Yref, tr = orc.im_propose({"full": inj, "fc": inj}, (c["H"], c["W"]), c["scale"], orc.OracleCfg(Tz=R.TZ),
                              return_trace=True)
    assert st.depth == tr["depth"] and st.num_eval == tr["num_eval"]
    for l, lev in enumerate(tr["levels"]):
        assert st.level_regions[l] == lev["B"].shape[0] and st.level_zoomed[l] == len(lev["indZ"])
        assert st.level_unique[l] == sum(f["U"] for f in lev["fwd"])
    assert got["Ya"].shape == tr["Y_all"].shape
    assert np.array_equal(got["Sa"].astype(np.float64), tr["aScores"])              # scores: same bits
    np.testing.assert_allclose(got["Ya"], tr["Y_all"], rtol=1e-6, atol=1e-4)        # decode: f32-exp ulps (px)
    ref_idx = np.argsort(-tr["aScores"], kind="stable")[:300]
    assert np.array_equal(got["Y"], got["Ya"][ref_idx]) and np.array_equal(got["S"], got["Sa"][ref_idx])


# ------------------------------------------------------------------------------------------------ every form, every case
# The whole-tree forms on the trees whose speculative pass is staged (<= SPEC_PRE rows): (n_reruns, search_form, n_passes)
# of a first search.  The closure rows hold every window any pruning can need: one pass, and past LV_R one hand-over that
# keeps the form (lv_limits).  The full tree's rows serve the three small pruned trees as they are; the 801 x 1201 trees
# keep a _sift_dup survivor the full tree drops, so that pass lacks a window and the search is repeated level by level
# (tests/test_gpu_full.py: test_tree_rows_can_miss_a_window_that_the_closure_holds) -- past the limit the repeat then
# meets LV_R as well.  The inputs are fixed (planted tree, fresh context, forced form), so each outcome is one value.
WHOLE = {("lv_r_at", "closure"): (0, 3, 1), ("lv_r_at", "full"): (1, 0, 4),
         ("lv_r_past", "closure"): (1, 3, 1), ("lv_r_past", "full"): (2, 0, 4)}
for _n in ("pre_49", "cap", "batch_fused"):
    WHOLE[(_n, "closure")], WHOLE[(_n, "full")] = (0, 3, 1), (0, 2, 1)


def expected_first(name, form, p):
    """(n_reruns, search_form or None, n_passes or None) of a FIRST search on a fresh context"""
    nlev = p["nlev"]
    over = overflows(p, 10000)
    if form in ("full", "closure"):
        if p["spec_rows"] <= R.SPEC_PRE:
            return WHOLE[(name, form)]
        # more than SPEC_PRE speculative rows: the whole-tree forms are not taken -- the default level loop, one pass for
        # levels 0-2 and one per level behind them, handed over once if the tree outgrows a table
        return (1 if over else 0, 0, nlev - 2)
    if form == "levels_only":                    # (fused=False turns the fused level kernel off with it: multi-launch forms)
        return (0, 0, None)
    if form == "fused_only":                     # k_spec_levels only: levels 1-3 and the hand-over of level 3
        return (1 if any(p["P"][l] > R.FL_R for l in range(1, min(nlev, 4))) else 0, 0, None)
    if form == "pair":
        # (a shape of fewer than five levels has no level whose pass could carry the next one's rows)
        if not over:
            return (0, 1 if nlev >= 5 else 0, None)
        return (1, None, None)
    return (1 if over else 0, 0, None)


# (a shape of fewer than four levels has nothing behind the speculative levels for a whole-tree pass to serve)
FORM_CASES = [(n, f) for n in sorted(CASES) for f in sorted(FORMS)
              if not (f in ("full", "closure") and R.orc.num_levels(CASES[n]["H"], CASES[n]["W"]) - 1 < 4)]


@pytest.mark.parametrize("name,form", FORM_CASES, ids=["%s-%s" % nf for nf in FORM_CASES])
def test_every_form_gives_the_plain_loops_bits_and_hands_over_only_past_the_limit(mods, world, name, form):
    ffi, synth, HipAZNet, orc = mods
    p = world.populations(name)
    net = fresh(mods, world, name, form)
    got = run(ffi, net, name, static_tree=False, **FORMS[form])
    same(got, world.plain(name), (name, form))
    st = got["st"]
    print(name, form, "n_reruns", st.n_reruns, "form", st.search_form, "passes", passes(st))
    want = expected_first(name, form, p)
    assert st.n_reruns == want[0], (name, form, st.n_reruns, st.search_form)
    if want[1] is not None:
        assert st.search_form == want[1], (name, form, st.search_form)
    if want[2] is not None:
        assert st.n_passes == want[2], (name, form, passes(st))
    assert st.root_deferred == 0                                   # (a fresh context never defers the root)
    # the same search again: whatever the first one learnt, same bits and no second hand-over (the forced tree-rows pass
    # that lacked a window is forced again)
    again = run(ffi, net, name, static_tree=False, **FORMS[form])
    same(again, world.plain(name), (name, form, "again"))
    if not (form == "full" and want[1] == 0 and p["spec_rows"] <= R.SPEC_PRE):
        assert again["st"].n_reruns == 0, (name, form, again["st"].n_reruns)


# ------------------------------------------------------------------------------------------------ the deferred root
@pytest.mark.parametrize("name", ["p1_254", "p1_257"])
def test_roots_children_at_and_past_fl_r_with_and_without_the_deferred_root(mods, world, name):
    """The root's children (P1spec) against FL_R = 256 at level 1 of k_spec_levels: 254 fit, 257 are handed over ONCE, to
    the multi-launch kernels.  The deferred root is a decision from history (four searches of the context that reached
    level 4), so the context is primed with a fitting tree of another shape first."""
    ffi, synth, HipAZNet, orc = mods
    LOOP = dict(static_tree=False, pair_spec=False, full_spec=False)
    reruns = 1 if world.populations(name)["P1"] > R.FL_R else 0
    plainly = run(ffi, fresh(mods, world, name, "nodefer"), name, **LOOP)
    same(plainly, world.plain(name), "not deferred")
    assert (plainly["st"].root_deferred, plainly["st"].n_reruns) == (0, reruns)
    net = fresh(mods, world, "cap", "primed_" + name)
    for i in range(4):
        assert run(ffi, net, "cap", **LOOP)["st"].root_deferred == 0
    fifth = run(ffi, net, "cap", **LOOP)
    same(fifth, world.plain("cap"), "primed")
    assert fifth["st"].root_deferred == 1 and fifth["st"].n_reruns == 0
    net.set_conv(world.fmap[name])
    got = run(ffi, net, name, **LOOP)
    same(got, world.plain(name), "deferred")
    # at 254 the search keeps its deferred root; at 257 the deferred attempt is given up for the multi-launch form
    assert (got["st"].n_reruns, got["st"].root_deferred) == (reruns, 1 - reruns), (got["st"].n_reruns, got["st"].root_deferred)
    again = run(ffi, net, name, **LOOP)
    same(again, world.plain(name), "again")
    assert (again["st"].n_reruns, again["st"].root_deferred) == (0, 1 - reruns)
    if not reruns:
        assert passes(got["st"])[0][0] == 6 and passes(got["st"])[0][1] == world.populations(name)["spec_rows"] - 1
        assert passes(plainly["st"])[0] == (7, world.populations(name)["spec_rows"])


# ------------------------------------------------------------------------------------------------ hand-over past the limit
@pytest.mark.parametrize("at,past,level", [("lv_r_at", "lv_r_past", 4), ("fl_r_at", "fl_r_past", 2),
                                           ("fl_r_last_at", "fl_r_last_past", 2)])
def test_past_the_limit_one_rerun_then_remembered_and_other_shapes_stay_fused(mods, world, at, past, level):
    ffi, synth, HipAZNet, orc = mods
    # (the level loop by decision, not by history: what a second search of a shape would cost decides nothing here)
    LOOP = dict(static_tree=False, pair_spec=False, full_spec=False)
    other = "cap"                                              # another shape, whose tree fits every table
    ref_other = run(ffi, fresh(mods, world, other, "ref"), other, **LOOP)
    assert ref_other["st"].n_reruns == 0
    twin = run(ffi, fresh(mods, world, at, "twin"), at, **LOOP)
    assert twin["st"].n_reruns == 0 and twin["st"].search_form == 0

    net = fresh(mods, world, past, "three")
    first = run(ffi, net, past, **LOOP)
    net.ctx.set_profiling(2)
    second = run(ffi, net, past, **LOOP)
    launches = [(n, l) for n, l, _ in net.ctx.last_kernel_times()]
    net.ctx.set_profiling(0)
    net.set_conv(world.fmap[other])
    third = run(ffi, net, other, **LOOP)
    assert (first["st"].n_reruns, second["st"].n_reruns, third["st"].n_reruns) == (1, 0, 0)
    same(first, world.plain(past), "first")
    same(second, world.plain(past), "second")
    same(third, world.plain(other), "third")
    # the other shape runs as on a context that never met the overflowing one: same passes, same rows
    assert passes(third["st"]) == passes(ref_other["st"])
    names = [n for n, _ in launches]
    if level > 3:
        # past LV_R behind the first k_level_geom level: the levels before it keep their fused kernels, from it on the
        # multi-launch ones; passes and rows equal the at-limit twin's up to the overflowing level
        assert "spec_levels" in names and ("level_geom", 3) in launches
        assert not any(n == "level_geom" and l >= level for n, l in launches)
        assert ("sift_dup", level) in launches
        for r in (first, second):
            assert passes(r["st"], below=level + 1) == passes(twin["st"], below=level + 1)
            assert passes(r["st"])[-1] == (1 << (level + 1), world.populations(past)["U"][level + 1])
    else:
        # levels 1-3 themselves outgrew k_spec_levels: everything on the multi-launch kernels
        assert "spec_levels" not in names and "level_geom" not in names and ("sift_dup", level) in launches
    # the at-limit twin on THIS context (which remembers the shape): still the same bits
    net.set_conv(world.fmap[at])
    same(run(ffi, net, at, **LOOP), world.plain(at), "twin after")


# ------------------------------------------------------------------------------------------------ batch_size
BATCH = [("batch_fused", 3, 0), ("batch_fused", 3, -1), ("cap", 4, 0), ("cap", 4, -1), ("lv_r_at", 4, 0), ("lv_r_at", 4, -1)]


@pytest.mark.parametrize("name,level,delta", BATCH, ids=["%s-P%d%+d" % b for b in BATCH])
def test_batch_size_at_a_level_and_one_below(mods, world, name, level, delta):
    """batch_size == P of a level: one dedup chunk, the single-workgroup kernels keep the level.  One below: the level goes
    to the chunked multi-launch dedup (one rerun), whose counts are the oracle's per-chunk np.unique."""
    ffi, synth, HipAZNet, orc = mods
    p0 = world.populations(name)
    batch = p0["P"][level] + delta
    p = world.populations(name, batch)
    assert max(p["P"]) == p["P"][level] or name == "lv_r_at"
    ref = world.plain(name, batch)
    assert [ref["st"].level_unique[l] for l in range(p["nlev"])] == p["U"]
    net = fresh(mods, world, name, "batch")
    got = run(ffi, net, name, batch, static_tree=False)
    same(got, ref, (name, batch))
    over = overflows(p, batch)
    assert over == (delta < 0 or name == "lv_r_at")          # (lv_r_at: level 5 is larger than level 4)
    assert got["st"].n_reruns == (1 if over else 0), (name, batch, got["st"].n_reruns)
    again = run(ffi, net, name, batch, static_tree=False)
    same(again, ref, (name, batch, "again"))
    assert again["st"].n_reruns == 0
    # the oracle's chunked search: same tree, same per-chunk unique counts, same candidates
    onet = orc.OracleNet(world.head, feat_fn=lambda d: world.fmap[name])
    c = CASES[name]
    _, tr = orc.im_propose({"full": onet, "fc": onet}, (c["H"], c["W"]), c["scale"],
                           orc.OracleCfg(Tz=R.TZ, BATCH_SIZE=batch), return_trace=True)
    for l, lev in enumerate(tr["levels"]):
        assert [f["R"] for f in lev["fwd"]] == [min(batch, p["P"][l] - s) for s in range(0, p["P"][l], batch)]
        assert got["st"].level_unique[l] == sum(f["U"] for f in lev["fwd"])
    assert got["Ya"].shape == tr["Y_all"].shape
    np.testing.assert_allclose(got["Sa"], tr["aScores"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(got["Ya"], tr["Y_all"], rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------------ context capacity
def test_first_fit_inside_max_regions(mods, world):
    """max_regions == the largest level (and pass) of the tree: the search succeeds, in the plain and the default form.  One
    region less: AZ_ERR_CAPACITY naming az_set_limits, and the next search on that context, one that fits, is right.
    (The child capacity is 4 * max_regions and at most three children share a _sift_dup hash, so a level's children can
    only outgrow it after its regions have outgrown max_regions: there is no case for it, see DESIGN.md.)"""
    ffi, synth, HipAZNet, orc = mods
    name, small = "cap", "batch_fused"                       # (same image shape; the small tree's levels are <= 25 regions)
    p = world.populations(name)
    ref = world.plain(name)
    probe = run(ffi, fresh(mods, world, name, "probe"), name, static_tree=False)
    need = max(max(p["P"]), max(r for _, r in passes(probe["st"])), max(r for _, r in passes(ref["st"])))
    assert need == max(p["P"]) == 245 and need - 1 >= 64
    ncand = 11 * sum(p["P"])
    for form in (PLAIN, dict(static_tree=False)):
        net = HipAZNet(world.head, name="limits_fit", ctx=ffi.AzContext(0, max_regions=need, max_candidates=ncand))
        pin_costs(ffi, net)
        net.set_conv(world.fmap[name])
        got = run(ffi, net, name, **form)
        same(got, ref, "exact fit")
    for form in (PLAIN, dict(static_tree=False)):
        ctx = ffi.AzContext(0, max_regions=need - 1, max_candidates=ncand)
        net = HipAZNet(world.head, name="limits_tight", ctx=ctx)
        pin_costs(ffi, net)
        net.set_conv(world.fmap[name])
        with pytest.raises(ffi.AzError) as e:
            net.propose(params(ffi, name, **form))
        assert e.value.code == ffi.AZ_ERR_CAPACITY and "az_set_limits" in str(e.value)
        net.set_conv(world.fmap[small])
        same(run(ffi, net, small, **form), world.plain(small), "after the capacity error")


# ------------------------------------------------------------------------------------------------ queued and staged
@pytest.mark.parametrize("order", [("lv_r_past", "lv_r_at"), ("lv_r_at", "lv_r_past")], ids=["past_first", "at_first"])
def test_queued_and_staged_searches_across_the_limit(mods, world, order):
    """Two searches launched before the first fetch, each with a staged result record: the one past the limit is run again
    inside its fetch (behind the one queued after it), its record restaged; records equal the fetched results, which
    equal the plain level loop's."""
    import torch
    from aznet_hip import dist as azdist
    ffi, synth, HipAZNet, orc = mods
    k = 300
    maps = {n: torch.from_numpy(world.fmap[n]).cuda() for n in order}
    layout = ffi.AzContext.result_record_layout(k)
    net = HipAZNet(world.head, name="limits_queue")
    pin_costs(ffi, net)
    for rnd in range(2):
        bufs = [torch.zeros(layout[0], dtype=torch.uint8, device="cuda") for _ in order]
        for n, buf in zip(order, bufs):
            net.ctx.propose_launch(params(ffi, n, static_tree=False), fmap=maps[n])
            net.ctx.stage_result(buf.data_ptr(), layout[0])
        got = [net.ctx.propose_fetch(want_scores=True, want_stats=True) for _ in order]
        torch.cuda.synchronize()
        for n, buf, (Y, S, st) in zip(order, bufs, got):
            ref = world.plain(n)
            assert np.array_equal(Y, ref["Y"]) and np.array_equal(S, ref["S"]), (rnd, n)
            assert list(st.level_regions) == list(ref["st"].level_regions)
            # first round: the search past the limit is handed over once; the at-limit one never (queued behind the other
            # it was launched before the shape was remembered: it fits the fused kernels anyway)
            assert st.n_reruns == (1 if (rnd == 0 and n.endswith("past")) else 0), (rnd, n, st.n_reruns)
            rec = azdist.unpack_device_record(buf.cpu().numpy(), layout, k)
            assert rec is not None and np.array_equal(rec[0], Y) and np.array_equal(rec[1], S), (rnd, n)
