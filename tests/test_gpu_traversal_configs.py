"""The BVH traversal code (csrc/ff_k_traverse.h, ff_k_lds.h, trace_bvh_kernel, nee_path_kernel, ray_batch_kernel) in the
configurations that the test scenes do not produce by themselves: every workgroup size (forced with FF_BLOCK_THREADS and chosen by
finalize_layout for deep trees), both stack residencies (the default, which spills the deepest levels to global memory, and
FF_NO_STACK_SPILL), the node-residency boundaries (FF_DEBUG_LDS_NODE_CAP) and the time slices (FF_SETUP_THRESHOLD,
FF_LEAF_THRESHOLD).  The bar is the project's own: the same call in FF_TRACE_BRUTE_FORCE on the same tracer, bit for bit - rgb8, the
radiance bits, `hit` and the `t` bits of ray batches - with no tolerance; the scenes that are cases of tests/cases.py also against the
oracle's golden frames, so that BVH and brute force cannot be wrong together; ff_gbuffer against the CPU oracle.  Across the
configurations of one scene the results and rays_traced are equal.  ff_debug_layout and ff_debug_stack_spill prove that the path a
test names is the one that ran.  Frames are 48 x 32, 3 bounces, 2 spp; ray batches 3 000 rays."""
import functools
import os

import numpy as np
import pytest

import traversal_cases as tc
from gbuffer_ref import oracle_gbuffer
from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
from test_gpu_dynamic import check_trees

pytestmark = pytest.mark.gpu

W, H, BOUNCES, SPP, SEED = 48, 32, 3, 2, 3
GW, GH = 32, 24
PATH, NEE = T.SHADE_DIFFUSE_PATH, T.SHADE_DIFFUSE_PATH_NEE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames.npz")
SWITCHES = ("FF_BLOCK_THREADS", "FF_NO_STACK_SPILL", "FF_DEBUG_LDS_NODE_CAP", "FF_SETUP_THRESHOLD", "FF_LEAF_THRESHOLD", "FF_POOL", "FF_POOL_STACK_LEVELS",
            "FF_REUSE_MIN_SPP", "FF_NO_START_RECORDS", "FF_NO_WORLD_NORMALS", "FF_NO_PRIMARY_REUSE") + tc.BUILDER_SWITCHES

# name -> (scene, camera pose, where the ray batch starts and how far around it, golden case rendered on it or None)
SCENES = {
    "small": (tc.small_scene, tc.INSIDE, ((0.0, 0.0, 2.4), 1.5), tc.SMALL_GOLDEN),
    "extras": (tc.extras_scene, tc.INSIDE, ((0.0, 0.0, 2.4), 1.5), tc.EXTRAS_GOLDEN),
    "crowd1": (lambda: tc.crowd_scene(tc.CROWD_CLASS1), tc.INSIDE, ((0.0, 0.0, 2.4), 1.5), None),
    "crowd2": (lambda: tc.crowd_scene(tc.CROWD_CLASS2), tc.INSIDE, ((0.0, 0.0, 2.4), 1.5), None),
}
for _d in tc.DEEP_TREES:
    SCENES[_d.name] = (_d.scene, tc.DEEP_CAMERA, ((0.0, 0.3, 4.0), 1.5), None)
for _b in tc.SPILL_EXTRAS:
    SCENES[f"spill_{_b}"] = (functools.partial(tc.spill_scene, _b), tc.INSIDE, ((0.0, 0.0, 2.4), 1.5), None)
SCENES["deep_crowd"] = (tc.deep_crowd_scene, tc.DEEP_CAMERA, ((0.0, 0.3, 4.0), 1.5), None)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture
def env(monkeypatch):
    """The environment without any of the switches this file sets; tests set theirs through the returned monkeypatch."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def P(w=W, h=H, bounces=BOUNCES, spp=SPP, shade=PATH, trace=T.TRACE_BVH):
    return lib.render_params(w, h, bounces, spp, SEED, trace, shade, T.GRID_FULL, 0)


def bits(frame):
    return frame[0].copy(), frame[1].view(np.uint32).copy()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def gbuffer_want(name):
    scene_fn, pose, _, _ = SCENES[name]
    return oracle_gbuffer(scene_fn(), tc.camera(GW, GH, **pose), P(GW, GH, 1, 1))


BASELINE = {}  # scene -> {kind: (bits, rays_traced or None)} as a tracer created under NONE of the switches renders it


def builder_of(name):
    deep = tc.DEEP_BY_NAME.get(name)
    return deep.builder if deep else (T.BUILD_GPU_LBVH if name == "deep_crowd" else T.BUILD_HOST_SAH)


def baseline(name):
    """The scene's frame, NEE frame (each with rays_traced) and ray batch in the DEFAULT configuration: a tracer of its own, created
    and uploaded with every switch of this file taken out of the environment, whichever test asks first and whatever that test has set."""
    if name not in BASELINE:
        held = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
        try:
            with lib.Tracer(0) as t:
                for k, v in (tc.DEEP_BY_NAME[name].env if name in tc.DEEP_BY_NAME else {}).items():
                    os.environ[k] = v
                t.set_builder(builder_of(name))
                t.upload_scene(SCENES[name][0]())
                for k in (tc.DEEP_BY_NAME[name].env if name in tc.DEEP_BY_NAME else {}):
                    del os.environ[k]
                _, pose, origin, _ = SCENES[name]
                cam, out = tc.camera(W, H, **pose), {}
                t.set_collect_stats(True)
                for kind, shade in (("frame", PATH), ("nee", NEE)):
                    out[kind] = (bits(t.render(cam, P(shade=shade))), int(t.stats().rays_traced))
                t.set_collect_stats(False)
                a = t.intersect_rays(*tc.ray_batch(origin=origin[0], spread=origin[1]), T.TRACE_BVH)
                out["rays"] = ((a["hit"].copy(), a["t"].view(np.uint32).copy()), None)
        finally:
            os.environ.update(held)
        BASELINE[name] = out
    return BASELINE[name]


def check(t, name, kinds=("frame", "rays"), golden=None):
    """The uploaded scene `name` through the launches named by `kinds` on tracer `t`, each against brute force on the same tracer
    (the G-buffer, which has no brute-force mode: against the CPU oracle), against the default configuration (baseline), and - frames, once more with
    statistics on - for rays_traced equal to the default configuration's."""
    _, pose, origin, golden_name = SCENES[name]
    cam = tc.camera(W, H, **pose)
    for kind in kinds:
        if kind in ("frame", "nee"):
            shade = NEE if kind == "nee" else PATH
            got = bits(t.render(cam, P(shade=shade)))
            t.set_collect_stats(True)
            counted = bits(t.render(cam, P(shade=shade)))
            rays = int(t.stats().rays_traced)
            t.set_collect_stats(False)
            want = bits(t.render(cam, P(shade=shade, trace=T.TRACE_BRUTE_FORCE)))
            assert same(got, want), f"{name} {kind}: {(got[1] != want[1]).any(axis=2).sum()} pixels differ from brute force"
            assert same(counted, want), f"{name} {kind}: with statistics on, {(counted[1] != want[1]).any(axis=2).sum()} pixels differ from brute force"
            assert want[1].any(), f"{name} {kind}: a black frame compares nothing"
            assert baseline(name)[kind][1] == rays, f"{name} {kind}: rays_traced differs from the default configuration's"
        elif kind == "rays":
            o, d = tc.ray_batch(origin=origin[0], spread=origin[1])
            a, b = t.intersect_rays(o, d, T.TRACE_BVH), t.intersect_rays(o, d, T.TRACE_BRUTE_FORCE)
            got, want = (a["hit"].copy(), a["t"].view(np.uint32).copy()), (b["hit"].copy(), b["t"].view(np.uint32).copy())
            assert same(got, want), f"{name} ray batch: {(got[1] != want[1]).sum()} of {len(o)} rays differ from brute force"
            assert b["hit"].any(), f"{name}: a ray batch without a hit compares nothing"
        elif kind == "gbuffer":
            got_g, want_g = t.gbuffer(tc.camera(GW, GH, **pose), P(GW, GH, 1, 1)), gbuffer_want(name)
            for k in want_g:
                assert np.array_equal(got_g[k].view(np.uint32), want_g[k].view(np.uint32)), f"{name} G-buffer: {k} differs from the oracle"
            assert (want_g["ids"][..., 0] >= 0).any()
            continue
        else:
            raise ValueError(kind)
        assert same(baseline(name)[kind][0], got), f"{name} {kind}: differs from the default configuration"
    if golden is not None and golden_name is not None:
        scene, gcam, gparams = tc.golden_case(golden_name)
        rgb8, rad = t.render(gcam, gparams)
        assert np.array_equal(rgb8, golden[golden_name + "/rgb8"]), f"{golden_name}: rgb8 differs from the oracle's golden frame"
        assert np.array_equal(rad.view(np.uint32), golden[golden_name + "/radiance"].view(np.uint32)), f"{golden_name}: radiance differs from the oracle's golden frame"


def upload(t, name, builder=T.BUILD_HOST_SAH):
    t.set_builder(builder)
    t.upload_scene(SCENES[name][0]())
    return t.debug_layout()


def upload_deep(t, env, deep, name=None):
    """A deep tree under its builder switches (read at the upload), which are taken out again."""
    for k, v in deep.env.items():
        env.setenv(k, v)
    layout = upload(t, name or deep.name, deep.builder)
    for k in deep.env:
        env.delenv(k)
    return layout


# ---- d. node residency -------------------------------------------------------------------------------------------------------------------

def expected_shares(counts, mesh_cap):
    """finalize_layout's division of mesh_cap LDS node slots among meshes of `counts` nodes, in record order: min(count, 8) each while
    slots remain, then what is left in proportion to what each still wants (rounded down)."""
    share, left = [], mesh_cap
    for c in counts:
        share.append(min(c, 8, left))
        left -= share[-1]
    wanting = sum(c - s for c, s in zip(counts, share))
    if wanting > 0:
        share = [s + (c - s if wanting <= left else left * (c - s) // wanting) for c, s in zip(counts, share)]
    return share


@pytest.mark.parametrize("name", ["small", "crowd1"])
@pytest.mark.parametrize("cap", [0, 1, 8, 9, 64, None])
def test_node_residency(tracer, env, golden, name, cap):
    """FF_DEBUG_LDS_NODE_CAP at the boundaries of the split: nothing in LDS, one node, the small-tree first share and one past it, a
    partial proportional share, everything (unset)."""
    if cap is not None:
        env.setenv("FF_DEBUG_LDS_NODE_CAP", str(cap))
    tracer.reload_switches()
    layout = upload(tracer, name)
    n = len(SCENES[name][0]())
    _, table4 = tracer.download_bvh4(n)
    check_trees(tracer, n)  # (check_tree4: the shares lie inside the slots and do not overlap)
    meshes = table4[table4[:, 0] >= 0]
    total = int(meshes[:, 1].sum())
    top = int(meshes[:, 3].min())  # the geometry tree's nodes come first: the first mesh's share starts behind them
    if cap is None:
        assert layout["lds_cap"] >= 64 and meshes[:, 4].sum() > 64, "the default keeps more than the largest cap of this test in LDS"
        cap = layout["lds_cap"] if layout["lds_cap"] < total + top else 10 ** 9  # (lds_cap: the slots in use, at most every node)
    else:
        assert layout["lds_cap"] <= cap
    assert top <= cap and (top > 0) == (layout["top_depth"] > 0 and cap > 0)
    assert top + meshes[:, 4].sum() <= cap
    order = np.lexsort((meshes[:, 4] == 0, meshes[:, 3]))  # record order: by first slot, the meshes without a share last
    got = meshes[order]
    assert got[:, 4].tolist() == expected_shares(got[:, 1].tolist(), cap - top)
    if cap == 0:
        assert (table4[:, 4] == 0).all()
    check(tracer, name, ("frame", "nee", "rays"), golden)


# ---- c. stack residency ------------------------------------------------------------------------------------------------------------------

def touched_words(t, run):
    """Words of the spill area a launch writes: once to grow the area to the launch's size, the sentinel, the launch again."""
    run()
    t.reset_stack_spill()
    run()
    return t.stack_spill_words()


DEEPEST_RENDERING = "lbvh_768"  # (PLOC goes deeper, to 46 levels, but numbers its nodes differently from run to run)


SPILL_NAMES = [f"spill_{b}" for b in tc.SPILL_EXTRAS]


@pytest.mark.parametrize("name", ["small", "crowd1", DEEPEST_RENDERING, "deep_crowd"] + SPILL_NAMES)
def test_stack_residency(env, golden, name):
    """The default layout against FF_NO_STACK_SPILL, through the four launches whose block sizes and grids the spill index depends on:
    the frame (pre-pass and trace kernel at the scene's size), the NEE frame and the ray batch (512 threads, grids of their own) and
    the G-buffer's pre-pass.  spill_1024 / spill_768 / spill_512 are C2 filled up (tests/traversal_cases.py SPILL_EXTRAS) so that at
    that workgroup size - the last two under FF_BLOCK_THREADS - only four or five of the ten stack entries stay in LDS: there every
    launch must write spilled entries, read them back and give the brute-force bits.  Words of the spill area written under the
    default layout, measured on an MI355X (frame / G-buffer / NEE frame / ray batch):
      spill_1024   4 of 10 entries in LDS, 1 024 threads: 96 / 36 / 433 / 36      (asserted > 0)
      spill_768    4 of 10 in LDS, 768 threads:           88 / 34 / 402 / 32      (asserted > 0)
      spill_512    5 of 10 in LDS, 512 threads:           18 /  8 /  80 / 10      (asserted > 0)
      small        6 of 10 in LDS, 1 024 threads:          4 /  0 /  12 /  2      (frame, NEE frame and ray batch asserted > 0)
      crowd1       12 of 12 in LDS, no spill area:         0 /  0 /   0 /  0      (asserted 0)
      lbvh_768     31 of 42 in LDS, 768 threads (chosen):  0 /  0 /   0 /  0
      deep_crowd   12 of 48 in LDS, 512 threads (chosen):  0 /  0 /   0 /  0
    On the two deep trees the layout spills but no query of these launches holds more entries than LDS keeps (a query of the chain
    leaves an entry only where the ray also meets a peeled-off sibling; the same tree forced to 16 of 42 levels writes 0 too), so
    nothing is asserted about their counts: they cover the layout, the results and FF_NO_STACK_SPILL on a deep tree."""
    deep = tc.DEEP_BY_NAME.get(name)
    block = int(name.split("_")[1]) if name in SPILL_NAMES else None
    if block is not None and block != 1024:
        env.setenv("FF_BLOCK_THREADS", str(block))
    _, pose, origin, _ = SCENES[name]
    n = len(SCENES[name][0]())
    cam, o_d = tc.camera(W, H, **pose), tc.ray_batch(origin=origin[0], spread=origin[1])
    with lib.Tracer(0) as t:
        launches = {
            "frame": lambda: t.render(cam, P()),
            "gbuffer": lambda: t.gbuffer(tc.camera(GW, GH, **pose), P(GW, GH, 1, 1)),
            "nee": lambda: t.render(cam, P(shade=NEE)),
            "rays": lambda: t.intersect_rays(*o_d, T.TRACE_BVH),
        }
        layout = upload_deep(t, env, deep) if deep else upload(t, name, builder_of(name))
        spills = layout["stack_lds_levels"] < layout["stack_entries"]
        if n <= 32:  # (the arithmetic of scenes without a geometry tree)
            _, table4 = t.download_bvh4(n)
            want = tc.expected_lds_levels(int(table4[:, 1].sum()), layout["stack_entries"], n, layout["scene_block_threads"])
            assert layout["stack_lds_levels"] == want, layout
        assert 4 <= layout["stack_lds_levels"] <= layout["stack_entries"]
        check(t, name, tuple(launches), golden)
        words = {k: touched_words(t, run) for k, run in launches.items()}
        print(f"stack spill, {name}: {layout['scene_block_threads']} threads, entries {layout['stack_entries']}, in LDS {layout['stack_lds_levels']}, words written {words}")
        if not spills:
            assert not any(words.values()), words
        if name != "crowd1":
            assert spills, layout
        if block is not None:
            assert layout["scene_block_threads"] == block and layout["stack_lds_levels"] <= 5
            t.render(cam, lib.render_params(W, H, 2, 1, seed=3))
            assert t.kernel_name().startswith(f"trace_bvh_kernel<false, {block}, false, 0, false"), t.kernel_name()
            assert min(words.values()) > 0, f"a launch at {block} threads wrote no spilled stack entry ({words})"
        if name == "small":
            assert min(words["frame"], words["nee"], words["rays"]) > 0, f"a launch wrote no spilled stack entry ({words})"
        env.setenv("FF_NO_STACK_SPILL", "1")
        t.reload_switches()
        layout = upload_deep(t, env, deep) if deep else upload(t, name, builder_of(name))
        assert layout["stack_lds_levels"] == layout["stack_entries"]
        check(t, name, tuple(launches), golden)
        # (the area of the default layout is still allocated: the launches must not be handed it)
        assert {k: touched_words(t, run) for k, run in launches.items()} == dict.fromkeys(launches, 0)


# ---- e. slices ---------------------------------------------------------------------------------------------------------------------------

SETUPS, LEAVES = (0, 1, 2, 24, 16384), (1, 64)
SLICES = [(s, l) for s in SETUPS for l in LEAVES + (None,)] + [(None, l) for l in LEAVES]


@pytest.mark.parametrize("setup,leaf", SLICES, ids=[f"setup_{s}-leaf_{l}" for s, l in SLICES])
def test_slices(env, golden, setup, leaf):
    """FF_SETUP_THRESHOLD 0 (every query runs to completion), 1 (every query parks and resumes each round), 2, 24 and 16 384, crossed
    with FF_LEAF_THRESHOLD 1 and 64 (no leaf quorum can end a phase) on the small scene; on the scene with extras, a crowd of each
    size class and the deep LBVH tree one of the two at a time."""
    if setup is not None:
        env.setenv("FF_SETUP_THRESHOLD", str(setup))
    if leaf is not None:
        env.setenv("FF_LEAF_THRESHOLD", str(leaf))
    names = ["small"]
    if setup is None or leaf is None:
        names += ["extras", "crowd1", "crowd2", DEEPEST_RENDERING]
    with lib.Tracer(0) as t:
        for name in names:
            deep = tc.DEEP_BY_NAME.get(name)
            layout = upload_deep(t, env, deep) if deep else upload(t, name)
            assert layout["leaf_threshold"] == (20 if leaf is None else leaf)
            if setup is None:
                assert 4 <= layout["setup_threshold"] <= 32
            else:
                assert layout["setup_threshold"] == setup
            check(t, name, ("frame", "rays"), golden)


# ---- a. forced workgroup size ------------------------------------------------------------------------------------------------------------

def _name(t, scene_name, stats, **params):
    """The kernel of a one-off 16 x 16 frame of 1 spp and 2 bounces on a fresh upload, as tests/test_gpu_kernel_names.py renders it."""
    t.upload_scene(SCENES[scene_name][0]())
    t.set_collect_stats(stats)
    t.render(tc.camera(16, 16), lib.render_params(16, 16, 2, 1, seed=3, **params))
    t.set_collect_stats(False)
    return t.kernel_name()


@pytest.mark.parametrize("block", [512, 768])
def test_forced_workgroup_size_runs_every_instantiation(env, block):
    """FF_BLOCK_THREADS (read at ff_create): the non-prepass rows of FF_TRACE_BVH_KERNELS_OF at 512 and 768 threads by name - without
    and with extras, size classes 1 and 2, on start records, each with and without statistics.  WN does not show in the name: the two
    diffuse small-scene kernels run once on the normal tables and once under FF_NO_WORLD_NORMALS.  The pre-pass rows' name is not
    reported: test_forced_workgroup_size_frames runs them through ff_gbuffer and through frames on stored hits."""
    env.setenv("FF_BLOCK_THREADS", str(block))
    rows = [("small", "false", "0"), ("extras", "true", "0"), ("crowd1", "true", "1"), ("crowd2", "true", "2")]
    with lib.Tracer(0) as t:
        for no_wn in (False, True):
            if no_wn:
                env.setenv("FF_NO_WORLD_NORMALS", "1")
            t.reload_switches()
            for scene_name, extras, big in rows if not no_wn else rows[:1]:
                for stats in (False, True):
                    want = f"trace_bvh_kernel<{str(stats).lower()}, {block}, {extras}, {big}, false>"
                    assert _name(t, scene_name, stats) == want, (scene_name, stats, no_wn)
                    assert t.debug_layout()["scene_block_threads"] == block
                    assert _name(t, scene_name, stats, trace_mode=T.TRACE_BRUTE_FORCE) == f"trace_brute_kernel<{str(stats).lower()}>"
            env.setenv("FF_REUSE_MIN_SPP", "1")  # every frame on stored hits: the diffuse scene runs START, a scene with extras the raw-hit kernel
            t.reload_switches()
            for stats in (False, True):
                assert _name(t, "small", stats) == f"trace_bvh_kernel<{str(stats).lower()}, {block}, false, 0, false, true>", (stats, no_wn)
            assert _name(t, "extras", False) == f"trace_bvh_kernel<false, {block}, true, 0, false>"
            env.delenv("FF_REUSE_MIN_SPP")


@pytest.mark.parametrize("block", [512, 768])
def test_forced_workgroup_size_frames(tracer, env, golden, block):
    """Every scene at the forced size: frames, NEE frames, ray batches and the G-buffer (the three pre-pass instantiations, one per
    size class; the 2-spp frames run the same pre-pass and then start from its stored hits) equal brute force, the oracle and what
    the session's tracer renders at 1 024 threads."""
    tracer.reload_switches()
    names = ("small", "extras", "crowd1", "crowd2")
    for name in names:  # (the session's tracer at 1 024 threads, under the same checks)
        assert upload(tracer, name)["scene_block_threads"] == 1024
        check(tracer, name, ("frame", "nee", "rays", "gbuffer"), golden)
    env.setenv("FF_BLOCK_THREADS", str(block))
    with lib.Tracer(0) as t:
        for no_wn in (False, True):
            if no_wn:
                env.setenv("FF_NO_WORLD_NORMALS", "1")
                t.reload_switches()
            for name in names if not no_wn else names[:1]:
                assert upload(t, name)["scene_block_threads"] == block
                t.render(tc.camera(W, H, **SCENES[name][1]), P())
                assert f", {block}, " in t.kernel_name()
                check(t, name, ("frame", "nee", "rays", "gbuffer"), golden)


def test_pool_falls_back_to_the_lane_owned_kernel_below_1024_threads(env):
    """trace_pool_kernel is instantiated for 1 024 threads only, by design: FF_POOL=1 with FF_BLOCK_THREADS=512 runs the lane-owned kernel."""
    env.setenv("FF_POOL", "1")
    with lib.Tracer(0) as t:
        assert _name(t, "small", False) == "trace_pool_kernel<false, 1024, false>"
    env.setenv("FF_BLOCK_THREADS", "512")
    with lib.Tracer(0) as t:
        assert _name(t, "small", False) == "trace_bvh_kernel<false, 512, false, 0, false>"
        assert t.debug_layout()["scene_block_threads"] == 512
        check(t, "small", ("frame", "rays"))


# ---- b. chosen workgroup size ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deep", tc.DEEP_TREES, ids=[d.name for d in tc.DEEP_TREES])
def test_chosen_workgroup_size(env, deep):
    """No FF_BLOCK_THREADS: finalize_layout leaves 1 024 threads by itself for a tree whose lane-strided stacks do not fit.  The depth of
    each input was measured on an MI355X and must stay inside its band.  No input reaches the last band (79 levels or more: tests/
    traversal_cases.py lists the depths measured), so FF_ERR_UNSUPPORTED from render, ff_gbuffer and ff_intersect_rays on a tree too
    deep for 512 threads has no test here yet."""
    with lib.Tracer(0) as t:
        layout = upload_deep(t, env, deep)
        n = len(deep.scene())
        check_trees(t, n)
        _, table4 = t.download_bvh4(n)
        depth4 = int(table4[:, 2].max())
        print(f"{deep.name}: depth4 {depth4} (recorded {deep.measured_depth4}), layout {layout}")
        assert deep.band[0] <= depth4 <= deep.band[1], f"{deep.name}: depth4 {depth4} has left its band {deep.band}"
        assert layout["max_depth4"] == depth4 and layout["top_depth"] == 0 and layout["stack_entries"] == depth4 + 1
        assert layout["scene_block_threads"] == tc.expected_block(layout["stack_entries"], n) == deep.block
        cam = tc.camera(W, H, **tc.DEEP_CAMERA)
        t.render(cam, lib.render_params(W, H, 2, 1, seed=3))
        assert t.kernel_name().startswith(f"trace_bvh_kernel<false, {deep.block}, "), t.kernel_name()
        check(t, deep.name, ("frame", "nee", "rays", "gbuffer"))


def test_chosen_workgroup_size_512_with_many_records(env):
    """With three records no builder's tree is deep enough for finalize_layout's 512 choice (tests/traversal_cases.py lists the measured
    depths): the 768-band tree among 124 cubes reaches it, since 127 records and the geometry tree's own entries leave the stacks of
    512 threads only.  The forced-size tests above stay the only cover of 512 threads on small scenes and of size class 2."""
    with lib.Tracer(0) as t:
        layout = upload(t, "deep_crowd", builder_of("deep_crowd"))
        n = len(tc.deep_crowd_scene())
        assert n == 3 + tc.DEEP_CROWD_CUBES and 32 < n <= 128
        check_trees(t, n)
        print(f"deep_crowd: layout {layout}")
        lo, hi = tc.BANDS[768]
        assert lo <= layout["max_depth4"] <= hi and layout["top_depth"] > 0
        assert layout["stack_entries"] == layout["max_depth4"] + 1 + layout["top_depth"] + 1
        assert layout["scene_block_threads"] == tc.expected_block(layout["stack_entries"], n) == 512
        t.render(tc.camera(W, H, **tc.DEEP_CAMERA), lib.render_params(W, H, 2, 1, seed=3))
        assert t.kernel_name() == "trace_bvh_kernel<false, 512, true, 1, false>"
        check(t, "deep_crowd", ("frame", "nee", "rays", "gbuffer"))


def test_debug_exports_before_an_upload(env):
    """ff_debug_layout is an error before a scene is uploaded; ff_debug_stack_spill reports 0 words where there is no area."""
    with lib.Tracer(0) as t:
        with pytest.raises(lib.FireflyError) as e:
            t.debug_layout()
        assert e.value.status == T.FF_ERR_NO_SCENE and "ff_debug_layout" in e.value.message
        t.reset_stack_spill()
        assert t.stack_spill_words() == 0
        assert upload(t, "small")["scene_block_threads"] == 1024
