"""Scenes and host arithmetic of tests/test_gpu_traversal_configs.py: the configurations of the BVH traversal code that the layout
(csrc/ff_scene_api.cpp finalize_layout, bvh_block_threads) and the experiment switches choose - workgroup size, stack residency,
node residency and time slice.  Nothing here needs a GPU (tests/test_traversal_cases_host.py)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_parity as fz  # noqa: E402
from cases import build_case  # noqa: E402
from gpupathtracer_amd import lib, scenes  # noqa: E402
from gpupathtracer_amd import types as T  # noqa: E402

# ---- bvh_block_threads, restated ---------------------------------------------------------------------------------------------------------
LDS_BUDGET_BYTES = 160 * 1024   # csrc/ff_kernels.h kLdsBudgetBytes
STACK_ENTRY_BYTES = 4           # one traversal-stack entry of one lane
RECORD_BYTES = 288              # one geometry record in LDS (sizeof(GeomRecord))
NODE_BYTES = 112                # one 4-wide node (sizeof(Bvh4Node))
MIN_LDS_STACK = 4               # finalize_layout kMinLdsStack
BLOCK_SIZES = (1024, 768, 512)  # the instantiated workgroup sizes of trace_bvh_kernel


def expected_block(stack_entries, records, preferred=1024):
    """The workgroup size finalize_layout picks: the largest instantiated size up to `preferred` whose lane-strided stacks
    (stack_entries x 4 bytes x size) and `records` geometry records fit the 160 KiB of LDS; 0 if not even 512 threads do."""
    for block in BLOCK_SIZES:
        if block <= preferred and stack_entries * STACK_ENTRY_BYTES * block + records * RECORD_BYTES <= LDS_BUDGET_BYTES:
            return block
    return 0


def expected_lds_levels(nodes, stack_entries, records, block):
    """How many of a lane's stack entries finalize_layout keeps in LDS on a scene of up to 32 geometries whose trees have `nodes`
    4-wide nodes: all of them if the nodes fit beside them or do not fit beside four either; else as many (at least four) as leave
    room for every node.  The deeper entries go to the global spill area."""
    def fit(levels):
        return max(0, LDS_BUDGET_BYTES - records * RECORD_BYTES - levels * STACK_ENTRY_BYTES * block) // NODE_BYTES
    levels = stack_entries
    while levels > MIN_LDS_STACK and fit(levels) < nodes:
        levels -= 1
    return levels if fit(levels) >= nodes else stack_entries


# The depth bands of a scene of three records and no geometry tree (stack_entries = depth4 + 1), from the arithmetic above:
# 39 entries are the last that fit 1024 threads, 53 the last for 768, 79 the last for 512.
BANDS = {768: (39, 52), 512: (53, 78), 0: (79, 10 ** 6)}

# ---- the shared small inputs -------------------------------------------------------------------------------------------------------------
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
SMALL_GOLDEN = "path_cornell_96x64_b4_s4"   # cases of tests/cases.py whose oracle frames are in tests/golden/frames.npz:
EXTRAS_GOLDEN = "path_mirror_80x60_b6_s3"   # the small diffuse scene and the scene with extras
CROWD_CLASS1, CROWD_CLASS2 = 80, 500        # tools/fuzz_parity.py rand_scene crowds of size class 1 (33-128 records) and 2 (more)


@functools.lru_cache(maxsize=None)
def small_scene():
    return scenes.cornell_wahoo_scene()


@functools.lru_cache(maxsize=None)
def extras_scene():
    return scenes.cornell_mirror_scene()


@functools.lru_cache(maxsize=None)
def crowd_scene(crowd):
    """The crowds of tests/test_gpu_kernel_names.py."""
    scene = fz.rand_scene(np.random.default_rng(3), small=True, crowd=crowd)
    assert (32 < len(scene) <= 128) if crowd == CROWD_CLASS1 else len(scene) > 128
    return scene


# What fills LDS to within a few stack levels at each workgroup size: C2 (1 202 nodes, 10 stack entries) plus these small meshes
# (sphere.obj has 67 nodes, cube.obj 2).  Measured on an MI355X: entries kept in LDS, then the words of the spill area written by a
# 48 x 32 frame / the G-buffer's pre-pass / an NEE frame / a batch of 3 000 rays.
SPILL_EXTRAS = {
    1024: (("sphere", 1),),                # 4 of 10 in LDS: 96 / 36 / 433 / 36
    768: (("sphere", 1), ("cube", 10)),    # 4 of 10 in LDS: 88 / 34 / 402 / 32
    512: (("sphere", 2),),                 # 5 of 10 in LDS: 18 / 8 / 80 / 10
}


@functools.lru_cache(maxsize=None)
def spill_scene(block):
    """C2 with SPILL_EXTRAS[block] scattered in the box: at `block` threads its trees fit LDS only beside four or five stack levels, so
    every launch on it writes spilled entries."""
    rng = np.random.default_rng(7)
    s = scenes.Scene()
    s.add_mesh(scenes.load_mesh("wahoo"), (0, -2.4, 0), (0, 0, 0), (0.28, 0.28, 0.28), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 0, 0)))
    s.add_mesh(scenes.load_mesh("cube"), (1.5, -2.0, 1.0), (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.75, 0.75, 0.75)))
    grey = scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.6, 0.6, 0.6))
    for name, count in SPILL_EXTRAS[block]:
        for _ in range(count):
            s.add_mesh(scenes.load_mesh(name), tuple(rng.uniform(-2.0, 2.0, 3)), tuple(rng.uniform(-180, 180, 3)), (0.3, 0.3, 0.3), grey)
    return scenes._box(s).finalize()


@functools.lru_cache(maxsize=None)
def golden_case(name):
    return build_case(name)


def camera(w, h, **pose):
    return scenes.posed_camera(w, h, **(pose or INSIDE))


def ray_batch(n=3000, seed=5, origin=(0.0, 0.0, 2.4), spread=1.5):
    """n world-space rays from within `spread` of `origin` in every direction: (origins, directions) float32 [n, 3].  Three partial-to-full
    workgroups of the ray-batch kernel at the default n."""
    rng = np.random.default_rng(seed)
    o = (np.asarray(origin) + rng.uniform(-spread, spread, size=(n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


# ---- deep trees --------------------------------------------------------------------------------------------------------------------------
DEEP_CAMERA = dict(position=(0.0, 0.3, 4.0), yaw=-90.0, pitch=0.0)
DEEP_RECORDS = 3  # the mesh and two planes


def deep_tree_triangles(count, period, seed=3):
    """The geometric cluster of tests/test_gpu_dynamic.py test_clustered_mesh_gives_a_deep_tree_that_still_renders (count = 1500,
    period = 25 there): triangle i sits at 2^-(i / period) of the way out, its size shrinks with it, so every split of a
    top-down builder peels a few triangles off one end and a bottom-up builder chains them.  float32 [count, 24]."""
    rng = np.random.default_rng(seed)
    i = np.arange(count)
    tris = np.zeros((count, 24), dtype=np.float32)
    centre = np.stack([2.0 ** -(i / period), 0.7 * 2.0 ** -(i / (1.24 * period)), 0.4 * 2.0 ** -(i / (0.76 * period))], axis=1)
    size = 0.02 * 2.0 ** -(i / period)
    for v in range(3):
        tris[:, 3 * v:3 * v + 3] = (centre + rng.normal(size=(count, 3)) * size[:, None]).astype(np.float32)
    return tris


def deep_tree_scene(count, period, seed=3):
    red = scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.8, 0.3, 0.2))
    light = scenes.make_bxdf(T.BXDF_EMITTER, emissive=(1, 1, 1), intensity=2.0)
    scene = scenes.Scene().add_mesh(deep_tree_triangles(count, period, seed), (-1.0, -0.5, 0.0), (0, 30, 0), (3, 3, 3), red) \
        .add_plane((0, 0, -2.5), (0, 0, 0), (8, 8, 8), red).add_plane((0, 3, 0), (90, 0, 0), (8, 8, 8), light).finalize()
    assert len(scene) == DEEP_RECORDS
    return scene


class DeepTree:
    """One input of the chosen-workgroup-size tests: generator parameters, device builder, builder switches (environment, read at
    the upload), the workgroup size finalize_layout must choose for it, and the depth of the 4-wide tree measured on an MI355X."""

    def __init__(self, name, count, period, builder, env, block, measured_depth4):
        self.name, self.count, self.period, self.builder, self.env = name, count, period, builder, dict(env)
        self.block, self.measured_depth4 = block, measured_depth4

    @property
    def band(self):
        return BANDS[self.block] if self.block in BANDS else (self.measured_depth4, 38)  # (the 1 024-thread input sits AT the edge)

    def scene(self):
        return deep_tree_scene(self.count, self.period)


BUILDER_SWITCHES = ("FF_TREELET_PASSES", "FF_GPU_REINSERT", "FF_COLLAPSE_PARITY", "FF_GPU_LEAF")

# name, triangles, period, builder, switches, chosen workgroup size, measured depth4 (MI355X)
DEEP_TREES = [
    # the deepest tree that still fits 1 024 threads: 39 stack entries
    DeepTree("lbvh_1024_edge", 700, 8, T.BUILD_GPU_LBVH, {}, 1024, 38),
    DeepTree("lbvh_768", 2200, 25, T.BUILD_GPU_LBVH, {}, 768, 41),
]
DEEP_BY_NAME = {d.name: d for d in DEEP_TREES}
# Depths measured on the same MI355X for the other inputs tried (counts 60 .. 9 000, periods 2 .. 60, both device builders, with
# FF_TREELET_PASSES 0 / 8, FF_GPU_REINSERT 0 / 16 / 64, FF_COLLAPSE_PARITY, FF_GPU_LEAF=1, FF_PLOC_RADIUS=1): LBVH at most 45 (9 000
# triangles, period 60), PLOC at most 46 (600 triangles, period 2); without the optimisation passes 19 (LBVH) and 36 (PLOC).  No
# input reaches 53 levels: with three records the 512-thread and the unsupported choices are out of every builder's reach.

DEEP_CROWD_CUBES = 124


@functools.lru_cache(maxsize=None)
def deep_crowd_scene():
    """The 768-band tree among 124 small cubes: 127 records (size class 1, 36 576 bytes of LDS) and the walk through the tree over
    them leave 512 threads as the only size whose stacks fit - finalize_layout's 512 choice, reached without FF_BLOCK_THREADS."""
    deep = DEEP_BY_NAME["lbvh_768"]
    rng = np.random.default_rng(11)
    red = scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.8, 0.3, 0.2))
    grey = scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.6, 0.6, 0.6))
    light = scenes.make_bxdf(T.BXDF_EMITTER, emissive=(1, 1, 1), intensity=2.0)
    s = scenes.Scene().add_mesh(deep_tree_triangles(deep.count, deep.period), (-1.0, -0.5, 0.0), (0, 30, 0), (3, 3, 3), red)
    s.add_plane((0, 0, -2.5), (0, 0, 0), (8, 8, 8), red).add_plane((0, 3, 0), (90, 0, 0), (8, 8, 8), light)
    cube = scenes.load_mesh("cube")
    for _ in range(DEEP_CROWD_CUBES):
        s.add_mesh(cube, tuple(rng.uniform(-2.5, 2.5, 3)), tuple(rng.uniform(-180, 180, 3)), (0.15, 0.15, 0.15), grey)
    return s.finalize()
