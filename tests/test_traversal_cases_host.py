"""Host checks of tests/traversal_cases.py (no GPU): the workgroup-size arithmetic at the edges of its bands, and the deep-tree
generator."""
import ctypes as C
import os
import re

import numpy as np

import traversal_cases as tc
from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expected_block_at_the_band_edges():
    """Three records (864 bytes) leave 162 976 bytes for the stacks: 39 entries x 4 096 bytes fit and 40 do not; at 768 threads 53 x
    3 072 fit and 54 do not; at 512 threads 79 x 2 048 fit and 80 do not."""
    for entries, block in [(1, 1024), (39, 1024), (40, 768), (53, 768), (54, 512), (79, 512), (80, 0), (500, 0)]:
        assert tc.expected_block(entries, 3) == block, entries
    # a preferred size below 1 024 (FF_BLOCK_THREADS) caps the choice, and is refused no later
    assert [tc.expected_block(e, 3, 768) for e in (39, 53, 54, 80)] == [768, 768, 512, 0]
    assert [tc.expected_block(e, 3, 512) for e in (39, 79, 80)] == [512, 512, 0]
    # 128 records (a full class-1 scene, 36 864 bytes) move every edge down; records read from global memory (class 2) cost nothing
    assert [tc.expected_block(e, 128) for e in (31, 32, 41, 42, 62, 63)] == [1024, 768, 768, 512, 512, 0]
    assert tc.expected_block(40, 0) == 1024 and tc.expected_block(41, 0) == 768
    # the bands are these edges, for stack_entries = depth4 + 1
    for block, (lo, hi) in tc.BANDS.items():
        assert tc.expected_block(lo + 1, tc.DEEP_RECORDS) == block and tc.expected_block(lo, tc.DEEP_RECORDS) != block
        assert tc.expected_block(min(hi, 400) + 1, tc.DEEP_RECORDS) == block


def test_expected_lds_levels_at_the_measured_layouts():
    """(nodes, entries, records, block) -> entries in LDS, as ff_debug_layout reported them on an MI355X; and the edges by hand: at 512
    threads and 10 records five levels leave (163 840 - 2 880 - 10 240) / 112 = 1 345 nodes, six leave 1 327."""
    for args, levels in [((1202, 10, 8, 1024), 6), ((1202, 10, 8, 768), 8), ((1202, 10, 8, 512), 10), ((1269, 10, 9, 1024), 4),
                         ((1289, 10, 19, 768), 4), ((1336, 10, 10, 512), 5), ((594, 42, 3, 768), 31), ((189, 39, 3, 1024), 34)]:
        assert tc.expected_lds_levels(*args) == levels, args
    assert [tc.expected_lds_levels(n, 10, 10, 512) for n in (1254, 1255, 1327, 1328, 1345, 1346, 1364, 1365)] == [10, 9, 6, 5, 5, 4, 4, 10]
    for block, extras in tc.SPILL_EXTRAS.items():
        assert len(tc.spill_scene(block)) == 8 + sum(c for _, c in extras) <= 32


def test_the_new_debug_exports_refuse_null_arguments(ff):
    handle = ff.load()
    buf, n = (C.c_int * 8)(), C.c_ulonglong(7)
    assert handle.ff_debug_layout(None, buf) == T.FF_ERR_INVALID_ARG and "ff_debug_layout" in handle.ff_last_error().decode()
    assert handle.ff_debug_stack_spill(None, 0, C.byref(n)) == T.FF_ERR_INVALID_ARG and "ff_debug_stack_spill" in handle.ff_last_error().decode()
    assert handle.ff_debug_stack_spill(None, 1, None) == T.FF_ERR_INVALID_ARG


def test_the_constants_are_the_library_s():
    src = open(os.path.join(ROOT, "gpupathtracer_amd", "csrc", "ff_kernels.h")).read()
    assert re.search(r"kLdsBudgetBytes\s*=\s*160\s*\*\s*1024\s*;", src) and tc.LDS_BUDGET_BYTES == 160 * 1024
    assert re.search(r"kMaxLdsRecords\s*=\s*128\s*;", src)
    table = open(os.path.join(ROOT, "gpupathtracer_amd", "csrc", "ff_kernels.hip")).read()
    assert "FF_TRACE_BVH_KERNELS_OF(X, 512) FF_TRACE_BVH_KERNELS_OF(X, 768) FF_TRACE_BVH_KERNELS_OF(X, 1024)" in table
    assert tc.BLOCK_SIZES == (1024, 768, 512)
    assert lib.LAYOUT_FIELDS[:3] == ("scene_block_threads", "stack_entries", "stack_lds_levels") and len(lib.LAYOUT_FIELDS) == 8


def test_deep_tree_generator_is_deterministic_and_is_the_clustered_mesh():
    a, b = tc.deep_tree_triangles(300, 25), tc.deep_tree_triangles(300, 25)
    assert a.dtype == np.float32 and a.shape == (300, 24) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, tc.deep_tree_triangles(300, 25, seed=4)) and not np.array_equal(a[:, :9], tc.deep_tree_triangles(300, 8)[:, :9])
    # count = 1500, period = 25: the mesh of tests/test_gpu_dynamic.py test_clustered_mesh_gives_a_deep_tree_that_still_renders
    rng = np.random.default_rng(3)
    n = 1500
    want = np.zeros((n, 24), dtype=np.float32)
    centre = np.stack([2.0 ** -(np.arange(n) / 25.0), 0.7 * 2.0 ** -(np.arange(n) / 31.0), 0.4 * 2.0 ** -(np.arange(n) / 19.0)], axis=1)
    size = 0.02 * 2.0 ** -(np.arange(n) / 25.0)
    for v in range(3):
        want[:, 3 * v:3 * v + 3] = (centre + rng.normal(size=(n, 3)) * size[:, None]).astype(np.float32)
    assert np.array_equal(tc.deep_tree_triangles(n, 25).view(np.uint32), want.view(np.uint32))
    for d in tc.DEEP_TREES:
        tris = tc.deep_tree_triangles(d.count, d.period)
        assert np.isfinite(tris).all() and len(d.scene()) == tc.DEEP_RECORDS
        assert d.band[0] <= d.measured_depth4 <= d.band[1], d.name
        assert tc.expected_block(d.measured_depth4 + 1, tc.DEEP_RECORDS) == d.block, d.name
    assert len({d.name for d in tc.DEEP_TREES}) == len(tc.DEEP_TREES)


def test_ray_batch_is_deterministic_unit_length_and_spans_three_workgroups():
    o, d = tc.ray_batch()
    o2, d2 = tc.ray_batch()
    assert np.array_equal(o, o2) and np.array_equal(d, d2) and o.shape == d.shape == (3000, 3) and o.dtype == d.dtype == np.float32
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert 5 * 512 < len(o) < 6 * 512  # a last, partial workgroup of the 512-thread ray-batch kernel
