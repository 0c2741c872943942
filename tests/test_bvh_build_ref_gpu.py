"""The device BVH builder (cuda_pathtracer_amd/csrc/bvh_build.hip) against the numpy restatement of
BVH_tree.cpp (tests/bvh_build_ref.py), which shares no code with it: flattened nodes and triangle order
byte for byte on every case of tests/bvh_build_cases.py but the signed-zero pair (-0 cannot reach a
builder through the scene API: test_bvh_build_ref_cpu.py asserts it).  The cases aim at paths of
k_bvh_big and k_bvh_small that the random family of test_bvh_device_gpu.py does not visit on purpose;
each says which in bvh_build_cases.ARRAY_CASES.

Every case asserts where its build ran (Scene.bvh_build_info): a build the device hands back to the host
(bvh_build.hip's `err` bits) would make the comparison vacuous.  HOST_BUILT names the cases that are
expected on the host; there are none: the deepest task stack any case needs in k_bvh_small is 13 of 64
entries (replayed on the restated trees), no box holds a NaN and no split leaves a side empty."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import bvh_build_cases as K
import bvh_build_ref as R

pytestmark = pytest.mark.gpu

DEVICE_ARRAY_CASES = [c for c in K.ARRAY_CASES if c not in K.SIGNED_ZERO]
HOST_BUILT = ()      # cases bvh_build.hip hands to the host build


@functools.lru_cache(maxsize=None)
def _ref(name):
    return R.build(K.vertices(name))


def _assert_device_equals_ref(name, scene, v, ref_nodes, ref_order):
    on_device, ms = scene.bvh_build_info()
    assert on_device == (name not in HOST_BUILT), \
        f"{name}: built on the {'device' if on_device else 'host'}, expected the other"
    tris, nodes = K.tables(scene, R.NODE_DTYPE)
    assert nodes.tobytes() == ref_nodes.tobytes(), f"{name}: device vs restatement: {R.first_difference(nodes, ref_nodes)}"
    order = tris["id"].astype(np.int64)
    assert np.array_equal(order, ref_order), \
        f"{name}: triangle order differs first at position {int(np.flatnonzero(order != ref_order)[0])}"
    assert tris["v"].tobytes() == v[ref_order].tobytes(), f"{name}: reordered vertices differ"
    print(f"{name}: {len(v)} triangles, {len(nodes)} nodes, built on the "
          f"{'device' if on_device else 'host'} in {ms:.2f} ms")


@pytest.mark.parametrize("name", DEVICE_ARRAY_CASES)
def test_device_build_equals_restatement(gpu_device, name):
    v = K.vertices(name)
    _assert_device_equals_ref(name, K.api_scene(v, device=True), v, *_ref(name))


@pytest.mark.parametrize("name", list(K.FILE_CASES))
def test_device_build_of_scene_file_equals_restatement(gpu_device, name, tmp_path):
    from cuda_pathtracer_amd import Scene
    path = K.scene_file(name, tmp_path)
    host_tris, _ = K.tables(Scene(path), R.NODE_DTYPE)
    v = K.load_order(host_tris)              # the world vertices in load order, from the host scene
    _assert_device_equals_ref(name, Scene(path, device_bvh=True), v, *R.build(v))


def test_repeated_device_builds_are_identical(gpu_device):
    """alloc_pair hands out node ids by atomicAdd and the task lists fill in any order; the flattening
    hides both: three builds of one scene in one process give the same bytes."""
    v = K.vertices("adv4097")
    ref_nodes, ref_order = _ref("adv4097")
    for k in range(3):
        _assert_device_equals_ref("adv4097", K.api_scene(v, device=True), v, ref_nodes, ref_order)


WORKGROUP_CAP = 4096     # k_bvh_big's launch: min(ranges of the level, 4096) workgroups, a stride loop over the rest


def _small_triangles(n):
    rng = np.random.default_rng(n)
    centre = rng.uniform(-4.0, 4.0, size=(n, 1, 3))
    return (centre + rng.normal(0.0, 0.01, size=(n, 3, 3))).astype(np.float32)


@pytest.mark.slow
def test_more_big_ranges_on_a_level_than_workgroups(gpu_device):
    """The smallest of three random meshes whose HOST tree has more than 4096 ranges of more than 128
    triangles on one level, so that k_bvh_big's workgroups loop over tasks; the count is asserted, so the cap
    is known to be crossed.  Compared with the host build only (the restatement would take minutes)."""
    for n in (1_300_000, 1_500_000, 1_800_000):
        v = _small_triangles(n)
        host = K.api_scene(v)
        assert not host.bvh_build_info()[0]
        host_tris, host_nodes = K.tables(host, R.NODE_DTYPE)
        fullest = int(K.level_counts(host_nodes).max())
        print(f"{n} triangles: {len(host_nodes)} nodes, fullest level {fullest} big ranges")
        if fullest > WORKGROUP_CAP:
            break
    assert fullest > WORKGROUP_CAP, f"no candidate crosses the cap: {fullest}"
    del host
    dev = K.api_scene(v, device=True)
    on_device, ms = dev.bvh_build_info()
    assert on_device, "the device build was handed to the host"
    dev_tris, dev_nodes = K.tables(dev, R.NODE_DTYPE)
    assert dev_nodes.tobytes() == host_nodes.tobytes(), f"device vs host: {R.first_difference(dev_nodes, host_nodes)}"
    assert dev_tris.tobytes() == host_tris.tobytes(), "triangle order differs"
    print(f"{n} triangles on the device: {ms:.1f} ms")
