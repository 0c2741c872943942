"""The analytic bounce kernels' wave-owned segments against the CPU oracle.

Workgroup b of a launch owns tpb whole 256-path tiles of one iteration; its wave w owns the w-th
quarter of that range (tpb wave-tiles of 64 paths) and writes its survivors in order from
out[b * chunk + w * chunk / 4].  The next launch maps logical survivor i through the segment words
(one per workgroup) and the four wave counts beside each.  Default flags throughout: the shading
key is the index within the iteration's compacted array, so any slip in the order changes the
image, and `bounce_live` must equal the oracle's counts.  At these sizes tpb is 1: a segment holds
at most 256 paths and a sub-segment at most 64.

What each case reaches:
  * 35 pixels: less than one wave-tile per iteration — waves 1-3 of every workgroup own nothing
    (all-zero wave counts but the first) and wave 0's only tile is partial; spp 1 runs the SPP1
    instantiations, spp 5 the batched ones.
  * 264 pixels: four whole wave-tiles plus 8 paths — `last` cuts inside wave 0 of an iteration's
    second workgroup.
  * sparse survivors (far camera): ~19 (or ~48) survivors per iteration out of 3072 camera paths,
    so almost every sub-segment is empty and a later bounce's wave-tile gathers its 64 paths from
    many sub-segments of several segments (the mapping's loop over segments, empty segments
    skipped); with 64 iterations some iterations have no survivor at the deep bounces.
  * odd width and shards: 50 x 37 over world 3 — row counts and iteration sizes that are no
    multiple of 64 in every rank.
  * 256 iterations of 120 pixels: the `grid - spp` corner of the layout (one workgroup per
    iteration, every iteration's last tile partial), on one and two lanes.
  * one pass of 8 iterations equals two passes of 4: the layout does not depend on how the
    iterations are batched.
"""
import numpy as np
import pytest

from oracle import binding as O

pytestmark = pytest.mark.gpu

NEAR = (0, 5, 10.5)
FAR = (0, 5, 60.0)
MID = (0, 5, 40.0)


def _view(cornell_path, res, eye):
    from cuda_pathtracer_amd import Scene
    s = Scene(cornell_path)
    s.set_camera(res, 45.0, eye, (0, 5, 0), (0, 1, 0))
    s.finalize()
    o = O.OracleScene.from_json(cornell_path)
    o.set_camera(res, 45.0, eye, (0, 5, 0), (0, 1, 0))
    return s, o


def _gui():
    from cuda_pathtracer_amd import GuiDataContainer
    return GuiDataContainer()


def _oflags(g):
    return O.flags(g.russianRoulette, g.useBVHtree, g.useBBox, g.sortbyMaterial, g.useThrustPartition, g.SSAA,
                   g.DoF, g.aperture, g.focal_len, g.singleAlbedo, g.rngKeyPixel)


def _gpu(scene, passes, spp, rank=0, world=1):
    """Image and bounce_live after passes of `spp` iterations starting at the iterations `passes`."""
    from cuda_pathtracer_amd import PathTracer
    pt = PathTracer(scene, _gui(), rank=rank, world=world, spp=spp)
    for it in passes:
        pt.render_pass(it)
    img, live = pt.image(), pt.stats()["bounce_live"]
    pt.free()
    return img, live


def _oracle(oscene, passes, spp, rank=0, world=1):
    img, total = None, [0] * oscene.depth
    for it in passes:
        img, live = O.render_pass(oscene, _oflags(_gui()), it, spp=spp, rank=rank, world=world, image=img)
        total = [a + b for a, b in zip(total, live)]
    return img, total


def _assert_bitexact(gpu, ref, what):
    g, r = np.asarray(gpu, np.float32), np.asarray(ref, np.float32)
    assert g.shape == r.shape, what
    bad = np.argwhere(~((g == r) | (np.isnan(g) & np.isnan(r))))
    assert bad.size == 0, f"{what}: {len(bad)} mismatching values, first at {bad[:3].tolist()}"


def _check(scene, oscene, passes, spp, what, want_live=None, **shard):
    g, glive = _gpu(scene, passes, spp, **shard)
    r, rlive = _oracle(oscene, passes, spp, **shard)
    if want_live is not None:   # the view is the one the case was chosen for
        assert rlive[:len(want_live)] == want_live, what
    _assert_bitexact(g, r, what)
    assert glive == rlive, what
    return g, glive


@pytest.mark.parametrize("spp,passes,want", [
    (1, range(1, 9), [280, 159, 111, 87, 20, 13, 11, 6]),
    (5, (1, 6), None),
])
def test_less_than_one_wave_tile(cornell_path, spp, passes, want):
    s, o = _view(cornell_path, (7, 5), NEAR)
    _check(s, o, list(passes), spp, f"35 pixels spp {spp}", want)


def test_last_cuts_inside_wave_0(cornell_path):
    s, o = _view(cornell_path, (24, 11), NEAR)
    _check(s, o, [1, 4, 7], 3, "264 pixels spp 3")


@pytest.mark.parametrize("eye,spp,want", [
    (FAR, 8, [24576, 154, 127, 97, 20, 17, 11, 6]),
    (MID, 8, [24576, 385, 312]),
    (FAR, 64, None),
    (MID, 64, None),
])
def test_sparse_survivors(cornell_path, eye, spp, want):
    s, o = _view(cornell_path, (64, 48), eye)
    _check(s, o, [1], spp, f"sparse eye {eye} spp {spp}", want)


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_odd_width_shards(cornell_path, rank):
    s, o = _view(cornell_path, (50, 37), NEAR)
    _check(s, o, [1], 4, f"50x37 rank {rank} of 3", rank=rank, world=3)


@pytest.fixture(scope="module")
def ref_256(cornell_path):
    _, o = _view(cornell_path, (12, 10), NEAR)
    return _oracle(o, [1], 256)


@pytest.mark.parametrize("lanes", [None, "1", "2"])
def test_256_iterations(cornell_path, monkeypatch, ref_256, lanes):
    if lanes is None:
        monkeypatch.delenv("PT_AMD_LANES", raising=False)
    else:
        monkeypatch.setenv("PT_AMD_LANES", lanes)
    s, _ = _view(cornell_path, (12, 10), NEAR)
    g, glive = _gpu(s, [1], 256)
    _assert_bitexact(g, ref_256[0], f"256 iterations, lanes {lanes}")
    assert glive == ref_256[1]


def test_one_pass_equals_its_halves(cornell_path):
    s, o = _view(cornell_path, (64, 48), FAR)
    whole, wlive = _check(s, o, [1], 8, "one pass of 8")
    halves, hlive = _gpu(s, [1, 5], 4)
    _assert_bitexact(halves, whole, "two passes of 4 vs one of 8")
    assert hlive == wlive
