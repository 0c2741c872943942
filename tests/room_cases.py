"""The room cases shared by tests/test_room_bound_gpu.py (contexts on the GPU, against the oracle) and
tests/test_room_bound_cpu.py (the host's scene preparation alone): the scenes, their flags and the
walls the host is expected to group.  The builders take any scene object with add_material /
add_geom / set_camera: the product's Scene or the oracle's."""
import numpy as np
import pytest

SPP, PASSES, DEPTH = 4, 2, 8
EYE, LOOK = (0, 5, 10.5), (0, 5, 0)


def _materials(sc):
    return dict(light=sc.add_material(rgb=(1, 1, 1), emittance=5.0),
                white=sc.add_material(rgb=(0.98, 0.98, 0.98)),
                red=sc.add_material(rgb=(0.85, 0.35, 0.35)),
                green=sc.add_material(rgb=(0.35, 0.85, 0.35)),
                mirror=sc.add_material(rgb=(0.98, 0.98, 0.98), specrgb=(0.98, 0.98, 0.98), reflective=1.0),
                glass=sc.add_material(rgb=(0.98, 0.98, 0.98), specrgb=(0.98, 0.98, 0.98), refractive=1.0, ior=1.5))


def _shell(sc, m, left=True):
    """cornell.json's shell: light, floor, ceiling (rotated 90 degrees), back (rotated), right, left."""
    from cuda_pathtracer_amd import CUBE
    sc.add_geom(CUBE, m["light"], (0, 10, 0), (0, 0, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m["white"], (0, 0, 0), (0, 0, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], (0, 10, 0), (0, 0, 90), (0.01, 10, 10))
    sc.add_geom(CUBE, m["white"], (0, 5, -5), (0, 90, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["green"], (5, 5, 0), (0, 0, 0), (0.01, 10, 10))
    if left:
        sc.add_geom(CUBE, m["red"], (-5, 5, 0), (0, 0, 0), (0.01, 10, 10))


def _inside_aperture(sc):
    """Camera inside the room, wide lens: ray origins all over the room, close to the walls."""
    from cuda_pathtracer_amd import SPHERE
    m = _materials(sc)
    _shell(sc, m)
    sc.add_geom(SPHERE, m["mirror"], (-1, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera((56, 48), 70.0, (3.5, 1.0, 3.5), (-2, 4, -3), (0, 1, 0))


def _axis_parallel(sc):
    """A closed room (six walls, none rotated, so their normals are exact axes) seen along -z from
    inside, no jitter and no lens: the camera's view and up vectors have x == +-0, so the centre column
    of pixels has d_x == +-0 exactly, and the mirror back wall, front wall and floor keep that zero
    through the later bounces."""
    from cuda_pathtracer_amd import CUBE
    m = _materials(sc)
    sc.add_geom(CUBE, m["light"], (0, 10, 0), (0, 0, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m["mirror"], (0, 0, 0), (0, 0, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], (0, 10, 0), (0, 0, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["mirror"], (0, 5, -5), (0, 0, 0), (10, 10, 0.01))
    sc.add_geom(CUBE, m["red"], (-5, 5, 0), (0, 0, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["green"], (5, 5, 0), (0, 0, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["mirror"], (0, 5, 5), (0, 0, 0), (10, 10, 0.01))
    sc.set_camera((48, 48), 40.0, (0, 4, 4), (0, 4, 0), (0, 1, 0))


def _window(sc):
    """The left wall as two half-walls with a gap between them: neither covers its face, so the host
    leaves the -x face without a wall (four walls where cornell.json has five) and the half-walls stay
    in the loop; rays leave through the gap and come back from a sphere behind it."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    _shell(sc, m, left=False)
    sc.add_geom(CUBE, m["red"], (-5, 5, -3), (0, 0, 0), (0.01, 10, 4))
    sc.add_geom(CUBE, m["red"], (-5, 5, 3), (0, 0, 0), (0.01, 10, 4))
    sc.add_geom(SPHERE, m["white"], (-8, 4, 0), (0, 0, 0), (3, 3, 3))   # seen through the gap
    sc.set_camera((64, 48), 35.0, (3, 4, 9), (-5, 4, 0), (0, 1, 0))


def _outside(sc):
    """Surfaces outside the room's box: a sphere in front of the open face, a rotated and an axis-aligned
    cube that straddle the right wall, and the wall's own outer side, all in view of a camera beside
    the room — their rays start outside."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    _shell(sc, m)
    sc.add_geom(SPHERE, m["mirror"], (2, 3, 7.5), (0, 0, 0), (3, 3, 3))
    sc.add_geom(CUBE, m["white"], (5, 3, 3), (0, 30, 0), (2.5, 2.5, 2.5))
    sc.add_geom(CUBE, m["red"], (5, 7, 4), (0, 0, 0), (2, 2, 2))
    sc.set_camera((64, 48), 35.0, (11, 6, 13), (5, 4, 2), (0, 1, 0))


def _coplanar_floor(sc):
    """Ties between a grouped wall and a wall of the loop: a smaller tile with the floor's top plane
    before the floor in index order, and an exact duplicate of the floor after it."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    sc.add_geom(CUBE, m["red"], (0, 0, 0), (0, 0, 0), (6, 0.01, 6))
    _shell(sc, m)
    sc.add_geom(CUBE, m["green"], (0, 0, 0), (0, 0, 0), (10, 0.01, 10))
    sc.add_geom(SPHERE, m["mirror"], (-1, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera((56, 48), 45.0, EYE, LOOK, (0, 1, 0))


def _glass_cube(sc):
    """Glass cubes inside the room, one axis-aligned (a world-box cube of the loop) and one rotated:
    rays that start inside the glass, and NaN directions after total internal reflection."""
    from cuda_pathtracer_amd import CUBE
    m = _materials(sc)
    _shell(sc, m)
    sc.add_geom(CUBE, m["glass"], (-2, 2.5, 0), (0, 0, 0), (3, 3, 3))
    sc.add_geom(CUBE, m["glass"], (2.2, 3, 1), (20, 35, 10), (2.5, 2.5, 2.5))
    sc.set_camera((56, 48), 45.0, EYE, LOOK, (0, 1, 0))


def _two_walls(sc):
    """No room, inside the bounded pass's table: the shell with its ceiling, left and right walls
    tilted by 5 degrees (oriented cubes).  The floor and the back wall are the only candidates that
    cover a face; the light is the candidate of +y and is dropped because it does not cover it; two
    walls are not a room.  The bounds pass runs with room_n == 0."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    sc.add_geom(CUBE, m["light"], (0, 10, 0), (0, 0, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m["white"], (0, 0, 0), (0, 0, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], (0, 10, 0), (0, 0, 95), (0.01, 10, 10))
    sc.add_geom(CUBE, m["white"], (0, 5, -5), (0, 90, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["green"], (5, 5, 0), (0, 5, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["red"], (-5, 5, 0), (0, -5, 0), (0.01, 10, 10))
    sc.add_geom(SPHERE, m["mirror"], (-1, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera((56, 48), 45.0, EYE, LOOK, (0, 1, 0))


def _rotated_shell(sc):
    """No room and no world-box cube at all: the whole shell, light included, turned by 30 degrees
    about the y axis, so every cube is an oriented one."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    c, s = 0.8660254, 0.5   # (x, z) -> (c x + s z, -s x + c z): glm's rotation about y by 30 degrees
    def at(x, y, z):
        return (c * x + s * z, y, -s * x + c * z)
    sc.add_geom(CUBE, m["light"], at(0, 10, 0), (0, 30, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m["white"], at(0, 0, 0), (0, 30, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], at(0, 10, 0), (0, 30, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], at(0, 5, -5), (0, 30, 0), (10, 10, 0.01))
    sc.add_geom(CUBE, m["green"], at(5, 5, 0), (0, 30, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["red"], at(-5, 5, 0), (0, 30, 0), (0.01, 10, 10))
    sc.add_geom(SPHERE, m["mirror"], at(-1, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera((56, 48), 45.0, EYE, LOOK, (0, 1, 0))


# name -> (builder or generator arguments, flags, expected faces (-x, +x, -y, +y, -z, +z) or wall count)
CASES = {
    "cornell": (None, dict(), [4, 5, 1, 2, 3, -1]),
    "inside_aperture": (_inside_aperture, dict(aperture=2.0, focal_len=4.0), [5, 4, 1, 2, 3, -1]),
    "axis_parallel": (_axis_parallel, dict(SSAA=False, DoF=False), [4, 5, 1, 2, 3, 6]),
    "window": (_window, dict(), [-1, 4, 1, 2, 3, -1]),
    "outside": (_outside, dict(), [5, 4, 1, 2, 3, -1]),
    "coplanar_floor": (_coplanar_floor, dict(), [6, 5, 2, 3, 4, -1]),
    "glass_cube": (_glass_cube, dict(), [5, 4, 1, 2, 3, -1]),
    "two_walls": (_two_walls, dict(), 0),
    "rotated_shell": (_rotated_shell, dict(), 0),
    # more geoms than the bounded pass takes (its table and tags hold 32): the plain loop, no room
    "random_primitives": (dict(n=30, seed=11), dict(), 0),
    # the same stress scene within the table: the shell is a room among rotated, overlapping primitives
    "random_primitives_room": (dict(n=20, seed=12), dict(), [4, 5, 1, 2, 3, -1]),
}


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("room_scenes")


def scene_path(name, scene_dir, cornell_path):
    """The JSON file of a case that has one (cornell.json or a generated stress scene), else None."""
    from cuda_pathtracer_amd import scenes
    how = CASES[name][0]
    if how is None:
        return cornell_path
    if isinstance(how, dict):
        return scenes.random_primitives(scene_dir / name, res=(48, 36), depth=DEPTH, **how)
    return None


def make_scene(name, scene_dir, cornell_path):
    """The product's Scene of a case."""
    from cuda_pathtracer_amd import Scene
    path = scene_path(name, scene_dir, cornell_path)
    if path is not None:
        s = Scene(path)
        if CASES[name][0] is None:
            s.set_camera((64, 64), 45.0, EYE, LOOK, (0, 1, 0))
            s.finalize()
        return s
    s = Scene()
    CASES[name][0](s)
    s.set_render(PASSES * SPP, DEPTH, name)
    s.finalize()
    return s


def _gui(**kw):
    from cuda_pathtracer_amd import GuiDataContainer
    g = GuiDataContainer()
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def assert_room(info, want):
    """room_info() reports the walls CASES expects."""
    if want == 0:
        assert info["walls"] == 0 and info["faces"] == [-1] * 6
    else:
        assert info["faces"] == want and info["walls"] == sum(f >= 0 for f in want)
        for a in range(3):
            assert info["lo"][a] < info["hi"][a]
            assert np.isinf(info["lo"][a]) == (want[2 * a] < 0) and np.isinf(info["hi"][a]) == (want[2 * a + 1] < 0)
