"""Which walls the host groups into a room (pt_bounds.cpp find_room), without a GPU.

The room is decided by the scene preparation alone (make_dgeoms -> update_bounds -> find_room: double
arithmetic on the geom table), so Scene.room_info(gui) derives it without a context.  Every case of
tests/room_cases.py gets the assertions tests/test_room_bound_gpu.py's test_room_found makes on the
context's PathTracer.room_info(); that test also checks that the two agree bit for bit.
"""
import pytest

from room_cases import CASES, _gui, assert_room, make_scene, scene_dir   # noqa: F401  (scene_dir: a fixture)


@pytest.mark.parametrize("name", list(CASES))
def test_room_found_on_the_host(name, scene_dir, cornell_path):
    s = make_scene(name, scene_dir, cornell_path)
    assert_room(s.room_info(_gui(**CASES[name][1])), CASES[name][2])


def test_room_off_knob_on_the_host(scene_dir, cornell_path, monkeypatch):
    """PT_AMD_ROOM=0 leaves the walls in the per-cube loop: no room."""
    s = make_scene("cornell", scene_dir, cornell_path)
    assert s.room_info(_gui())["walls"] == 5
    monkeypatch.setenv("PT_AMD_ROOM", "0")
    info = s.room_info(_gui())
    assert info["walls"] == 0 and info["faces"] == [-1] * 6
