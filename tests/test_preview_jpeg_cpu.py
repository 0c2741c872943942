"""The preview's JPEG mode (preview.py, --jpeg QUALITY) on the CPU, with a stand-in render context: the
session keeps the file instead of the RGBA array and reads the PBO only on demand; the server adds
/frame.jpg and the pushed /stream.mjpg, keeps /frame.png, and answers 404 for both without the mode."""
import io
import urllib.error
import urllib.request

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import preview as V
from tests import jpeg_enc_ref as R
from tests.conftest import SCENES


def _pbo(h, w, it):
    a = np.zeros((h, w, 4), np.uint8)
    a[..., 0] = 40 * it
    a[:, 0, 1] = 200   # column x = 0: shown at the window's right edge
    return a


class FakeCtx:
    """preview_jpeg answers with the restatement's file of the PBO in the window's orientation."""

    def __init__(self, h, w, log):
        self.h, self.w, self.log = h, w, log

    def set_flags(self, gui):
        pass

    def render_pass(self, it):
        self.log.append(("pass", it))

    def preview_jpeg(self, it, enc):
        assert isinstance(enc, P.JpegEncoder) and (enc.width, enc.height) == (self.w, self.h)
        self.log.append(("jpeg", it))
        return R.encode(_pbo(self.h, self.w, it), 80, R.S420, mirror_x=True).data

    def image(self):
        return np.full((self.h, self.w, 3), 0.5, np.float32)

    def free(self):
        self.log.append(("free",))


def _session(tmp_path, jpeg, iterations=5):
    s = P.Scene(str(SCENES / "cornell.json"))
    s.set_camera((48, 32), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    st = s.state()
    s.set_render(iterations, st.traceDepth, st.imageName)
    s.finalize()
    log = []

    def read(ctx, it):
        log.append(("read", it))
        return _pbo(ctx.h, ctx.w, it)

    ses = V.PreviewSession(s, out_dir=str(tmp_path), tracer_factory=lambda sc, g: FakeCtx(32, 48, log), read_preview=read,
                           jpeg=jpeg)
    return ses, log


def _read_part(resp):
    assert resp.readline().strip() == b"--frame"
    head = {}
    for line in iter(lambda: resp.readline().strip(), b""):
        k, v = line.split(b":", 1)
        head[k.strip().lower()] = v.strip()
    data = resp.read(int(head[b"content-length"]))
    assert resp.readline() == b"\r\n" and head[b"content-type"] == b"image/jpeg"
    return int(head[b"x-iteration"]), data


def test_session_keeps_the_file_and_reads_the_pbo_on_demand(tmp_path):
    ses, log = _session(tmp_path, 80)
    ses.run_cuda()
    ses.run_cuda()
    assert ses.iteration == 2 and ses.frame_serial == 2
    assert [e for e in log if e[0] in ("jpeg", "read")] == [("jpeg", 1), ("jpeg", 2)]   # no RGBA copy per frame
    assert ses.jpeg_bytes == R.encode(_pbo(32, 48, 2), 80, R.S420, mirror_x=True).data
    shown = ses.display_rgb()
    assert np.array_equal(shown, _pbo(32, 48, 2)[:, ::-1, :3]) and ("read", 2) in log
    ses.display_rgb()
    assert log.count(("read", 2)) == 1   # (read once per frame at most)
    assert ses.jpeg_bytes == R.encode(shown, 80, R.S420).data
    ses.close()
    with pytest.raises(ValueError):
        _session(tmp_path, 0)
    with pytest.raises(ValueError):
        _session(tmp_path, 101)


def test_the_last_frame_survives_the_end_of_the_render(tmp_path):
    ses, log = _session(tmp_path, 80, iterations=2)
    for _ in range(3):
        ses.run_cuda()
    assert ses.done and ses.iteration == 2 and ("free",) in log
    assert np.array_equal(ses.display_rgb(), _pbo(32, 48, 2)[:, ::-1, :3])
    assert ses.jpeg_bytes == R.encode(_pbo(32, 48, 2), 80, R.S420, mirror_x=True).data


def test_server_routes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    ses, _ = _session(tmp_path, None)
    srv = V.PreviewServer(ses, jpeg=80).start(render=False)   # (the server's argument turns the mode on)
    try:
        stream = urllib.request.urlopen(srv.url + "stream.mjpg", timeout=30)
        assert stream.headers["Content-Type"] == "multipart/x-mixed-replace; boundary=frame"
        parts = []
        for _ in range(3):
            ses.run_cuda()
            parts.append(_read_part(stream))
        stream.close()
        assert [it for it, _ in parts] == [1, 2, 3]
        assert [d for _, d in parts] == [R.encode(_pbo(32, 48, it), 80, R.S420, mirror_x=True).data for it in (1, 2, 3)]
        with urllib.request.urlopen(srv.url + "frame.jpg?it=3", timeout=10) as r:
            assert r.headers["Content-Type"] == "image/jpeg" and r.read() == parts[-1][1]
        with urllib.request.urlopen(srv.url + "frame.png", timeout=10) as r:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(r.read()))), _pbo(32, 48, 3)[:, ::-1, :3])
        with urllib.request.urlopen(srv.url, timeout=10) as r:
            page = r.read()
        assert b'src="/frame.jpg"' in page and b"/frame.png" not in page
    finally:
        srv.stop()
        ses.close()


def test_without_the_mode_nothing_changes(tmp_path):
    ses, log = _session(tmp_path, None)
    srv = V.PreviewServer(ses).start(render=False)
    try:
        ses.run_cuda()
        assert ("read", 1) in log and not any(e[0] == "jpeg" for e in log) and ses.jpeg_bytes == b""
        for path in ("frame.jpg", "stream.mjpg"):
            with pytest.raises(urllib.error.HTTPError) as err:
                urllib.request.urlopen(srv.url + path, timeout=10)
            assert err.value.code == 404
        with urllib.request.urlopen(srv.url, timeout=10) as r:
            assert b"/frame.jpg" not in r.read()
    finally:
        srv.stop()
        ses.close()
