"""Interactive preview: the reference's window (path_tracer/src/preview.cpp, main.cpp) without GL.

The reference shows the running render in a GLFW window (a PBO written by sendImageToPBO,
pathtrace.cu:64-86, blitted as a texture, preview.cpp:289-322), orbits the camera with the mouse
(main.cpp:228-271), takes ESC / S / SPACE (main.cpp:189-213) and draws an ImGui panel of toggles
(preview.cpp:212-282).  A GPU host has no display, so here the window is a web page served from the
render process:

  PreviewSession   main.cpp's state (zoom, theta, phi, look-at, mouse buttons, iteration) and its
                   callbacks, runCuda (main.cpp:114-168) and the panel's settings; the camera
                   recompute is pt_scene_set_orbit, the PBO write is pt_preview_rgba.
  PreviewServer    the window: GET / (page: the image, mouse and keys, the panel), GET /frame.png
                   (the PBO as the window shows it), GET /state (title, panel text, settings),
                   POST /event (GLFW-shaped input events and panel edits).  With --jpeg QUALITY
                   the frames are baseline JPEG files encoded on the device (pt_preview_jpeg,
                   DESIGN.md §14): GET /frame.jpg, and GET /stream.mjpg, which pushes each new
                   iteration's file once (multipart/x-mixed-replace).  With --png-device
                   /frame.png is written on the device too (pt_preview_png): the
                   same pixels, another file.  GET /frame.hdr is the current accumulation as a
                   Radiance HDR file, always written on the device (pt_preview_hdr).
                   The panel's Display settings (tone curve, exposure, metering, sRGB) send the
                   frames through the display transform on the device.

    python -m cuda_pathtracer_amd.preview SCENE.json [--port 8080]   (then open the printed URL)

Rendering stays on the HIP path (pt_render_pass + pt_preview_rgba on the device); the server only
encodes the latest frame.  Iterations restart at 1 whenever the camera or a visual setting changes,
as in the reference (runCuda: iteration = 0, pathtraceFree + pathtraceInit).
"""
from __future__ import annotations

import argparse
import json
import struct
import threading
import time
import zlib
from collections import deque
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer
from pathlib import Path

import numpy as np

from . import _native as N
from .pathtrace import (Bloom, BloomParams, DenoiseVarParams, DisplayParams, DisplayTransform, GuiDataContainer, HdrEncoder, HdrParams, JpegEncoder,
                        PathTracer, PngEncoder, Scene, TemporalHistory, _jpeg_params, _png_params, display_transform, encode_jpeg,
                        encode_png, save_image, tonemap)
from .pathtrace import bloom as bloom_host

F32 = np.float32
PI = F32(3.1415926535897932384626422832795028841971)   # utilities.h PI (a float)

# GLFW's codes (glfw3.h): mouse buttons and the key actions main.cpp tests
MOUSE_LEFT, MOUSE_RIGHT, MOUSE_MIDDLE = 0, 1, 2
RELEASE, PRESS = 0, 1
# panel settings that restart the accumulation (preview.cpp:258-271: visual_settings_changed)
VISUAL_SETTINGS = ("SSAA", "DoF", "aperture", "focal_len")
GENERAL_SETTINGS = ("russianRoulette", "sortbyMaterial", "useThrustPartition")
SLIDERS = {"aperture": (0.1, 1.0), "focal_len": (10.0, 80.0)}   # ImGui::SliderFloat ranges
# panel settings of the display transform: display only, like `denoise`
TONEMAPS = {"none": N.DISPLAY_NONE, "reinhard": N.DISPLAY_REINHARD, "aces": N.DISPLAY_ACES, "hable": N.DISPLAY_HABLE}
EXPOSURE_EV = (-16.0, 16.0)
# panel settings of the bloom: display only too; strength 0 is off
BLOOM_STRENGTH, BLOOM_THRESHOLD = (0.0, 4.0), (0.0, 65504.0)
AUTO_EXPOSURE_RATE = 32   # of 256: the share of the way to the metered target a frame goes


def _normalize(v: np.ndarray) -> np.ndarray:   # glm::normalize: v * inversesqrt(dot(v, v))
    v = v.astype(F32)
    return v * (F32(1.0) / np.sqrt(F32(np.dot(v, v))))


class PreviewSession:
    """main.cpp's interactive state and callbacks for one scene (display-free).

    tracer_factory(scene, gui) -> a PathTracer-like context (pathtraceInit); read_preview(ctx, it)
    -> the (H, W, 4) uint8 PBO contents for `it` accumulated iterations; history_factory(width, height)
    -> a TemporalHistory-like object (the `denoise_temporal` setting).  The defaults render on the
    current HIP device; tests substitute them to drive the state machine on the CPU.

    jpeg: None (the default: frames are the RGBA PBO copied to the host), or a quality 1..100: the
    session keeps a JpegEncoder and each frame is a JPEG file encoded on the device in the window's
    orientation (jpeg_bytes); the PBO is then read only when display_rgb() asks for it.

    png_device: False (the default: /frame.png is png_bytes of the PBO, on the host), or True: the frame's
    PNG is written on the device (png_frame: pt_preview_png for a raw frame, encode_png for the host arrays
    of the denoised paths), with display_rgb()'s pixels; as in JPEG mode the PBO of a raw frame is read only
    when display_rgb() asks for it.

    tonemap, exposure_ev, auto_exposure, srgb (panel settings, all off by default): the frames go through the
    session's DisplayTransform instead of the linear clip: raw frames on the device
    (pt_preview_display, into the encoders' pixel entries in JPEG mode and with png_device), denoised and temporal
    frames through display_transform on their host arrays.  With auto_exposure the exposure is metered every frame
    and adapts over frames (exposure_ev is then the compensation).  With all four at their defaults every path is
    the one described above.

    bloom, bloom_threshold (panel settings; bloom is the glare's strength, 0 and off by default): the frames go
    through the session's Bloom first and then through the DisplayTransform, which then also runs
    at its defaults: raw frames on the device (the bloom= of preview_display, preview_jpeg and preview_png), denoised
    and temporal frames through bloom() on their host arrays."""

    def __init__(self, scene: Scene, gui: GuiDataContainer | None = None, out_dir: str | None = None,
                 tracer_factory=None, read_preview=None, history_factory=None, jpeg: int | None = None,
                 png_device: bool = False):
        self.scene = scene
        cam = scene.camera()
        self.width, self.height = int(cam.res[0]), int(cam.res[1])
        # main.cpp:59-73: the orbit of the loaded camera
        phi, theta, zoom = scene.orbit()
        self.phi, self.theta, self.zoom = F32(phi), F32(theta), F32(zoom)
        self.og_look_at = np.array(cam.look_at[:3], dtype=F32)
        self.look_at = self.og_look_at.copy()
        st = scene.state()
        self.iterations, self.traced_depth, self.image_name = st.iterations, st.traceDepth, st.imageName
        self.gui = gui or GuiDataContainer()
        self.gui.TracedDepth = self.traced_depth   # pathtraceInit's guiData->TracedDepth
        self.out_dir = out_dir
        self.start_time = time.strftime("%Y-%m-%d_%H-%M-%Sz", time.gmtime())   # currentTimeString
        self.camchanged = True
        self.visual_changed = False
        self.left = self.right = self.middle = False
        self.last_x = self.last_y = 0.0
        self.iteration = 0
        self.ctx = None
        self.rgba = np.zeros((self.height, self.width, 4), np.uint8)   # the PBO
        self.done = False            # iterations reached: image saved, context freed (runCuda's exit)
        self.should_close = False    # ESC (glfwSetWindowShouldClose)
        self.saved: list[str] = []
        self._frame_times: deque[float] = deque(maxlen=120)   # ImGui's io.Framerate window
        self._last_frame = None
        self._factory = tracer_factory or (lambda sc, g: PathTracer(sc, g))
        self._read = read_preview or self._device_preview
        self._dbuf = None
        self.denoise = False         # panel: show the a-trous-filtered image (PathTracer.denoised)
        # panel: show the variance-guided filter's image (PathTracer.denoised_variance); the context
        # tracks the variance while it is on (_tracking: the current context has been told to)
        self.denoise_variance = False
        self._tracking = False
        # panel: show the temporally reprojected, variance-filtered image (TemporalHistory).  The history
        # belongs to the session, not to a context: it survives the restart a camera change causes.
        self.denoise_temporal = False
        self._history = None
        self._history_factory = history_factory or (lambda w, h: TemporalHistory(w, h))
        self._temporal_stats = {"frames": 0, "mean_history": 0.0}
        # The history takes batches of one sample.  Switched on in a context that has already accumulated
        # k samples, it is fed what that context accumulates from then on: (k, the accumulator at k, the
        # context's G-buffer, its camera), until the next context starts (None: the whole accumulator).
        self._history_base = None
        self.jpeg = None if jpeg is None else int(jpeg)
        if self.jpeg is not None and not 1 <= self.jpeg <= 100:
            raise ValueError(f"jpeg quality {jpeg!r}: 1..100")
        self._enc = None
        self.png_device = bool(png_device)
        self._png_enc = None
        self._hdr_enc = None         # /frame.hdr's encoder, made at the first request
        self.tonemap, self.exposure_ev, self.auto_exposure, self.srgb = "none", 0.0, False, False
        self._display = None         # the session's DisplayTransform, made when a frame needs it
        self.bloom, self.bloom_threshold = 0.0, 1.0
        self._bloom = None           # the session's Bloom, likewise
        self._raw_frame = False      # the current frame is the context's accumulator as pt_preview_rgba converts it
        self.jpeg_bytes = b""        # the current frame's file (JPEG mode)
        self.frame_serial = 0        # counts the files: /stream.mjpg sends each once
        self._rgba_current = True    # self.rgba holds the current frame (JPEG mode reads it on demand)
        self.lock = threading.RLock()
        self.frame_ready = threading.Condition(self.lock)   # notified after every run_cuda

    # ---- callbacks (main.cpp:189-271) --------------------------------------------------------
    def key(self, key: str) -> None:
        """keyCallback on GLFW_PRESS: ESCAPE saves and closes, S saves, SPACE re-centres the look-at."""
        with self.lock:
            k = key.upper()
            if k in ("ESCAPE", "ESC"):
                self.save_image()
                self.should_close = True
            elif k == "S":
                self.save_image()
            elif k in ("SPACE", " "):
                self.camchanged = True
                self.look_at = self.og_look_at.copy()

    def mouse_button(self, button: int, action: int) -> None:
        """mouseButtonCallback: each event sets all three button states (a press of one releases
        the others, any release clears them)."""
        with self.lock:
            self.left = button == MOUSE_LEFT and action == PRESS
            self.right = button == MOUSE_RIGHT and action == PRESS
            self.middle = button == MOUSE_MIDDLE and action == PRESS

    def mouse_move(self, x: float, y: float) -> None:
        """mousePositionCallback: orbit (left), zoom (right), pan the look-at (middle)."""
        with self.lock:
            x, y = float(x), float(y)
            if x == self.last_x or y == self.last_y:
                return   # main.cpp:230 (either coordinate unchanged: the event is dropped)
            if self.left:
                self.phi = F32(float(self.phi) - (x - self.last_x) / self.width)
                self.theta = F32(float(self.theta) - (y - self.last_y) / self.height)
                self.theta = max(F32(0.001), min(self.theta, PI))
                self.camchanged = True
            elif self.right:
                self.zoom = F32(float(self.zoom) + (y - self.last_y) / self.height)
                self.zoom = max(F32(0.1), self.zoom)
                self.camchanged = True
            elif self.middle:
                cam = self.scene.camera()
                fwd = np.array(cam.view[:3], dtype=F32)
                fwd[1] = 0
                fwd = _normalize(fwd)
                rgt = np.array(cam.right[:3], dtype=F32)
                rgt[1] = 0
                rgt = _normalize(rgt)
                self.look_at = self.look_at - (F32(x - self.last_x) * rgt) * F32(0.01)
                self.look_at = self.look_at + (F32(y - self.last_y) * fwd) * F32(0.01)
                self.camchanged = True
            self.last_x, self.last_y = x, y

    def set_setting(self, name: str, value) -> None:
        """An edit in the panel (preview.cpp:243-271).  The general settings apply to the next
        iteration; the visual ones restart the accumulation (visual_settings_changed)."""
        with self.lock:
            if name == "denoise":   # display only: the accumulation, saving and S are untouched
                self.denoise = bool(value)
            elif name == "denoise_variance":   # display only too; tracking starts at the next iteration
                self.denoise_variance = bool(value)
            elif name == "denoise_temporal":   # display only; the history starts with the next iteration
                self.denoise_temporal = bool(value)
                if not self.denoise_temporal:
                    self._free_history()
            elif name == "tonemap":   # display only, as are the three below: no restart, S is untouched
                if value not in TONEMAPS:
                    raise ValueError(f"tonemap {value!r}: one of {', '.join(TONEMAPS)}")
                self._set_display(tonemap=value)
            elif name == "exposure_ev":
                if isinstance(value, (bool, str)) or value is None:
                    raise ValueError(f"exposure_ev {value!r}: a number of stops")
                ev = float(value)
                if not EXPOSURE_EV[0] <= ev <= EXPOSURE_EV[1]:   # (false for NaN)
                    raise ValueError(f"exposure_ev {value!r}: {EXPOSURE_EV[0]} .. {EXPOSURE_EV[1]}")
                self._set_display(exposure_ev=ev)
            elif name in ("auto_exposure", "srgb"):
                self._set_display(**{name: bool(value)})
            elif name in ("bloom", "bloom_threshold"):   # display only as well
                lo, hi = BLOOM_STRENGTH if name == "bloom" else BLOOM_THRESHOLD
                if isinstance(value, (bool, str)) or value is None or not lo <= float(value) <= hi:   # (false for NaN)
                    raise ValueError(f"{name} {value!r}: a number in {lo} .. {hi}")
                if getattr(self, name) != float(value):
                    setattr(self, name, float(value))
                    self._free_bloom()   # (its parameters are fixed at creation: the next frame makes another)
            elif name in GENERAL_SETTINGS or name in ("SSAA", "DoF"):
                if name == "sortbyMaterial" and value and self.scene.environment() is not None:
                    # (pt_set_flags would refuse it inside the render loop and end the session: refused here instead)
                    raise ValueError("sortbyMaterial: a scene with an environment renders with the fused pipeline only")
                setattr(self.gui, name, bool(value))
            elif name in SLIDERS:
                lo, hi = SLIDERS[name]
                setattr(self.gui, name, float(min(max(float(value), lo), hi)))
            else:
                raise ValueError(f"unknown setting {name!r}")
            if name in VISUAL_SETTINGS:
                self.visual_changed = True

    # ---- the display transform ------------------------------------------------
    def _set_display(self, **kw) -> None:
        if any(getattr(self, k) != v for k, v in kw.items()):
            for k, v in kw.items():
                setattr(self, k, v)
            self._free_display()   # (its parameters are fixed at creation: the next frame makes another)

    def _display_on(self) -> bool:
        return self.tonemap != "none" or self.exposure_ev != 0.0 or self.auto_exposure or self.srgb or self.bloom > 0.0

    def _display_params(self) -> DisplayParams:
        """The bytes land in the PBO's orientation (the encoders and display_rgb mirror x)."""
        p = DisplayParams.default()
        p.curve, p.transfer = TONEMAPS[self.tonemap], N.DISPLAY_SRGB if self.srgb else N.DISPLAY_LINEAR
        if self.auto_exposure:
            p.exposure_mode, p.rate, p.compensation_ev = N.DISPLAY_AUTO, AUTO_EXPOSURE_RATE, self.exposure_ev
        else:
            p.exposure = 2.0 ** self.exposure_ev
        return p

    def _display_obj(self) -> DisplayTransform:
        if self._display is None:
            self._display = DisplayTransform(self.width, self.height, self._display_params())
        return self._display

    # ---- the bloom ------------------------------------------------------------
    def _bloom_params(self) -> BloomParams:
        p = BloomParams.default()
        p.strength, p.threshold = self.bloom, self.bloom_threshold
        return p

    def _bloom_obj(self) -> "Bloom | None":
        """The bloom= of the context's preview methods: None while the strength is 0."""
        if not self.bloom > 0.0:
            return None
        if self._bloom is None:
            self._bloom = Bloom(self.width, self.height, self._bloom_params())
        return self._bloom

    def _free_bloom(self) -> None:
        if self._bloom is not None:
            self._bloom.free()
            self._bloom = None

    def _free_display(self) -> None:
        if self._display is not None:
            self._display.free()
            self._display = None

    # ---- runCuda (main.cpp:114-168) -----------------------------------------------------------
    def run_cuda(self) -> None:
        with self.lock:
            if self.done:
                return
            t0 = time.perf_counter()
            if self.visual_changed and self._history is not None:
                self._history.reset()   # (another image: a camera change alone keeps the history)
            if self.visual_changed and self._display is not None:
                self._display.reset()   # (likewise: the next metering jumps to its target)
            if self.camchanged or self.visual_changed:
                self.iteration = 0
                self.scene.set_orbit(float(self.phi), float(self.theta), float(self.zoom), self.look_at)
                self.camchanged = False
                self.visual_changed = False
            if self.iteration == 0:   # pathtraceFree + pathtraceInit
                self._free()
                self.ctx = self._factory(self.scene, self.gui)
                self._tracking = False
                self._history_base = None
            if self.iteration < self.iterations:
                if self.denoise_variance != self._tracking:   # from the accumulator as it stands: no restart
                    self.ctx.track_variance(self.denoise_variance)
                    self._tracking = self.denoise_variance
                if self.denoise_temporal and self._history is None and self.iteration > 0:
                    self._history_base = (self.iteration, self.ctx.image(), self.ctx.gbuffer(), self.scene.camera())
                self.iteration += 1
                # pathtrace(pbo, frame, iteration): InitDataContainer's flags, one iteration, the PBO
                self.ctx.set_flags(self.gui)
                self.ctx.render_pass(self.iteration)
                if self._tracking:
                    self.ctx.variance_update()
                if self.denoise_temporal:
                    self.rgba = self._temporal_preview()
                elif self.denoise or self.denoise_variance:
                    self.rgba = self._denoised_preview()
                elif self.jpeg is not None:   # only the file crosses to the host
                    self.jpeg_bytes = self._jpeg_preview()
                    self._rgba_current = False
                    self._raw_frame = True
                elif self.png_device:          # /frame.png encodes from the accumulator: no RGBA copy per frame
                    self._rgba_current = False
                    self._raw_frame = True
                else:
                    self.rgba = self._read(self.ctx, self.iteration)
                    self._raw_frame = True
                if self.jpeg is not None and self._rgba_current:   # (a host array: the denoised paths)
                    self.jpeg_bytes = encode_jpeg(self.rgba, self.jpeg, "420", mirror_x=True)
                if self.jpeg is not None:
                    self.frame_serial += 1
            else:
                self.save_image()
                self._current_rgba()
                self._free()
                self.done = True
            self.frame_ready.notify_all()
            now = time.perf_counter()
            self._frame_times.append(now - (self._last_frame if self._last_frame is not None else t0))
            self._last_frame = now

    def _device_preview(self, ctx, it: int) -> np.ndarray:
        import torch
        if self._dbuf is None:
            self._dbuf = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device="cuda")
        if self._display_on():
            ctx.preview_display(it, self._display_obj(), self._dbuf.data_ptr(), 4, bloom=self._bloom_obj())
        else:
            ctx.preview_rgba(it, self._dbuf.data_ptr())   # (the render's stream: NULL)
        return self._dbuf.cpu().numpy()

    def _jpeg_preview(self) -> bytes:
        if self._enc is None:
            self._enc = JpegEncoder(self.width, self.height, _jpeg_params(self.jpeg, "420", True))
        if self._display_on():
            return self.ctx.preview_jpeg(self.iteration, self._enc, display=self._display_obj(), bloom=self._bloom_obj())
        return self.ctx.preview_jpeg(self.iteration, self._enc)

    def png_frame(self) -> bytes:
        """png_device: the current frame as a PNG file written on the device, display_rgb()'s pixels.  A raw
        frame is encoded from the accumulator (only the file crosses to the host); a denoised or temporal
        frame, and the last frame of a finished session, are host arrays and go through encode_png."""
        with self.lock:
            if self._raw_frame and self.ctx is not None and self.iteration > 0:
                if self._png_enc is None:
                    self._png_enc = PngEncoder(self.width, self.height, _png_params(mirror_x=True))
                if self._display_on():
                    return self.ctx.preview_png(self.iteration, self._png_enc, display=self._display_obj(), bloom=self._bloom_obj())
                return self.ctx.preview_png(self.iteration, self._png_enc)
            self._current_rgba()
            return encode_png(self.rgba, mirror_x=True)

    def hdr_frame(self) -> bytes | None:
        """/frame.hdr: the current accumulation (accumulator / iteration, x-mirrored like every saved image) as a
        Radiance HDR file, always written on the device (pt_preview_hdr); None when there is nothing to encode
        (no iteration yet, or the session is finished and its context freed)."""
        with self.lock:
            if self.ctx is None or self.iteration <= 0:
                return None
            if self._hdr_enc is None:
                prm = HdrParams.default()
                prm.mirror_x = 1
                self._hdr_enc = HdrEncoder(self.width, self.height, prm)
            return self.ctx.preview_hdr(self.iteration, self._hdr_enc)

    def _current_rgba(self) -> None:
        """JPEG mode and png_device: the PBO of the current frame, read when something asks for it."""
        if not self._rgba_current and self.ctx is not None:
            self.rgba = self._read(self.ctx, self.iteration)
        self._rgba_current = True

    def _denoised_preview(self) -> np.ndarray:
        """The PBO contents of the denoised image: the tonemapped bytes, un-mirrored back into the
        PBO's pixel order (display_rgb mirrors x), alpha 0 as sendImageToPBO leaves it.  The
        variance-guided image once two batches exist, the plain filter's before that."""
        if self.denoise_variance and self._tracking and self.ctx.variance_info()["batches"] >= 2:
            img = self.ctx.denoised_variance(float(self.iteration))
        else:
            img = self.ctx.denoised(float(self.iteration))
        return self._pbo_of(img)

    def _pbo_of(self, img: np.ndarray) -> np.ndarray:
        self._rgba_current = True
        self._raw_frame = False
        if self.bloom > 0.0:
            img = bloom_host(img, 1.0, self._bloom_params())
        rgb = display_transform(img, 1.0, self._display_params()) if self._display_on() else tonemap(img, 1.0)[:, ::-1]
        out = np.zeros((self.height, self.width, 4), np.uint8)
        out[..., :3] = rgb
        return out

    def _temporal_preview(self) -> np.ndarray:
        """One frame of the pass just rendered into the session's history (created at the first use),
        and the PBO contents of its variance-filtered image."""
        if self._history is None:
            self._history = self._history_factory(self.width, self.height)
        if self._history_base is None:
            self._history.frame(self.ctx, self.iteration)
        else:   # the samples since the box was switched on (the accumulator's gain: the render is untouched)
            k, base, gbuffer, camera = self._history_base
            self._history.frame_arrays(camera, self.ctx.image() - base, self.iteration - k, gbuffer)
        img, his = self._history.image(DenoiseVarParams.default(), return_history=True)
        self._temporal_stats = {"frames": int(self._history.info()["frames"]), "mean_history": float(np.mean(his))}
        return self._pbo_of(img)

    def _free_history(self) -> None:
        if self._history is not None:
            if hasattr(self._history, "free"):
                self._history.free()
            self._history = None
        self._history_base = None
        self._temporal_stats = {"frames": 0, "mean_history": 0.0}

    def _free(self) -> None:
        if self.ctx is not None:
            if hasattr(self.ctx, "free"):
                self.ctx.free()
            self.ctx = None

    def save_image(self) -> str | None:
        """saveImage (main.cpp:88-112): the accumulator / iterations as imageName.<start>.<N>samp.png."""
        with self.lock:
            if self.ctx is None or self.iteration == 0 or self.out_dir is None:
                return None
            name = f"{self.image_name}.{self.start_time}.{self.iteration}samp.png"
            path = save_image(str(Path(self.out_dir) / name), self.ctx.image(), float(self.iteration))
            self.saved.append(path)
            return path

    def close(self) -> None:
        with self.lock:
            self._current_rgba()
            self._free()
            self._free_history()
            self._dbuf = None
            if self._enc is not None:
                self._enc.free()
                self._enc = None
            if self._png_enc is not None:
                self._png_enc.free()
                self._png_enc = None
            if self._hdr_enc is not None:
                self._hdr_enc.free()
                self._hdr_enc = None
            self._free_display()
            self._free_bloom()
            self.frame_ready.notify_all()

    # ---- what the window shows ----------------------------------------------------------------
    def title(self) -> str:   # preview.cpp:297
        return f"Path Tracer | {self.iteration} Iterations"

    def display_rgb(self) -> np.ndarray:
        """The window's pixels: the PBO through the quad's texture coordinates (preview.cpp:43-68:
        u = 1 at the left edge, v = 0 at the top), i.e. x mirrored, rows top-down."""
        with self.lock:
            self._current_rgba()
            return np.ascontiguousarray(self.rgba[:, ::-1, :3])

    def state(self) -> dict:
        with self.lock:
            ft = sum(self._frame_times) / len(self._frame_times) if self._frame_times else 0.0
            cam = self.scene.camera()
            extra = {"temporal": dict(self._temporal_stats)} if self.denoise_temporal else {}
            return {
                **extra, "title": self.title(), "iteration": self.iteration, "iterations": self.iterations,
                "done": self.done, "closed": self.should_close,
                "traced_depth": self.traced_depth,   # "Traced Depth %d"
                "ms_per_frame": ft * 1e3, "fps": (1.0 / ft) if ft > 0 else 0.0,
                "settings": {**{k: getattr(self.gui, k) for k in GENERAL_SETTINGS + VISUAL_SETTINGS},
                             "denoise": self.denoise, "denoise_variance": self.denoise_variance,
                             "denoise_temporal": self.denoise_temporal, "tonemap": self.tonemap,
                             "exposure_ev": self.exposure_ev, "auto_exposure": self.auto_exposure, "srgb": self.srgb,
                             "bloom": self.bloom, "bloom_threshold": self.bloom_threshold},
                "camera": {"phi": float(self.phi), "theta": float(self.theta), "zoom": float(self.zoom),
                           "look_at": [float(v) for v in self.look_at],
                           "position": [float(v) for v in cam.position[:3]]},
                "size": [self.width, self.height], "saved": list(self.saved),
            }

    def handle_event(self, ev: dict) -> None:
        kind = ev.get("kind")
        if kind == "button":
            self.mouse_button(int(ev["button"]), int(ev["action"]))
        elif kind == "move":
            self.mouse_move(float(ev["x"]), float(ev["y"]))
        elif kind == "key":
            self.key(str(ev["key"]))
        elif kind == "setting":
            self.set_setting(str(ev["name"]), ev["value"])
        else:
            raise ValueError(f"unknown event kind {kind!r}")


def png_bytes(rgb: np.ndarray) -> bytes:
    """8-bit RGB PNG of an (H, W, 3) uint8 array (filter 0 rows, zlib level 1)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))


_PAGE = """<!doctype html><html><head><meta charset="utf-8"><title>Path Tracer</title>
<style>body{font:13px sans-serif;background:#222;color:#ddd;display:flex;gap:16px;margin:12px}
#img{image-rendering:pixelated;cursor:crosshair;user-select:none}
fieldset{border:1px solid #555;margin:0 0 8px 0} input[type=range]{width:160px}</style></head><body>
<img id="img" src="/frame.png" draggable="false" tabindex="0">
<div><div id="title"></div><fieldset><legend>Path Tracer Analytics</legend>
<div id="depth"></div><div id="rate"></div></fieldset>
<fieldset><legend>General settings</legend>
<label><input type="checkbox" id="russianRoulette"> Russian roulette</label><br>
<label><input type="checkbox" id="sortbyMaterial"> Sort by material (can harm performance)</label><br>
<label><input type="checkbox" id="useThrustPartition"> Use thrust library for path termination</label><br>
<label><input type="checkbox" id="denoise"> Show the denoised image (edge-avoiding a-trous filter)</label><br>
<label><input type="checkbox" id="denoise_variance"> Show the variance-guided denoised image (tracks per-pixel variance)</label><br>
<label><input type="checkbox" id="denoise_temporal"> Keep the denoiser's history across camera moves (temporal reprojection)</label></fieldset>
<fieldset><legend>Display</legend>
<label>Tone curve <select id="tonemap"><option>none</option><option>reinhard</option><option>aces</option><option>hable</option></select></label><br>
<label>Exposure (stops) <input type="range" id="exposure_ev" min="-8" max="8" step="0.25"></label><br>
<label><input type="checkbox" id="auto_exposure"> Meter the exposure (the slider compensates)</label><br>
<label><input type="checkbox" id="srgb"> sRGB transfer</label><br>
<label>Bloom strength <input type="range" id="bloom" min="0" max="2" step="0.05"></label><br>
<label>Bloom threshold <input type="range" id="bloom_threshold" min="0" max="8" step="0.1"></label></fieldset>
<fieldset><legend>Visual settings</legend>
<label><input type="checkbox" id="SSAA"> Enable stochastic sampled antialiasing</label><br>
<label><input type="checkbox" id="DoF"> Enable DoF effects</label><br>
<label>Aperture radius <input type="range" id="aperture" min="0.1" max="1" step="0.01"></label><br>
<label>Focal distance <input type="range" id="focal_len" min="10" max="80" step="0.1"></label></fieldset>
<div>Left drag: orbit; right drag: zoom; middle drag: pan; S: save; Space: re-centre; Esc: save and quit</div>
</div><script>
const img=document.getElementById('img');let shown=-1;
function post(ev){fetch('/event',{method:'POST',body:JSON.stringify(ev)});}
function pos(e){const r=img.getBoundingClientRect();return{x:(e.clientX-r.left)*img.naturalWidth/r.width,
 y:(e.clientY-r.top)*img.naturalHeight/r.height};}
const btn={0:0,1:2,2:1};  // DOM -> GLFW (left, right, middle)
img.addEventListener('mousedown',e=>{e.preventDefault();img.focus();post({kind:'button',button:btn[e.button],action:1});});
window.addEventListener('mouseup',e=>post({kind:'button',button:btn[e.button],action:0}));
img.addEventListener('mousemove',e=>{const p=pos(e);post({kind:'move',x:p.x,y:p.y});});
img.addEventListener('contextmenu',e=>e.preventDefault());
window.addEventListener('keydown',e=>{const k=e.key==='Escape'?'ESCAPE':e.key===' '?'SPACE':e.key.toUpperCase();
 if(['ESCAPE','SPACE','S'].includes(k)){e.preventDefault();post({kind:'key',key:k});}});
for(const id of ['russianRoulette','sortbyMaterial','useThrustPartition','denoise','denoise_variance','denoise_temporal','SSAA','DoF','auto_exposure','srgb'])
 document.getElementById(id).addEventListener('change',e=>post({kind:'setting',name:id,value:e.target.checked}));
document.getElementById('tonemap').addEventListener('change',e=>post({kind:'setting',name:'tonemap',value:e.target.value}));
for(const id of ['aperture','focal_len','exposure_ev','bloom','bloom_threshold'])
 document.getElementById(id).addEventListener('input',e=>post({kind:'setting',name:id,value:parseFloat(e.target.value)}));
async function poll(){try{const s=await (await fetch('/state')).json();
 document.getElementById('title').textContent=s.title;document.title=s.title;
 document.getElementById('depth').textContent='Traced Depth '+s.traced_depth;
 document.getElementById('rate').textContent='Application average '+s.ms_per_frame.toFixed(3)+' ms/frame ('+s.fps.toFixed(1)+' FPS)';
 for(const [k,v] of Object.entries(s.settings)){const el=document.getElementById(k);if(!el||el===document.activeElement)continue;
  if(el.type==='checkbox')el.checked=v;else el.value=v;}
 for(const id of ['aperture','focal_len'])document.getElementById(id).disabled=!s.settings.DoF;
 if(s.iteration!==shown){shown=s.iteration;img.src='/frame.png?it='+s.iteration+'&t='+Date.now();}
 if(s.closed){document.getElementById('title').textContent+=' (closed)';return;}}catch(e){}
 setTimeout(poll,100);}
poll();</script></body></html>"""


class PreviewServer:
    """The window: a render loop thread (preview.cpp:289-322's mainLoop) and an HTTP server."""

    def __init__(self, session: PreviewSession, host: str = "127.0.0.1", port: int = 0, jpeg: int | None = None,
                 png_device: bool | None = None):
        self.session = session
        if png_device is not None:
            session.png_device = bool(png_device)
        if jpeg is not None:
            if not 1 <= int(jpeg) <= 100:
                raise ValueError(f"jpeg quality {jpeg!r}: 1..100")
            session.jpeg = int(jpeg)
        self._stop = threading.Event()
        self._png = (-1, b"")   # (iteration, bytes) of the last encoded frame
        srv = self

        class Handler(BaseHTTPRequestHandler):
            def log_message(self, *a):   # quiet
                pass

            def _send(self, code: int, body: bytes, ctype: str) -> None:
                self.send_response(code)
                self.send_header("Content-Type", ctype)
                self.send_header("Content-Length", str(len(body)))
                self.send_header("Cache-Control", "no-store")
                self.end_headers()
                self.wfile.write(body)

            def do_GET(self):  # noqa: N802
                path = self.path.split("?", 1)[0]
                jpeg = srv.session.jpeg is not None
                if path == "/":
                    page = _PAGE.replace("/frame.png", "/frame.jpg") if jpeg else _PAGE
                    self._send(200, page.encode(), "text/html; charset=utf-8")
                elif path == "/frame.png":
                    self._send(200, srv.frame_png(), "image/png")
                elif path == "/frame.jpg" and jpeg:
                    self._send(200, srv.frame_jpeg()[1], "image/jpeg")
                elif path == "/stream.mjpg" and jpeg:
                    self._stream()
                elif path == "/frame.hdr":
                    data = srv.session.hdr_frame()
                    if data is None:
                        self._send(404, b"no accumulation to encode", "text/plain")
                    else:
                        self._send(200, data, "image/vnd.radiance")
                elif path == "/state":
                    self._send(200, json.dumps(srv.session.state()).encode(), "application/json")
                else:
                    self._send(404, b"not found", "text/plain")

            def _stream(self) -> None:
                """Each new iteration's file once, as multipart/x-mixed-replace, until the window closes."""
                self.send_response(200)
                self.send_header("Content-Type", "multipart/x-mixed-replace; boundary=frame")
                self.send_header("Cache-Control", "no-store")
                self.end_headers()
                ses, shown = srv.session, 0
                try:
                    while True:
                        with ses.frame_ready:
                            while ses.frame_serial == shown:
                                if srv._stop.is_set() or ses.should_close or ses.done:
                                    return
                                ses.frame_ready.wait(0.25)
                            shown, it, data = ses.frame_serial, ses.iteration, ses.jpeg_bytes
                        self.wfile.write(b"--frame\r\nContent-Type: image/jpeg\r\nContent-Length: %d\r\nX-Iteration: %d\r\n\r\n"
                                         % (len(data), it) + data + b"\r\n")
                        self.wfile.flush()
                except (BrokenPipeError, ConnectionResetError):
                    pass

            def do_POST(self):  # noqa: N802
                if self.path.split("?", 1)[0] != "/event":
                    self._send(404, b"not found", "text/plain")
                    return
                n = int(self.headers.get("Content-Length") or 0)
                try:
                    evs = json.loads(self.rfile.read(n) or b"[]")
                    for ev in evs if isinstance(evs, list) else [evs]:
                        srv.session.handle_event(ev)
                except (ValueError, KeyError, TypeError) as e:
                    self._send(400, str(e).encode(), "text/plain")
                    return
                self._send(200, b"{}", "application/json")

        self.httpd = ThreadingHTTPServer((host, port), Handler)
        self.httpd.daemon_threads = True
        self.url = f"http://{host}:{self.httpd.server_address[1]}/"
        self._threads: list[threading.Thread] = []
        self.error: BaseException | None = None

    def frame_png(self) -> bytes:
        s = self.session
        with s.lock:
            it = s.iteration
            if self._png[0] != it:   # (a display setting shows from the next iteration's frame on)
                self._png = (it, s.png_frame() if s.png_device else png_bytes(s.display_rgb()))
            return self._png[1]

    def frame_jpeg(self) -> tuple:
        """(iteration, file) of the current frame (JPEG mode)."""
        s = self.session
        with s.lock:
            return s.iteration, s.jpeg_bytes

    def _loop(self) -> None:
        try:
            while not self._stop.is_set() and not self.session.should_close:
                if self.session.done:
                    time.sleep(0.05)
                    continue
                self.session.run_cuda()
        except BaseException as e:   # surfaced by stop() / the CLI
            self.error = e
        finally:
            self.session.close()

    def start(self, render: bool = True) -> "PreviewServer":
        t = threading.Thread(target=self.httpd.serve_forever, name="preview-http", daemon=True)
        t.start()
        self._threads.append(t)
        if render:
            r = threading.Thread(target=self._loop, name="preview-render", daemon=True)
            r.start()
            self._threads.append(r)
        return self

    def stop(self) -> None:
        self._stop.set()
        self.httpd.shutdown()
        self.httpd.server_close()
        for t in self._threads:
            t.join(timeout=30)
        if self.error is not None:
            raise self.error

    def wait(self) -> None:
        """Block until ESC (should_close) or KeyboardInterrupt."""
        try:
            while not self.session.should_close and self.error is None:
                time.sleep(0.1)
        except KeyboardInterrupt:
            pass


def parse_rotate(text: str) -> tuple[float, float, float]:
    """--env-rotate's X,Y,Z."""
    parts = text.split(",")
    if len(parts) != 3:
        raise SystemExit(f"--env-rotate {text}: three angles in degrees, X,Y,Z")
    try:
        return tuple(float(v) for v in parts)
    except ValueError:
        raise SystemExit(f"--env-rotate {text}: three angles in degrees, X,Y,Z") from None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Interactive preview of a scene (the reference's window, served as a web page)")
    ap.add_argument("scene")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8080)
    ap.add_argument("--out-dir", default=".", help="where S / ESC / the last iteration save the PNG")
    ap.add_argument("--jpeg", type=int, default=None, metavar="QUALITY",
                    help="encode the frames as JPEG on the device (1..100); adds /frame.jpg and /stream.mjpg")
    ap.add_argument("--png-device", action="store_true",
                    help="write /frame.png on the device (pt_preview_png) instead of compressing the frame on the host")
    ap.add_argument("--env", default=None, metavar="FILE", help="a lat-long Radiance .hdr file as the scene's environment")
    ap.add_argument("--env-scale", type=float, default=1.0, metavar="X", help="multiplies the environment's radiance")
    ap.add_argument("--env-rotate", default="0,0,0", metavar="X,Y,Z", help="the environment's rotation in degrees")
    a = ap.parse_args(argv)
    scene = Scene(a.scene)
    if a.env:
        scene.set_environment(a.env, scale=a.env_scale, rotate=parse_rotate(a.env_rotate))
    print(f"Reading scene from {a.scene} ...", flush=True)
    srv = PreviewServer(PreviewSession(scene, out_dir=a.out_dir, jpeg=a.jpeg, png_device=a.png_device), a.host, a.port).start()
    print(f"preview at {srv.url}  (Esc in the page saves and quits)", flush=True)
    srv.wait()
    srv.stop()
    for p in srv.session.saved:
        print(f"Saved {p}.")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
