// pathtracer_amd — headless restatement of the reference's main loop (path_tracer/src/main.cpp):
// load the scene, InitDataContainer, then runCuda's sequence (main.cpp:114-168) without the GL
// window — pathtraceInit, `iterations` calls of pathtrace(), saveImage() (main.cpp:88-112) and
// pathtraceFree().  The camera is the first-frame orbit recompute (done by pt_scene_finalize).
//
//   pathtracer_amd SCENEFILE.json [--iterations N] [--out DIR] [--sort] [--no-png] [--hdr] [--denoise]
//                  [--denoise-variance] [--aov DIR] [--adaptive THRESHOLD] [--adaptive-every K] [--device-png]
//                  [--device-hdr] [--tonemap none|reinhard|aces|hable] [--exposure EV|auto] [--srgb] [--exr] [--exr-half]
//                  [--env FILE.hdr] [--env-scale X] [--env-rotate X,Y,Z]
//                  [--bloom STRENGTH] [--bloom-threshold X] [--bloom-levels K]
// --bloom, --bloom-threshold, --bloom-levels: any of them additionally writes ...samp.bloom.png, the accumulator through the
// bloom (pt_preview_bloom, DESIGN.md §20: the glare's strength, the luminance above which a pixel glares, the pyramid's
// levels) and then through the display transform of the display flags (without them: pt_tonemap's conversion),
// x-mirrored and written by the device PNG encoder.  The other files keep their names and bytes.
// --env gives the scene an environment (pt_scene_load_environment of a lat-long Radiance file; --env-scale
// multiplies its radiance, --env-rotate turns it by degrees about x, y, z); a scene file's own Extensions.ENVIRONMENT is replaced.
// --exr additionally writes ...samp.exr, an OpenEXR file written on the device (pt_preview_exr, DESIGN.md §18: FLOAT, ZIP,
// x-mirrored like every saved image) with the beauty layer R, G, B and, with --aov DIR, the six first-hit layers beside
// it in the same file; --exr-half stores the layers that may be HALF as HALF.  The other files keep their names and bytes.
// --tonemap, --exposure, --srgb: any of them additionally writes ...samp.display.png, the accumulator through the
// display transform (pt_preview_display, DESIGN.md §17: the tone curve, an exposure of EV stops or a metered one,
// the sRGB transfer), x-mirrored like every saved image and written by the device PNG encoder from the device
// bytes.  The other files keep their names and bytes.
// --device-hdr, with --hdr, writes the main .hdr file on the device (pt_preview_hdr: the same name and the same
// bytes; the denoised and adaptive .hdr files stay on the host writer).
// --device-png writes the final PNG on the device (pt_preview_png with pt_tonemap's conversion and the x
// mirror: the same name and the same pixels, another file; only the file crosses to the host).
// --denoise also writes the a-trous-filtered image (pt_denoise_image) as ...samp.denoised.png (and
// .denoised.hdr with --hdr); --denoise-variance tracks the per-pixel variance (pt_track_variance, one
// pt_variance_update per iteration; the raw image is the same) and writes the variance-guided filter's
// image (pt_denoise_image_var; the plain filter's with fewer than 2 iterations) as
// ...samp.denoised-var.png (and .hdr with --hdr); --aov DIR writes the first-hit G-buffer planes
// (pt_get_gbuffer) as raw little-endian float32 files with a one-line JSON sidecar of their shapes.
// --adaptive THRESHOLD samples adaptively (pt_adaptive_enable; the other parameters at their defaults):
// an update after every iteration, a selection of the active 64-pixel blocks every K (default 4)
// iterations, until no block is active or the iterations are done.  It writes the resolved image
// (every pixel divided by the samples of its block) as ...samp.adaptive.png instead of the raw one,
// with --denoise-variance also its variance-filtered version as ...samp.adaptive.denoised-var.png, and
// reports the samples per block and the segments traced.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <sstream>
#include <string>
#include <vector>

#include "pathtrace.h"

namespace {

std::string currentTimeString() {   // preview.cpp:21-28
    time_t now;
    time(&now);
    char buf[sizeof "0000-00-00_00-00-00z"];
    strftime(buf, sizeof buf, "%Y-%m-%d_%H-%M-%Sz", gmtime(&now));
    return std::string(buf);
}

// saveImage (main.cpp:88-112): divide by the sample count, mirror x, clamp, x255, PNG.
// `denoised`: a per-sample image to write instead (as ...samp.<tag>.png / .hdr).
std::string saveImage(const Scene& scene, const std::string& dir, const std::string& start, int iteration,
                      bool hdr = false, const float* denoised = nullptr, const char* tag = "denoised") {
    const float samples = (float)iteration;
    std::ostringstream ss;
    ss << scene.state.imageName << "." << start << "." << samples << "samp";
    std::string filename = ss.str();
    if (!dir.empty()) filename = dir + "/" + filename;
    if (denoised) filename += std::string(".") + tag;
    filename += hdr ? ".hdr" : ".png";   // Image::savePNG / saveHDR append the extension (image.cpp:22-49)
    const int W = scene.state.camera.res[0], H = scene.state.camera.res[1];
    const float* rgb = denoised ? denoised : reinterpret_cast<const float*>(scene.state.image.data());
    const float div = denoised ? 1.0f : samples;
    if (hdr ? pt_save_hdr(filename.c_str(), rgb, W, H, div) : pt_save_png(filename.c_str(), rgb, W, H, div)) {
        std::fprintf(stderr, "saveImage: %s\n", pt_last_error());
        std::exit(EXIT_FAILURE);
    }
    return filename;
}

// --device-png, --device-hdr: saveImage's file name, the file written by a device encoder.  encode(d_out, cap,
// d_size) queues it; the size word, then that many bytes, cross to the host.
template <class Encode>
std::string saveDeviceFile(const Scene& scene, const std::string& dir, const std::string& start, int iteration, const char* ext,
                           int64_t cap, Encode encode) {
    std::ostringstream ss;
    ss << scene.state.imageName << "." << start << "." << (float)iteration << "samp";
    std::string filename = (dir.empty() ? std::string() : dir + "/") + ss.str() + ext;
    auto die = [](const char* what, const char* why) {
        std::fprintf(stderr, "saveImage (device): %s: %s\n", what, why);
        std::exit(EXIT_FAILURE);
    };
    uint8_t* d = nullptr;   // size word | file
    if (hipMalloc((void**)&d, 256 + (size_t)cap) != hipSuccess) die("hipMalloc", "out of device memory");
    if (encode(d + 256, cap, (int64_t*)d)) die("encode", pt_last_error());
    int64_t size = 0;
    if (hipMemcpy(&size, d, sizeof(size), hipMemcpyDeviceToHost) != hipSuccess || size <= 0) die("size", "copy failed");
    std::vector<uint8_t> file((size_t)size);
    if (hipMemcpy(file.data(), d + 256, (size_t)size, hipMemcpyDeviceToHost) != hipSuccess) die("file", "copy failed");
    (void)hipFree(d);
    FILE* f = std::fopen(filename.c_str(), "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f)) die("write", filename.c_str());
    return filename;
}

// --device-png: saveImage's pixels (pt_tonemap's conversion, x-mirrored).
std::string saveImageDevice(const Scene& scene, const std::string& dir, const std::string& start, int iteration) {
    pt_png_params prm;
    pt_png_params_default(&prm);
    prm.conv = PT_PNG_CONV_SAVE;
    prm.mirror_x = 1;
    pt_png_enc* enc = nullptr;
    if (pt_png_enc_create(scene.state.camera.res[0], scene.state.camera.res[1], &prm, &enc)) {
        std::fprintf(stderr, "saveImage (device): encoder: %s\n", pt_last_error());
        std::exit(EXIT_FAILURE);
    }
    const std::string filename = saveDeviceFile(scene, dir, start, iteration, ".png", pt_png_enc_bound(enc),
                                                [&](uint8_t* d_out, int64_t cap, int64_t* d_size) {
        return pt_preview_png(pathtraceContext(), iteration, enc, d_out, cap, d_size, nullptr);
    });
    pt_png_enc_destroy(enc);
    return filename;
}

// --device-hdr: pt_save_hdr's bytes (x-mirrored, accumulator / iteration).
std::string saveHdrDevice(const Scene& scene, const std::string& dir, const std::string& start, int iteration) {
    pt_hdr_params prm;
    pt_hdr_params_default(&prm);
    prm.mirror_x = 1;
    pt_hdr_enc* enc = nullptr;
    if (pt_hdr_enc_create(scene.state.camera.res[0], scene.state.camera.res[1], &prm, &enc)) {
        std::fprintf(stderr, "saveImage (device): encoder: %s\n", pt_last_error());
        std::exit(EXIT_FAILURE);
    }
    const std::string filename = saveDeviceFile(scene, dir, start, iteration, ".hdr", pt_hdr_enc_bound(enc),
                                                [&](uint8_t* d_out, int64_t cap, int64_t* d_size) {
        return pt_preview_hdr(pathtraceContext(), iteration, enc, d_out, cap, d_size, nullptr);
    });
    pt_hdr_enc_destroy(enc);
    return filename;
}

// --exr: ...samp.exr, the layers `layers` (HALF for those of `half` that may be) in one OpenEXR file written on the device.
std::string saveExrDevice(const Scene& scene, const std::string& dir, const std::string& start, int iteration, int32_t layers,
                          int32_t half) {
    pt_exr_params prm;
    pt_exr_params_default(&prm);
    prm.mirror_x = 1;
    pt_exr_channel channels[16];
    int32_t n = 0;
    pt_exr_enc* enc = nullptr;
    if (pt_exr_ctx_channels(layers, half, channels, &n) ||
        pt_exr_enc_create(scene.state.camera.res[0], scene.state.camera.res[1], channels, n, &prm, &enc)) {
        std::fprintf(stderr, "saveImage (device): encoder: %s\n", pt_last_error());
        std::exit(EXIT_FAILURE);
    }
    const std::string filename = saveDeviceFile(scene, dir, start, iteration, ".exr", pt_exr_enc_bound(enc),
                                                [&](uint8_t* d_out, int64_t cap, int64_t* d_size) {
        return pt_preview_exr(pathtraceContext(), iteration, layers, enc, d_out, cap, d_size, nullptr);
    });
    pt_exr_enc_destroy(enc);
    return filename;
}

// --tonemap, --exposure, --srgb: ...samp.display.png, the display transform's bytes through the device PNG encoder.
std::string saveDisplayDevice(const Scene& scene, const std::string& dir, const std::string& start, int iteration,
                              const pt_display_params& dprm) {
    const int W = scene.state.camera.res[0], H = scene.state.camera.res[1];
    auto die = [](const char* what) {
        std::fprintf(stderr, "saveImage (display): %s: %s\n", what, pt_last_error());
        std::exit(EXIT_FAILURE);
    };
    pt_display* disp = nullptr;
    if (pt_display_create(W, H, &dprm, &disp)) die("display transform");
    pt_png_params prm;
    pt_png_params_default(&prm);   // (no mirror: the display transform's bytes are mirrored already)
    pt_png_enc* enc = nullptr;
    if (pt_png_enc_create(W, H, &prm, &enc)) die("encoder");
    uint8_t* d_pix = nullptr;
    if (hipMalloc((void**)&d_pix, (size_t)W * H * 3) != hipSuccess) {
        std::fprintf(stderr, "saveImage (display): out of device memory\n");
        std::exit(EXIT_FAILURE);
    }
    if (pt_preview_display(pathtraceContext(), iteration, disp, d_pix, 3, nullptr)) die("pt_preview_display");
    const std::string filename = saveDeviceFile(scene, dir, start, iteration, ".display.png", pt_png_enc_bound(enc),
                                                [&](uint8_t* d_out, int64_t cap, int64_t* d_size) {
        return pt_png_enc_pixels(enc, d_pix, 3, d_out, cap, d_size, nullptr);
    });
    pt_png_enc_destroy(enc);
    pt_display_destroy(disp);
    (void)hipFree(d_pix);
    return filename;
}

// --bloom: ...samp.bloom.png, the accumulator through the bloom (pt_preview_bloom) into a device buffer, that buffer
// through the display transform (the display flags', or the defaults: pt_tonemap's conversion) and the device PNG encoder.
std::string saveBloomDevice(const Scene& scene, const std::string& dir, const std::string& start, int iteration,
                            const pt_bloom_params& bprm, const pt_display_params& dprm) {
    const int W = scene.state.camera.res[0], H = scene.state.camera.res[1];
    auto die = [](const char* what) {
        std::fprintf(stderr, "saveImage (bloom): %s: %s\n", what, pt_last_error());
        std::exit(EXIT_FAILURE);
    };
    pt_bloom* bloom = nullptr;
    if (pt_bloom_create(W, H, &bprm, &bloom)) die("bloom");
    pt_display* disp = nullptr;
    if (pt_display_create(W, H, &dprm, &disp)) die("display transform");
    pt_png_params prm;
    pt_png_params_default(&prm);   // (no mirror: the display transform's bytes are mirrored already)
    pt_png_enc* enc = nullptr;
    if (pt_png_enc_create(W, H, &prm, &enc)) die("encoder");
    float* d_rgb = nullptr;
    uint8_t* d_pix = nullptr;
    if (hipMalloc((void**)&d_rgb, (size_t)W * H * 3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&d_pix, (size_t)W * H * 3) != hipSuccess) {
        std::fprintf(stderr, "saveImage (bloom): out of device memory\n");
        std::exit(EXIT_FAILURE);
    }
    if (pt_preview_bloom(pathtraceContext(), iteration, bloom, d_rgb, nullptr)) die("pt_preview_bloom");
    if (dprm.exposure_mode == PT_DISPLAY_AUTO ? pt_display_frame(disp, d_rgb, (float)iteration, d_pix, 3, nullptr)
                                              : pt_display_apply(disp, d_rgb, (float)iteration, d_pix, 3, nullptr))
        die("display transform");
    const std::string filename = saveDeviceFile(scene, dir, start, iteration, ".bloom.png", pt_png_enc_bound(enc),
                                                [&](uint8_t* d_out, int64_t cap, int64_t* d_size) {
        return pt_png_enc_pixels(enc, d_pix, 3, d_out, cap, d_size, nullptr);
    });
    pt_png_enc_destroy(enc);
    pt_display_destroy(disp);
    pt_bloom_destroy(bloom);
    (void)hipFree(d_pix);
    (void)hipFree(d_rgb);
    return filename;
}

void writeFloats(const std::string& path, const std::vector<float>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size() || std::fclose(f)) {
        std::fprintf(stderr, "error: cannot write %s\n", path.c_str());
        std::exit(EXIT_FAILURE);
    }
}

// --aov: gA (normal, material id bits), gB (position, t), albedo, uv as DIR/<imageName>.<plane>.f32
void saveAovs(const Scene& scene, const std::string& dir) {
    const int W = scene.state.camera.res[0], H = scene.state.camera.res[1];
    const size_t n = (size_t)W * H;
    std::vector<float> gA(4 * n), gB(4 * n), alb(4 * n), uv(2 * n);
    if (pt_get_gbuffer(pathtraceContext(), gA.data(), gB.data(), alb.data(), uv.data())) {
        std::fprintf(stderr, "error: G-buffer: %s\n", pt_last_error());
        std::exit(EXIT_FAILURE);
    }
    const std::string base = dir + "/" + scene.state.imageName;
    writeFloats(base + ".gA.f32", gA);
    writeFloats(base + ".gB.f32", gB);
    writeFloats(base + ".albedo.f32", alb);
    writeFloats(base + ".uv.f32", uv);
    FILE* f = std::fopen((base + ".aov.json").c_str(), "w");
    if (!f) {
        std::fprintf(stderr, "error: cannot write %s.aov.json\n", base.c_str());
        std::exit(EXIT_FAILURE);
    }
    const char* names[4] = {"gA", "gB", "albedo", "uv"};
    const int chans[4] = {4, 4, 4, 2};
    std::fprintf(f, "{\"dtype\": \"<f4\", \"planes\": {");
    for (int k = 0; k < 4; ++k)
        std::fprintf(f, "%s\"%s\": {\"file\": \"%s.%s.f32\", \"shape\": [%d, %d, %d]}", k ? ", " : "", names[k],
                     scene.state.imageName.c_str(), names[k], H, W, chans[k]);
    std::fprintf(f, "}}\n");
    std::fclose(f);
    std::printf("wrote %s.{gA,gB,albedo,uv}.f32 and %s.aov.json\n", base.c_str(), base.c_str());
}

// --adaptive: the loop of main() with an update after every iteration and a selection every `every`
int runAdaptive(const Scene& scene, const char* sceneFile, int total, float threshold, int every, const std::string& out_dir,
                const std::string& start, bool png, bool hdr, bool denoise_var) {
    pt_ctx* c = pathtraceContext();
    pt_adaptive_params prm;
    pt_adaptive_params_default(&prm);
    prm.threshold = threshold;
    auto die = [](const char* what) {
        std::fprintf(stderr, "error: %s: %s\n", what, pt_last_error());
        return EXIT_FAILURE;
    };
    if (every < 1) {
        std::fprintf(stderr, "error: --adaptive-every must be >= 1\n");
        return EXIT_FAILURE;
    }
    if (pt_adaptive_enable(c, 1)) return die("adaptive sampling");
    const auto t0 = std::chrono::steady_clock::now();
    int iteration = 0;
    int32_t active = 0, blocks = 0;
    while (iteration < total) {
        ++iteration;
        pathtrace(nullptr, 0, iteration);
        if (pt_adaptive_update(c, 1, nullptr)) return die("adaptive update");
        if (iteration % every == 0 && iteration < total) {
            if (pt_adaptive_select(c, &prm, &active, &blocks)) return die("adaptive select");
            std::printf("iteration %d: %d of %d blocks active\n", iteration, active, blocks);
            if (active == 0) break;
        }
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    pt_stats_t st{};
    if (pt_stats(c, &st)) return die("stats");
    if (pt_adaptive_info(c, nullptr, &blocks, nullptr, nullptr, nullptr)) return die("adaptive info");
    std::vector<uint32_t> nb((size_t)blocks);
    if (pt_adaptive_get(c, nullptr, nullptr, nullptr, nb.data(), nullptr, nullptr)) return die("adaptive state");
    uint32_t lo = nb.empty() ? 0u : nb[0], hi = 0u;
    double sum = 0.0;
    for (uint32_t v : nb) {
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        sum += v;
    }
    std::printf("rendered %d iteration(s) of %s (%dx%d, depth %d) adaptively in %.3f s: %llu segments, samples per "
                "block min %u mean %.2f max %u over %d blocks\n", iteration, sceneFile, scene.state.camera.res[0],
                scene.state.camera.res[1], scene.state.traceDepth, secs, (unsigned long long)st.segments, lo,
                blocks ? sum / blocks : 0.0, hi, blocks);
    std::vector<float> img((size_t)scene.state.camera.res[0] * scene.state.camera.res[1] * 3);
    if (pt_adaptive_image(c, nullptr, img.data(), nullptr)) return die("adaptive image");
    if (png) std::printf("wrote %s\n", saveImage(scene, out_dir, start, iteration, false, img.data(), "adaptive").c_str());
    if (hdr) std::printf("wrote %s\n", saveImage(scene, out_dir, start, iteration, true, img.data(), "adaptive").c_str());
    if (denoise_var) {
        pt_denoise_var_params vp;
        pt_denoise_var_params_default(&vp);
        if (pt_adaptive_image(c, &vp, img.data(), nullptr)) return die("adaptive denoise");
        std::printf("wrote %s\n",
                    saveImage(scene, out_dir, start, iteration, false, img.data(), "adaptive.denoised-var").c_str());
    }
    pathtraceFree();
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string startTimeString = currentTimeString();
    if (argc < 2) {
        std::printf("Usage: %s SCENEFILE.json [--iterations N] [--out DIR] [--sort] [--no-png] [--hdr] [--denoise] "
                    "[--denoise-variance] [--aov DIR] [--adaptive THRESHOLD] [--adaptive-every K] [--device-png] [--device-hdr] "
                    "[--tonemap none|reinhard|aces|hable] [--exposure EV|auto] [--srgb] [--exr] [--exr-half] "
                    "[--env FILE.hdr] [--env-scale X] [--env-rotate X,Y,Z] "
                    "[--bloom STRENGTH] [--bloom-threshold X] [--bloom-levels K]\n", argv[0]);
        return 1;
    }
    const char* sceneFile = argv[1];
    int iterations = -1;
    std::string out_dir, aov_dir;
    bool sort = false, png = true, hdr = false, denoise = false, denoise_var = false, aov = false, adaptive = false;
    bool device_png = false, device_hdr = false, exr = false, exr_half = false;
    float adaptive_threshold = 0.0f;
    int adaptive_every = 4;
    bool display = false;
    pt_display_params dprm;
    pt_display_params_default(&dprm);
    dprm.mirror_x = 1;
    bool bloom = false;
    pt_bloom_params bprm;
    pt_bloom_params_default(&bprm);
    const char* env_file = nullptr;   // --env: a lat-long Radiance .hdr file as the scene's environment (pt_scene_load_environment)
    pt_env_params eprm;
    pt_env_params_default(&eprm);
    for (int i = 2; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--iterations") && i + 1 < argc) iterations = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--out") && i + 1 < argc) out_dir = argv[++i];
        else if (!std::strcmp(argv[i], "--sort")) sort = true;
        else if (!std::strcmp(argv[i], "--no-png")) png = false;
        else if (!std::strcmp(argv[i], "--device-png")) device_png = true;
        else if (!std::strcmp(argv[i], "--device-hdr")) device_hdr = true;
        else if (!std::strcmp(argv[i], "--hdr")) hdr = true;   // also write the saveHDR .hdr file
        else if (!std::strcmp(argv[i], "--exr")) exr = true;
        else if (!std::strcmp(argv[i], "--exr-half")) exr_half = true;
        else if (!std::strcmp(argv[i], "--denoise")) denoise = true;
        else if (!std::strcmp(argv[i], "--denoise-variance")) denoise_var = true;
        else if (!std::strcmp(argv[i], "--aov") && i + 1 < argc) { aov_dir = argv[++i]; aov = true; }
        else if (!std::strcmp(argv[i], "--adaptive") && i + 1 < argc) { adaptive_threshold = (float)std::atof(argv[++i]); adaptive = true; }
        else if (!std::strcmp(argv[i], "--adaptive-every") && i + 1 < argc) adaptive_every = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--env") && i + 1 < argc) env_file = argv[++i];
        else if (!std::strcmp(argv[i], "--env-scale") && i + 1 < argc) eprm.scale = (float)std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--env-rotate") && i + 1 < argc) {
            ++i;
            if (std::sscanf(argv[i], "%f,%f,%f", &eprm.rotate_deg[0], &eprm.rotate_deg[1], &eprm.rotate_deg[2]) != 3) {
                std::fprintf(stderr, "--env-rotate %s: three angles in degrees, X,Y,Z\n", argv[i]);
                return 1;
            }
        }
        else if (!std::strcmp(argv[i], "--tonemap") && i + 1 < argc) {
            const char* names[4] = {"none", "reinhard", "aces", "hable"};   // PT_DISPLAY_NONE .. PT_DISPLAY_HABLE
            int k = 0;
            ++i;
            while (k < 4 && std::strcmp(argv[i], names[k])) ++k;
            if (k == 4) {
                std::fprintf(stderr, "--tonemap %s: none, reinhard, aces or hable\n", argv[i]);
                return 1;
            }
            dprm.curve = k;
            display = true;
        } else if (!std::strcmp(argv[i], "--exposure") && i + 1 < argc) {
            ++i;
            if (!std::strcmp(argv[i], "auto")) {
                dprm.exposure_mode = PT_DISPLAY_AUTO;
            } else {
                char* end = nullptr;
                const double ev = std::strtod(argv[i], &end);
                if (end == argv[i] || *end || !(ev >= -64.0 && ev <= 64.0)) {
                    std::fprintf(stderr, "--exposure %s: a number of stops in -64 .. 64, or auto\n", argv[i]);
                    return 1;
                }
                dprm.exposure_mode = PT_DISPLAY_MANUAL;
                dprm.exposure = (float)std::exp2(ev);
            }
            display = true;
        } else if (!std::strcmp(argv[i], "--srgb")) {
            dprm.transfer = PT_DISPLAY_SRGB;
            display = true;
        } else if ((!std::strcmp(argv[i], "--bloom") || !std::strcmp(argv[i], "--bloom-threshold")) && i + 1 < argc) {
            const bool strength = !std::strcmp(argv[i], "--bloom");
            char* end = nullptr;
            ++i;
            const double v = std::strtod(argv[i], &end);
            if (end == argv[i] || *end || !(v >= 0.0 && v <= 3.0e38)) {
                std::fprintf(stderr, "%s %s: a number >= 0\n", argv[i - 1], argv[i]);
                return 1;
            }
            (strength ? bprm.strength : bprm.threshold) = (float)v;
            bloom = true;
        } else if (!std::strcmp(argv[i], "--bloom-levels") && i + 1 < argc) {
            bprm.levels = std::atoi(argv[++i]);
            if (bprm.levels < 0 || bprm.levels > 12) {
                std::fprintf(stderr, "--bloom-levels %s: 1 .. 12, or 0 for the size's own\n", argv[i]);
                return 1;
            }
            bloom = true;
        }
        else {
            std::fprintf(stderr, "unknown argument %s\n", argv[i]);
            return 1;
        }
    }

    Scene* scene = new Scene(sceneFile);
    if (env_file && pt_scene_load_environment(scene->handle(), env_file, &eprm)) {
        std::fprintf(stderr, "error: --env %s: %s\n", env_file, pt_last_error());
        return EXIT_FAILURE;
    }
    GuiDataContainer* guiData = new GuiDataContainer();
    guiData->sortbyMaterial = sort;
    InitDataContainer(guiData);
    const int total = iterations > 0 ? iterations : (int)scene->state.iterations;

    if (adaptive && bloom) {   // (runAdaptive writes its own files: the flags would be ignored)
        std::fprintf(stderr, "--bloom, --bloom-threshold and --bloom-levels cannot be combined with --adaptive\n");
        return 1;
    }
    pathtraceInit(scene);
    if (adaptive) return runAdaptive(*scene, sceneFile, total, adaptive_threshold, adaptive_every, out_dir, startTimeString,
                                     png, hdr, denoise_var);
    if (denoise_var && pt_track_variance(pathtraceContext(), 1)) {
        std::fprintf(stderr, "error: variance tracking: %s\n", pt_last_error());
        return EXIT_FAILURE;
    }
    const auto t0 = std::chrono::steady_clock::now();
    int iteration = 0;
    while (iteration < total) {
        ++iteration;
        pathtrace(nullptr, 0, iteration);
        if (denoise_var && pt_variance_update(pathtraceContext(), 1.0f, 1, nullptr)) {
            std::fprintf(stderr, "error: variance update: %s\n", pt_last_error());
            return EXIT_FAILURE;
        }
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    pt_stats_t st{};
    (void)st;
    std::printf("rendered %d iteration(s) of %s (%dx%d, depth %d) in %.3f s\n", iteration, sceneFile,
                scene->state.camera.res[0], scene->state.camera.res[1], scene->state.traceDepth, secs);
    if (png)
        std::printf("wrote %s\n", device_png ? saveImageDevice(*scene, out_dir, startTimeString, iteration).c_str()
                                             : saveImage(*scene, out_dir, startTimeString, iteration).c_str());
    if (hdr)
        std::printf("wrote %s\n", device_hdr ? saveHdrDevice(*scene, out_dir, startTimeString, iteration).c_str()
                                             : saveImage(*scene, out_dir, startTimeString, iteration, true).c_str());
    if (display) std::printf("wrote %s\n", saveDisplayDevice(*scene, out_dir, startTimeString, iteration, dprm).c_str());
    if (bloom) std::printf("wrote %s\n", saveBloomDevice(*scene, out_dir, startTimeString, iteration, bprm, dprm).c_str());
    if (exr)
        std::printf("wrote %s\n", saveExrDevice(*scene, out_dir, startTimeString, iteration, aov ? PT_EXR_ALL_LAYERS : PT_EXR_BEAUTY,
                                                exr_half ? PT_EXR_ALL_LAYERS : 0).c_str());
    if (denoise) {
        std::vector<float> dn((size_t)scene->state.camera.res[0] * scene->state.camera.res[1] * 3);
        pt_denoise_params prm;
        pt_denoise_params_default(&prm);
        if (pt_denoise_image(pathtraceContext(), (float)iteration, &prm, dn.data())) {
            std::fprintf(stderr, "error: denoise: %s\n", pt_last_error());
            return EXIT_FAILURE;
        }
        std::printf("wrote %s\n", saveImage(*scene, out_dir, startTimeString, iteration, false, dn.data()).c_str());
        if (hdr) std::printf("wrote %s\n", saveImage(*scene, out_dir, startTimeString, iteration, true, dn.data()).c_str());
    }
    if (denoise_var) {
        std::vector<float> dn((size_t)scene->state.camera.res[0] * scene->state.camera.res[1] * 3);
        int rc;
        if (iteration >= 2) {
            pt_denoise_var_params prm;
            pt_denoise_var_params_default(&prm);
            rc = pt_denoise_image_var(pathtraceContext(), (float)iteration, &prm, dn.data());
        } else {   // one batch gives no variance: the plain filter
            pt_denoise_params prm;
            pt_denoise_params_default(&prm);
            rc = pt_denoise_image(pathtraceContext(), (float)iteration, &prm, dn.data());
        }
        if (rc) {
            std::fprintf(stderr, "error: denoise: %s\n", pt_last_error());
            return EXIT_FAILURE;
        }
        std::printf("wrote %s\n",
                    saveImage(*scene, out_dir, startTimeString, iteration, false, dn.data(), "denoised-var").c_str());
        if (hdr)
            std::printf("wrote %s\n",
                        saveImage(*scene, out_dir, startTimeString, iteration, true, dn.data(), "denoised-var").c_str());
    }
    if (aov) saveAovs(*scene, aov_dir);
    pathtraceFree();
    delete guiData;
    delete scene;
    return 0;
}
