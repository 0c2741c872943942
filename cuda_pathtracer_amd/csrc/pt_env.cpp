// Environment lighting, host side: the Radiance HDR reader, the resampler from a lat-long
// image to the octahedral map, the gutter fill, the rotation matrix, and the scene's entry points.  No
// device code: the lookup is pt_env_dev.h, its stand-alone kernel pt_env.hip.  The format is the public one
// (Ward, "Real Pixels", Graphics Gems II); the reader is the inverse of pt_encode_hdr (pt_image.cpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_internal.h"

namespace pt {
namespace {

constexpr double kPiD = 3.14159265358979323846;
constexpr int kEnvMax = 4096, kEnvDefaultMax = 2048;
constexpr int64_t kMaxPixels = (int64_t)1 << 28;   // of a source image (the reader and pt_scene_set_environment)

// ---- Radiance HDR ------------------------------------------------------------------------------
// One text line of the header starting at pos: [pos, end) without the '\n'; false when no '\n' is left.
bool header_line(const uint8_t* d, int64_t size, int64_t& pos, std::string* line) {
    int64_t e = pos;
    while (e < size && d[e] != '\n') ++e;
    if (e >= size) return false;
    line->assign(reinterpret_cast<const char*>(d + pos), (size_t)(e - pos));
    pos = e + 1;
    return true;
}

// "-Y H +X W" with plain decimal numbers of at most 6 digits each.
bool parse_resolution(const std::string& s, int32_t* W, int32_t* H) {
    size_t p = 0;
    auto lit = [&](const char* t) {
        const size_t n = std::strlen(t);
        if (s.compare(p, n, t) != 0) return false;
        p += n;
        return true;
    };
    auto num = [&](int32_t* out) {
        int64_t v = 0;
        size_t digits = 0;
        while (p < s.size() && s[p] >= '0' && s[p] <= '9' && digits < 7) { v = v * 10 + (s[p] - '0'); ++p; ++digits; }
        if (digits == 0 || digits > 6) return false;
        *out = (int32_t)v;
        return true;
    };
    return lit("-Y ") && num(H) && lit(" +X ") && num(W) && p == s.size() && *W > 0 && *H > 0;
}

inline float rgbe_value(uint8_t m, uint8_t e) { return e ? std::ldexp((float)m, (int)e - 136) : 0.0f; }

int decode_hdr(const uint8_t* d, int64_t size, int32_t* width, int32_t* height, float* out, int64_t cap) {
    int64_t pos = 0;
    std::string line;
    if (!header_line(d, size, pos, &line) || line.compare(0, 2, "#?") != 0)
        return fail(PT_ERR_PARSE, "hdr: no #? signature line");
    bool format = false;
    for (;;) {
        if (!header_line(d, size, pos, &line)) return fail(PT_ERR_PARSE, "hdr: header is not terminated");
        if (line.empty()) break;
        if (line.compare(0, 7, "FORMAT=") == 0) {
            if (line != "FORMAT=32-bit_rle_rgbe") return fail(PT_ERR_PARSE, "hdr: FORMAT is not 32-bit_rle_rgbe");
            format = true;
        }
    }
    if (!format) return fail(PT_ERR_PARSE, "hdr: no FORMAT=32-bit_rle_rgbe line");
    int32_t W = 0, H = 0;
    if (!header_line(d, size, pos, &line) || !parse_resolution(line, &W, &H))
        return fail(PT_ERR_PARSE, "hdr: the resolution line is not \"-Y H +X W\"");
    // Before anything is sized by the header: at most 2^28 pixels, and the rest of the buffer can hold H scanlines
    // in their shortest coding (flat: 4 W bytes; run-length coded: the 4-byte mark and, per channel, 2 bytes per run
    // of at most 127).
    if ((int64_t)W * H > kMaxPixels) return fail(PT_ERR_PARSE, "hdr: more than 2^28 pixels");
    int64_t shortest = (int64_t)W * 4;
    if (W >= 8 && W < 32768) shortest = std::min<int64_t>(shortest, 4 + 4 * 2 * (((int64_t)W + 126) / 127));
    if (size - pos < (int64_t)H * shortest) return fail(PT_ERR_PARSE, "hdr: truncated (fewer bytes than its scanlines need)");
    *width = W;
    *height = H;
    if (!out) return PT_OK;
    if (cap < (int64_t)W * H * 3) return fail(PT_ERR_ARG, "hdr: output buffer too small");
    std::vector<uint8_t> scan((size_t)W * 4);
    for (int y = 0; y < H; ++y) {
        float* row = out + (size_t)y * W * 3;
        const bool rle = W >= 8 && W < 32768 && size - pos >= 4 && d[pos] == 2 && d[pos + 1] == 2 && d[pos + 2] < 128 &&
                         ((int)d[pos + 2] << 8 | (int)d[pos + 3]) == W;
        if (!rle) {   // a flat scanline: W RGBE quadruples
            if (size - pos < (int64_t)W * 4) return fail(PT_ERR_PARSE, "hdr: truncated flat scanline");
            for (int x = 0; x < W; ++x) {
                const uint8_t* q = d + pos + 4 * (int64_t)x;
                for (int k = 0; k < 3; ++k) row[3 * x + k] = rgbe_value(q[k], q[3]);
            }
            pos += (int64_t)W * 4;
            continue;
        }
        pos += 4;
        for (int k = 0; k < 4; ++k) {   // the four channels one after another, each W bytes of runs and literals
            uint8_t* ch = scan.data() + (size_t)k * W;
            int x = 0;
            while (x < W) {
                if (pos >= size) return fail(PT_ERR_PARSE, "hdr: truncated run-length scanline");
                const int n = d[pos++];
                if (n > 128) {
                    const int run = n - 128;
                    if (pos >= size) return fail(PT_ERR_PARSE, "hdr: truncated run");
                    if (run > W - x) return fail(PT_ERR_PARSE, "hdr: run past the end of its scanline");
                    std::memset(ch + x, d[pos++], (size_t)run);
                    x += run;
                } else {
                    if (n == 0) return fail(PT_ERR_PARSE, "hdr: empty literal");
                    if (n > W - x) return fail(PT_ERR_PARSE, "hdr: literal past the end of its scanline");
                    if (size - pos < n) return fail(PT_ERR_PARSE, "hdr: truncated literal");
                    std::memcpy(ch + x, d + pos, (size_t)n);
                    pos += n;
                    x += n;
                }
            }
        }
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < 3; ++k) row[3 * x + k] = rgbe_value(scan[(size_t)k * W + x], scan[(size_t)3 * W + x]);
    }
    return PT_OK;
}

// ---- the map -------------------------------------------------------------------------------------
// R = Rx Ry Rz of the angles in degrees, evaluated in double ((a b + c d) + e f per entry) and rounded once.
void rotation(const float deg[3], float out[9]) {
    double M[3][3][3];
    for (int a = 0; a < 3; ++a) {
        const double t = (double)deg[a] * (kPiD / 180.0);
        const double c = std::cos(t), s = std::sin(t);
        const int u = (a + 1) % 3, v = (a + 2) % 3;   // the plane the axis turns: (y, z), (z, x), (x, y)
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) M[a][r][q] = r == q ? 1.0 : 0.0;
        M[a][u][u] = c;
        M[a][u][v] = -s;
        M[a][v][u] = s;
        M[a][v][v] = c;
    }
    auto mul = [](const double A[3][3], const double B[3][3], double C[3][3]) {
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) C[r][q] = (A[r][0] * B[0][q] + A[r][1] * B[1][q]) + A[r][2] * B[2][q];
    };
    double XY[3][3], R[3][3];
    mul(M[0], M[1], XY);
    mul(XY, M[2], R);
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) out[3 * r + q] = (float)R[r][q];
}

// The octahedral edge rule: a step across an edge of the square lands at the mirrored position along that
// same edge (both are the same direction of the lower half), so gutter texel (-1, j) is interior texel
// (0, n - 1 - j), (n, j) is (n - 1, n - 1 - j), and likewise for the rows; a corner follows from the rule
// applied twice: the opposite corner.
void fill_gutter(std::vector<float>& rgba, int n) {
    const int S = n + 2;
    auto at = [&](int i, int j) { return &rgba[4 * ((size_t)(j + 1) * S + (size_t)(i + 1))]; };
    for (int t = 0; t < n; ++t) {
        std::memcpy(at(-1, t), at(0, n - 1 - t), 16);
        std::memcpy(at(n, t), at(n - 1, n - 1 - t), 16);
        std::memcpy(at(t, -1), at(n - 1 - t, 0), 16);
        std::memcpy(at(t, n), at(n - 1 - t, n - 1), 16);
    }
    std::memcpy(at(-1, -1), at(n - 1, n - 1), 16);
    std::memcpy(at(n, -1), at(0, n - 1), 16);
    std::memcpy(at(-1, n), at(n - 1, 0), 16);
    std::memcpy(at(n, n), at(0, 0), 16);
}

int check_params(const pt_env_params* p, pt_env_params* out) {
    pt_env_params_default(out);
    if (p) *out = *p;
    if (!std::isfinite(out->scale)) return fail(PT_ERR_ARG, "environment: scale is not finite");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(out->rotate_deg[k])) return fail(PT_ERR_ARG, "environment: rotate_deg is not finite");
    if (out->size < 0 || out->size > kEnvMax) return fail(PT_ERR_ARG, "environment: size must be 0 (default) or in 1..4096");
    return PT_OK;
}

// rgb: n * n * 3 interior texels
void install(Scene& S, int n, const float* rgb, const pt_env_params& prm) {
    EnvHost& E = S.env;
    E.n = n;
    E.params = prm;
    E.params.size = n;
    rotation(prm.rotate_deg, E.rot);
    const int St = n + 2;
    E.rgba.assign((size_t)St * St * 4, 0.0f);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            float* q = &E.rgba[4 * ((size_t)(j + 1) * St + (size_t)(i + 1))];
            const float* p = rgb + 3 * ((size_t)j * n + i);
            q[0] = p[0];
            q[1] = p[1];
            q[2] = p[2];
        }
    fill_gutter(E.rgba, n);
}

// The resampler.  Everything in double, one rounding to float32 per channel.
void resample(const float* src, int W, int H, int n, std::vector<float>& out) {
    // a source denser than the map (which spans 4n texels round the horizon and 2n from pole to pole): the mean of
    // fx x fy blocks first (the last block of a row or column may be smaller), fx = ceil(W / 4n), fy = ceil(H / 2n),
    // so that the bilinear taps below skip no source texel in either direction
    const int fx = (W + 4 * n - 1) / (4 * n), fy = (H + 2 * n - 1) / (2 * n);
    int Wr = W, Hr = H;
    std::vector<double> img;
    if (fx > 1 || fy > 1) {
        Wr = (W + fx - 1) / fx;
        Hr = (H + fy - 1) / fy;
        img.assign((size_t)Wr * Hr * 3, 0.0);
        for (int y = 0; y < Hr; ++y)
            for (int x = 0; x < Wr; ++x) {
                const int y1 = std::min(H, (y + 1) * fy), x1 = std::min(W, (x + 1) * fx);
                double acc[3] = {0, 0, 0};
                for (int yy = y * fy; yy < y1; ++yy)
                    for (int xx = x * fx; xx < x1; ++xx)
                        for (int k = 0; k < 3; ++k) acc[k] += (double)src[3 * ((size_t)yy * W + xx) + k];
                const double cnt = (double)(y1 - y * fy) * (double)(x1 - x * fx);
                for (int k = 0; k < 3; ++k) img[3 * ((size_t)y * Wr + x) + k] = acc[k] / cnt;
            }
    } else {
        img.assign(src, src + (size_t)W * H * 3);
    }
    out.resize((size_t)n * n * 3);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const double px = (2.0 * ((double)i + 0.5)) / (double)n - 1.0;
            const double pz = (2.0 * ((double)j + 0.5)) / (double)n - 1.0;
            const double ay = (1.0 - std::fabs(px)) - std::fabs(pz);
            double x = px, z = pz;
            if (ay < 0.0) {
                x = (1.0 - std::fabs(pz)) * (px >= 0.0 ? 1.0 : -1.0);
                z = (1.0 - std::fabs(px)) * (pz >= 0.0 ? 1.0 : -1.0);
            }
            const double len = std::sqrt((x * x + ay * ay) + z * z);
            double cy = ay / len;
            cy = cy < -1.0 ? -1.0 : (cy > 1.0 ? 1.0 : cy);
            const double phi = std::atan2(x, -z), theta = std::acos(cy);
            const double sx = (phi / (2.0 * kPiD) + 0.5) * (double)Wr - 0.5;
            const double sy = (theta / kPiD) * (double)Hr - 0.5;
            const double fx = std::floor(sx), fy = std::floor(sy);
            const double wx = sx - fx, wy = sy - fy;
            auto wrap = [&](long long v) { v %= Wr; return (int)(v < 0 ? v + Wr : v); };
            auto clamp = [&](long long v) { return (int)(v < 0 ? 0 : (v > Hr - 1 ? Hr - 1 : v)); };
            const int xa = wrap((long long)fx), xb = wrap((long long)fx + 1);
            const int ya = clamp((long long)fy), yb = clamp((long long)fy + 1);
            for (int k = 0; k < 3; ++k) {
                const double A = img[3 * ((size_t)ya * Wr + xa) + k], B = img[3 * ((size_t)ya * Wr + xb) + k];
                const double C = img[3 * ((size_t)yb * Wr + xa) + k], D = img[3 * ((size_t)yb * Wr + xb) + k];
                const double top = A + (B - A) * wx, bot = C + (D - C) * wx;
                out[3 * ((size_t)j * n + i) + k] = (float)(top + (bot - top) * wy);
            }
        }
}

}  // namespace

int load_environment_file(Scene& S, const std::string& path, const pt_env_params* params) {
    FILE* fp = std::fopen(path.c_str(), "rb");
    if (!fp) return fail(PT_ERR_IO, "cannot read environment file " + path);
    std::vector<uint8_t> data;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) data.insert(data.end(), buf, buf + got);
    std::fclose(fp);
    int32_t W = 0, H = 0;
    if (int rc = decode_hdr(data.data(), (int64_t)data.size(), &W, &H, nullptr, 0)) return rc;
    std::vector<float> rgb((size_t)W * H * 3);
    if (int rc = decode_hdr(data.data(), (int64_t)data.size(), &W, &H, rgb.data(), (int64_t)rgb.size())) return rc;
    return pt_scene_set_environment(reinterpret_cast<pt_scene*>(&S), W, H, rgb.data(), params);
}

}  // namespace pt

using pt::fail;

extern "C" {

void pt_env_params_default(pt_env_params* p) {
    if (!p) return;
    p->scale = 1.0f;
    p->rotate_deg[0] = p->rotate_deg[1] = p->rotate_deg[2] = 0.0f;
    p->size = 0;
}

int pt_decode_hdr(const uint8_t* data, int64_t size, int32_t* width, int32_t* height, float* out, int64_t cap) {
    if (!data || size < 0 || !width || !height) return fail(PT_ERR_ARG, "bad hdr arguments");
    try {
        return pt::decode_hdr(data, size, width, height, out, cap);
    } catch (const std::bad_alloc&) {
        return fail(PT_ERR_NOMEM, "hdr: out of host memory");
    }
}

int pt_scene_set_environment(pt_scene* s, int32_t W, int32_t H, const float* rgb, const pt_env_params* params) {
    if (!s || !rgb || W <= 0 || H <= 0) return fail(PT_ERR_ARG, "bad environment arguments");
    if ((int64_t)W * H > pt::kMaxPixels) return fail(PT_ERR_ARG, "environment: source larger than 2^28 texels");
    pt_env_params prm;
    if (int rc = pt::check_params(params, &prm)) return rc;
    const int n = prm.size > 0 ? prm.size : std::max(1, std::min(pt::kEnvDefaultMax, H / 2));
    try {
        std::vector<float> tex;
        pt::resample(rgb, W, H, n, tex);
        pt::install(*reinterpret_cast<pt::Scene*>(s), n, tex.data(), prm);
    } catch (const std::bad_alloc&) {
        return fail(PT_ERR_NOMEM, "environment: out of host memory");
    }
    return PT_OK;
}

int pt_scene_set_environment_octa(pt_scene* s, int32_t n, const float* rgb, const pt_env_params* params) {
    if (!s || !rgb) return fail(PT_ERR_ARG, "bad environment arguments");
    if (n < 1 || n > pt::kEnvMax) return fail(PT_ERR_ARG, "environment: n must be in 1..4096");
    pt_env_params prm;
    if (int rc = pt::check_params(params, &prm)) return rc;
    try {
        pt::install(*reinterpret_cast<pt::Scene*>(s), n, rgb, prm);
    } catch (const std::bad_alloc&) {
        return fail(PT_ERR_NOMEM, "environment: out of host memory");
    }
    return PT_OK;
}

int pt_scene_load_environment(pt_scene* s, const char* path, const pt_env_params* params) {
    if (!s || !path) return fail(PT_ERR_ARG, "null argument");
    try {
        return pt::load_environment_file(*reinterpret_cast<pt::Scene*>(s), path, params);
    } catch (const std::bad_alloc&) {
        return fail(PT_ERR_NOMEM, "environment: out of host memory");
    }
}

int pt_scene_clear_environment(pt_scene* s) {
    if (!s) return fail(PT_ERR_ARG, "null scene");
    reinterpret_cast<pt::Scene*>(s)->env = pt::EnvHost{};
    return PT_OK;
}

int pt_scene_get_environment(const pt_scene* s, int32_t* n, pt_env_params* out, float* rgba_padded, int64_t cap) {
    if (!s) return fail(PT_ERR_ARG, "null scene");
    const pt::EnvHost& E = reinterpret_cast<const pt::Scene*>(s)->env;
    if (n) *n = E.n;
    if (out) {
        if (E.n > 0) *out = E.params;
        else pt_env_params_default(out);
    }
    if (rgba_padded && E.n > 0) {
        if (cap < (int64_t)E.rgba.size()) return fail(PT_ERR_ARG, "environment: output buffer too small");
        std::memcpy(rgba_padded, E.rgba.data(), E.rgba.size() * sizeof(float));
    }
    return PT_OK;
}

}  // extern "C"
