// BVH layouts of the walk kernels, built on the host from the flattened reference tree: the device node
// encoding (DNode), the 4-wide collapse k_traverse4 walks (DQuad) and its exact t-cull margins.  Plain
// C++, no device needed: the context (pt_kernels.hip build_quads) uploads the results, and
// pt_scene_bvh_quads / pt_scene_bvh_tcull hand them to the tests.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pt_internal.h"

using namespace ptd;

namespace pt {

// The flattened reference tree (BVH_tree.h:54-61) in the device encoding (DNode).
std::vector<DNode> to_dnodes(const std::vector<pt_bvh_node>& bvh) {
    std::vector<DNode> nodes(bvh.size());
    for (size_t i = 0; i < bvh.size(); ++i) {
        const pt_bvh_node& b = bvh[i];
        const int32_t meta = b.sub_areas > 0 ? b.sub_areas : -(b.axis + 1);
        const int32_t link = b.sub_areas > 0 ? b.first_area_idx : b.rchild_idx;
        for (int k = 0; k < 3; ++k) { nodes[i].lo[k] = b.bmin[k]; nodes[i].hi[k] = b.bmax[k]; }
        nodes[i].lo[3] = bits_to_float(meta);
        nodes[i].hi[3] = bits_to_float(link);
    }
    return nodes;
}

// Every leaf fits the leaf code of the pair and quad layouts: count in the low 8 bits, first above them.
bool leaf_codes_fit(const std::vector<DNode>& nodes) {
    for (const DNode& n : nodes) {
        const int32_t meta = __float_as_int_host(n.lo[3]), link = __float_as_int_host(n.hi[3]);
        if (meta > 255 || (meta > 0 && (link < 0 || (int64_t)link + meta > (int64_t)1 << 23))) return false;
    }
    return true;
}

// The 4-wide layout (DQuad) of the flattened tree `nodes` (DNode encoding: left child = i + 1).
// An interior child X of a quad's node is replaced by its two children when both boxes lie inside
// X's box as floats (the nesting k_traverse4's exactness rests on); otherwise it keeps one slot.
// Also bounds the walk's stack: per quad (valid slots - 1) pushes, summed along the worst path.
// Leaves of zero triangles (never built by the SAH builder) or a bound beyond the stack's capacity
// leave the quad layout off (k_traverse's pair walk runs instead).  So does a leaf the leaf code cannot
// hold, -(first * 256 + count) - 1: more than 255 triangles (a range whose centre box is degenerate is
// one leaf, whatever its size) or a first triangle at 2^23 or beyond; no walk by codes runs then (the
// context builds no pair layout either), only the node-at-a-time walk.
// Host part: fills `quads`, the root's code and the stack bound; false = no quad layout.
bool make_quads(const std::vector<DNode>& nodes, std::vector<DQuad>& quads, int32_t& root_code, int32_t& root_occ,
                std::vector<int32_t>* slot_node) {
    const size_t n = nodes.size();
    quads.clear();
    if (slot_node) slot_node->clear();
    if (n == 0) return false;
    auto meta = [&](size_t i) { return __float_as_int_host(nodes[i].lo[3]); };
    auto link = [&](size_t i) { return __float_as_int_host(nodes[i].hi[3]); };
    for (size_t i = 0; i < n; ++i)
        if (meta(i) == 0 || (meta(i) < 0 && (link(i) <= (int32_t)i + 1 || (size_t)link(i) >= n)))
            return false;   // (a zero-triangle leaf is indistinguishable here; malformed links)
    if (!leaf_codes_fit(nodes)) return false;
    auto inside = [&](size_t in, size_t out) {
        for (int k = 0; k < 3; ++k)
            if (!(nodes[in].lo[k] >= nodes[out].lo[k] && nodes[in].hi[k] <= nodes[out].hi[k])) return false;
        return true;
    };
    std::vector<int32_t> occ;   // stack bound of the walk below each quad
    std::vector<int32_t> qid(n, -1);
    auto leaf_code = [&](size_t i) { return -(link(i) * 256 + meta(i)) - 1; };
    // first pass: assign quad ids in DFS order
    std::vector<size_t> order;
    {
        std::vector<size_t> stk{0};
        if (meta(0) > 0) stk.clear();
        while (!stk.empty()) {
            const size_t i = stk.back();
            stk.pop_back();
            qid[i] = (int32_t)order.size();
            order.push_back(i);
            const size_t ch[2] = {i + 1, (size_t)link(i)};
            std::vector<size_t> kids;
            for (size_t x : ch) {
                if (meta(x) > 0) continue;
                const size_t g[2] = {x + 1, (size_t)link(x)};
                if (inside(g[0], x) && inside(g[1], x)) {
                    for (size_t y : g)
                        if (meta(y) <= 0) kids.push_back(y);
                } else {
                    kids.push_back(x);
                }
            }
            for (auto it = kids.rbegin(); it != kids.rend(); ++it) stk.push_back(*it);
        }
    }
    if (order.size() > (size_t)kQuadIdxMask) return false;
    quads.resize(std::max<size_t>(order.size(), 1));
    if (slot_node) slot_node->assign(4 * quads.size(), -1);
    occ.assign(order.size(), 0);
    // each quad's meta first: the interior codes pointing at a quad carry it
    std::vector<uint32_t> qmeta(order.size(), 0);
    for (size_t qi = 0; qi < order.size(); ++qi) {
        const size_t i = order[qi];
        uint32_t valid = 0, axes[2] = {3u, 3u};
        const size_t ch[2] = {i + 1, (size_t)link(i)};
        for (int g = 0; g < 2; ++g) {
            const size_t x = ch[g];
            if (meta(x) <= 0 && inside(x + 1, x) && inside((size_t)link(x), x)) {
                valid |= 3u << (2 * g);
                axes[g] = (uint32_t)(-meta(x) - 1);
            } else {
                valid |= 1u << (2 * g);
            }
        }
        qmeta[qi] = valid | ((uint32_t)(-meta(i) - 1) << 4) | (axes[0] << 6) | (axes[1] << 8);
    }
    auto qcode = [&](size_t y) { return (int32_t)((uint32_t)qid[y] | (qmeta[(size_t)qid[y]] << kQuadMetaShift)); };
    for (size_t qi = 0; qi < order.size(); ++qi) {
        const size_t i = order[qi];
        DQuad& Q = quads[qi];
        std::memset(&Q, 0, sizeof Q);
        uint32_t valid = 0, axes[2] = {3u, 3u};
        int32_t codes[4] = {0, 0, 0, 0};
        size_t box[4] = {0, 0, 0, 0};
        const size_t ch[2] = {i + 1, (size_t)link(i)};
        for (int g = 0; g < 2; ++g) {
            const size_t x = ch[g];
            auto slot = [&](int s, size_t y) {
                valid |= 1u << s;
                box[s] = y;
                codes[s] = meta(y) > 0 ? leaf_code(y) : qcode(y);
                if (slot_node) (*slot_node)[4 * qi + (size_t)s] = (int32_t)y;
            };
            if (meta(x) <= 0 && inside(x + 1, x) && inside((size_t)link(x), x)) {
                slot(2 * g, x + 1);
                slot(2 * g + 1, (size_t)link(x));
                axes[g] = (uint32_t)(-meta(x) - 1);
            } else {
                slot(2 * g, x);
            }
        }
        for (int s = 0; s < 4; ++s) {
            const DNode& b = nodes[box[s]];
            Q.lox[s] = b.lo[0]; Q.hix[s] = b.hi[0];
            Q.loy[s] = b.lo[1]; Q.hiy[s] = b.hi[1];
            Q.loz[s] = b.lo[2]; Q.hiz[s] = b.hi[2];
            Q.code[s] = bits_to_float(codes[s]);
        }
        const uint32_t m = valid | ((uint32_t)(-meta(i) - 1) << 4) | (axes[0] << 6) | (axes[1] << 8);
        Q.meta[0] = bits_to_float((int32_t)m);
    }
    // stack bound: children quads come later in DFS order, so a reverse sweep sees them first
    root_occ = 0;
    for (size_t qi = order.size(); qi-- > 0;) {
        const DQuad& Q = quads[qi];
        const uint32_t m = (uint32_t)__float_as_int_host(Q.meta[0]);
        int32_t deepest = 0, nv = 0;
        for (int s = 0; s < 4; ++s) {
            if (!((m >> s) & 1u)) continue;
            ++nv;
            const int32_t cd = __float_as_int_host(Q.code[s]);
            if (cd >= 0) deepest = std::max(deepest, occ[(size_t)(cd & kQuadIdxMask)]);
        }
        occ[qi] = nv - 1 + deepest;
        root_occ = occ[qi];
    }
    if (order.empty()) root_occ = 0;
    root_code = meta(0) > 0 ? leaf_code(0) : qcode(0);
    return root_occ <= 64;   // HybStack holds rows + 64 >= 64 entries
}

namespace {
// IEEE binary16 bits of x >= 0 rounded down (toward 0) or up (toward +inf; +inf past the range).
uint16_t half_dir(double x, bool up) {
    if (!(x >= 0.0)) return up ? (uint16_t)0x7c00 : (uint16_t)0;
    auto val = [](uint16_t bits) {
        _Float16 t;
        std::memcpy(&t, &bits, 2);
        return (double)t;
    };
    const _Float16 h = (_Float16)(float)x;
    uint16_t b;
    std::memcpy(&b, &h, 2);
    if (up) {
        while (b < 0x7c00 && val(b) < x) ++b;
    } else {
        while (b > 0 && val(b) > x) --b;
    }
    return b;
}

}  // namespace

// Exact t-cull margins of the 4-wide walk (DESIGN.md §4.3 "exact t-cull").  For a triangle with
// float edges e1, e2 that glm::intersectRayTriangle reports hit (gtx/intersect.inl:37-74: the
// determinant a >= FLT_EPSILON, barycentrics in range), its computed t satisfies
//     t >= (tau_min(B) - (g lambda + 4.8 u) diam / |d|) / (1 + g),   g = c (1 + u) / (1 - c),
//     c = (1 + u)(9 |e1||e2| |d| + 1.74 u),  lambda = 1 + 3.01 u,  diam = max(|e1|, |e2|),
// for every box B that holds the triangle, tau_min(B) = min over B of (X - o).d / |d|^2 (u = 2^-24).
// Per quad slot (a node of the reference tree) with the maxima of |e1||e2| and diam over its
// subtree: the slot's children are culled when A tau_lo > B + best (with relative slack), where
// A = 1 / ((1 + g)(1 + 2^-18)) (|d|^2 in [1 - 2^-18, 1 + 2^-18], checked per ray) rounded down and
// B = (g lambda + 4.8 u) diam / ((1 - 2^-19)(1 + g)) rounded up, both as binary16: one 32-bit word
// per slot, A | B << 16.  c >= 1 (large triangles): A = 0, B = inf, never culled.
// Returns the fraction of valid slots with A >= 1/2 (the share where the cull can pay).
double build_qcull(const std::vector<DNode>& nodes, const std::vector<pt_triangle>& tris,
                   const std::vector<int32_t>& slot_node, std::vector<uint32_t>& qcull) {
    const size_t n = nodes.size();
    std::vector<double> mmax(n, 0.0), dmax(n, 0.0);
    for (size_t i = n; i-- > 0;) {
        const int32_t meta = __float_as_int_host(nodes[i].lo[3]), link = __float_as_int_host(nodes[i].hi[3]);
        if (meta > 0) {
            for (int32_t k = link; k < link + meta && (size_t)k < tris.size(); ++k) {
                const pt_triangle& t = tris[(size_t)k];
                double l1 = 0.0, l2 = 0.0;
                for (int a = 0; a < 3; ++a) {
                    const float e1 = t.v[1][a] - t.v[0][a], e2 = t.v[2][a] - t.v[0][a];   // the device's e1, e2
                    l1 += (double)e1 * e1;
                    l2 += (double)e2 * e2;
                }
                l1 = std::sqrt(l1) * (1.0 + 1e-12);
                l2 = std::sqrt(l2) * (1.0 + 1e-12);
                mmax[i] = std::max(mmax[i], l1 * l2 * (1.0 + 1e-12));
                dmax[i] = std::max(dmax[i], std::max(l1, l2));
                if (!std::isfinite(l1 * l2)) mmax[i] = HUGE_VAL;
            }
        } else if ((size_t)link < n && i + 1 < n) {
            mmax[i] = std::max(mmax[i + 1], mmax[(size_t)link]);
            dmax[i] = std::max(dmax[i + 1], dmax[(size_t)link]);
        }
    }
    const double u = std::ldexp(1.0, -24), lam = 1.0 + 3.01 * u;
    const double dhi = 1.0 + std::ldexp(1.0, -19), dlo = 1.0 - std::ldexp(1.0, -19);
    qcull.assign(slot_node.size(), 0x7c000000u);   // A = 0, B = inf
    size_t valid = 0, good = 0;
    for (size_t k = 0; k < slot_node.size(); ++k) {
        const int32_t y = slot_node[k];
        if (y < 0) continue;
        ++valid;
        const double c = (1.0 + u) * (9.0 * mmax[(size_t)y] * dhi + 1.74 * u);
        if (!(c < 1.0)) continue;
        const double g = c * (1.0 + u) / (1.0 - c);
        const double A = 1.0 / ((1.0 + g) * (1.0 + std::ldexp(1.0, -18))) * (1.0 - 1e-12);
        const double B = (g * lam + 4.8 * u) * dmax[(size_t)y] / (dlo * (1.0 + g)) * (1.0 + 1e-12);
        qcull[k] = (uint32_t)half_dir(A, false) | ((uint32_t)half_dir(B, true) << 16);
        if (A >= 0.5) ++good;
    }
    return valid ? (double)good / (double)valid : 0.0;
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_scene_bvh_quads(const pt_scene* scene, void* out, int32_t cap, int32_t* root_code, int32_t* stack_bound) {
    if (!scene) return -PT_ERR_ARG;
    const auto& S = *reinterpret_cast<const pt::Scene*>(scene);
    std::vector<DQuad> quads;
    int32_t rc = 0, occ = 0;
    if (!make_quads(to_dnodes(S.bvh), quads, rc, occ)) return 0;
    if (root_code) *root_code = rc;
    if (stack_bound) *stack_bound = occ;
    if (out && cap > 0) std::memcpy(out, quads.data(), std::min<size_t>((size_t)cap, quads.size()) * sizeof(DQuad));
    return (int)quads.size();
}

int pt_scene_bvh_tcull(const pt_scene* scene, uint32_t* words, int32_t cap, double* cullable_frac) {
    if (!scene) return -PT_ERR_ARG;
    const auto& S = *reinterpret_cast<const pt::Scene*>(scene);
    std::vector<DQuad> quads;
    std::vector<int32_t> slot_node;
    int32_t rc = 0, occ = 0;
    const std::vector<DNode> nodes = to_dnodes(S.bvh);
    if (!make_quads(nodes, quads, rc, occ, &slot_node)) return 0;
    std::vector<uint32_t> q;
    const double frac = build_qcull(nodes, S.triangles, slot_node, q);
    if (cullable_frac) *cullable_frac = frac;
    if (words && cap > 0) std::memcpy(words, q.data(), std::min<size_t>((size_t)cap, q.size()) * sizeof(uint32_t));
    return (int)q.size();
}

}  // extern "C"
