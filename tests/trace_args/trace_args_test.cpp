// trace_args_test.cpp — stand-alone host test of the trace and query calls' argument checks
// (mirror-maze_amd/csrc/mm_trace_args.cpp) and of the staging rings' policy (mm_stage_ring.h ring_place): for
// each family every rejection the code makes, with its code and its full message, which check wins when two
// fail, and the accepted neighbours of the rejections.  The buffers are stand-in addresses, never dereferenced;
// only the parameter structs and the offsets are real.
//
//     trace_args_test {tile | lists | aov | query | ring}...      prints "ok <checks>" and returns 0, or says what failed
//
// The cases reach the checks through the five functions below `the calls`, one per entry-point shape.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mm_stage_ring.h"
#include "mm_trace_args.h"

using namespace mm;

// ---- the calls -----------------------------------------------------------------------------------------------
enum Entry { kTile, kFrames, kCameras, kVar, kVarCameras };  // (kVar: mm_trace_tile_var without cameras)
constexpr uint64_t kMaxRays = 0x7FFFFFFFull * 256;           // mm_aov.h aov_max_items()
ArgCheck call_tile(Entry en, const mm_uniform* u, const mm_ext* e, uint32_t n_frames, uint32_t x0, uint32_t y0,
                   uint32_t w, uint32_t h, uint32_t ys, void* out, float* var) {
    const bool cams = en == kCameras || en == kVarCameras;
    return check_trace_tile(cams ? "mm_trace_tile_cameras" : "mm_trace_tile_frames", en == kVar || en == kVarCameras, u,
                            e, n_frames, x0, y0, w, h, ys, out, var);
}
ArgCheck call_pixels(bool var, const mm_uniform* u, const mm_ext* e, const uint32_t* pix, uint64_t n, void* out,
                     float* var_dev) {
    const uint64_t offsets[2] = {0, n};
    uint64_t total = ~0ull;
    const ArgCheck r = check_trace_lists(false, var, u, e, offsets, 1, pix, out, var_dev, total);
    if (total != n) return {-100, "n_entries is not n_pixels"};
    return r;
}
ArgCheck call_lists(const mm_uniform* u, const mm_ext* e, uint32_t n_lists, const uint32_t* pix,
                    const uint64_t* offsets, void* out, float* var_dev) {
    uint64_t total = ~0ull;
    const ArgCheck r = check_trace_lists(true, var_dev != nullptr, u, e, offsets, n_lists, pix, out, var_dev, total);
    // (the total of valid offsets, 0 of refused ones)
    const bool valid = offsets && n_lists >= 1 && n_lists <= 65535 && r.error.find("offsets") == std::string::npos;
    if (total != (valid ? offsets[n_lists] : 0)) return {-100, "n_entries is not the lists' total"};
    return r;
}
ArgCheck call_aov(const mm_uniform* u, bool cams, uint32_t n_frames, uint32_t ml, uint32_t x0, uint32_t y0, uint32_t w,
                  uint32_t h, uint32_t ys, const mm_aov* out) {
    return check_trace_aov(u, cams, n_frames, ml, x0, y0, w, h, ys, out);
}
ArgCheck call_query(const float* rays, uint64_t n, void* hits) { return check_query_rays(rays, n, hits, kMaxRays); }

namespace {

int g_checks = 0, g_failed = 0;

void expect(const ArgCheck& r, int code, const std::string& text, const char* what, int line) {
    ++g_checks;
    if (r.code == code && r.error == text) return;
    ++g_failed;
    printf("line %d: %s\n  got  %d \"%s\"\n  want %d \"%s\"\n", line, what, r.code, r.error.c_str(), code, text.c_str());
}
#define OK(call) expect(call, MM_OK, "", #call, __LINE__)
// the full text, its name included
#define BAD(call, text) expect(call, MM_ERR_INVALID, text, #call, __LINE__)
#define CHECK(cond)                                                \
    do {                                                           \
        ++g_checks;                                                \
        if (!(cond)) {                                             \
            ++g_failed;                                            \
            printf("line %d: %s is false\n", __LINE__, #cond);     \
        }                                                          \
    } while (0)

// Stand-in device buffers 2^45 bytes apart.
template <typename T = float>
T* buf(int i, uint64_t off = 0) { return reinterpret_cast<T*>((1ull << 46) + ((uint64_t)i << 45) + off); }
template <typename T>
T* at(const void* base, uint64_t off) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + off); }

mm_uniform view(float w, float h) {
    mm_uniform u{};
    u.view_w = w;
    u.view_h = h;
    u.chunk_w = 4;
    return u;
}
const float kNan = __builtin_nanf("");

// ---- mm_trace_tile, _frames, _cameras, _var -------------------------------------------------------------------
struct Tile {
    Entry en;
    mm_uniform u = view(320, 180);
    mm_ext e{8, 8, 8, 3, 0, 0};
    uint32_t n = 3, x0 = 4, y0 = 2, w = 6, h = 5, ys = 1;  // 90 pixels in all: 1440 bytes of float4, 360 of RGBA8
    void* out = buf(0);
    float* var = buf(1);
    bool no_u = false, no_e = false;
    ArgCheck operator()() const {
        return call_tile(en, no_u ? nullptr : &u, no_e ? nullptr : &e, n, x0, y0, w, h, ys, out, var);
    }
};

void tile_cases(Entry en) {
    const bool var = en == kVar || en == kVarCameras;
    const std::string T = "mm_trace_tile: ";  // the shared checks say this whichever entry point was used
    const std::string F = en == kCameras || en == kVarCameras ? "mm_trace_tile_cameras: " : "mm_trace_tile_frames: ";
    const std::string V = "mm_trace_tile_var: ";
    Tile good{en};
    if (en == kTile) good.n = 1;
    const uint64_t f4 = 16ull * good.n * 30, f1 = 4ull * good.n * 30;
    Tile t = good;
    OK(t());
    // null arguments, and against a bad view
    t = good; t.no_u = true; BAD(t(), T + "null argument");
    t = good; t.no_e = true; BAD(t(), T + "null argument");
    t = good; t.out = nullptr; BAD(t(), T + "null argument");
    t = good; t.out = nullptr; t.u.view_w = 0.0f; BAD(t(), T + "null argument");
    t = good; t.var = nullptr;
    if (var) BAD(t(), V + "null var_dev"); else OK(t());
    // the view
    for (float bad : {0.0f, 0.5f, -4.0f, 65537.0f, kNan}) {
        t = good; t.u.view_w = bad; BAD(t(), T + "bad view size");
        t = good; t.u.view_h = bad; BAD(t(), T + "bad view size");
    }
    t = good; t.u.view_w = 65536.0f; t.u.view_h = 1.0f; t.y0 = 0; t.h = 1; OK(t());
    t = good; t.u.view_w = 0.0f; t.w = 0; BAD(t(), T + "bad view size");  // (ahead of the empty tile)
    // the tile's shape and spp
    t = good; t.w = 0; BAD(t(), T + "empty tile or bad spp");
    t = good; t.h = 0; BAD(t(), T + "empty tile or bad spp");
    t = good; t.ys = 0; BAD(t(), T + "empty tile or bad spp");
    t = good; t.e.spp = 0; BAD(t(), T + "empty tile or bad spp");
    t = good; t.e.spp = 4097; BAD(t(), T + "empty tile or bad spp");
    t = good; t.e.spp = 4096; OK(t());
    t = good; t.w = 0; t.x0 = 400; BAD(t(), T + "empty tile or bad spp");  // empty wins over outside the frame
    t = good; t.h = 0; t.y0 = 400; BAD(t(), T + "empty tile or bad spp");
    t = good; t.w = 0; t.e.bounce_limit = 40000; BAD(t(), T + "empty tile or bad spp");
    // the limits
    t = good; t.e.bounce_limit = 32768; BAD(t(), T + "bounce or mirror limit above 32767");
    t = good; t.e.mirror_limit = 32768; BAD(t(), T + "bounce or mirror limit above 32767");
    t = good; t.e.bounce_limit = 32767; t.e.mirror_limit = 32767; OK(t());
    t = good; t.e.mirror_limit = 32768; t.x0 = 400; BAD(t(), T + "bounce or mirror limit above 32767");
    // the tile inside the frame
    t = good; t.x0 = 315; BAD(t(), T + "tile outside the frame");
    t = good; t.x0 = 314; OK(t());
    t = good; t.x0 = 0xFFFFFFFFu; BAD(t(), T + "tile outside the frame");  // (no 32-bit wrap)
    t = good; t.y0 = 176; BAD(t(), T + "tile outside the frame");
    t = good; t.y0 = 175; OK(t());
    t = good; t.ys = 44; t.y0 = 3; OK(t());  // rows 3, 47, .., 179: the last row of the frame
    t = good; t.ys = 44; t.y0 = 4; BAD(t(), T + "tile outside the frame");
    t = good; t.ys = 0xFFFFFFFFu; t.h = 0xFFFFFFFFu; BAD(t(), T + "tile outside the frame");
    t = good; t.ys = 1000; t.h = 1; t.y0 = 179; OK(t());  // (a one-row tile: the stride is not used)
    // no frames: under the multi-frame entry point's name, behind the tile checks
    t = good; t.n = 0; BAD(t(), F + "no frames");
    t = good; t.n = 0; t.x0 = 400; BAD(t(), T + "tile outside the frame");
    t = good; t.n = 0; t.e.flags = MM_EXT_RGBA8 | MM_EXT_ACCUMULATE; BAD(t(), F + "no frames");
    // RGBA8 and accumulation, and against misalignment
    t = good; t.e.flags = MM_EXT_RGBA8 | MM_EXT_ACCUMULATE; BAD(t(), T + "MM_EXT_RGBA8 frames cannot accumulate");
    t.out = buf(0, 2); BAD(t(), T + "MM_EXT_RGBA8 frames cannot accumulate");
    t = good; t.e.flags = MM_EXT_COUNT_STATS; OK(t());
    // alignment: a float4 per pixel, or one RGBA8 word
    for (uint64_t off : {1, 2, 4, 8, 12}) { t = good; t.out = buf(0, off); BAD(t(), T + "output not 16-byte aligned"); }
    t = good; t.out = buf(0, 16); OK(t());
    t = good; t.e.flags = MM_EXT_RGBA8; t.out = buf(0, 4); OK(t());  // 4-byte but not 16-byte aligned
    t.out = buf(0, 2); BAD(t(), T + "output not 4-byte aligned");
    // misalignment wins over the variance conditions
    t = good; t.out = buf(0, 4); t.e.spp = 1; t.var = nullptr; BAD(t(), T + "output not 16-byte aligned");
    // the variance conditions, in their order
    t = good; t.e.spp = 1;
    if (var) BAD(t(), V + "a sample variance needs spp >= 2"); else OK(t());
    t = good; t.e.spp = 2; OK(t());
    t = good; t.e.spp = 1; t.e.flags = MM_EXT_ACCUMULATE; t.var = nullptr;
    if (var) BAD(t(), V + "a sample variance needs spp >= 2"); else OK(t());
    t = good; t.e.flags = MM_EXT_ACCUMULATE;
    if (var) BAD(t(), V + "MM_EXT_ACCUMULATE is not supported"); else OK(t());
    t.var = nullptr;
    if (var) BAD(t(), V + "MM_EXT_ACCUMULATE is not supported"); else OK(t());
    t = good; t.var = buf(1, 2);
    if (var) BAD(t(), V + "var_dev not 4-byte aligned"); else OK(t());
    t = good; t.var = buf(1, 4); OK(t());
    t = good; t.var = at<float>(t.out, 2);  // misaligned and overlapping
    if (var) BAD(t(), V + "var_dev not 4-byte aligned"); else OK(t());
    // var_dev against out_dev: n_frames * w * h elements each
    t = good; t.var = at<float>(t.out, 0);
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
    t = good; t.var = at<float>(t.out, f4 - 4);
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
    t = good; t.var = at<float>(t.out, f4); OK(t());  // directly behind the output
    t = good; t.out = at<void>(t.var, f1 / 16 * 16 - 16);
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
    t = good; t.out = at<void>(t.var, (f1 + 15) / 16 * 16); OK(t());
    t = good; t.e.flags = MM_EXT_RGBA8; t.var = at<float>(t.out, f1); OK(t());  // (4 bytes per RGBA8 pixel)
    t.var = at<float>(t.out, f1 - 4);
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
    // (the element count is capped at 2^40, where the plan refuses anyway: the byte counts cannot wrap)
    t = good; t.u = view(65536, 65536); t.x0 = t.y0 = 0; t.w = t.h = 65536; t.n = 0xFFFFFFFFu;
    t.var = at<float>(t.out, (16ull << 40) - 16 * 256 - 4);  // its last element
    if (en == kTile) t.n = 1;
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
}

// ---- mm_trace_pixels, _var and mm_trace_pixel_lists ------------------------------------------------------------
struct Lists {
    bool lists, var;
    mm_uniform u = view(320, 180);
    mm_ext e{8, 8, 8, 3, 0, 0};
    std::vector<uint64_t> off{0, 5, 5, 12};  // (a one-list call: its entries are off.back())
    uint32_t n_lists = 3;
    const uint32_t* pix = buf<uint32_t>(2);
    void* out = buf(0);
    float* vd = buf(1);
    bool no_u = false, no_e = false, no_off = false;
    ArgCheck operator()() const {
        const mm_uniform* up = no_u ? nullptr : &u;
        const mm_ext* ep = no_e ? nullptr : &e;
        if (!lists) return call_pixels(var, up, ep, pix, off.back(), out, vd);
        return call_lists(up, ep, n_lists, pix, no_off ? nullptr : off.data(), out, var ? vd : nullptr);
    }
};

void lists_cases(bool lists, bool var) {
    const std::string N = lists ? "mm_trace_pixel_lists: " : "mm_trace_pixels: ";
    const std::string V = lists ? N : "mm_trace_pixels_var: ";
    const std::string L = lists ? "lists" : "list";
    const Lists good{lists, var};
    const uint64_t f4 = 16 * 12, f1 = 4 * 12;
    Lists t = good;
    OK(t());
    if (lists) {
        // the offsets come first: ahead of null arguments and of everything else
        for (uint32_t n : {0u, 65536u, 0xFFFFFFFFu}) {
            t = good; t.n_lists = n; t.no_u = true; t.out = nullptr; BAD(t(), N + "n_lists outside 1..65535");
        }
        t = good; t.n_lists = 0; t.no_off = true; BAD(t(), N + "n_lists outside 1..65535");
        t = good; t.no_off = true; BAD(t(), N + "null offsets");
        t = good; t.no_off = true; t.no_e = true; t.pix = nullptr; BAD(t(), N + "null offsets");
        t = good; t.off[0] = 1; BAD(t(), N + "offsets[0] is not 0");
        t = good; t.off[0] = 1; t.no_u = true; BAD(t(), N + "offsets[0] is not 0");
        t = good; t.off = {0, 5, 4, 12}; BAD(t(), N + "offsets decrease");
        t = good; t.off = {0, 5, 4, 12}; t.out = nullptr; t.u.view_w = 0.0f; BAD(t(), N + "offsets decrease");
        t = good; t.off = {0, 5, 12, 11}; BAD(t(), N + "offsets decrease");
        t = good; t.off = {3, 2, 4, 12}; BAD(t(), N + "offsets[0] is not 0");
        t = good; t.off.assign(65536, 0); t.off.back() = 12; t.n_lists = 65535; OK(t());
        t = good; t.off = {0, 12}; t.n_lists = 1; OK(t());
    }
    // nothing to do: MM_OK ahead of the null checks and of everything else
    t = good; t.off.assign(t.off.size(), 0); t.no_u = t.no_e = true; t.pix = nullptr; t.out = nullptr; t.vd = nullptr;
    OK(t());
    t = good; t.off.assign(t.off.size(), 0); t.u.view_w = 0.0f; t.e.spp = 0; t.out = buf(0, 2); OK(t());
    // null arguments, and against a bad view
    t = good; t.no_u = true; BAD(t(), N + "null argument");
    t = good; t.no_e = true; BAD(t(), N + "null argument");
    t = good; t.pix = nullptr; BAD(t(), N + "null argument");
    t = good; t.out = nullptr; BAD(t(), N + "null argument");
    t = good; t.pix = nullptr; t.u.view_h = 0.0f; BAD(t(), N + "null argument");
    // the view, spp and the limits: the tile calls' checks on a one-pixel tile
    for (float bad : {0.0f, 0.5f, 65537.0f, kNan}) {
        t = good; t.u.view_w = bad; BAD(t(), N + "bad view size");
        t = good; t.u.view_h = bad; BAD(t(), N + "bad view size");
    }
    t = good; t.u = view(1, 1); OK(t());
    t = good; t.u = view(65536, 65536); OK(t());
    t = good; t.e.spp = 0; BAD(t(), N + "empty tile or bad spp");
    t = good; t.e.spp = 4097; BAD(t(), N + "empty tile or bad spp");
    t = good; t.e.spp = 4096; OK(t());
    t = good; t.e.spp = 0; t.u.view_w = 0.0f; BAD(t(), N + "bad view size");
    t = good; t.e.spp = 0; t.e.bounce_limit = 32768; BAD(t(), N + "empty tile or bad spp");
    t = good; t.e.bounce_limit = 32768; BAD(t(), N + "bounce or mirror limit above 32767");
    t = good; t.e.mirror_limit = 32768; BAD(t(), N + "bounce or mirror limit above 32767");
    t = good; t.e.bounce_limit = t.e.mirror_limit = 32767; OK(t());
    // RGBA8 and accumulation, and against misalignment
    t = good; t.e.flags = MM_EXT_RGBA8 | MM_EXT_ACCUMULATE; BAD(t(), N + "MM_EXT_RGBA8 results cannot accumulate");
    t.pix = buf<uint32_t>(2, 4); BAD(t(), N + "MM_EXT_RGBA8 results cannot accumulate");
    t = good; t.e.flags = MM_EXT_RGBA8 | MM_EXT_ACCUMULATE; t.e.mirror_limit = 40000;
    BAD(t(), N + "bounce or mirror limit above 32767");
    // alignment: 8 bytes for the list, a float4 or an RGBA8 word for the output
    t = good; t.pix = buf<uint32_t>(2, 4); BAD(t(), N + L + " not 8-byte or output not 16-byte aligned");
    t = good; t.pix = buf<uint32_t>(2, 8); OK(t());
    for (uint64_t off : {2, 4, 8}) {
        t = good; t.out = buf(0, off); BAD(t(), N + L + " not 8-byte or output not 16-byte aligned");
    }
    t = good; t.e.flags = MM_EXT_RGBA8; t.out = buf(0, 4); OK(t());  // 4-byte but not 16-byte aligned
    t.out = buf(0, 2); BAD(t(), N + L + " not 8-byte or output not 4-byte aligned");
    t = good; t.e.flags = MM_EXT_RGBA8; t.pix = buf<uint32_t>(2, 4);
    BAD(t(), N + L + " not 8-byte or output not 4-byte aligned");
    // misalignment wins over the variance conditions
    t = good; t.out = buf(0, 4); t.e.spp = 1; t.vd = nullptr;
    BAD(t(), N + L + " not 8-byte or output not 16-byte aligned");
    // the 2^32 refusal: the variance call's, ahead of its conditions (the plain call leaves it to the plan)
    t = good; t.off.back() = 1ull << 32; t.e.spp = 1; t.vd = buf(1, 2);
    if (var) BAD(t(), N + "more paths than one launch holds (2^32)"); else OK(t());
    t = good; t.off.back() = 1ull << 63; t.vd = at<float>(t.out, 0);
    if (var) BAD(t(), N + "more paths than one launch holds (2^32)"); else OK(t());
    t = good; t.off.back() = 0xFFFFFFFFull; OK(t());
    t = good; t.off.back() = 0xFFFFFFFFull; t.e.spp = 1;
    if (var) BAD(t(), V + "a sample variance needs spp >= 2"); else OK(t());
    // the variance conditions, in their order
    t = good; t.e.spp = 1;
    if (var) BAD(t(), V + "a sample variance needs spp >= 2"); else OK(t());
    t = good; t.e.spp = 2; OK(t());
    t = good; t.e.spp = 1; t.e.flags = MM_EXT_ACCUMULATE;
    if (var) BAD(t(), V + "a sample variance needs spp >= 2"); else OK(t());
    t = good; t.e.flags = MM_EXT_ACCUMULATE;
    if (var) BAD(t(), V + "MM_EXT_ACCUMULATE is not supported"); else OK(t());
    if (!lists) {  // (mm_trace_pixel_lists without var_dev is the plain call)
        t = good; t.vd = nullptr;
        if (var) BAD(t(), V + "null var_dev"); else OK(t());
        t = good; t.vd = nullptr; t.e.flags = MM_EXT_ACCUMULATE;
        if (var) BAD(t(), V + "MM_EXT_ACCUMULATE is not supported"); else OK(t());
    }
    t = good; t.vd = buf(1, 2);
    if (var) BAD(t(), V + "var_dev not 4-byte aligned"); else OK(t());
    t = good; t.vd = at<float>(t.out, 2);
    if (var) BAD(t(), V + "var_dev not 4-byte aligned"); else OK(t());
    // var_dev against out_dev: one element per entry
    t = good; t.vd = at<float>(t.out, 0);
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
    t = good; t.vd = at<float>(t.out, f4 - 4);
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
    t = good; t.vd = at<float>(t.out, f4); OK(t());  // directly behind the output
    t = good; t.out = at<void>(t.vd, f1 - 16);
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
    t = good; t.out = at<void>(t.vd, f1); OK(t());
    t = good; t.e.flags = MM_EXT_RGBA8; t.vd = at<float>(t.out, f1); OK(t());
    t.vd = at<float>(t.out, f1 - 4);
    if (var) BAD(t(), V + "var_dev overlaps out_dev"); else OK(t());
}

// ---- mm_trace_aov ------------------------------------------------------------------------------------------------
struct Aov {
    mm_uniform u = view(320, 180);
    bool cams = true;
    uint32_t n = 3, ml = 8, x0 = 4, y0 = 2, w = 6, h = 5, ys = 1;
    mm_aov o{buf(0), buf(1), buf<uint32_t>(2)};
    bool no_u = false, no_o = false;
    ArgCheck operator()() const { return call_aov(no_u ? nullptr : &u, cams, n, ml, x0, y0, w, h, ys, no_o ? nullptr : &o); }
};

// cams: a sequence of three frames with their cameras; else the one frame a call without cameras takes
void aov_cases(bool cams) {
    const std::string N = "mm_trace_aov: ";
    Aov good;
    good.cams = cams;
    good.n = cams ? 3 : 1;
    Aov t = good;
    OK(t());
    t = good; t.no_u = true; BAD(t(), N + "null argument");
    t = good; t.no_o = true; BAD(t(), N + "null argument");
    t = good; t.no_o = true; t.u.view_w = 0.0f; t.n = 0; BAD(t(), N + "null argument");
    t = good; t.o = {nullptr, nullptr, nullptr}; BAD(t(), N + "no output");
    t = good; t.o = {nullptr, nullptr, nullptr}; t.n = 0; BAD(t(), N + "no output");
    for (int keep = 0; keep < 3; ++keep) {  // any one output is enough
        t = good;
        if (keep != 0) t.o.normal_depth = nullptr;
        if (keep != 1) t.o.albedo = nullptr;
        if (keep != 2) t.o.id = nullptr;
        OK(t());
    }
    t = good; t.n = 0; BAD(t(), N + "no frames");
    t = good; t.n = 0; t.cams = false; BAD(t(), N + "no frames");
    t = good; t.cams = false; t.n = 2; BAD(t(), N + "several frames need their cameras");
    t = good; t.cams = false; t.n = 1; OK(t());
    t = good; t.cams = true; t.n = 1; OK(t());
    t = good; t.cams = false; t.n = 2; t.u.view_w = 0.0f; BAD(t(), N + "several frames need their cameras");
    for (float bad : {0.0f, 65537.0f, kNan}) {
        t = good; t.u.view_w = bad; BAD(t(), N + "bad view size");
        t = good; t.u.view_h = bad; BAD(t(), N + "bad view size");
    }
    // (a call without sampling parameters: its own texts)
    t = good; t.w = 0; BAD(t(), N + "empty tile");
    t = good; t.h = 0; BAD(t(), N + "empty tile");
    t = good; t.ys = 0; BAD(t(), N + "empty tile");
    t = good; t.w = 0; t.x0 = 400; BAD(t(), N + "empty tile");
    t = good; t.ml = 32768; BAD(t(), N + "mirror limit above 32767");
    t = good; t.ml = 32767; OK(t());
    t = good; t.ml = 32768; t.y0 = 400; BAD(t(), N + "mirror limit above 32767");
    t = good; t.x0 = 315; BAD(t(), N + "tile outside the frame");
    t = good; t.y0 = 176; BAD(t(), N + "tile outside the frame");
    t = good; t.ys = 44; t.y0 = 3; OK(t());
    t = good; t.ys = 44; t.y0 = 4; BAD(t(), N + "tile outside the frame");
    t = good; t.y0 = 176; t.o.id = buf<uint32_t>(2, 2); BAD(t(), N + "tile outside the frame");
    const std::string mis = N + "float4 outputs not 16-byte or id not 4-byte aligned";
    t = good; t.o.normal_depth = buf(0, 4); BAD(t(), mis);
    t = good; t.o.albedo = buf(1, 8); BAD(t(), mis);
    t = good; t.o.id = buf<uint32_t>(2, 2); BAD(t(), mis);
    t = good; t.o.id = buf<uint32_t>(2, 4); OK(t());
    // more pixels than one launch: w * h up to 2^31 - 1, and its 256-pixel blocks times the frames
    t = good; t.u = view(65536, 65536); t.x0 = t.y0 = 0; t.n = 1; t.w = 65536; t.h = 32768;
    BAD(t(), N + "more pixels than one launch holds");
    t.h = 32767; OK(t());
    t.o.id = buf<uint32_t>(2, 1); t.h = 32768; BAD(t(), mis);  // misalignment comes first
    t = good; t.cams = true; t.u = view(65536, 65536); t.x0 = t.y0 = 0; t.w = 256; t.h = 1; t.n = 0x7FFFFFFFu; OK(t());
    t.w = 257; BAD(t(), N + "more pixels than one launch holds");
    t.w = 256; t.n = 0x80000000u; BAD(t(), N + "more pixels than one launch holds");
}

// ---- mm_query_rays -----------------------------------------------------------------------------------------------
void query_cases() {
    const std::string N = "mm_query_rays: ";
    float* rays = buf(0);
    void* hits = buf(1);
    OK(call_query(rays, 100, hits));
    OK(call_query(nullptr, 0, nullptr));  // nothing to do: ahead of the null checks
    OK(call_query(buf(0, 2), 0, buf(1, 2)));
    BAD(call_query(nullptr, 1, hits), N + "null argument");
    BAD(call_query(rays, 1, nullptr), N + "null argument");
    BAD(call_query(nullptr, kMaxRays + 1, buf(1, 4)), N + "null argument");
    const std::string mis = N + "rays not 16-byte or hits not 8-byte aligned";
    for (uint64_t off = 1; off < 16; ++off) BAD(call_query(buf(0, off), 1, hits), mis);
    for (uint64_t off = 1; off < 8; ++off) BAD(call_query(rays, 1, buf(1, off)), mis);
    OK(call_query(buf(0, 16), 1, buf(1, 8)));
    BAD(call_query(rays, kMaxRays + 1, buf(1, 4)), mis);  // misalignment comes first
    BAD(call_query(rays, kMaxRays + 1, hits), N + "more rays than one launch holds");
    BAD(call_query(rays, ~0ull, hits), N + "more rays than one launch holds");
    OK(call_query(rays, kMaxRays, hits));
}

// ---- the staging rings' policy -----------------------------------------------------------------------------------
// A ring as mm_trace_calls.hip stage() drives it; `unit` words per item of a request.
struct Ring {
    size_t min_cap, wrap_cap, unit;
    size_t cap = 0, next = 0;
    RingPlace take(size_t items) {
        const RingPlace p = ring_place(cap, next, items * unit, min_cap, wrap_cap);
        if (p.grow) cap = p.grow;
        next = p.at + items * unit;
        return p;
    }
};
// The rings as they were before there was one policy, each in its own unit: the camera ring in records (8 to
// 4096), the list ring in words.
struct OldRing {
    size_t min_cap, wrap_cap;
    size_t cap = 0, next = 0;
    bool waited = false;
    size_t take(size_t n) {
        waited = false;
        if (next + n > cap) {
            waited = true;
            if (n > cap || cap < wrap_cap) cap = std::max<size_t>({min_cap, 2 * cap, n});
            next = 0;
        }
        const size_t at = next;
        next += n;
        return at;
    }
};

bool placed(const RingPlace& p, size_t at, bool wait, size_t grow) { return p.at == at && p.wait == wait && p.grow == grow; }
#define PLACE(p, at_, wait_, grow_) CHECK(placed(p, at_, wait_, grow_))

void ring_cases(size_t mn, size_t wrap, size_t unit) {
    // mn, wrap: in items of `unit` words
    const size_t M = mn * unit, W = wrap * unit;
    // from empty, the first request grows to max(min, request)
    { Ring r{M, W, unit}; PLACE(r.take(1), 0, true, M); CHECK(r.cap == M); }
    { Ring r{M, W, unit}; PLACE(r.take(mn), 0, true, M); }
    { Ring r{M, W, unit}; PLACE(r.take(mn + 3), 0, true, (mn + 3) * unit); }
    { Ring r{M, W, unit}; PLACE(r.take(4 * wrap), 0, true, 4 * W); }
    // filling exactly to capacity takes no wait; the next request waits and doubles
    Ring r{M, W, unit};
    r.take(1);
    PLACE(r.take(mn - 2), unit, false, 0);
    PLACE(r.take(1), (mn - 1) * unit, false, 0);
    CHECK(r.next == r.cap);
    PLACE(r.take(1), 0, true, 2 * M);
    PLACE(r.take(2 * mn - 1), unit, false, 0);
    PLACE(r.take(1), 0, true, 4 * M);
    // doubling up to the wrap capacity, by requests of half the ring each
    while (r.cap < W) {
        const size_t half = r.cap / unit / 2, cap = r.cap;
        r.next = 0;
        PLACE(r.take(half), 0, false, 0);
        PLACE(r.take(half), half * unit, false, 0);
        PLACE(r.take(half), 0, true, 2 * cap);
    }
    CHECK(r.cap == W);
    // at the wrap capacity a full ring waits and restarts at 0 without growing
    r.next = 0;
    PLACE(r.take(wrap / 2), 0, false, 0);
    PLACE(r.take(wrap / 2), W / 2, false, 0);
    PLACE(r.take(wrap / 2), 0, true, 0);
    PLACE(r.take(wrap / 2), W / 2, false, 0);
    PLACE(r.take(1), 0, true, 0);
    PLACE(r.take(wrap - 1), unit, false, 0);
    PLACE(r.take(wrap), 0, true, 0);  // a request of the whole ring
    CHECK(r.cap == W);
    // a request larger than a wrap-sized ring grows it: to the request, or to twice the ring where that is more;
    // the larger ring then wraps too
    { Ring s = r; PLACE(s.take(wrap + 5), 0, true, 2 * W); }
    PLACE(r.take(3 * wrap + 5), 0, true, (3 * wrap + 5) * unit);
    PLACE(r.take(wrap), 0, true, 0);
    PLACE(r.take(wrap), W, false, 0);
    CHECK(r.cap == (3 * wrap + 5) * unit);
    // a request larger than a ring below the wrap size: the larger of twice the ring and the request
    { Ring s{M, W, unit}; s.take(1); PLACE(s.take(mn + 1), 0, true, 2 * M); }
    { Ring s{M, W, unit}; s.take(1); PLACE(s.take(3 * mn), 0, true, 3 * M); }
    // the GPU tests' sequences: four requests of half the wrap size; the last lands at 0 of a wrap-sized ring
    Ring g{M, W, unit};
    PLACE(g.take(wrap / 2), 0, true, W / 2);
    PLACE(g.take(wrap / 2), 0, true, W);
    PLACE(g.take(wrap / 2), W / 2, false, 0);
    PLACE(g.take(wrap / 2), 0, true, 0);
}

// The one policy against the two rings it replaced, on a pseudo-random request sequence: the same offsets (the
// camera ring's, measured in words, against the old one's in records), waits and capacities.
void ring_against_old(size_t mn, size_t wrap, size_t unit, size_t align) {
    Ring r{mn * unit, wrap * unit, unit};
    OldRing o{mn, wrap};
    uint32_t x = 12345u;
    bool same = true;
    for (int i = 0; i < 4000 && same; ++i) {
        x = x * 1664525u + 1013904223u;
        const uint32_t k = x >> 8;
        // mostly small requests, some of the ring's order, a few beyond it
        size_t n = k % 16 == 0 ? k % (2 * wrap) + 1 : k % 16 == 1 ? wrap : k % (wrap / 64 + 1) + 1;
        n = (n + align - 1) / align * align;
        const RingPlace p = r.take(n);
        const size_t at = o.take(n);
        same = p.at == at * unit && p.wait == o.waited && r.cap == o.cap * unit && r.next == o.next * unit &&
               p.at % 16 == 0 && p.at + n * unit <= r.cap;
    }
    CHECK(same);
    CHECK(r.cap >= wrap * unit);
}

}  // namespace

int main(int argc, char** argv) {
    for (int a = 1; a < argc || a == 1; ++a) {
    const std::string what = a < argc ? argv[a] : "";
    if (what == "tile") {
        for (Entry en : {kTile, kFrames, kCameras, kVar, kVarCameras}) tile_cases(en);
    } else if (what == "lists") {
        for (bool lists : {false, true})
            for (bool var : {false, true}) lists_cases(lists, var);
    } else if (what == "aov") {
        for (bool cams : {false, true}) aov_cases(cams);
    } else if (what == "query") {
        query_cases();
    } else if (what == "ring") {
        ring_cases(8, 4096, 16);        // cameras: records of kCamStride words
        ring_cases(1024, 1u << 22, 1);  // list tables: words
        ring_against_old(8, 4096, 16, 1);
        ring_against_old(1024, 1u << 22, 1, 16);
    } else {
        printf("usage: trace_args_test tile | lists | aov | query | ring\n");
        return 2;
    }
    }
    if (g_failed) {
        printf("%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
