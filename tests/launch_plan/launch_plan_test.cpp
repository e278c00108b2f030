// CPU driver for the launch policy (mirror-maze_amd/csrc/mm_plan.cpp): builds the maze scene of size n -- or,
// with rects=PATH, the scene of a rect file (n x 12 float32: o, v, u, colour) under its own BVH -- as
// mm_upload_scene does (BVH, compact records, grid), takes its SceneFacts, and prints the plan for the call
// given on the command line as one JSON object.
// Usage: launch_plan_test key=value ...   (keys below; every one has a default)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "grid_build.h"
#include "mm_api.h"
#include "mm_plan.h"
#include "mm_scene.h"

namespace mm {
size_t build_compact_rects(const mm_rect* rects, uint32_t n_rects, const uint32_t* idx, std::vector<uint32_t>& out,
                           size_t* n_slow);
}
using namespace mm;

namespace {

std::map<std::string, std::string> g_args;
long long arg(const char* key, long long dflt) {
    const auto it = g_args.find(key);
    return it == g_args.end() ? dflt : strtoll(it->second.c_str(), nullptr, 0);
}
std::string args(const char* key, const char* dflt) {
    const auto it = g_args.find(key);
    return it == g_args.end() ? dflt : it->second;
}

// "nb": not built; "room+K" / "room-K": what is left beside the staged bytes, plus K; else a byte count
size_t static_lds_arg(const char* key, size_t img) {
    const std::string v = args(key, "0");
    if (v == "nb") return kNotBuilt;
    if (v.rfind("room", 0) == 0) return (size_t)((long long)kLdsPerBlock - (long long)img + strtoll(v.c_str() + 4, nullptr, 0));
    return (size_t)strtoull(v.c_str(), nullptr, 0);
}

std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char ch : s) {
        if (ch == '"' || ch == '\\') o += '\\';
        o += ch;
    }
    return o + "\"";
}

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            fprintf(stderr, "bad argument %s\n", argv[i]);
            return 2;
        }
        g_args[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    // the scene, and what mm_upload_scene derives from it
    mm_scene* s = nullptr;
    mm_scene from_file{};
    std::vector<mm_rect> file_rects;
    std::vector<mm_node> file_nodes;
    std::vector<uint32_t> file_idx;
    const std::string rect_path = args("rects", "");
    if (!rect_path.empty()) {
        FILE* rf = fopen(rect_path.c_str(), "rb");
        if (!rf) {
            fprintf(stderr, "cannot read rects=%s\n", rect_path.c_str());
            return 2;
        }
        mm_rect r;
        while (fread(&r, sizeof r, 1, rf) == 1) file_rects.push_back(r);
        fclose(rf);
        const uint32_t n = (uint32_t)file_rects.size();
        if (n == 0) {
            fprintf(stderr, "no rects\n");
            return 2;
        }
        file_nodes.resize(2 * (size_t)n);
        file_idx.resize(n);
        uint32_t n_nodes = 0;
        if (mm_bvh_build(file_rects.data(), n, file_nodes.data(), &n_nodes, file_idx.data()) != MM_OK) return 3;
        from_file.n_rects = n;
        from_file.rects = file_rects.data();
        from_file.n_nodes = n_nodes;
        from_file.nodes = file_nodes.data();
        from_file.idx = file_idx.data();
        s = &from_file;
    } else if (mm_scene_build((uint32_t)arg("n", 10), 0, &s) != MM_OK) {
        return 3;
    }
    uint32_t interior = 0;
    for (uint32_t i = 0; i < s->n_nodes; ++i) interior += s->nodes[i].count == 0;
    std::vector<uint32_t> recs;
    size_t n_slow = s->n_rects;
    build_compact_rects(s->rects, s->n_rects, s->idx, recs, &n_slow);
    GridHost gh;
    std::string gwhy;
    const bool grid_ok = build_grid(s->rects, s->n_rects, s->nodes, s->n_nodes, s->idx, wavepersist_grid_cap(0), gh,
                                    gwhy, arg("grid_merge", 1) != 0, arg("grid_cell", 100) / 100.0,
                                    arg("grid_wide", 1) != 0);
    SceneFacts f;
    f.grid_ok = grid_ok;
    f.grid_slow = grid_ok && gh.n_slow > 0;
    f.grid_wide = grid_ok && gh.wide;
    f.grid_flat = grid_ok && gh.flat_ok;
    f.lean_ok = n_slow == 0;
    f.n_nodes = 2 + 2 * interior;  // the production layout: pairs from node 2 on
    f.n_rects = s->n_rects;
    if (grid_ok) { f.bytes = gh.bytes; f.off_box = gh.off_box; f.off_data = gh.off_data; }
    f.grid_why = gwhy.c_str();
    // facts a test overrides by hand (scenes the mazes do not give)
    if (arg("grid_ok", 1) == 0) { f.grid_ok = false; f.grid_why = "overridden by the test"; }
    if (arg("lean_ok", 1) == 0) f.lean_ok = false;
    if (arg("grid_slow", 0) != 0) f.grid_slow = true;

    PlanOptions o;
    o.pipe = (int)arg("pipe", MM_PIPE_AUTO);
    o.opt_ww = (int)arg("ww", -1);
    o.opt_lds = arg("lds", 1) != 0;
    o.opt_lds_rects = (int)arg("lds_rects", 1);
    o.opt_fuse = arg("fuse", 1) != 0;
    o.opt_persist = 2;
    o.opt_defer = (int)arg("defer", -1);
    o.opt_defer_min = (uint32_t)arg("defer_min", 1 << 24);

    mm_ext e{};
    e.spp = (uint32_t)arg("spp", 8);
    e.bounce_limit = (uint32_t)arg("bounce", 8);
    e.mirror_limit = (uint32_t)arg("mirror", 8);
    e.flags = (uint32_t)arg("flags", 0);
    const uint32_t w = (uint32_t)arg("w", 1920), h = (uint32_t)arg("h", 1080), n_frames = (uint32_t)arg("frames", 1);
    const std::string multi = args("multi", "");

    printf("{\"facts\": {\"grid_ok\": %d, \"grid_slow\": %d, \"grid_wide\": %d, \"grid_flat\": %d, \"lean_ok\": %d, "
           "\"n_nodes\": %u, \"n_rects\": %u, \"bytes\": %u, \"off_box\": %u, \"off_data\": %u}",
           f.grid_ok, f.grid_slow, f.grid_wide, f.grid_flat, f.lean_ok, f.n_nodes, f.n_rects, f.bytes, f.off_box,
           f.off_data);
    Choice m = choose_method(f, o);
    printf(", \"method\": {\"code\": %d, \"error\": %s, \"form\": %d}", m.code, quoted(m.error).c_str(), m.form);
    if (m.code == MM_OK) {
        m = choose_placement(f, o, m.form);
        printf(", \"placement\": {\"code\": %d, \"error\": %s, \"form\": %d, \"mode\": %d, \"built\": %d, "
               "\"defer_built\": %d, \"staged\": %zu}",
               m.code, quoted(m.error).c_str(), m.form, m.mode, wavepersist_built(m.mode, m.form),
               wavepersist_defer_built(m.mode, m.form), lds_stage_bytes(f, m.mode));
    }
    if (m.code == MM_OK) {
        const size_t img = lds_stage_bytes(f, m.mode);
        const size_t static_lds[2] = {static_lds_arg("s1", img), static_lds_arg("s2", img)};
        const LaunchPlan p = plan_tile(f, o, m.form, m.mode, static_lds, e, w, h, n_frames,
                                       multi.empty() ? nullptr : multi.c_str());
        printf(", \"plan\": {\"code\": %d, \"error\": %s, \"defer\": %d, \"ring\": %d, \"fuse\": %d, \"rows_per_batch\": %u}",
               p.code, quoted(p.error).c_str(), p.defer, p.ring, p.fuse, p.rows_per_batch);
    }
    printf("}\n");
    if (s != &from_file) mm_scene_free(s);
    return 0;
}
