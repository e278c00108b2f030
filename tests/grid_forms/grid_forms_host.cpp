// CPU driver for the grid build (mirror-maze_amd/csrc/grid_build.cpp, rect_compact.cpp): reads a rect array
// (n x 12 float32: o, v, u, colour), builds its BVH and its grid as mm_upload_scene does, and prints the
// facts of the image it built as one JSON object; dump=PATH also writes the image's bytes.
// Usage: grid_forms_host rects=PATH [cell=PERCENT] [wide=0|1] [merge=0|1] [dump=PATH]
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

using namespace mm;

int main(int argc, char** argv) {
    std::map<std::string, std::string> args;
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            fprintf(stderr, "bad argument %s\n", argv[i]);
            return 2;
        }
        args[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    auto num = [&](const char* key, long dflt) {
        const auto it = args.find(key);
        return it == args.end() ? dflt : strtol(it->second.c_str(), nullptr, 0);
    };
    FILE* f = fopen(args["rects"].c_str(), "rb");
    if (!f) {
        fprintf(stderr, "cannot read rects=%s\n", args["rects"].c_str());
        return 2;
    }
    std::vector<mm_rect> rects;
    mm_rect r;
    while (fread(&r, sizeof r, 1, f) == 1) rects.push_back(r);
    fclose(f);
    const uint32_t n = (uint32_t)rects.size();
    if (n == 0) {
        fprintf(stderr, "no rects\n");
        return 2;
    }
    std::vector<mm_node> nodes(2 * (size_t)n);
    std::vector<uint32_t> idx(n);
    uint32_t n_nodes = 0;
    if (mm_bvh_build(rects.data(), n, nodes.data(), &n_nodes, idx.data()) != MM_OK) return 3;
    GridHost g;
    std::string why;
    const bool ok = build_grid(rects.data(), n, nodes.data(), n_nodes, idx.data(), wavepersist_grid_cap(0), g, why,
                               num("merge", 1) != 0, num("cell", 100) / 100.0, num("wide", 1) != 0);
    if (!ok) {
        printf("{\"ok\": 0, \"n\": %u, \"why\": \"%s\"}\n", n, why.c_str());
        return 0;
    }
    // the longest list and the whole-list flag, from the cell words themselves
    const size_t cells = (size_t)g.n[0] * g.n[1] * g.n[2];
    uint32_t longest = 0;
    int bit63 = 0;
    for (size_t c = 0; c < cells; ++c) {
        uint32_t m;
        if (g.wide) {
            uint64_t w;
            memcpy(&w, &g.image[8 * c], 8);
            const bool whole = (w >> 63) != 0;
            bit63 |= whole;
            m = (uint32_t)(w >> 22) & (whole ? 0x3FFu : 7u);
        } else {
            uint32_t w;
            memcpy(&w, &g.image[4 * c], 4);
            m = w >> 22;
        }
        if (m > longest) longest = m;
    }
    const char* axis_of[4] = {"x", "y", "z", "?"};
    const uint32_t rec_bytes = g.flat_ok ? 16u : 32u;
    std::string glob = "[", axes = "[";
    for (uint32_t j = 0; j < g.n_glob; ++j) {
        uint32_t meta;
        memcpy(&meta, &g.image[g.off_recs + rec_bytes * g.glob[j] + (g.flat_ok ? 12u : 28u)], 4);
        const bool fast = (meta >> 30) == 0u;
        glob += (j ? ", " : "") + std::to_string(g.glob[j]);
        axes += std::string(j ? ", \"" : "\"") + axis_of[fast ? (meta >> 20) & 3u : 3u] + "\"";
    }
    printf("{\"ok\": 1, \"n\": %u, \"cells\": [%d, %d, %d], \"n_glob\": %u, \"glob\": %s], \"glob_axes\": %s], "
           "\"slab\": %d, \"slab_y\": [%.9g, %.9g], \"flat_ok\": %d, \"wide\": %d, \"n_class\": %u, \"n_slow\": %u, "
           "\"longest\": %u, \"bit63\": %d, \"bytes\": %u, \"off_data\": %u, \"off_list\": %u, \"n_list\": %u, "
           "\"off_class\": %u, \"off_recs\": %u, \"off_box\": %u}\n",
           n, g.n[0], g.n[1], g.n[2], g.n_glob, glob.c_str(), axes.c_str(), g.slab, g.slab_y[0], g.slab_y[1], g.flat_ok,
           g.wide, g.n_class, g.n_slow, longest, bit63, g.bytes, g.off_data, g.off_list, g.n_list, g.off_class,
           g.off_recs, g.off_box);
    if (args.count("dump")) {
        FILE* o = fopen(args["dump"].c_str(), "wb");
        if (!o || fwrite(g.image.data(), 1, g.image.size(), o) != g.image.size()) {
            fprintf(stderr, "cannot write dump=%s\n", args["dump"].c_str());
            return 2;
        }
        fclose(o);
    }
    return 0;
}
