// CPU driver for the plan of mm_trace_pixel_lists (mirror-maze_amd/csrc/mm_plan.cpp plan_pixel_lists): prints
// the plan of the lists given on the command line as one JSON object -- the per-list spans, the table of first
// chunks the kernel searches, and the list every chunk of the queue belongs to by the host restatement of that
// search (mm_plan.h list_of_chunk).
// Usage: plan_pixel_lists_test offsets=0,1,9 [spp=8] [pipe=0] [fuse=1] [null_offsets=1] [n_lists=N]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mm_api.h"
#include "mm_plan.h"

using namespace mm;

namespace {

std::map<std::string, std::string> g_args;
long long arg(const char* key, long long dflt) {
    const auto it = g_args.find(key);
    return it == g_args.end() ? dflt : strtoll(it->second.c_str(), nullptr, 0);
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
    std::vector<uint64_t> offsets;
    {
        const std::string v = g_args.count("offsets") ? g_args["offsets"] : "0";
        for (size_t at = 0; at <= v.size();) {
            const size_t comma = std::min(v.find(',', at), v.size());
            offsets.push_back(strtoull(v.substr(at, comma - at).c_str(), nullptr, 0));
            at = comma + 1;
        }
    }
    if (arg("zeros", 0) > 0) offsets.assign((size_t)arg("zeros", 0), 0);  // that many empty lists + 1
    // n_lists: the offsets given, unless overridden (0 and 65536 are refused before an offset is read)
    const uint32_t n_lists = (uint32_t)arg("n_lists", (long long)offsets.size() - 1);
    PlanOptions o;
    o.pipe = (int)arg("pipe", MM_PIPE_AUTO);
    o.opt_fuse = arg("fuse", 1) != 0;
    o.opt_persist = 2;
    mm_ext e{};
    e.spp = (uint32_t)arg("spp", 8);
    e.bounce_limit = 8;
    e.mirror_limit = 8;

    const ListsPlan p = plan_pixel_lists(o, e, arg("null_offsets", 0) ? nullptr : offsets.data(), n_lists);
    printf("{\"code\": %d, \"error\": %s, \"fuse\": %d, \"n_entries\": %llu, \"n_chunks\": %u", p.plan.code,
           quoted(p.plan.error).c_str(), p.plan.fuse, (unsigned long long)p.n_entries, p.n_chunks);
    if (p.plan.code == MM_OK) {
        // the table the kernel searches: every list's first chunk, then the queue's chunks
        std::vector<uint32_t> first;
        printf(", \"lists\": [");
        for (size_t f = 0; f < p.lists.size(); ++f) {
            const ListSpan& l = p.lists[f];
            printf("%s[%u, %u, %u, %u, %u]", f ? ", " : "", l.first_chunk, l.n_chunks, l.first_entry, l.n_entries,
                   l.n_paths);
            first.push_back(l.first_chunk);
        }
        first.push_back(p.n_chunks);
        printf("]");
        if (p.n_chunks <= 65536) {  // (the bound cases have millions of chunks: their owners are not printed)
            printf(", \"owner\": [");
            for (uint32_t c = 0; c < p.n_chunks; ++c)
                printf("%s%u", c ? ", " : "", list_of_chunk(first.data(), (uint32_t)p.lists.size(), c));
            printf("]");
        }
    }
    printf("}\n");
    return 0;
}
