// CPU driver for the launch policy of a pixel-list launch (mirror-maze_amd/csrc/mm_plan.cpp plan_pixels): prints
// the plan of the call given on the command line as one JSON object.
// Usage: plan_pixels_test key=value ...   (n, spp, bounce, pipe, fuse, persist, defer, defer_min; all defaulted)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "mm_api.h"
#include "mm_plan.h"

using namespace mm;

int main(int argc, char** argv) {
    std::map<std::string, std::string> a;
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            fprintf(stderr, "bad argument %s\n", argv[i]);
            return 2;
        }
        a[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    auto arg = [&](const char* key, long long dflt) {
        const auto it = a.find(key);
        return it == a.end() ? dflt : strtoll(it->second.c_str(), nullptr, 0);
    };
    PlanOptions o;
    o.pipe = (int)arg("pipe", MM_PIPE_AUTO);
    o.opt_fuse = arg("fuse", 1) != 0;
    o.opt_persist = (int)arg("persist", 2);
    o.opt_defer = (int)arg("defer", -1);
    o.opt_defer_min = (uint32_t)arg("defer_min", 1 << 24);
    mm_ext e{};
    e.spp = (uint32_t)arg("spp", 8);
    e.bounce_limit = (uint32_t)arg("bounce", 8);
    e.mirror_limit = (uint32_t)arg("mirror", 8);
    const LaunchPlan p = plan_pixels(o, e, (uint64_t)arg("n", 1000));
    std::string err;
    for (char ch : p.error) {
        if (ch == '"' || ch == '\\') err += '\\';
        err += ch;
    }
    printf("{\"code\": %d, \"error\": \"%s\", \"defer\": %s, \"ring\": %d, \"fuse\": %s, \"rows_per_batch\": %u, "
           "\"predraw\": %u, \"predraw_pool\": %u}\n",
           p.code, err.c_str(), p.defer ? "true" : "false", p.ring, p.fuse ? "true" : "false", p.rows_per_batch,
           p.predraw, p.predraw_pool);
    return 0;
}
