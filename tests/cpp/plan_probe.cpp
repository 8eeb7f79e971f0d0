// plan_probe — the launch planner (acquire-zarr_amd/csrc/ds_plan.cpp) on the
// CPU.  Links ds_plan.cpp alone; tests/test_launch_plan.py builds it with the
// host compiler under ASan + UBSan and reads its output.
//
// One request per line on stdin:
//   <family> <dtype code> <method> <W> <H> <n_out> <frames | planes> [key=value ...]
// family is cascade, tiled or volume.  The levels are dense halvings of W x H
// (frame stride w * h).  Keys:
//   off=b0,b1,...   byte offset of the source (b0) and of each level's buffer
//                   from a 256-byte aligned address (default 0)
//   tile=RxC        tile rows x columns of every level (tiled; default 64x64)
//   flags=0|1       tiled levels carry zero-scan flags (default 1)
//   lds=BYTES       the device LDS cap handed to plan_cascade (default 160 KiB - 16)
//   AQZ_*=value     switches of this request's LaunchSwitches (the
//                   environment is never read)
// Per request one line: the plan's format_plan() line, or `invalid`.
// No buffer is allocated: the planner looks at addresses, never through them.
#include "ds_plan.hh"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

int
main()
{
    using namespace aqz;
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string family, kv;
        int dtype = 0, method = 0, n_out = 0;
        uint32_t W = 0, H = 0, n = 0;
        if (!(in >> family >> dtype >> method >> W >> H >> n_out >> n))
            continue; // blank line
        std::map<std::string, std::string> env;
        std::vector<uintptr_t> off;
        uint32_t tr = 64, tc = 64, lds = 160 * 1024 - 16;
        bool flags = true;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), v = eq == kv.npos ? "" : kv.substr(eq + 1);
            if (k.rfind("AQZ_", 0) == 0) {
                env[k] = v;
            } else if (k == "off") {
                std::istringstream o(v);
                for (std::string s; std::getline(o, s, ',');)
                    off.push_back(uintptr_t(std::strtoull(s.c_str(), nullptr, 10)));
            } else if (k == "tile") {
                if (std::sscanf(v.c_str(), "%ux%u", &tr, &tc) != 2) {
                    std::fprintf(stderr, "bad tile: %s\n", text.c_str());
                    return 2;
                }
            } else if (k == "flags") {
                flags = v != "0";
            } else if (k == "lds") {
                lds = uint32_t(std::strtoul(v.c_str(), nullptr, 10));
            } else {
                std::fprintf(stderr, "unknown key %s: %s\n", k.c_str(), text.c_str());
                return 2;
            }
        }
        if (n_out < 0 || n_out > 16) {
            std::fprintf(stderr, "bad n_out: %s\n", text.c_str());
            return 2;
        }
        const LaunchSwitches sw = LaunchSwitches::from([&](const char* name) -> const char* {
            const auto it = env.find(name);
            return it == env.end() ? nullptr : it->second.c_str();
        });
        // made-up addresses 16 MiB apart, 256-byte aligned before the offset
        auto addr = [&](size_t i) {
            return reinterpret_cast<void*>((uintptr_t(i + 1) << 24) + (i < off.size() ? off[i] : 0));
        };
        std::vector<LevelOut> outs(n_out);
        std::vector<TiledOut> touts(n_out);
        uint32_t w = W, h = H;
        for (int i = 0; i < n_out; ++i) {
            w = (w + 1) / 2;
            h = (h + 1) / 2;
            outs[i] = LevelOut{addr(i + 1), uint64_t(w) * h, w, h};
            touts[i] = TiledOut{addr(i + 32), tr, tc,
                                flags ? static_cast<uint8_t*>(addr(i + 64)) : nullptr};
        }
        const uint64_t frame = uint64_t(W) * H;
        std::string out = "invalid";
        if (family == "cascade") {
            const CascadePlan p = plan_cascade(dtype, method, addr(0), frame, W, H, outs.data(),
                                               n_out, n, lds, sw);
            if (p.valid)
                out = format_plan(p);
        } else if (family == "tiled") {
            const TiledPlan p = plan_cascade_tiled(dtype, method, addr(0), frame, W, H,
                                                   outs.data(), touts.data(), n_out, n, sw);
            if (p.valid)
                out = format_plan(p);
        } else if (family == "volume") {
            const VolumePlan p = plan_volume(dtype, method, addr(0), frame, W, H, outs.data(),
                                             n_out, n, sw);
            if (p.valid)
                out = format_plan(p);
        } else {
            std::fprintf(stderr, "unknown family: %s\n", text.c_str());
            return 2;
        }
        std::puts(out.c_str());
    }
    return 0;
}
