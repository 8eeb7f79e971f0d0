// volume_tiled_plan_probe — plan_volume_tiled (acquire-zarr_amd/csrc/ds_plan.cpp)
// on the CPU.  Links ds_plan.cpp alone; tests/test_volume_tiled_plan.py builds
// it with the host compiler under ASan + UBSan and reads its output.
//
// One request per line on stdin, one fused run each:
//   <dtype code> <method> <W> <H> <n_out> <planes> [key=value ...]
// The levels are dense halvings of W x H.  Keys:
//   tile=RxC      tile rows x columns of every level (default 64x64)
//   tile2=RxC     level 2's tile shape, where it differs from level 1's
//   flags=0|1     the levels carry zero-scan flags (default 1)
//   toff=BYTES    byte offset of every tile buffer from a 256-byte aligned
//                 address (default 0)
//   stride=ELEMS  a chunk lattice with that tile stride (default: none)
//   zi=N          $AQZ_TILED_ZROWS_PER_WAVE as the planner would have read it
//                 (default: unset)
// Per request one line: the plan's format_plan() line, followed by
// ` clear<L>=0|1` per level, or `invalid`.
// No buffer is allocated: the planner looks at addresses, never through them.
#include "ds_plan.hh"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int
main()
{
    using namespace aqz;
    const LaunchSwitches unset =
      LaunchSwitches::from([](const char*) -> const char* { return nullptr; });
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string kv;
        int dtype = 0, method = 0, n_out = 0;
        uint32_t W = 0, H = 0, n = 0;
        if (!(in >> dtype >> method >> W >> H >> n_out >> n))
            continue; // blank line
        uint32_t tr = 64, tc = 64, tr2 = 0, tc2 = 0;
        uintptr_t toff = 0;
        uint64_t stride = 0;
        bool flags = true, lattice = false;
        LaunchSwitches sw = unset;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), v = eq == kv.npos ? "" : kv.substr(eq + 1);
            if (k == "tile") {
                if (std::sscanf(v.c_str(), "%ux%u", &tr, &tc) != 2) {
                    std::fprintf(stderr, "bad tile: %s\n", text.c_str());
                    return 2;
                }
            } else if (k == "tile2") {
                if (std::sscanf(v.c_str(), "%ux%u", &tr2, &tc2) != 2) {
                    std::fprintf(stderr, "bad tile2: %s\n", text.c_str());
                    return 2;
                }
            } else if (k == "flags") {
                flags = v != "0";
            } else if (k == "toff") {
                toff = uintptr_t(std::strtoull(v.c_str(), nullptr, 10));
            } else if (k == "stride") {
                stride = std::strtoull(v.c_str(), nullptr, 10);
                lattice = true;
            } else if (k == "zi") {
                sw.tiled_zrows_per_wave = std::atoi(v.c_str());
            } else {
                std::fprintf(stderr, "unknown key %s: %s\n", k.c_str(), text.c_str());
                return 2;
            }
        }
        if (n_out < 0 || n_out > 16) {
            std::fprintf(stderr, "bad n_out: %s\n", text.c_str());
            return 2;
        }
        // made-up addresses 16 MiB apart, 256-byte aligned before the offset
        auto addr = [&](size_t i, uintptr_t off = 0) {
            return reinterpret_cast<void*>((uintptr_t(i + 1) << 24) + off);
        };
        std::vector<LevelOut> outs(n_out);
        std::vector<TiledOut> touts(n_out);
        uint32_t w = W, h = H;
        for (int i = 0; i < n_out; ++i) {
            w = (w + 1) / 2;
            h = (h + 1) / 2;
            outs[i] = LevelOut{ nullptr, uint64_t(w) * h, w, h };
            touts[i] = TiledOut{ addr(i + 32, toff), i == 1 && tr2 ? tr2 : tr,
                                 i == 1 && tc2 ? tc2 : tc,
                                 flags ? static_cast<uint8_t*>(addr(i + 64)) : nullptr };
            if (lattice) {
                touts[i].frame_offsets = static_cast<const uint64_t*>(addr(i + 96));
                touts[i].tile_stride = stride;
            }
        }
        std::string out = "invalid";
        const VolumeTiledPlan p = plan_volume_tiled(dtype, method, addr(0), uint64_t(W) * H, W, H,
                                                    outs.data(), touts.data(), n_out, n, sw);
        if (p.valid) {
            out = format_plan(p);
            for (int i = 0; i < p.n_out; ++i)
                out += " clear" + std::to_string(i + 1) + "=" +
                       std::to_string(int(p.lv[i].clear_flags));
        }
        std::puts(out.c_str());
    }
    return 0;
}
