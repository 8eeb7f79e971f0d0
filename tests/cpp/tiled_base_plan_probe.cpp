// tiled_base_plan_probe — plan_cascade_tiled with a base level
// (acquire-zarr_amd/csrc/ds_plan.cpp) on the CPU.  Links ds_plan.cpp alone;
// tests/test_tiled_base_plan.py builds it with the host compiler under
// ASan + UBSan and reads its output.
//
// One request per line on stdin, one fused run each:
//   <dtype code> <method> <W> <H> <n_out> <frames> [key=value ...]
// The levels are dense halvings of W x H.  Keys:
//   tiles=R0xC0,R1xC1,...  tile rows x columns of levels 0 .. n_out; a list
//                 shorter than that repeats its last entry (default 64x64)
//   base=0|1      plan with the base level (default 1)
//   flags=0|1     the levels carry zero-scan flags (default 1)
//   toff=BYTES    byte offset of every tile buffer from a 256-byte aligned
//                 address (default 0)
//   stride=ELEMS  a chunk lattice with that tile stride (default: none)
// Per request one line: the plan's format_plan() line, then ` zitems=`, and
// per level L (0 only with a base) ` ntx<L>= nty<L>= pw<L>= ph<L>= cov_w<L>=
// cov_h<L>= zrows<L>= slots<L>= slots_x<L>= clear<L>=`; or `invalid`.
// No buffer is allocated: the planner looks at addresses, never through them.
#include "ds_plan.hh"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <utility>
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
        std::vector<std::pair<uint32_t, uint32_t>> tiles;
        uintptr_t toff = 0;
        uint64_t stride = 0;
        bool flags = true, lattice = false, base = true;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), v = eq == kv.npos ? "" : kv.substr(eq + 1);
            if (k == "tiles") {
                std::istringstream list(v);
                std::string one;
                while (std::getline(list, one, ',')) {
                    uint32_t r = 0, c = 0;
                    if (std::sscanf(one.c_str(), "%ux%u", &r, &c) != 2) {
                        std::fprintf(stderr, "bad tiles: %s\n", text.c_str());
                        return 2;
                    }
                    tiles.emplace_back(r, c);
                }
            } else if (k == "base") {
                base = v != "0";
            } else if (k == "flags") {
                flags = v != "0";
            } else if (k == "toff") {
                toff = uintptr_t(std::strtoull(v.c_str(), nullptr, 10));
            } else if (k == "stride") {
                stride = std::strtoull(v.c_str(), nullptr, 10);
                lattice = true;
            } else {
                std::fprintf(stderr, "unknown key %s: %s\n", k.c_str(), text.c_str());
                return 2;
            }
        }
        if (n_out < 1 || n_out > kMaxFusedLevels) {
            std::fprintf(stderr, "bad n_out: %s\n", text.c_str());
            return 2;
        }
        if (tiles.empty())
            tiles.emplace_back(64u, 64u);
        // made-up addresses 16 MiB apart, 256-byte aligned before the offset
        auto addr = [&](size_t i, uintptr_t off = 0) {
            return reinterpret_cast<void*>((uintptr_t(i + 1) << 24) + off);
        };
        auto tiled_out = [&](int level) {
            const auto& rc = tiles[std::min<size_t>(size_t(level), tiles.size() - 1)];
            TiledOut t{ addr(size_t(level) + 32, toff), rc.first, rc.second,
                        flags ? static_cast<uint8_t*>(addr(size_t(level) + 64)) : nullptr };
            if (lattice) {
                t.frame_offsets = static_cast<const uint64_t*>(addr(size_t(level) + 96));
                t.tile_stride = stride;
            }
            return t;
        };
        std::vector<LevelOut> outs(n_out);
        std::vector<TiledOut> touts(n_out);
        uint32_t w = W, h = H;
        for (int i = 0; i < n_out; ++i) {
            w = (w + 1) / 2;
            h = (h + 1) / 2;
            outs[i] = LevelOut{ nullptr, uint64_t(w) * h, w, h };
            touts[i] = tiled_out(i + 1);
        }
        const TiledOut t0 = tiled_out(0);
        std::string out = "invalid";
        const TiledPlan p =
          plan_cascade_tiled(dtype, method, addr(0), uint64_t(W) * H, W, H, outs.data(),
                             touts.data(), n_out, n, unset, base ? &t0 : nullptr);
        if (p.valid) {
            out = format_plan(p) + " zitems=" + std::to_string(p.zitems);
            for (int L = p.base ? 0 : 1; L <= p.n_out; ++L) {
                const TiledLevelPlan& q = L ? p.lv[L - 1] : p.base_lv;
                const std::string s = std::to_string(L);
                auto field = [&](const char* name, uint64_t v) {
                    out += std::string(" ") + name + s + "=" + std::to_string(v);
                };
                field("ntx", q.ntx);
                field("nty", q.nty);
                field("pw", q.pw);
                field("ph", q.ph);
                field("cov_w", q.cov_w);
                field("cov_h", q.cov_h);
                field("zrows", q.zrows);
                field("slots", q.slots);
                field("slots_x", q.slots_x);
                field("clear", q.clear_flags);
            }
        }
        std::puts(out.c_str());
    }
    return 0;
}
