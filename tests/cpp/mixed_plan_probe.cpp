// mixed_plan_probe — plan_pyramid_runs and plan_zrun
// (acquire-zarr_amd/csrc/ds_plan.cpp) on the CPU.  Links ds_plan.cpp alone;
// tests/test_mixed_plan.py builds it with the host compiler under ASan + UBSan
// and reads its output.
//
// One request per line on stdin:
//   runs <n_frames> <w>x<h>x<planes>[*] ...
//     a pyramid, one token per level; `*` marks a level that holds an earlier
//     plane.  Answer: `ok` and one `<class>:<first level>:<levels>:<frames in>`
//     per run (class XYZ, XY or Z), or `refused <reason>`.
//   zrun <dtype code> <method> <elems> <n_out> <planes> [key=value ...]
//     soff=BYTES / ooff=BYTES   byte offset of the source / of every level
//                               from a 256-byte aligned address (default 0)
//     sstride=ELEMS / ostride=ELEMS   frame stride of the source / of every
//                               level (default: elems)
//     Answer: the plan's format_plan() line, or `invalid`.
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
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string what;
        if (!(in >> what))
            continue; // blank line
        if (what == "runs") {
            uint32_t n_frames = 0;
            in >> n_frames;
            std::vector<PyramidLevel> lv;
            std::string tok;
            while (in >> tok) {
                PyramidLevel l;
                l.holds_plane = !tok.empty() && tok.back() == '*';
                if (std::sscanf(tok.c_str(), "%ux%ux%u", &l.w, &l.h, &l.planes) != 3) {
                    std::fprintf(stderr, "bad level: %s\n", text.c_str());
                    return 2;
                }
                lv.push_back(l);
            }
            const PyramidRuns r = plan_pyramid_runs(lv.data(), uint32_t(lv.size()), n_frames);
            if (!r.ok) {
                if (!r.runs.empty() || r.reason.empty()) {
                    std::fprintf(stderr, "refusal with runs or no reason: %s\n", text.c_str());
                    return 3;
                }
                std::puts(("refused " + r.reason).c_str());
                continue;
            }
            std::string out = "ok";
            for (const PyramidRun& q : r.runs) {
                const char* cls = q.cls == kClassXYZ ? "XYZ" : q.cls == kClassXY ? "XY"
                                  : q.cls == kClassZ ? "Z"
                                                     : "none";
                out += " " + std::string(cls) + ":" + std::to_string(q.first) + ":" +
                       std::to_string(q.levels) + ":" + std::to_string(q.frames_in);
            }
            std::puts(out.c_str());
        } else if (what == "zrun") {
            int dtype = 0, method = 0, n_out = 0;
            uint64_t elems = 0;
            uint32_t planes = 0;
            if (!(in >> dtype >> method >> elems >> n_out >> planes)) {
                std::fprintf(stderr, "bad zrun: %s\n", text.c_str());
                return 2;
            }
            uintptr_t soff = 0, ooff = 0;
            uint64_t sstride = elems, ostride = elems;
            std::string kv;
            while (in >> kv) {
                const size_t eq = kv.find('=');
                const std::string k = kv.substr(0, eq);
                const uint64_t v =
                  eq == kv.npos ? 0 : std::strtoull(kv.c_str() + eq + 1, nullptr, 10);
                if (k == "soff")
                    soff = uintptr_t(v);
                else if (k == "ooff")
                    ooff = uintptr_t(v);
                else if (k == "sstride")
                    sstride = v;
                else if (k == "ostride")
                    ostride = v;
                else {
                    std::fprintf(stderr, "unknown key %s: %s\n", k.c_str(), text.c_str());
                    return 2;
                }
            }
            // made-up addresses 1 TiB apart, 256-byte aligned before the offset
            auto addr = [&](size_t i, uintptr_t off) {
                return reinterpret_cast<void*>((uintptr_t(i + 1) << 40) + off);
            };
            // room for a request past the planner's depth: it must refuse, not read
            std::vector<LevelOut> outs(size_t(n_out > 0 ? n_out : 0) + 1);
            for (size_t i = 0; i < outs.size(); ++i)
                outs[i] = LevelOut{ addr(i + 1, ooff), ostride, 0, 0 };
            const ZRunPlan p =
              plan_zrun(dtype, method, addr(0, soff), sstride, elems, outs.data(), n_out, planes);
            std::puts(p.valid ? format_plan(p).c_str() : "invalid");
        } else {
            std::fprintf(stderr, "unknown request: %s\n", text.c_str());
            return 2;
        }
    }
    return 0;
}
