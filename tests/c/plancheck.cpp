// plancheck -- replays the keys of tests/golden/kernel_choice.txt (written by
// tools/record_kernel_choice.py on a GPU) through plan_march() and prints, per
// case line, the key and plan_kernel_name().  Links csrc/vr_plan.cpp only; no GPU.
//
//   plancheck < kernel_choice.txt
//
// '@vol NAME nx ny nz', '@view NAME m0 m4 m8', '@frame NAME W H' define names;
// a case line is 'VOL NB METHOD FLAGS VIEW FRAME TILES KNOBS [KERNEL]' with FLAGS
// '-' or any of h (f16), b (baked), a (adopted), z (no layout copy can be made),
// g (method-7 grid (10, 12, 20) instead of the volume's), c (the footprint-count
// pass, which the recording cannot see: test_plan.py's own lines), TILES '-' or the tile
// count of a tile list, KNOBS '-' or KEY=VALUE[,KEY=VALUE...].
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "vr_plan.h"

namespace {

struct Vol { int nx, ny, nz; };
struct View { float m0, m4, m8; };
struct Frame { unsigned w, h; };

std::map<std::string, std::string> g_knobs;  // the case's knobs (plan_march's lookup is a plain function)

const char *knob(const char *key) {
    auto it = g_knobs.find(key);
    return it == g_knobs.end() ? nullptr : it->second.c_str();
}

}  // namespace

int main() {
    std::map<std::string, Vol> vols;
    std::map<std::string, View> views;
    std::map<std::string, Frame> frames;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string a;
        ss >> a;
        if (a == "@vol" || a == "@view" || a == "@frame") {
            std::string name, x, y, z;
            ss >> name >> x >> y >> z;
            if (a == "@vol") vols[name] = {std::atoi(x.c_str()), std::atoi(y.c_str()), std::atoi(z.c_str())};
            if (a == "@view") views[name] = {std::strtof(x.c_str(), nullptr), std::strtof(y.c_str(), nullptr),
                                             std::strtof(z.c_str(), nullptr)};
            if (a == "@frame") frames[name] = {(unsigned)std::atoi(x.c_str()), (unsigned)std::atoi(y.c_str())};
            continue;
        }
        std::string flags, view, frame, tiles, knobs;
        int nb = 0, method = 0;
        ss >> nb >> method >> flags >> view >> frame >> tiles >> knobs;
        if (!ss || !vols.count(a) || !views.count(view) || !frames.count(frame)) {
            std::fprintf(stderr, "plancheck: bad line: %s\n", line.c_str());
            return 2;
        }
        const auto has = [&](char c) { return flags.find(c) != std::string::npos; };
        const Vol &v = vols[a];
        vr::PlanIn in = {};
        in.m0 = views[view].m0;
        in.m4 = views[view].m4;
        in.m8 = views[view].m8;
        in.W = in.CW = frames[frame].w;
        in.H = in.CH = frames[frame].h;
        in.tile_list = tiles != "-";
        in.n_tiles = in.tile_list ? (unsigned)std::atoi(tiles.c_str()) : 0;
        in.method = method;
        in.nb = nb;
        in.nx = v.nx;
        in.ny = v.ny;
        in.nz = v.nz;
        in.owned = !has('a');
        in.f16 = has('h');
        in.baked = has('b');
        // the baked planes' brick pitches: only their side of 2^24 matters (plane_narrow),
        // and these volumes are far below it
        in.plane_sy = 2ull * (uint64_t)((v.nx + 15) / 16 * 16);
        in.plane_sz = in.plane_sy * (uint64_t)((v.ny + 1) / 2);
        in.m7x = has('g') ? 10 : v.nx;
        in.m7y = has('g') ? 12 : v.ny;
        in.m7z = has('g') ? 20 : v.nz;
        in.count = has('c');
        g_knobs.clear();
        if (knobs != "-") {
            std::istringstream ks(knobs);
            std::string kv;
            while (std::getline(ks, kv, ',')) {
                const size_t eq = kv.find('=');
                g_knobs[kv.substr(0, eq)] = kv.substr(eq + 1);
            }
        }
        in.tuning = knob;
        vr::MarchPlan pl = vr::plan_march(in);
        // budget 0: every copy the plan asks for is refused, one request at a time,
        // as render_frame asks
        while (has('z') && pl.layout != vr::kLayoutNone) {
            in.denied |= pl.layout;
            pl = vr::plan_march(in);
        }
        char name[96];
        std::printf("%s %d %d %s %s %s %s %s %s\n", a.c_str(), nb, method, flags.c_str(), view.c_str(),
                    frame.c_str(), tiles.c_str(), knobs.c_str(),
                    vr::plan_kernel_name(pl, name, sizeof name));
    }
    return 0;
}
