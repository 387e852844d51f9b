// pullstar.cpp - see pullstar.h
#include "pullstar.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>

namespace ttsweep {

std::vector<ttsweep_pull_entry> build_pull_star(const ttsweep_fs *fs, int starstart,
                                                int starstop, std::vector<float> *lengths)
{
    // key: offset + bit pattern of the length d, so parallel edges of different
    // length (possible only with a hand-made fs[]) stay separate - also two whose
    // halves round to the same float (subnormal d with an odd last bit)
    std::map<std::tuple<int, int, int, uint32_t>, int> merged;
    for (int l = starstart; l < starstop; l++) {
        const ttsweep_fs &f = fs[l];
        if (f.i == 0 && f.j == 0 && f.k == 0) continue;
        uint32_t db;
        std::memcpy(&db, &f.d, 4);
        merged[std::make_tuple(f.i, f.j, f.k, db)] |= 1;      // forward: centre = c
        merged[std::make_tuple(-f.i, -f.j, -f.k, db)] |= 2;   // reverse: centre = o
    }
    std::vector<ttsweep_pull_entry> out;
    out.reserve(merged.size());
    if (lengths) lengths->clear();
    for (const auto &kv : merged) {
        ttsweep_pull_entry e;
        e.di = std::get<0>(kv.first);
        e.dj = std::get<1>(kv.first);
        e.dk = std::get<2>(kv.first);
        const uint32_t db = std::get<3>(kv.first);
        float d;
        std::memcpy(&d, &db, 4);
        e.h = d * 0.5f;     // exact unless d is subnormal with an odd last bit (half_exact)
        e.flags = kv.second;
        out.push_back(e);
        if (lengths) lengths->push_back(d);
    }
    return out;
}

bool half_exact(float d)
{
    const float h = d * 0.5f;
    return h + h == d;
}

int pull_star_radius(const std::vector<ttsweep_pull_entry> &pull)
{
    int r = 0;
    for (const auto &e : pull)
        r = std::max(r, std::max(std::abs(e.di), std::max(std::abs(e.dj), std::abs(e.dk))));
    return r;
}

} // namespace ttsweep
