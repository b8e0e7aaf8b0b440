// rlap_ppr_tiles.h -- the tile and group table of the PPR diffusion (rlap_snapshot_ppr, rlap_ppr.hip): where every tile
// (segment, 64 sources) lies in the tile area, which tiles run together as a group, and the sizes the arena is carved from.  Plain
// host functions without any HIP dependency: tests/csrc/ppr_tiles_main.cc compiles this file with g++ and checks the table for
// lists of segment sizes that only a device call could reach otherwise.
//
// A tile of a segment of n nodes holds two n x PPR_TILE float64 copies from XOFF (elements into the tile area).  Tiles of segments up
// to PPR_SMALL_MAX nodes come first (the small regime), then the others; within a regime they follow the segments and, within a
// segment, the sources.  A group is a run of tiles of one regime whose live bytes stay within PPR_TILE_BUDGET and whose count stays
// within GROUP_TILES; a single tile larger than the budget is a group of its own.  ROFF is the tile's first row among the rows of
// its group (one row per node per tile).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rlap {

constexpr int PPR_TILE = 64;                  // sources per tile: one lane each
constexpr int PPR_SMALL_MAX = 4096;           // segments of up to this many nodes run each tile's K steps in one workgroup
constexpr size_t PPR_TILE_BUDGET = (size_t)1 << 30;   // bytes of live tiles (two n_s x 64 float64 copies each) per group

namespace pprtiles {

constexpr int64_t GROUP_TILES = 65535;        // tiles per group (k_pp_init's grid.y)
enum { T_SEG = 0, T_C0 = 1, T_XOFF = 2, T_ROFF = 3, T_FIELDS = 4 };   // tile table: int64 fields per tile

// the tile area in elements: one tile of the largest possible segment, or the budget when the tiles of all segments could exceed it
// (bcap: the blocks the call can hold, at least the nodes of all segments together)
inline int64_t area_elems(int64_t bcap) {
    const int64_t budget = (int64_t)(PPR_TILE_BUDGET / sizeof(double));
    const int64_t one = 2 * PPR_TILE * bcap;
    const int64_t tiles = (bcap + PPR_TILE - 1) / PPR_TILE;
    const int64_t all = (one > 0 && tiles > budget / one) ? budget : one * tiles;   // (min(budget, one * tiles) without the overflow)
    return std::max<int64_t>(one, std::min<int64_t>(budget, all));
}

struct Sizes {
    int64_t tcap;        // tiles the table can hold
    int64_t area;        // elements of the tile area
    int64_t area_rows;   // rows a group can have (the per-row counters)
};

inline Sizes sizes(int64_t bcap, int64_t S) {
    Sizes z;
    z.tcap = bcap / PPR_TILE + std::min<int64_t>(S, bcap) + 1;
    z.area = area_elems(bcap);
    z.area_rows = z.area / (2 * PPR_TILE) + 1;
    return z;
}

struct Table {
    std::vector<int64_t> tab;      // [tiles][T_FIELDS]
    std::vector<int64_t> gstart;   // first tile of each group
    std::vector<int> gsmall;       // the group's regime
    std::vector<int64_t> grows;    // rows of each group
    int64_t small_tiles = 0, large_tiles = 0;
    int64_t ntiles() const { return (int64_t)tab.size() / T_FIELDS; }
    int64_t ngroups() const { return (int64_t)gstart.size(); }
};

// the table of S segments with nodes[s] nodes each (small segments' tiles first)
inline void build(const int64_t* nodes, int64_t S, Table* t) {
    *t = Table{};
    for (int pass = 0; pass < 2; ++pass) {
        int64_t gbytes = 0, groff = 0, ntile_g = 0;
        bool open = false;
        for (int64_t s = 0; s < S; ++s) {
            const int64_t n = nodes[s];
            if (n == 0 || (pass == 0) != (n <= PPR_SMALL_MAX)) continue;
            const int64_t tbytes = 2 * PPR_TILE * n * (int64_t)sizeof(double);
            for (int64_t c0 = 0; c0 < n; c0 += PPR_TILE) {
                if (!open || gbytes + tbytes > (int64_t)PPR_TILE_BUDGET || ntile_g >= GROUP_TILES) {
                    if (open) t->grows.push_back(groff);
                    t->gstart.push_back(t->ntiles());
                    t->gsmall.push_back(pass == 0);
                    gbytes = 0; groff = 0; ntile_g = 0; open = true;
                }
                t->tab.push_back(s); t->tab.push_back(c0); t->tab.push_back(gbytes / (int64_t)sizeof(double)); t->tab.push_back(groff);
                gbytes += tbytes; groff += n; ++ntile_g;
                if (pass == 0) t->small_tiles += 1; else t->large_tiles += 1;
            }
        }
        if (open) t->grows.push_back(groff);
    }
}

// what the run checks before it uploads the table: the tiles fit the table, every group's rows fit the counters, and both copies
// of every tile lie inside the tile area
inline bool fits(const Table& t, const Sizes& z, const int64_t* nodes) {
    if (t.ntiles() > z.tcap) return false;
    for (int64_t g = 0; g < t.ngroups(); ++g) if (t.grows[(size_t)g] > z.area_rows) return false;
    for (int64_t u = 0; u < t.ntiles(); ++u) {
        const int64_t* d = t.tab.data() + u * T_FIELDS;
        if (d[T_XOFF] < 0 || d[T_XOFF] + 2 * PPR_TILE * nodes[d[T_SEG]] > z.area) return false;
    }
    return true;
}

}  // namespace pprtiles
}  // namespace rlap
