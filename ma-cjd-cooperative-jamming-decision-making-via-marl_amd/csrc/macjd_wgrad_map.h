// macjd_wgrad_map.h — block map of the staged ROWS reduce (wgrad_reduce_rows_staged_kernel, macjd_wgrad.hip).  Plain
// host C++, no HIP: included by the .hip file and by the stand-alone checker tests/wgrad_map_check.cpp.
//
// The reduce launch's flat item order is problem after problem: M N weight items, then M bias items (the contracted
// problem: 2 N items).  Items are taken in groups of 64 (group g = items [64 g, 64 g + 64), partials[g] = the squares of
// what the group stored).  A FAST block owns four consecutive groups that lie wholly inside the weight items of one ROW
// PRODUCTS problem whose N is within the caps; every other group is one PLAIN block of its own.  The map is a list of
// segments in group order, alternating as the problems demand: at most 2 n + 1 of them.
#pragma once
#include <stdint.h>

namespace macjd {

constexpr int WGMAP_MAX_PROBLEMS = 8;                       // = MACJD_WGRAD_MAX_BATCH (static_assert in macjd_wgrad.hip)
constexpr int WGMAP_MAX_SEG = 2 * WGMAP_MAX_PROBLEMS + 1;
constexpr int WGMAP_GROUP = 64;                             // items per group (= WG_RED)
constexpr int WGMAP_FAST_GROUPS = 4;                        // groups per fast block
constexpr int WGMAP_FAST_ITEMS = WGMAP_GROUP * WGMAP_FAST_GROUPS;
constexpr int WGMAP_N_CAP = 128;                            // widest `inp` row a fast block stages
constexpr int WGMAP_GCOLS = 8;                              // `gout` columns a fast block stages
constexpr int64_t WGMAP_MAX_GROUPS = 8192;                  // above: the plain kernel's grid-stride launch

// 256 consecutive items of an [M, N] problem touch at most (255 / N) + 2 rows m
inline bool wgmap_fast_n(const int N) { return N >= 1 && N <= WGMAP_N_CAP && 255 / N + 2 <= WGMAP_GCOLS; }

struct WgradRowsMap {
    int n_seg;
    int block_start[WGMAP_MAX_SEG + 1];   // prefix of blocks per segment; block_start[n_seg] = blocks of the launch
    int group0[WGMAP_MAX_SEG];            // first group of the segment
    int prob[WGMAP_MAX_SEG];              // fast segment: its problem; plain segment: -1
};

// out_start: prefix of items per problem (n + 1 entries); fast_ok[p]: problem p is ROW PRODUCTS (never the contracted
// one) — M, N its output shape.  Returns the number of blocks, or -1 when the launch is the plain kernel's
// (no group at all, or more than WGMAP_MAX_GROUPS).
inline int wgmap_build(const int n, const int64_t* out_start, const int32_t* M, const int32_t* N, const bool* fast_ok,
                       WgradRowsMap* map) {
    *map = WgradRowsMap{};
    const int64_t groups = (out_start[n] + WGMAP_GROUP - 1) / WGMAP_GROUP;
    if (n < 1 || n > WGMAP_MAX_PROBLEMS || groups < 1 || groups > WGMAP_MAX_GROUPS) return -1;
    int s = 0, blocks = 0;
    int64_t cur = 0;   // first group no segment covers yet
    auto plain_until = [&](const int64_t g) {
        if (g > cur) {
            map->block_start[s] = blocks; map->group0[s] = (int)cur; map->prob[s] = -1;
            blocks += (int)(g - cur); cur = g; ++s;
        }
    };
    for (int p = 0; p < n; ++p) {
        if (!fast_ok[p] || !wgmap_fast_n(N[p])) continue;
        const int64_t w0 = out_start[p], w1 = w0 + (int64_t)M[p] * N[p];   // the weight items
        const int64_t g_lo = (w0 + WGMAP_GROUP - 1) / WGMAP_GROUP;
        const int64_t nb = w1 - g_lo * WGMAP_GROUP >= WGMAP_FAST_ITEMS ? (w1 - g_lo * WGMAP_GROUP) / WGMAP_FAST_ITEMS : 0;
        if (nb < 1) continue;
        plain_until(g_lo);
        map->block_start[s] = blocks; map->group0[s] = (int)g_lo; map->prob[s] = p;
        blocks += (int)nb; cur = g_lo + nb * WGMAP_FAST_GROUPS; ++s;
    }
    plain_until(groups);
    map->n_seg = s;
    for (int q = s; q <= WGMAP_MAX_SEG; ++q) map->block_start[q] = blocks;
    return blocks;
}

}  // namespace macjd
