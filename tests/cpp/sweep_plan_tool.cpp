// Host check of csrc/sweep_plan_math.h (tests/test_sweep_plan_cpu.py builds it with the address and undefined-behaviour
// sanitizers): the arithmetic the brute-force MFMA sweeps share, against literal restatements of the formulas it
// replaced -- the three columns-per-split computations, the two split-count functions and the tile map's word count --
// and the dispatch on a row's length.  Includes nothing else of the library; exit status 0 = every check held.
#include "sweep_plan_math.h"

#include <cstdio>
#include <vector>

using namespace ivfhnsw_gpu_impl;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                printf("FAIL: " __VA_ARGS__); \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

// ---- what the three launchers and the two split functions computed before the header existed
static size_t old_knn_cps(size_t nx, int nsplit)
{
    size_t cps = (nx + nsplit - 1) / nsplit;
    cps = (cps + 31) & ~(size_t)31;
    return cps;
}
static size_t old_exact_cps(size_t nx, int nsplit)
{
    size_t cps = (nx + nsplit - 1) / nsplit;
    cps = (cps + 31) & ~(size_t)31;
    cps = cps ? cps : 32;
    return cps;
}
static size_t old_range_cps(size_t nx, int nsplit)
{
    size_t cps = (nx + nsplit - 1) / nsplit;
    cps = (cps + 31) & ~(size_t)31;
    return cps ? cps : 32;
}
static int old_range_map_words(size_t nx, int nsplit, int map_shift)
{
    const size_t tiles = old_range_cps(nx, nsplit) / 32;
    const size_t bits = (tiles + ((size_t)1 << map_shift) - 1) >> map_shift;
    return (int)((bits + 31) / 32);
}
static int old_knn_splits_for(size_t nq, size_t nx)
{
    const size_t row_blocks = (nq + 127) / 128;
    size_t s = (512 + row_blocks - 1) / row_blocks;
    const size_t max_s = (nx + 4095) / 4096;
    s = s < 1 ? 1 : s;
    s = s > max_s ? max_s : s;
    return (int)(s > 64 ? 64 : s);
}
static int old_exact_rows_per_block(int k) { return k <= 32 ? 128 : 64; }
static int old_exact_splits_for(size_t nq, size_t nx, int k)
{
    const size_t rpb = (size_t)old_exact_rows_per_block(k);
    const size_t row_blocks = (nq + rpb - 1) / rpb;
    size_t s = (512 + row_blocks - 1) / row_blocks;
    const size_t max_s = (nx + 4095) / 4096;
    s = s > max_s ? max_s : s;
    s = s < 1 ? 1 : s;
    return (int)(s > 64 ? 64 : s);
}

int main()
{
    // nx >= 1 over the tile, the shortest-split and the 32-bit boundaries; nq over the strip boundaries (and the
    // workgroup counts at which the split count changes)
    std::vector<size_t> nxs;
    for (size_t c : {(size_t)32, (size_t)4096, (size_t)8192, (size_t)64 * 4096, (size_t)1 << 20, (size_t)10000000,
                     (size_t)1000000000, ((size_t)1 << 32) - 2})
        for (size_t v : {c - 1, c, c + 1})
            if (v >= 1 && v <= ((size_t)1 << 32) - 2)
                nxs.push_back(v);
    nxs.push_back(1);
    nxs.push_back(2);
    const size_t nqs[] = {1, 63, 64, 65, 127, 128, 129, 1000, 16384, 65536, 65537, 1 << 17};

    for (size_t nx : nxs) {
        for (int nsplit = 1; nsplit <= 64; nsplit++) {
            const size_t cps = sweep_cols_per_split(nx, nsplit);
            CHECK(cps == old_knn_cps(nx, nsplit) && cps == old_exact_cps(nx, nsplit) && cps == old_range_cps(nx, nsplit),
                  "sweep_cols_per_split(%zu, %d) = %zu, before %zu / %zu / %zu", nx, nsplit, cps, old_knn_cps(nx, nsplit),
                  old_exact_cps(nx, nsplit), old_range_cps(nx, nsplit));
            // what the kernels rely on: whole tiles, and the splits cover the store
            CHECK(cps % 32 == 0 && cps >= 32 && cps * (size_t)nsplit >= nx, "cps %zu of nx %zu in %d splits", cps, nx, nsplit);
            for (int shift = 0; shift <= 20; shift++) {
                const int w = sweep_map_words(nx, nsplit, shift);
                CHECK(w == old_range_map_words(nx, nsplit, shift), "sweep_map_words(%zu, %d, %d) = %d, before %d", nx, nsplit,
                      shift, w, old_range_map_words(nx, nsplit, shift));
                // one bit per 2^shift tiles: the last tile's bit is inside the words
                CHECK(w >= 1 && (((cps / 32 - 1) >> shift) >> 5) < (size_t)w, "map of %d words, %zu tiles, shift %d", w, cps / 32,
                      shift);
            }
        }
        for (size_t nq : nqs) {
            const int sk = sweep_splits_for(nq, nx, 128);
            CHECK(sk == old_knn_splits_for(nq, nx), "knn: sweep_splits_for(%zu, %zu, 128) = %d, before %d", nq, nx, sk,
                  old_knn_splits_for(nq, nx));
            CHECK(sk >= 1 && sk <= 64, "knn: %d splits", sk);
            for (int k : {1, 32, 33, 100}) {
                const int se = sweep_splits_for(nq, nx, old_exact_rows_per_block(k));
                CHECK(se == old_exact_splits_for(nq, nx, k), "exact: sweep_splits_for(%zu, %zu, k = %d) = %d, before %d", nq, nx, k,
                      se, old_exact_splits_for(nq, nx, k));
                CHECK(se >= 1 && se <= 64, "exact: %d splits", se);
            }
        }
    }
    // an empty store: the exact launchers' value (knn's caller never asks: it passes nx ? nx : 1)
    CHECK(sweep_cols_per_split(0, 1) == 32 && sweep_cols_per_split(0, 64) == 32, "empty store: a split of one tile");
    CHECK(sweep_splits_for(1, 0, 128) == 1 && old_exact_splits_for(1, 0, 1) == 1, "empty store: one split");
    CHECK(sweep_map_words(0, 1, 0) == old_range_map_words(0, 1, 0), "empty store: map words");

    // the dispatcher: NS = ceil(d / 32) for every d the exact launchers accept, every NS reached
    bool reached[9] = {};
    for (int d = 16; d <= 256; d += 16) {
        const int ns = by_row_steps(d, [](auto c) { return (int)decltype(c)::value; });
        CHECK(ns == (d + 31) / 32 && ns >= 1 && ns <= 8, "by_row_steps(%d) chose NS = %d", d, ns);
        if (ns >= 1 && ns <= 8)
            reached[ns] = true;
    }
    for (int ns = 1; ns <= 8; ns++)
        CHECK(reached[ns], "by_row_steps never chose NS = %d", ns);

    if (failures)
        printf("%d checks failed\n", failures);
    else
        printf("sweep_plan ok\n");
    return failures ? 1 : 0;
}
