// Host check of the base filter's arithmetic in csrc/sweep_plan_math.h (tests/test_exact_filter_plan_cpu.py builds it
// with the address and undefined-behaviour sanitizers): the rule that picks the form of a filtered sweep, the number of
// pass words, the splits and tile-map words of the compact column space of the list form, and the tile -> pass word map
// of the masked form, each against a literal restatement.  Includes nothing else of the library; exit status 0 = every
// check held.
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

// ---- literal restatements
static int lit_words(size_t n) { return (int)(n / 32 + (n % 32 ? 1 : 0)); }
static size_t lit_cps(size_t nx, int nsplit)
{
    size_t share = nx / nsplit + (nx % nsplit ? 1 : 0);
    while (share % 32)
        share++;
    return share ? share : 32;
}
static int lit_splits(size_t nq, size_t nx, int rows_per_block)
{
    size_t blocks = nq / rows_per_block + (nq % rows_per_block ? 1 : 0);
    size_t s = 512 / blocks + (512 % blocks ? 1 : 0);
    const size_t longest = nx / 4096 + (nx % 4096 ? 1 : 0); // no split shorter than 4096 columns
    if (s > longest)
        s = longest;
    if (s < 1)
        s = 1;
    return (int)(s > 64 ? 64 : s);
}
static int lit_map_words(size_t nx, int nsplit, int shift)
{
    const size_t tiles = lit_cps(nx, nsplit) / 32, per_bit = (size_t)1 << shift;
    const size_t bits = tiles / per_bit + (tiles % per_bit ? 1 : 0);
    return (int)(bits / 32 + (bits % 32 ? 1 : 0));
}

int main()
{
    // the rule: the list (Indirect) exactly when it is kept, npass <= n / 8; the option overrides it either way
    // (the threshold e is taken from the function: n / 8 as a memory bound, or a lower power-of-two fraction of n)
    for (size_t n : {(size_t)8, (size_t)64, (size_t)6001, (size_t)10000000, (size_t)1000000000, ((size_t)1 << 32) - 2}) {
        size_t e = 0, hi = n;
        while (e < hi) { // the largest npass whose list is kept (kept is monotone: checked below at the ends)
            const size_t mid = e + (hi - e + 1) / 2;
            if (sweep_pass_list_kept(mid, n))
                e = mid;
            else
                hi = mid - 1;
        }
        bool fraction = false;
        for (int j = 3; j < 32; j++)
            fraction |= e == n >> j;
        CHECK(fraction && e <= n / 8, "n %zu: the threshold %zu is n / 8 or a lower power-of-two fraction", n, e);
        CHECK(sweep_pass_list_kept(e, n) && sweep_filter_form(e, n, -1) == kSweepColsIndirect, "n %zu: npass = threshold is the list", n);
        CHECK(sweep_pass_list_kept(e - 1, n) && sweep_filter_form(e - 1, n, -1) == kSweepColsIndirect, "n %zu: n/8 - 1", n);
        CHECK(!sweep_pass_list_kept(e + 1, n) && sweep_filter_form(e + 1, n, -1) == kSweepColsMasked, "n %zu: n/8 + 1 is masked", n);
        CHECK(sweep_filter_form(n, n, -1) == kSweepColsMasked && sweep_filter_form(1, n, -1) == kSweepColsIndirect, "n %zu: ends", n);
        for (size_t npass : {(size_t)1, e, e + 1, n}) {
            CHECK(sweep_filter_form(npass, n, 0) == kSweepColsMasked, "n %zu npass %zu: option 0 forces the words", n, npass);
            CHECK(sweep_filter_form(npass, n, 1) == kSweepColsIndirect, "n %zu npass %zu: option 1 forces the list", n, npass);
        }
        // the memory bound the rule stands for: a kept list is at most n / 2 bytes
        CHECK(e * sizeof(uint32_t) <= n / 2, "n %zu: a kept list of %zu bytes", n, e * sizeof(uint32_t));
    }
    for (size_t n = 1; n < 8; n++) // n / 8 == 0: any passing row at all is beyond it
        for (size_t npass = 1; npass <= n; npass++)
            CHECK(!sweep_pass_list_kept(npass, n) && sweep_filter_form(npass, n, -1) == kSweepColsMasked, "n %zu npass %zu", n, npass);
    CHECK(sweep_pass_list_kept(0, 5), "nothing passes: a list of nothing");

    // pass words: one bit per row, 32 to a word
    for (size_t n : {(size_t)1, (size_t)31, (size_t)32, (size_t)33, (size_t)6001, (size_t)1000000000, ((size_t)1 << 32) - 2}) {
        CHECK((int)sweep_pass_words(n) == lit_words(n), "sweep_pass_words(%zu) = %zu, literally %d", n, sweep_pass_words(n), lit_words(n));
        CHECK(sweep_pass_words(n) * 32 >= n && (sweep_pass_words(n) - 1) * 32 < n, "words of %zu rows", n);
    }
    CHECK(sweep_pass_words(0) == 0, "no row, no word");

    // the compact column space of the list form: npass takes the store's place in every formula
    std::vector<size_t> npasses = {0, 1, 31, 32, 33};
    for (size_t k = 1; k <= 70; k += 23)
        for (size_t v : {4096 * k - 1, 4096 * k, 4096 * k + 1})
            npasses.push_back(v);
    for (size_t npass : npasses) {
        for (int nsplit : {1, 2, 5, 7, 64}) {
            const size_t cps = sweep_cols_per_split(npass, nsplit);
            CHECK(cps == lit_cps(npass, nsplit), "cps(%zu, %d) = %zu, literally %zu", npass, nsplit, cps, lit_cps(npass, nsplit));
            CHECK(cps % 32 == 0 && cps >= 32 && cps * (size_t)nsplit >= npass, "cps %zu covers %zu in %d", cps, npass, nsplit);
            for (int shift : {0, 1, 5, 20})
                CHECK(sweep_map_words(npass, nsplit, shift) == lit_map_words(npass, nsplit, shift) &&
                          sweep_map_words(npass, nsplit, shift) >= 1,
                      "map words(%zu, %d, %d)", npass, nsplit, shift);
        }
        for (size_t nq : {(size_t)1, (size_t)129, (size_t)10000})
            for (int rpb : {128, 64}) {
                const int s = sweep_splits_for(nq, npass, rpb);
                CHECK(s == lit_splits(nq, npass, rpb) && s >= 1 && s <= 64, "splits(%zu, %zu, %d) = %d, literally %d", nq, npass, rpb, s,
                      lit_splits(nq, npass, rpb));
            }
    }

    // the masked form: tile t of split s is pass word (c_begin >> 5) + t -- the word's 32 rows are the tile's 32 columns,
    // the words of the splits' tiles are distinct, in order, and reach exactly the last word of the store
    for (size_t n : {(size_t)1, (size_t)33, (size_t)6001, (size_t)200003, (size_t)10000000}) {
        for (int nsplit : {1, 2, 5, 64}) {
            const size_t cps = sweep_cols_per_split(n, nsplit);
            size_t expect = 0;
            for (int s = 0; s < nsplit; s++) {
                const size_t c_begin = (size_t)s * cps < n ? (size_t)s * cps : n;
                const size_t c_end = c_begin + cps < n ? c_begin + cps : n;
                const size_t ntiles = (c_end - c_begin + 31) >> 5;
                CHECK(ntiles == 0 || c_begin % 32 == 0, "n %zu, %d splits: split %d begins at %zu", n, nsplit, s, c_begin);
                for (size_t t = 0; t < ntiles; t += (ntiles > 64 ? ntiles / 7 : 1)) {
                    const size_t w = sweep_tile_word(c_begin, t);
                    CHECK(w * 32 == c_begin + t * 32 && w < sweep_pass_words(n), "n %zu, %d splits: tile %zu of split %d is word %zu", n,
                          nsplit, t, s, w);
                }
                if (ntiles) {
                    CHECK(sweep_tile_word(c_begin, 0) == expect, "n %zu, %d splits: split %d starts at word %zu, not %zu", n, nsplit, s,
                          sweep_tile_word(c_begin, 0), expect);
                    expect = sweep_tile_word(c_begin, ntiles - 1) + 1;
                }
            }
            CHECK(expect == sweep_pass_words(n), "n %zu, %d splits: the tiles end at word %zu of %zu", n, nsplit, expect, sweep_pass_words(n));
        }
    }

    if (failures)
        printf("%d checks failed\n", failures);
    else
        printf("exact_filter ok\n");
    return failures ? 1 : 0;
}
