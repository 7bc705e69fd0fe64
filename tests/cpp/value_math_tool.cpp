// Host check of csrc/value_math.h (tests/test_value_math_cpu.py builds it with the address and undefined-behaviour
// sanitizers as a stand-alone program): the fill a query's pair becomes and the pass predicate of the row values against
// the plain rule lo <= v && v <= hi, over the whole cross product of the boundary values, inverted intervals included,
// with and without a table.  Without a table every row counts as 0xffffffff whatever word was loaded.  Includes nothing
// else of the library; exit status 0 = every check held.
#include "value_math.h"

#include <stdint.h>
#include <stdio.h>

using namespace ivfhnsw_gpu_impl;

static int failures = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            failures++;                                                                                                \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                                \
            printf(__VA_ARGS__);                                                                                       \
            printf("\n");                                                                                              \
        }                                                                                                              \
    } while (0)

static const uint32_t kEdge[] = {0u, 1u, 76u, 77u, 78u, 0xffffu, 0x10000u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
static const int kEdges = (int)(sizeof(kEdge) / sizeof(kEdge[0]));

// the rule, in 64-bit arithmetic so that nothing here can wrap
static bool plain_rule(uint64_t v, uint64_t lo, uint64_t hi) { return lo <= v && v <= hi; }

int main()
{
    long checked = 0;
    for (int table = 0; table < 2; table++)
        for (int a = 0; a < kEdges; a++)
            for (int b = 0; b < kEdges; b++) {
                const uint32_t lo = kEdge[a], hi = kEdge[b];
                const ValueFill f = value_fill(lo, hi, table != 0);
                CHECK(f.keep == (table ? ~0u : 0u), "keep %08x with table %d", f.keep, table);
                CHECK(f.lo == lo && f.span == (uint32_t)(hi - lo), "lo %08x span %08x for (%08x, %08x)", f.lo, f.span, lo, hi);
                CHECK(f.live == (lo <= hi ? ~0u : 0u), "live %08x for (%08x, %08x)", f.live, lo, hi);
                for (int c = 0; c < kEdges; c++) {
                    const uint32_t w = kEdge[c];                    // the word a lane loaded
                    const uint32_t v = table ? w : 0xffffffffu;     // what the row counts as
                    const bool want = plain_rule(v, lo, hi);
                    const bool got = value_pass(w, f), got5 = value_pass(w, f.keep, f.lo, f.span, f.live);
                    CHECK(got == want && got5 == want, "table %d, v %08x (word %08x) in (%08x, %08x): %d, want %d", table, v, w, lo,
                          hi, (int)got, (int)want);
                    checked++;
                }
                // a row index is kept with a table and becomes 0 without one
                CHECK(value_index(12345u, f.keep) == (table ? 12345u : 0u), "value_index with table %d", table);
            }
    // the statements of the header, one by one
    CHECK(value_pass(0xffffffffu, value_fill(0u, 0xffffffffu, true)), "(0, 0xffffffff) passes a row without a value");
    CHECK(!value_pass(0xffffffffu, value_fill(0u, 0xfffffffeu, true)), "(0, 0xfffffffe) refuses a row without a value");
    CHECK(value_pass(0u, value_fill(0u, 0u, true)) && !value_pass(1u, value_fill(0u, 0u, true)), "the point 0");
    CHECK(!value_pass(5000u, value_fill(5000u, 4999u, true)) && !value_pass(4999u, value_fill(5000u, 4999u, true)),
          "an inverted interval passes neither of its ends");
    CHECK(!value_pass(0u, value_fill(1u, 0u, true)) && !value_pass(0xffffffffu, value_fill(0xffffffffu, 0u, true)),
          "inverted intervals at the ends of the range");
    CHECK(value_pass(0x80000000u, value_fill(0x7fffff00u, 0x800000ffu, true)) &&
              value_pass(0x7fffffffu, value_fill(0x7fffff00u, 0x800000ffu, true)) &&
              !value_pass(0x7ffffeffu, value_fill(0x7fffff00u, 0x800000ffu, true)) &&
              !value_pass(0x80000100u, value_fill(0x7fffff00u, 0x800000ffu, true)),
          "the band across the sign bit");
    CHECK(value_pass(123u, value_fill(0u, 0xffffffffu, false)) && !value_pass(123u, value_fill(0u, 0xfffffffeu, false)) &&
              !value_pass(77u, value_fill(77u, 77u, false)),
          "without a table every row is 0xffffffff");
    if (failures == 0)
        printf("value_math ok (%ld cases)\n", checked);
    return failures ? 1 : 0;
}
