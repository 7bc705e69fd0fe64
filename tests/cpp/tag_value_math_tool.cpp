// Host check of csrc/tag_value_math.h (tests/test_tag_value_math_cpu.py builds it with the address and undefined-behaviour
// sanitizers as a stand-alone program): the fill a query's tag and pair become and the pass predicate of "tag AND value"
//  against the plain rule
//     (t == 0xffff || tag == t) && lo <= v && v <= hi
// written with 64-bit integers, over the cross product of value_math_tool.cpp's boundary values for v / lo / hi, the row
// tags and the query tags {0, 255, 256, 0xfffe, 0xffff}, with and without each row array.  Without an array every row
// counts as 0xffff / 0xffffffff whatever word was loaded.  Includes nothing else of the library; exit status 0 = every
// check held.
#include "tag_value_math.h"

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
static const uint32_t kTag[] = {0u, 255u, 256u, 0xfffeu, 0xffffu};
static const int kTags = (int)(sizeof(kTag) / sizeof(kTag[0]));

// the rule, in 64-bit arithmetic so that nothing here can wrap
static bool plain_rule(uint64_t tag, uint64_t v, uint64_t t, uint64_t lo, uint64_t hi)
{
    return (t == 0xffffu || tag == t) && lo <= v && v <= hi;
}

int main()
{
    long checked = 0;
    for (int has_tags = 0; has_tags < 2; has_tags++)
        for (int has_values = 0; has_values < 2; has_values++)
            for (int qt = 0; qt < kTags; qt++)
                for (int a = 0; a < kEdges; a++)
                    for (int b = 0; b < kEdges; b++) {
                        const uint32_t t = kTag[qt], lo = kEdge[a], hi = kEdge[b];
                        const TagValueFill f = tag_value_fill(t, lo, hi, has_tags != 0, has_values != 0);
                        const ValueFill vf = value_fill(lo, hi, has_values != 0);
                        CHECK(f.tkeep == (has_tags ? ~0u : 0u), "tkeep %08x with tags %d", f.tkeep, has_tags);
                        CHECK(f.value.keep == vf.keep && f.value.lo == vf.lo && f.value.span == vf.span && f.value.live == vf.live,
                              "the value side is value_fill's for (%08x, %08x)", lo, hi);
                        CHECK((f.tag & 0xffffu) == t, "tag scalar %08x for %04x", f.tag, t);
                        CHECK(tag_index(12345u, f.tkeep) == (has_tags ? 12345u : 0u), "tag_index with tags %d", has_tags);
                        for (int rt = 0; rt < kTags; rt++)
                            for (int c = 0; c < kEdges; c++) {
                                const uint32_t wt = kTag[rt], wv = kEdge[c];         // the words a lane loaded
                                const uint32_t tag = has_tags ? wt : 0xffffu;        // what the row counts as
                                const uint32_t v = has_values ? wv : 0xffffffffu;
                                const bool want = plain_rule(tag, v, t, lo, hi);
                                const bool got = tag_value_pass(wt, wv, f);
                                const bool got7 = tag_value_pass(wt, wv, f.tag, f.value.keep, f.value.lo, f.value.span, f.value.live);
                                // ... and it is the AND of the two shipped predicates
                                const bool both = tag_pass(wt, f.tag) && value_pass(wv, vf);
                                CHECK(got == want && got7 == want && both == want,
                                      "tags %d values %d, row (%04x, %08x) words (%04x, %08x), query (%04x, (%08x, %08x)): %d, want %d",
                                      has_tags, has_values, tag, v, wt, wv, t, lo, hi, (int)got, (int)want);
                                checked++;
                            }
                    }
    // the statements of the header, one by one
    CHECK(tag_value_pass(7u, 123u, tag_value_fill(0xffffu, 0u, 0xffffffffu, true, true)), "(NONE, FULL) passes every row");
    CHECK(tag_value_pass(0xffffu, 0xffffffffu, tag_value_fill(0xffffu, 0u, 0xffffffffu, true, true)),
          "(NONE, FULL) passes a row with neither");
    CHECK(tag_value_pass(7u, 123u, tag_value_fill(7u, 0u, 0xffffffffu, true, true)) &&
              !tag_value_pass(8u, 123u, tag_value_fill(7u, 0u, 0xffffffffu, true, true)),
          "(t, FULL) is the tag rule");
    CHECK(tag_value_pass(8u, 123u, tag_value_fill(0xffffu, 100u, 200u, true, true)) &&
              !tag_value_pass(8u, 99u, tag_value_fill(0xffffu, 100u, 200u, true, true)),
          "(NONE, (lo, hi)) is the value rule");
    CHECK(!tag_value_pass(256u, 1u, tag_value_fill(256u, 0u, 0u, true, true)) &&
              !tag_value_pass(255u, 0u, tag_value_fill(256u, 0u, 0u, true, true)) &&
              tag_value_pass(256u, 0u, tag_value_fill(256u, 0u, 0u, true, true)),
          "AND, not OR: one side alone does not pass");
    CHECK(!tag_value_pass(7u, 5000u, tag_value_fill(7u, 5000u, 4999u, true, true)) &&
              !tag_value_pass(7u, 5000u, tag_value_fill(0xffffu, 5000u, 4999u, true, true)),
          "an inverted interval passes nothing, whatever the tag");
    CHECK(!tag_value_pass(7u, 123u, tag_value_fill(7u, 0u, 0xffffffffu, false, true)) &&
              tag_value_pass(7u, 123u, tag_value_fill(0xffffu, 100u, 200u, false, true)),
          "without row tags only the wildcard passes, and the value still decides");
    CHECK(!tag_value_pass(7u, 123u, tag_value_fill(7u, 100u, 200u, true, false)) &&
              tag_value_pass(7u, 123u, tag_value_fill(7u, 100u, 0xffffffffu, true, false)),
          "without row values every row is 0xffffffff, and the tag still decides");
    CHECK(tag_value_pass(0u, 0u, tag_value_fill(0xffffu, 0u, 0xffffffffu, false, false)) &&
              !tag_value_pass(0u, 0u, tag_value_fill(0u, 0u, 0xffffffffu, false, false)) &&
              !tag_value_pass(0u, 0u, tag_value_fill(0xffffu, 0u, 0xfffffffeu, false, false)),
          "with neither array only (NONE, (.., 0xffffffff)) passes");
    if (failures == 0)
        printf("tag_value_math ok (%ld cases)\n", checked);
    return failures ? 1 : 0;
}
