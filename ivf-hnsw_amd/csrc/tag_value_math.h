// The conjunction of a row tag and a row value: what a query's tag and pair (t, lo, hi) become before
// the scan loop and how a row's two words are judged against them.  The rule is
//     (t == 0xffff || tag(row) == t) && lo <= value(row) <= hi
// which is the AND of the two shipped rules and nothing else: the tag side restates filter_pass<3> (scan_steps.h) with
// the fill filter_mask(TagMask) (device_common.h) derives, the value side CALLS value_pass (value_math.h).  A row without
// a tag holds 0xffff, a row without a value 0xffffffff, and a handle may lack either row array.  Plain C++ with no HIP in
// it: filter_mask(TagValueMask) and filter_pass<5> call it on the device, tests/cpp/tag_value_math_tool.cpp on the host.
#pragma once

#include <stdint.h>

#include "value_math.h"

namespace ivfhnsw_gpu_impl {

constexpr uint32_t kRowTagNone = 0xffffu; // IVFHNSW_TAG_NONE

// The scalars of one query, all wave-uniform in a scan.
//   tkeep: ~0 with a row-tag array, 0 without one.  It masks the row INDEX a lane loads its tag from (0: every lane reads
//          element 0 of some readable array of uint16 and ignores it).
//   tag:   what a row's zero-extended 16-bit tag is compared with.  With a row array, or for the wildcard, the query's
//          tag itself; without one every row counts as 0xffff, so any other tag gets bit 16 set, which no zero-extended
//          16-bit load equals.
//   value: value_fill's four scalars (keep, lo, span, live).
struct TagValueFill {
    uint32_t tkeep, tag;
    ValueFill value;
};

IVFHNSW_VALUE_FN TagValueFill tag_value_fill(uint32_t t, uint32_t lo, uint32_t hi, bool has_tags, bool has_values)
{
    return {has_tags ? ~0u : 0u, has_tags || t == kRowTagNone ? t : t | 0x10000u, value_fill(lo, hi, has_values)};
}

// the index a lane loads its row's tag from (its value: value_index)
IVFHNSW_VALUE_FN uint32_t tag_index(uint32_t row, uint32_t tkeep) { return row & tkeep; }

// the tag side: equal to the query's scalar, or the query is the wildcard; one compare and one wave-uniform OR, no branch
IVFHNSW_VALUE_FN bool tag_pass(uint32_t wt, uint32_t tag) { return (uint32_t)(wt == tag) | (uint32_t)(tag == kRowTagNone); }

// does a row whose loaded words are wt (its tag, zero-extended) and wv (its value) pass?  No branch.
IVFHNSW_VALUE_FN bool tag_value_pass(uint32_t wt, uint32_t wv, uint32_t tag, uint32_t vkeep, uint32_t lo, uint32_t span,
                                     uint32_t live)
{
    return (uint32_t)tag_pass(wt, tag) & (uint32_t)value_pass(wv, vkeep, lo, span, live);
}
IVFHNSW_VALUE_FN bool tag_value_pass(uint32_t wt, uint32_t wv, const TagValueFill &f)
{
    return tag_value_pass(wt, wv, f.tag, f.value.keep, f.value.lo, f.value.span, f.value.live);
}

} // namespace ivfhnsw_gpu_impl
