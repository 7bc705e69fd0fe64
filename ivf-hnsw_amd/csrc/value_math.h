// The interval arithmetic of the row values: what a query's pair (lo, hi) becomes before the scan loop
// and how a row's uint32 is judged against it.  The rule is lo <= v <= hi, unsigned and inclusive at both ends, with no
// special value: a row without a value holds 0xffffffff and lo > hi passes nothing.  This is the one place the fifth
// form of the mask pack can be silently wrong -- the wrap-around of hi - lo, a signed compare, an inverted interval,
// valueless rows against hi = 0xffffffff -- so it is plain C++ with no HIP in it: filter_mask (device_common.h) and
// filter_pass<4> (scan_steps.h) call it on the device, tests/cpp/value_math_tool.cpp on the host.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define IVFHNSW_VALUE_FN __host__ __device__ __forceinline__
#else
#define IVFHNSW_VALUE_FN inline
#endif

namespace ivfhnsw_gpu_impl {

constexpr uint32_t kValueNone = 0xffffffffu; // IVFHNSW_VALUE_NONE

// The scalars of one query, all wave-uniform in a scan.
//   keep: ~0 with a row array, 0 without one.  It masks the row INDEX a lane loads from (0: every lane reads element 0 of
//         some readable array and ignores it), and ~keep is OR-ed into the loaded word where it is consumed, which makes
//         every row of a handle without a table read as 0xffffffff.
//   lo, span = hi - lo: v lies in [lo, hi] iff (v - lo) <= span as unsigned numbers, for lo <= hi.  (v < lo wraps to at
//         least 2^32 - lo > hi - lo; v > hi gives more than span without wrapping.)
//   live: ~0 iff lo <= hi.  For lo > hi the subtraction hi - lo wraps and the compare alone would pass rows; live is
//         AND-ed behind it.
struct ValueFill {
    uint32_t keep, lo, span, live;
};

IVFHNSW_VALUE_FN ValueFill value_fill(uint32_t lo, uint32_t hi, bool has_table)
{
    return {has_table ? ~0u : 0u, lo, hi - lo, lo <= hi ? ~0u : 0u};
}

// the index a lane loads its row's word from
IVFHNSW_VALUE_FN uint32_t value_index(uint32_t row, uint32_t keep) { return row & keep; }

// does a row whose loaded word is w pass?  One unsigned subtract, one unsigned compare, no branch.
IVFHNSW_VALUE_FN bool value_pass(uint32_t w, uint32_t keep, uint32_t lo, uint32_t span, uint32_t live)
{
    const uint32_t v = w | ~keep;
    return (uint32_t)((uint32_t)(v - lo) <= span) & (live & 1u);
}
IVFHNSW_VALUE_FN bool value_pass(uint32_t w, const ValueFill &f) { return value_pass(w, f.keep, f.lo, f.span, f.live); }

} // namespace ivfhnsw_gpu_impl
