// How a scan launcher turns two run-time facts -- the code size and how the call is filtered (not at all, by the handle's
// label filter, by a filter slot per query, by a row tag per query, by a value interval per query, by both) -- into the template arguments of its kernel.  No HIP in here: tests/cpp/dispatch_tool.cpp checks it on the host.
//
//     by_code_size<4, 8, 16, 32>(t.M, [&](auto cs) {          // decltype(cs)::value: 4, 8, 16, 32, or 0 = run-time form
//         return with_mask(fmask, [&](auto... m) {            // m: nothing, the mask, a SlotMask, a TagMask, a ValueMask or a TagValueMask
//             launch kernel<decltype(cs)::value, ..., decltype(m)...> with the arguments (..., m...)
//         });
//     });
#pragma once

#include <cstddef>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

namespace ivfhnsw_gpu_impl {

// dynamic LDS the run-time-code-size scan kernels may ask for (1 KB per code byte; the rest of the 160 KB holds
// the plan chunk, the norm table and the top-k buffers)
constexpr size_t kScanDynLdsMax = 128 * 1024;

template <int N> using int_c = std::integral_constant<int, N>;

// f(int_c<M>()) when M is one of Sizes (a kernel compiled for that code size), else f(int_c<0>()): the run-time form
template <class F> auto by_code_size(int, F &&f) { return f(int_c<0>()); }
template <int CS, int... Rest, class F> auto by_code_size(int M, F &&f)
{
    if (M == CS)
        return f(int_c<CS>());
    return by_code_size<Rest...>(M, f);
}

// what the run-time form can take: any multiple of 4 (IndexIVF_HNSW.cpp:805) whose table fits the dynamic LDS
inline bool runtime_code_size_ok(int M) { return M % 4 == 0 && (size_t)M * 1024 <= kScanDynLdsMax; }

// f(fmask) with a label filter's pass mask, f() without: the kernels take the mask as an optional trailing argument
template <class F> auto with_mask(const uint32_t *fmask, F &&f) { return fmask ? f(fmask) : f(); }

// The third form of that argument: every query of the batch names the filter slot it is judged by.
// planes: one pass mask per slot, plane s at planes + s * stride words, bit r = local row r passes slot s; slots: one
// byte per query of the launch.  A byte of 0xff (IVFHNSW_SLOT_NONE) passes every row, any other byte at or beyond
// nplanes passes none (filter_mask, device_common.h); planes points at one readable word at least, also when nplanes
// is 0 (queries without a plane read word 0 and ignore it).
struct SlotMask {
    const uint32_t *planes;
    uint32_t stride, nplanes;
    const uint8_t *slots;
};

// The fourth form: disjoint sets as one 16-bit tag per row.  row_tags: the tag of every local row;
// query_tags: one tag per query of the launch.  A row passes a query iff the two are equal; a query tagged 0xffff
// (IVFHNSW_TAG_NONE) passes every row.  A handle without tags has no row array: row_tags is then null and every row
// reads as 0xffff (filter_mask, device_common.h, points such a launch at one readable element instead).
struct TagMask {
    const uint16_t *row_tags;
    const uint16_t *query_tags;
};

// The fifth form: a uint32 value per row, an interval per query.  row_values: the value of every local
// row; query_ranges: the pair (lo, hi) of query q at [2q], [2q + 1].  A row passes iff lo <= value <= hi, unsigned and
// inclusive (value_math.h); a row without a value holds 0xffffffff.  A handle without a table has no row array:
// row_values is then null and every row reads as 0xffffffff (filter_mask points such a launch at one readable element).
struct ValueMask {
    const uint32_t *row_values;
    const uint32_t *query_ranges;
};

// The sixth form: the fourth AND the fifth.  A row passes query q iff its tag passes query_tags[q] as
// under a TagMask and its value passes the pair at query_ranges[2q] as under a ValueMask (tag_value_math.h).  Either row
// array may be null (the handle lacks that table: every row reads as 0xffff / 0xffffffff); both query arrays are given.
struct TagValueMask {
    const uint16_t *row_tags;
    const uint32_t *row_values;
    const uint16_t *query_tags;
    const uint32_t *query_ranges;
};

// What a scan launcher is told about the filter of its call: nothing, the pass mask of the handle's filter, filter
// slots per query (slots.slots non-null), a tag per query (tags.query_tags non-null), an interval per query
// (values.query_ranges non-null) or both (tag_values.query_tags non-null).  A bare mask pointer converts, so a caller
// with one filter passes it as before.
struct ScanFilter {
    const uint32_t *fmask = nullptr;
    SlotMask slots{nullptr, 0, 0, nullptr};
    TagMask tags{nullptr, nullptr};
    ValueMask values{nullptr, nullptr};
    TagValueMask tag_values{nullptr, nullptr, nullptr, nullptr};
    ScanFilter() = default;
    ScanFilter(const uint32_t *m) : fmask(m) {}
    ScanFilter(std::nullptr_t) {}
    ScanFilter(const SlotMask &s) : slots(s) {}
    ScanFilter(const TagMask &t) : tags(t) {}
    ScanFilter(const ValueMask &v) : values(v) {}
    ScanFilter(const TagValueMask &tv) : tag_values(tv) {}
    bool by_slot() const { return slots.slots != nullptr; }
    bool by_tag() const { return tags.query_tags != nullptr; }
    bool by_value() const { return values.query_ranges != nullptr; }
    bool by_tag_value() const { return tag_values.query_tags != nullptr; }
    bool any() const { return fmask || by_slot() || by_tag() || by_value() || by_tag_value(); }
    // the name a launcher reports: the plain kernel's, "+filter", "+slots" or "+tags" behind it
    const char *name(const char *plain, const char *filtered, const char *slotted, const char *tagged) const
    {
        return by_tag() ? tagged : by_slot() ? slotted : fmask ? filtered : plain;
    }
    // ... and of a launcher that has a value form too: "+values" behind it
    const char *name(const char *plain, const char *filtered, const char *slotted, const char *tagged, const char *valued) const
    {
        return by_value() ? valued : name(plain, filtered, slotted, tagged);
    }
    // ... and a tag-and-value form: "+tags+values" behind it
    const char *name(const char *plain, const char *filtered, const char *slotted, const char *tagged, const char *valued,
                     const char *tag_valued) const
    {
        return by_tag_value() ? tag_valued : name(plain, filtered, slotted, tagged, valued);
    }
    // the queries [q0, ...) of the same call
    ScanFilter from(size_t q0) const
    {
        ScanFilter r = *this;
        if (r.by_slot())
            r.slots.slots += q0;
        if (r.by_tag())
            r.tags.query_tags += q0;
        if (r.by_value())
            r.values.query_ranges += 2 * q0;
        if (r.by_tag_value()) {
            r.tag_values.query_tags += q0;
            r.tag_values.query_ranges += 2 * q0;
        }
        return r;
    }
};

// f(tag_values) with a tag and an interval per query, f(values) with an interval per query, f(tags) with a tag per query,
// f(slots) with filter slots, else as above
template <class F> auto with_mask(const ScanFilter &flt, F &&f)
{
    return flt.by_tag_value() ? f(flt.tag_values)
           : flt.by_value()   ? f(flt.values)
           : flt.by_tag()     ? f(flt.tags)
           : flt.by_slot()    ? f(flt.slots)
                              : with_mask(flt.fmask, f);
}

} // namespace ivfhnsw_gpu_impl
