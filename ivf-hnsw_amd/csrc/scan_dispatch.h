// How a scan launcher turns two run-time facts -- the code size and whether a label filter is set -- into the template
// arguments of its kernel.  No HIP in here: tests/cpp/dispatch_tool.cpp checks it on the host.
//
//     by_code_size<4, 8, 16, 32>(t.M, [&](auto cs) {          // decltype(cs)::value: 4, 8, 16, 32, or 0 = run-time form
//         return with_mask(fmask, [&](auto... m) {            // m: the mask, or nothing
//             launch kernel<decltype(cs)::value, ..., decltype(m)...> with the arguments (..., m...)
//         });
//     });
#pragma once

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

} // namespace ivfhnsw_gpu_impl
