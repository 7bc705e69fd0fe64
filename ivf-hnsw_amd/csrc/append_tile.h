// The destination-tiled row copy the append (kernels_append.hip) and the grouping append (kernels_add_groups.hip) share:
// a workgroup fills s_src[j] = the old local row that tile row j takes (kSkip: none), then copies codes, ids and norm
// codes of the tile.  Every address is dword aligned; the destination groups are 16-byte aligned (a tile is 2048 rows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ivfhnsw_gpu_impl {
namespace {

constexpr uint32_t kSkip = 0xffffffffu; // a tile row with no old source row (a new code, or past the end)

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4))); // 16 bytes, dword aligned

// the largest c in [lo, hi] with lstart[c] <= r (lstart[lo] <= r holds)
__device__ __forceinline__ uint32_t list_of_row(const uint32_t *__restrict__ lstart, uint32_t lo, uint32_t hi, uint32_t r)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (lstart[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// dst dwords [0, ndw) of the tile from src dword s_src[row] * q + k; 16-byte groups, a group whose four source dwords
// are consecutive is one dword-aligned 16-byte load
__device__ __forceinline__ void copy_tile_dwords(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, const uint32_t *s_src,
                                                 uint32_t ndw, uint32_t q)
{
    for (uint32_t e = threadIdx.x * 4; e < ndw; e += 1024) {
        uint32_t j = e / q, k = e - j * q;
        size_t s[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t sr = e + u < ndw ? s_src[j] : kSkip;
            ok[u] = sr != kSkip;
            s[u] = (size_t)(ok[u] ? sr : 0u) * q + k;
            if (++k == q) {
                k = 0;
                j++;
            }
        }
        uint32_t v[4];
        if (ok[0] && ok[1] && ok[2] && ok[3] && s[1] == s[0] + 1 && s[2] == s[0] + 2 && s[3] == s[0] + 3) {
            const u32x4_a4 w = *reinterpret_cast<const u32x4_a4 *>(src + s[0]);
            v[0] = w.x;
            v[1] = w.y;
            v[2] = w.z;
            v[3] = w.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++)
                v[u] = ok[u] ? src[s[u]] : 0u;
        }
        if (e + 4 <= ndw) {
            *reinterpret_cast<uint4 *>(dst + e) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (e + u < ndw)
                    dst[e + u] = v[u];
        }
    }
}

// norm codes of the tile: one byte per row, four rows per dword store
__device__ __forceinline__ void copy_tile_norm_codes(const uint8_t *__restrict__ ncodes, uint8_t *__restrict__ ncodes2,
                                                     const uint32_t *s_src, uint32_t r0, uint32_t rows)
{
    for (uint32_t e = threadIdx.x * 4; e < rows; e += 1024) {
        uint32_t w = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t sr = e + u < rows ? s_src[e + u] : kSkip;
            w |= (uint32_t)(sr != kSkip ? ncodes[sr] : 0u) << (8 * u);
        }
        if (e + 4 <= rows) {
            *reinterpret_cast<uint32_t *>(ncodes2 + r0 + e) = w;
        } else {
            for (uint32_t u = 0; e + u < rows; u++)
                ncodes2[r0 + e + u] = (uint8_t)(w >> (8 * u));
        }
    }
}

} // namespace
} // namespace ivfhnsw_gpu_impl
