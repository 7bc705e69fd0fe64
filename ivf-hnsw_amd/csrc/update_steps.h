// The device steps the in-place updates of the resident lists share (kernels_append.hip, kernels_remove.hip,
// kernels_add_groups.hip, and the scan of kernels_kmeans.hip): the gathered copy of a tile's rows, the
// block-wide exclusive scan, and a few one-liners.  A workgroup of 256 threads fills s_src[j] = the old local row that
// row j of its destination range takes (kSkip: none), then copies codes, ids and norm codes with the steps below.  The
// arithmetic is update_math.h's; every address is dword aligned (code_size is a multiple of 4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "update_math.h"

namespace ivfhnsw_gpu_impl {
namespace {

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4))); // 16 bytes, dword aligned

inline unsigned blocks_of(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        v += __shfl_xor(v, o);
    return v;
}

// Exclusive prefix sum of v over a workgroup of NW wavefronts (s_w: NW words of LDS, free again on return); total = the
// workgroup's sum, in every thread.  ALL 64 LANES OF EVERY WAVEFRONT MUST BE ACTIVE at the call: wave_incl_scan's DPP
// adds read an inactive lane as 0.  Every caller (and every direct caller of wave_incl_scan in the update kernels)
// branches on wavefront-uniform conditions only in front of it and pads with v = 0 instead of leaving.
template <int NW> __device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_w, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v, lane);
    if (lane == 63)
        s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll 4
    for (int w = 0; w < NW; w++) {
        if (w == wave)
            base = sum;
        sum += s_w[w];
    }
    total = sum;
    __syncthreads();
    return base + inc - v;
}

// the memory of update_math.h's copy_group_dwords / copy_group_bytes: dbase = the 16-byte aligned start of group 0
struct TileDwords {
    const uint32_t *__restrict__ src;
    uint32_t *__restrict__ dbase;
    __device__ __forceinline__ uint32_t load(size_t s) const { return src[s]; }
    __device__ __forceinline__ void load4(size_t s, uint32_t v[4]) const
    {
        const u32x4_a4 w = *reinterpret_cast<const u32x4_a4 *>(src + s);
        v[0] = w.x;
        v[1] = w.y;
        v[2] = w.z;
        v[3] = w.w;
    }
    __device__ __forceinline__ void store(size_t d, uint32_t x) const { dbase[d] = x; }
    __device__ __forceinline__ void store4(size_t d, const uint32_t v[4]) const
    {
        *reinterpret_cast<uint4 *>(dbase + d) = make_uint4(v[0], v[1], v[2], v[3]);
    }
};
struct TileBytes {
    const uint8_t *__restrict__ src;
    uint8_t *__restrict__ dbase;
    __device__ __forceinline__ uint32_t load(size_t s) const { return src[s]; }
    __device__ __forceinline__ void store(size_t d, uint8_t x) const { dbase[d] = x; }
    __device__ __forceinline__ void store4(size_t d, uint32_t w) const { *reinterpret_cast<uint32_t *>(dbase + d) = w; }
};

// dst dwords [d0, d0 + rows * q) from source dwords s_src[j] * q + k, one 16-byte group per thread and step.  ALIGNED:
// d0 % 4 == 0 by construction (the merge's tiles of 2048 rows), so no head arithmetic is compiled; the compaction's
// ranges start at any dword.
template <bool ALIGNED>
__device__ __forceinline__ void copy_gathered_dwords(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, const uint32_t *s_src,
                                                     uint32_t rows, uint32_t q, uint64_t d0)
{
    const uint32_t ndw = rows * q, head = group_head<ALIGNED>(d0), ngroups = group_count(head, ndw);
    const TileDwords m{src, dst + (d0 - head)};
    for (uint32_t gi = threadIdx.x; gi < ngroups; gi += 256)
        copy_group_dwords<ALIGNED>(m, s_src, gi, head, ndw, q);
}

// norm codes [d0, d0 + rows) from bytes s_src[j]: dword stores where the range owns the dword, byte stores at its ends
template <bool ALIGNED>
__device__ __forceinline__ void copy_gathered_bytes(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const uint32_t *s_src,
                                                    uint32_t rows, uint64_t d0)
{
    const uint32_t head = group_head<ALIGNED>(d0), ngroups = group_count(head, rows);
    const TileBytes m{src, dst + (d0 - head)};
    for (uint32_t gi = threadIdx.x; gi < ngroups; gi += 256)
        copy_group_bytes<ALIGNED>(m, s_src, gi, head, rows);
}

// codes, ids and norm codes of the rows s_src[0 .. rows) to new local rows [d0, d0 + rows)
template <bool ALIGNED>
__device__ __forceinline__ void copy_gathered_rows(const uint32_t *__restrict__ codes, const uint8_t *__restrict__ ncodes,
                                                   const uint32_t *__restrict__ ids, uint32_t *__restrict__ codes2,
                                                   uint8_t *__restrict__ ncodes2, uint32_t *__restrict__ ids2, const uint32_t *s_src,
                                                   uint32_t rows, uint32_t q, uint64_t d0)
{
    copy_gathered_dwords<ALIGNED>(codes, codes2, s_src, rows, q, d0 * q);
    copy_gathered_dwords<ALIGNED>(ids, ids2, s_src, rows, 1u, d0);
    copy_gathered_bytes<ALIGNED>(ncodes, ncodes2, s_src, rows, d0);
}

} // namespace
} // namespace ivfhnsw_gpu_impl
