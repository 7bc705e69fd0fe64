// Reconstruction of stored rows and the label -> row lookup (ivfhnsw_gpu_reconstruct*, ivfhnsw_gpu_locate*, DESIGN.md
// 3.16).  Everything here reads the resident lists and writes caller buffers: nothing of the index changes, and none of
// the scan, walk, plan or top-k kernels is involved.
//
// Float contract: a ROTATED-space component is ONE add, anchor[j] + code word[j]; Grouping's anchor is the three steps of
// group_table_kernel (kernels_encode.hip MODE 0 / 1): cv = V[nn] + (-1 * V[c]), anchor = V[c] + alpha * cv.  Explicit
// round-to-nearest intrinsics, built with -ffp-contract=off like the rest.
#include "ivfhnsw_kernels.h"
#include "device_common.h"

namespace ivfhnsw_gpu_impl {

namespace {

constexpr int kReconTileRows = 64; // rows of the request per 256-thread workgroup

// What phase 1 leaves in LDS for every row of the tile.
struct ReconRow {
    uint32_t row; // resident row, kNotOwned = an empty slot
    uint32_t c;   // its list
    uint32_t nn;  // Grouping: the neighbour centroid of its sub-group
    float alpha;  // Grouping: alpha[c]
};

// last c in [0, nc) with goff[c] <= r (r < goff[nc]): the list row r lies in, empty lists skipped
__device__ __forceinline__ uint32_t list_of_row(const uint64_t *__restrict__ goff, uint32_t nc, uint64_t r)
{
    uint32_t a = 0, b = nc - 1;
    while (a < b) {
        const uint32_t mid = (uint32_t)(((uint64_t)a + b + 1) >> 1);
        if (goff[mid] <= r)
            a = mid;
        else
            b = mid - 1;
    }
    return a;
}

// One workgroup = kReconTileRows entries of the request.  Phase 1, one thread per entry: the row's list (the bounds of
// the list the wave's first entry lies in are tried before a search of goff, so a run of contiguous rows pays one search
// per wave and list, not one per row) and, for Grouping, its sub-group from the prefix of the list's sub_sizes row.
// Phase 2, all threads over the tile's [rows][d] floats, VEC floats per thread and step: coalesced stores of anchor + code
// word.  VEC = 4 needs dsub % 4 == 0 (a float4 never straddles two code words) and a 16-byte aligned out.
template <int VEC, bool GROUP>
__global__ __launch_bounds__(256) void recon_rows_kernel(IvfTables t, GroupTables g, const float *__restrict__ V,
                                                         uint64_t n_local, const long long *__restrict__ rows, size_t n,
                                                         float *__restrict__ out)
{
    __shared__ ReconRow s_row[kReconTileRows];
    const size_t i0 = (size_t)blockIdx.x * kReconTileRows;
    const int ntile = (int)min((size_t)kReconTileRows, n - i0);
    if (threadIdx.x < kReconTileRows) { // exactly the first wavefront
        const int i = threadIdx.x;
        const long long rr = i < ntile ? rows[i0 + i] : -1;
        const bool ok = rr >= 0 && (unsigned long long)rr < n_local;
        ReconRow e{kNotOwned, 0u, 0u, 0.f};
        // the list of the wave's first valid entry, shared by every lane whose row it holds
        const unsigned long long valid = __ballot(ok);
        uint64_t lo = 1, hi = 0; // an empty range
        uint32_t c0 = 0;
        if (valid) {
            const int first = __ffsll((long long)valid) - 1;
            const uint64_t r0 = (uint64_t)__shfl(rr, first);
            c0 = list_of_row(t.goff, t.nc, r0);
            lo = t.goff[c0];
            hi = t.goff[c0 + 1];
        }
        if (ok) {
            const uint64_t r = (uint64_t)rr;
            const uint32_t c = (r >= lo && r < hi) ? c0 : list_of_row(t.goff, t.nc, r);
            e.row = (uint32_t)r;
            e.c = c;
            if (GROUP) {
                const uint32_t *sz = g.sub_sizes + (size_t)c * g.nsubc;
                uint64_t pos = r - t.goff[c];
                int s = 0;
                while (s < g.nsubc - 1 && pos >= sz[s]) {
                    pos -= sz[s];
                    s++;
                }
                e.nn = g.nn_idx[(size_t)c * g.nsubc + s];
                e.alpha = g.alphas[c];
                if (e.nn >= t.nc) // no such centroid: nothing to reconstruct from
                    e.row = kNotOwned;
            }
        }
        s_row[i] = e;
    }
    __syncthreads();
    const int d = t.d, dsub = t.dsub, M = t.M;
    const int per_row = d / VEC;
    const float empty = __uint_as_float(kReconEmptyBits);
    for (int e = threadIdx.x; e < ntile * per_row; e += 256) {
        const int i = e / per_row, j = (e - i * per_row) * VEC;
        const ReconRow rw = s_row[i];
        float *dst = out + (i0 + i) * (size_t)d + j;
        float v[VEC];
        if (rw.row == kNotOwned) {
#pragma unroll
            for (int u = 0; u < VEC; u++)
                v[u] = empty;
        } else {
            const int m = j / dsub;
            const uint32_t code = t.codes[(size_t)rw.row * M + m];
            const float *cw = t.pq_centroids + ((size_t)m * 256 + code) * dsub + (j - m * dsub);
            const float *vc = V + (size_t)rw.c * d + j;
            const float *vn = V + (size_t)rw.nn * d + j;
            float a[VEC], w[VEC], b[VEC];
            if (VEC == 4) {
                const float4 a4 = *reinterpret_cast<const float4 *>(vc), w4 = *reinterpret_cast<const float4 *>(cw);
                a[0] = a4.x, a[1] = a4.y, a[2] = a4.z, a[3] = a4.w;
                w[0] = w4.x, w[1] = w4.y, w[2] = w4.z, w[3] = w4.w;
                if (GROUP) {
                    const float4 b4 = *reinterpret_cast<const float4 *>(vn);
                    b[0] = b4.x, b[1] = b4.y, b[2] = b4.z, b[3] = b4.w;
                }
            } else {
                a[0] = vc[0];
                w[0] = cw[0];
                if (GROUP)
                    b[0] = vn[0];
            }
#pragma unroll
            for (int u = 0; u < VEC; u++) {
                float anchor = a[u];
                if (GROUP) {
                    const float cv = __fadd_rn(b[u], __fmul_rn(-1.f, a[u]));
                    anchor = __fadd_rn(a[u], __fmul_rn(rw.alpha, cv));
                }
                v[u] = __fadd_rn(anchor, w[u]);
            }
        }
        if (VEC == 4)
            *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        else
            dst[0] = v[0];
    }
}

__global__ __launch_bounds__(256) void recon_refill_kernel(uint64_t n_local, const long long *__restrict__ rows, size_t n, int d,
                                                           float *__restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * (size_t)d)
        return;
    const long long rr = rows[e / (size_t)d];
    if (rr < 0 || (unsigned long long)rr >= n_local)
        out[e] = __uint_as_float(kReconEmptyBits);
}

// key -> Seg -> start + (vpos - seg.vpos): resolve_key's lookup (kernels_search.hip) with the row instead of its id
__global__ __launch_bounds__(256) void resolve_rows_kernel(const Seg *__restrict__ segs, const PlanHdr *__restrict__ hdr,
                                                           int max_seg, const long long *__restrict__ skeys, int nq, int k,
                                                           long long *__restrict__ rows)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nq * k)
        return;
    const int q = (int)(i / k);
    const unsigned long long key = (unsigned long long)skeys[i] ^ kSignFlip;
    long long row = -1;
    const uint32_t nseg = min(hdr[q].nseg, (uint32_t)max_seg);
    if (key < kKeyInit && nseg) {
        const Seg *sq = segs + (size_t)q * max_seg;
        const uint32_t vpos = (uint32_t)key;
        uint32_t a = 0, b = nseg - 1; // last segment with seg.vpos <= vpos
        while (a < b) {
            const uint32_t mid = (a + b + 1) >> 1;
            if (sq[mid].vpos <= vpos)
                a = mid;
            else
                b = mid - 1;
        }
        const Seg sg = sq[a];
        if (vpos >= sg.vpos && vpos - sg.vpos < sg.len)
            row = (long long)sg.start + (vpos - sg.vpos);
    }
    rows[i] = row;
}

// ---- locate ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void locate_gather_kernel(const uint32_t *__restrict__ labels, const uint32_t *__restrict__ perm,
                                                            size_t n, uint32_t *__restrict__ sorted)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) {
        const uint32_t i = perm[j];
        sorted[j] = i < n ? labels[i] : 0u; // (perm is a permutation of 0 .. n - 1; the test keeps it so)
    }
}

// first j in [0, n) with sorted[j] >= v, n if none
__device__ __forceinline__ size_t lower_bound_u32(const uint32_t *__restrict__ sorted, size_t n, uint32_t v)
{
    size_t a = 0, b = n;
    while (a < b) {
        const size_t mid = (a + b) >> 1;
        if (sorted[mid] < v)
            a = mid + 1;
        else
            b = mid;
    }
    return a;
}

constexpr int kLocateRowsPerThread = 8;

// The mark pass of remove_ids / set_filter over ids with the bitmap test (filter_mark_kernel); a hit, which is rare, is
// looked up in the sorted request.  Coalesced: thread t of a workgroup reads rows base + t, base + 256 + t, ...
__global__ __launch_bounds__(256) void locate_hit_kernel(const uint32_t *__restrict__ ids, uint64_t n_local,
                                                         const uint32_t *__restrict__ bits, uint32_t max_label,
                                                         const uint32_t *__restrict__ sorted, size_t n, uint32_t *__restrict__ lo,
                                                         uint32_t *__restrict__ cnt)
{
    const uint64_t base = (uint64_t)blockIdx.x * (256 * kLocateRowsPerThread) + threadIdx.x;
    uint32_t id[kLocateRowsPerThread];
#pragma unroll
    for (int u = 0; u < kLocateRowsPerThread; u++) {
        const uint64_t r = base + (uint64_t)u * 256;
        id[u] = r < n_local ? ids[r] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kLocateRowsPerThread; u++) {
        const uint64_t r = base + (uint64_t)u * 256;
        if (r >= n_local || id[u] > max_label || !((bits[id[u] >> 5] >> (id[u] & 31)) & 1u))
            continue;
        const size_t p = lower_bound_u32(sorted, n, id[u]);
        if (p < n && sorted[p] == id[u]) {
            atomicMin(&lo[p], (uint32_t)r);
            atomicAdd(&cnt[p], 1u);
        }
    }
}

__global__ __launch_bounds__(256) void locate_scatter_kernel(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ perm,
                                                             size_t n, const uint32_t *__restrict__ lo,
                                                             const uint32_t *__restrict__ cnt, long long *__restrict__ rows,
                                                             uint32_t *__restrict__ counts, unsigned long long *__restrict__ missing)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool miss = false;
    if (j < n) {
        const uint32_t i = perm[j];
        const size_t p = lower_bound_u32(sorted, n, sorted[j]); // the first place of this label: p <= j
        const uint32_t c = p < n ? cnt[p] : 0u;
        miss = c == 0;
        if (i < n) {
            rows[i] = miss ? -1ll : (long long)lo[p];
            if (counts)
                counts[i] = c;
        }
    }
    if (missing) {
        const unsigned long long b = __ballot(miss);
        if ((threadIdx.x & 63) == 0 && b)
            atomicAdd(missing, (unsigned long long)__popcll(b));
    }
}

} // namespace

hipError_t launch_recon_rows(hipStream_t s, const IvfTables &t, const GroupTables *g, const float *V, uint64_t n_local,
                             const int64_t *rows, size_t n, float *out)
{
    if (n == 0)
        return hipSuccess;
    const size_t blocks = (n + kReconTileRows - 1) / kReconTileRows;
    if (blocks > 0x7fffffffull || t.nc == 0 || t.d <= 0 || t.dsub <= 0 || t.d != t.M * t.dsub || (g && g->nsubc <= 0))
        return hipErrorInvalidValue;
    const bool vec = t.dsub % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)V & 15) == 0 &&
                     ((uintptr_t)t.pq_centroids & 15) == 0;
    const dim3 grid((unsigned)blocks), block(256);
    const GroupTables g0 = g ? *g : GroupTables{};
    auto *r = reinterpret_cast<const long long *>(rows);
    if (g) {
        if (vec)
            hipLaunchKernelGGL((recon_rows_kernel<4, true>), grid, block, 0, s, t, g0, V, n_local, r, n, out);
        else
            hipLaunchKernelGGL((recon_rows_kernel<1, true>), grid, block, 0, s, t, g0, V, n_local, r, n, out);
    } else {
        if (vec)
            hipLaunchKernelGGL((recon_rows_kernel<4, false>), grid, block, 0, s, t, g0, V, n_local, r, n, out);
        else
            hipLaunchKernelGGL((recon_rows_kernel<1, false>), grid, block, 0, s, t, g0, V, n_local, r, n, out);
    }
    return hipGetLastError();
}

hipError_t launch_recon_refill(hipStream_t s, uint64_t n_local, const int64_t *rows, size_t n, int d, float *out)
{
    const size_t total = n * (size_t)d;
    if (total == 0)
        return hipSuccess;
    const size_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(recon_refill_kernel, dim3((unsigned)blocks), dim3(256), 0, s, n_local,
                       reinterpret_cast<const long long *>(rows), n, d, out);
    return hipGetLastError();
}

hipError_t launch_resolve_rows(hipStream_t s, const PlanView &p, const int64_t *skeys, int k, int64_t *rows)
{
    const size_t n = (size_t)p.nq * k;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(resolve_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p.segs, p.hdr, p.max_seg,
                       reinterpret_cast<const long long *>(skeys), p.nq, k, reinterpret_cast<long long *>(rows));
    return hipGetLastError();
}

hipError_t launch_locate_gather(hipStream_t s, const uint32_t *labels, const uint32_t *perm, size_t n, uint32_t *sorted)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(locate_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, labels, perm, n, sorted);
    return hipGetLastError();
}

hipError_t launch_locate_hit(hipStream_t s, const uint32_t *ids, uint64_t n_local, const uint32_t *bits, uint32_t max_label,
                             const uint32_t *sorted, size_t n, uint32_t *lo, uint32_t *cnt)
{
    if (n_local == 0 || n == 0)
        return hipSuccess;
    const uint64_t per = 256 * kLocateRowsPerThread;
    hipLaunchKernelGGL(locate_hit_kernel, dim3((unsigned)((n_local + per - 1) / per)), dim3(256), 0, s, ids, n_local, bits,
                       max_label, sorted, n, lo, cnt);
    return hipGetLastError();
}

hipError_t launch_locate_scatter(hipStream_t s, const uint32_t *sorted, const uint32_t *perm, size_t n, const uint32_t *lo,
                                 const uint32_t *cnt, int64_t *rows, uint32_t *counts, unsigned long long *missing)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(locate_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sorted, perm, n, lo, cnt,
                       reinterpret_cast<long long *>(rows), counts, missing);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
