// Exact brute-force search of the uint8 base store on the int8 matrix cores (ivfhnsw_gpu_exact_search).
//
// What it stands for in the reference: the ground-truth file every driver scores Recall@1 against
// (tests/test_ivfhnsw_sift1b.cpp:28-32,173-215, -path_gt) is the exact nearest rows of the uint8 base by squared L2.
//
// Arithmetic: both operands are XORed with 0x80 per byte, u8 v -> i8 v - 128; q - x does not change, so
//     dist(q, x) = |q'|^2 + |x'|^2 - 2 q'.x'      in int32 (|.| <= 128^2 * 256 * 4 < 2^25 for d <= 256)
// is the integer sum of (q[j] - x[j])^2.  An integer sum has no order: the store's per-quad row permutation
// (rerank_permute) is left as it is, the queries are permuted by the same map once per call, and whatever k order
// v_mfma_i32_32x32x32_i8 gives the 16 bytes of a lane, it gives the same one to both operands.  Only the C/D map is
// relied on (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), the one knn_mfma_kernel uses.
//
// Shape: wave w of a workgroup owns the 32 query rows [32w, 32w + 32) of the workgroup's strip for the whole sweep
// (operand A: ceil(d/32) steps of 16 bytes per lane, in registers) and walks the columns of its split 32 at a time.
// Lane l loads bytes [32 s + 16 (l >> 5), + 16) of row c0 + (l & 31) for step s straight from the store -- the row
// norm comes from the same registers (v_dot4_i32_i8), so nothing is staged in LDS and the waves never meet at a
// barrier; the next tile's loads are in flight behind the current tile's MFMAs.  d % 32 == 16: the upper half of the
// last step is zero in both operands and is never read (it would lie in the next row, or past the store's end).
//
// Selection is kernels_knn.hip's: every lane holds the running k-th distance of its 16 rows; a candidate below it goes
// to the row's LDS buffer, placed by a ballot; a row whose buffer could overflow in the next tile is compacted by its
// wave by rank (keys are unique: label in the low word).  Columns arrive in increasing label order, so among equal
// distances the lower label wins by the strict '<' alone.  The common tile (no candidate in any of the wave's 32 x 32
// distances) costs two vector instructions per accumulator register: 2 acc - |x'|^2 > |q'|^2 - threshold.
// LDS bounds the strip: 4 waves (128 rows) up to k = 32, 2 waves (64 rows) of 136 keys per row up to k = 100.
//
// The exact range search (ivfhnsw_gpu_exact_range_search) is the same sweep with a fixed gate and no
// selection: exact_range_kernel, below the k-search.
#include "ivfhnsw_kernels.h"
#include "device_common.h"

#include <float.h>
#include <limits.h>

namespace ivfhnsw_gpu_impl {

namespace {

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned long long kExactKeyNone = ~0ull;

__device__ __forceinline__ int exact_sq4(const i32x4 &w, int acc)
{
    acc = __builtin_amdgcn_sdot4(w.x, w.x, acc, false);
    acc = __builtin_amdgcn_sdot4(w.y, w.y, acc, false);
    acc = __builtin_amdgcn_sdot4(w.z, w.z, acc, false);
    return __builtin_amdgcn_sdot4(w.w, w.w, acc, false);
}

// rank of up to NK keys per lane among the n keys of a row buffer, the k smallest written to dst in order
template <int NK>
__device__ __forceinline__ void exact_rank_row(const unsigned long long *rb, int n, int k, int lane,
                                               unsigned long long *dst, bool in_place)
{
    unsigned long long key[NK];
    int rk[NK];
#pragma unroll
    for (int u = 0; u < NK; u++) {
        key[u] = lane + 64 * u < n ? rb[lane + 64 * u] : kExactKeyNone;
        rk[u] = 0;
    }
    for (int i = 0; i < n; i++) {
        const unsigned long long v = rb[i];
#pragma unroll
        for (int u = 0; u < NK; u++)
            rk[u] += v < key[u] ? 1 : 0;
    }
    if (in_place)
        __builtin_amdgcn_wave_barrier(); // every lane has read the buffer before any lane rewrites it
#pragma unroll
    for (int u = 0; u < NK; u++)
        if (lane + 64 * u < n && rk[u] < k)
            dst[rk[u]] = key[u];
}

// NS = ceil(d / 32), the steps of 32 bytes a row is read in, CAP = keys of a row's candidate buffer (a row is
// compacted when it holds more than CAP - 32), WAVES = 32-row strips per workgroup.
// Qp: the queries in the store's byte order, [nq][d]; X: the store, [nx][d]; both 16-byte aligned, d % 16 == 0.
template <int NS, int CAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void exact_mfma_kernel(const uint8_t *__restrict__ Qp, const uint8_t *__restrict__ X,
                                                                int nq, size_t nx, int d, int k, size_t cols_per_split,
                                                                unsigned long long *__restrict__ out_keys)
{
    constexpr int NK = (CAP + 63) / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *s_buf = reinterpret_cast<unsigned long long *>(smem); // [WAVES][32][CAP]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_buf + WAVES * 32 * CAP);  // [WAVES][32]
    int *s_thr = reinterpret_cast<int *>(s_cnt + WAVES * 32);                  // [WAVES][32]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    const int r0 = blockIdx.x * (32 * WAVES) + wave * 32;
    const size_t c_begin = (size_t)blockIdx.y * cols_per_split < nx ? (size_t)blockIdx.y * cols_per_split : nx;
    const size_t c_end = c_begin + cols_per_split < nx ? c_begin + cols_per_split : nx;
    unsigned long long *buf = s_buf + (size_t)wave * 32 * CAP;
    uint32_t *cnt = s_cnt + wave * 32;
    int *thr_s = s_thr + wave * 32;

    // the 16 bytes of step s this lane owns.  Only the upper half of the last step can lie at or beyond byte d of the row
    // (d % 32 == 16): there the lane reads the row's first piece again, without a branch, and to_i8 replaces it by zeros.
    // The XOR to i8 waits until the bytes are used, so that a tile's loads stay in flight behind the tile before it.
    const bool tail_in = 32 * (NS - 1) + 16 * kk < d;
    auto load_row = [&](const uint8_t *row, i32x4 (&w)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; s++)
            w[s] = *reinterpret_cast<const i32x4 *>(row + (s < NS - 1 || tail_in ? 32 * s + 16 * kk : 0));
    };
    auto to_i8 = [&](const i32x4 (&raw)[NS], i32x4 (&w)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const i32x4 zero = {0, 0, 0, 0};
            w[s] = s < NS - 1 || tail_in ? raw[s] ^ (int)0x80808080 : zero;
        }
    };

    // operand A and the norms of the wave's 32 query rows
    i32x4 a[NS], cur[NS], nxt[NS];
    load_row(Qp + (size_t)min(r0 + m, nq - 1) * d, nxt);
    to_i8(nxt, a);
    int qn = 0;
#pragma unroll
    for (int s = 0; s < NS; s++)
        qn = exact_sq4(a[s], qn);
    qn += __shfl_xor(qn, 32);
    // the 16 rows whose dot products this lane holds (C/D layout of the 32x32 MFMA)
    // and what the common tile compares against: dist < thr  <=>  2 dot - |x'|^2 > |q'|^2 - thr = gate
    int qn_r[16], gate[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        qn_r[r] = __shfl(qn, (r & 3) + 8 * (r >> 2) + 4 * kk);
        gate[r] = qn_r[r] - INT_MAX;
    }
    if (lane < 32) {
        cnt[lane] = 0;
        thr_s[lane] = INT_MAX;
    }
    __builtin_amdgcn_wave_barrier();

    // a column at or beyond c_end is not read (the lane reads the split's first row and drops it)
    auto fetch = [&](size_t c0) { load_row(X + (c0 + m < c_end ? c0 + m : c_begin) * (size_t)d, nxt); };
    if (c_begin < c_end)
        fetch(c_begin);
    for (size_t c0 = c_begin; c0 < c_end; c0 += 32) {
        const size_t col = c0 + m;
        const bool col_ok = col < c_end;
        to_i8(nxt, cur); // a lane without a column scores a row it drops below
        if (c0 + 32 < c_end)
            fetch(c0 + 32); // in flight behind this tile's MFMAs
        i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int xn = 0;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], cur[s], acc, 0, 0, 0);
            xn = exact_sq4(cur[s], xn);
        }
        xn += __shfl_xor(xn, 32);
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; r++)
            any |= (acc[r] << 1) - xn > gate[r]; // all terms far inside int32
        if (!__ballot(any && col_ok))
            continue; // wave-uniform: the common tile once the thresholds have settled
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int dist = qn_r[r] + xn - 2 * acc[r];
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
            const bool pass = col_ok && dist < qn_r[r] - gate[r];
            const unsigned long long mask = __ballot(pass);
            if (mask) {
                const uint32_t half = kk ? (uint32_t)(mask >> 32) : (uint32_t)mask;
                const uint32_t base = cnt[row];
                if (pass)
                    buf[(size_t)row * CAP + base + __popc(half & ((1u << m) - 1u))] =
                        ((unsigned long long)(uint32_t)dist << 32) | (uint32_t)col;
                if (m == 0 && half)
                    cnt[row] = base + __popc(half);
            }
        }
        // rows that could overflow in the next tile (32 more entries at most): keep their k smallest
        __builtin_amdgcn_wave_barrier();
        unsigned long long need = __ballot(lane < 32 && cnt[lane] > (uint32_t)(CAP - 32));
        while (need) {
            const int row = __ffsll((long long)need) - 1;
            need &= need - 1;
            const int n = (int)cnt[row];
            unsigned long long *rb = buf + (size_t)row * CAP;
            exact_rank_row<NK>(rb, n, k, lane, rb, true);
            if (lane == 0)
                cnt[row] = (uint32_t)min(n, k);
            __builtin_amdgcn_wave_barrier();
            if (lane == 0 && n >= k)
                thr_s[row] = (int)(uint32_t)(rb[k - 1] >> 32);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; r++)
            gate[r] = qn_r[r] - thr_s[(r & 3) + 8 * (r >> 2) + 4 * kk];
    }

    // final order of every row, then out: [split][nq][k] keys ascending, kExactKeyNone beyond what was found
    __builtin_amdgcn_wave_barrier();
    for (int row = 0; row < 32; row++) {
        if (r0 + row >= nq)
            break;
        const int n = (int)cnt[row];
        unsigned long long *o = out_keys + ((size_t)blockIdx.y * nq + (r0 + row)) * (size_t)k;
        exact_rank_row<NK>(buf + (size_t)row * CAP, n, k, lane, o, false);
        for (int i = n + lane; i < k; i += 64)
            o[i] = kExactKeyNone;
    }
}

// one wavefront per query: the k smallest of the splits' sorted partial tables (keys distinct: labels differ)
__global__ __launch_bounds__(64) void exact_merge_kernel(const unsigned long long *__restrict__ part, int nsplit, int nq, int k,
                                                         float *__restrict__ dists, long long *__restrict__ labels)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    const int total = nsplit * k;
    int found = 0;
    for (int i = lane; i < total; i += 64) {
        const int s = i / k, j = i - s * k;
        const unsigned long long key = part[((size_t)s * nq + q) * k + j];
        if (key == kExactKeyNone)
            continue;
        found++;
        int rank = 0;
        for (int t = 0; t < nsplit; t++) {
            // keys of split t below `key`: the lists are sorted, binary search
            const unsigned long long *p = part + ((size_t)t * nq + q) * k;
            int lo = 0, hi = k;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (p[mid] < key)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            labels[(size_t)q * k + rank] = (long long)(uint32_t)key;
            dists[(size_t)q * k + rank] = (float)(uint32_t)(key >> 32); // an integer below 2^24: exact
        }
    }
    // slots nothing reached: the store has fewer than k rows
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        found += __shfl_xor(found, o);
    for (int i = min(found, k) + lane; i < k; i += 64) {
        labels[(size_t)q * k + i] = -1ll;
        dists[(size_t)q * k + i] = FLT_MAX;
    }
}

template <int NS, int CAP, int WAVES>
hipError_t launch_exact_t(hipStream_t s, const uint8_t *Qp, const uint8_t *X, int nq, size_t nx, int d, int k, int nsplit,
                          size_t cols_per_split, unsigned long long *part)
{
    const size_t shm = (size_t)WAVES * 32 * CAP * sizeof(unsigned long long) + (size_t)WAVES * 32 * (sizeof(uint32_t) + sizeof(int));
    constexpr auto kern = exact_mfma_kernel<NS, CAP, WAVES>;
    if (hipError_t e = dyn_lds<kern>(shm); e != hipSuccess)
        return e;
    // query tile is the fast index, column split the slow one: the tiles that run together stream the same columns
    hipLaunchKernelGGL(kern, dim3((unsigned)((nq + 32 * WAVES - 1) / (32 * WAVES)), (unsigned)nsplit), dim3(64 * WAVES), shm,
                       s, Qp, X, nq, nx, d, k, cols_per_split, part);
    return hipGetLastError();
}

// Exact range search (ivfhnsw_gpu_exact_range_search): the sweep above with a fixed gate, dist < thr, in
// two forms.  Nothing is selected, so there is no LDS at all: a lane keeps the counters of its 16 accumulator rows in
// registers (the 32 lanes of a half hold the same values, a half's ballot is uniform across it), and the strip is always
// 4 waves.  Rows beyond nq get a gate nothing passes.
//   count (FILL = false): cnt[r] += popcount of the row's half of the ballot; at the end of the split
//       slices[(q_off + row) * nsplit + split] = cnt -- query major, split minor, so that the exclusive prefix over the
//       array puts a query's results in ascending label -- and *total += the wave's sum (64 bit).
//   fill (FILL = true): cnt[r] starts at the prefix of the row's slice and is the row's cursor; a passing lane writes
//       (dist, col) at cnt[r] + popcount of the lower passing lanes of its half.  Columns of a tile are lane & 31: ballot
//       order is label order.
// The tile map (map != null): the count form records per wave ONE BIT per 2^map_shift tiles of its split -- did any lane
// pass in them -- 32 bits to a word, stored by one lane when the word is complete; map[((q_off + r0) / 32 * nsplit + split)
// * map_words + word].  The fill form visits only tiles whose bit is set, still in order, so the cursors stay right; a
// tile it skips is neither loaded nor multiplied.  Every word the fill form reads the count form wrote (the same tiles).
template <int NS, bool FILL>
__global__ __launch_bounds__(256) void exact_range_kernel(const uint8_t *__restrict__ Qp, const uint8_t *__restrict__ X, int nq,
                                                          size_t nx, int d, int thr, size_t cols_per_split, size_t q_off,
                                                          uint32_t *__restrict__ slices, unsigned long long *__restrict__ total,
                                                          uint32_t *__restrict__ map, int map_shift, int map_words,
                                                          float *__restrict__ out_d, long long *__restrict__ out_l,
                                                          size_t out_cap)
{
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    const int r0 = blockIdx.x * 128 + wave * 32;
    if (r0 >= nq)
        return; // no barrier anywhere below
    const int nsplit = gridDim.y, split = blockIdx.y;
    const size_t c_begin = (size_t)split * cols_per_split < nx ? (size_t)split * cols_per_split : nx;
    const size_t c_end = c_begin + cols_per_split < nx ? c_begin + cols_per_split : nx;
    const uint32_t ntiles = (uint32_t)((c_end - c_begin + 31) >> 5);

    const bool tail_in = 32 * (NS - 1) + 16 * kk < d;
    auto load_row = [&](const uint8_t *row, i32x4 (&w)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; s++)
            w[s] = *reinterpret_cast<const i32x4 *>(row + (s < NS - 1 || tail_in ? 32 * s + 16 * kk : 0));
    };
    auto to_i8 = [&](const i32x4 (&raw)[NS], i32x4 (&w)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const i32x4 zero = {0, 0, 0, 0};
            w[s] = s < NS - 1 || tail_in ? raw[s] ^ (int)0x80808080 : zero;
        }
    };

    i32x4 a[NS], cur[NS], nxt[NS];
    load_row(Qp + (size_t)min(r0 + m, nq - 1) * d, nxt);
    to_i8(nxt, a);
    int qn = 0;
#pragma unroll
    for (int s = 0; s < NS; s++)
        qn = exact_sq4(a[s], qn);
    qn += __shfl_xor(qn, 32);
    // dist < thr  <=>  2 dot - |x'|^2 > |q'|^2 - thr = gate, set once (|q'|^2 <= 2^22: no overflow for any thr >= 0)
    int qn_r[16], gate[16];
    uint32_t cnt[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
        qn_r[r] = __shfl(qn, row);
        gate[r] = r0 + row < nq ? qn_r[r] - thr : INT_MAX;
        cnt[r] = FILL && r0 + row < nq ? slices[(q_off + r0 + row) * nsplit + split] : 0u;
    }

    uint32_t *mw = map ? map + ((((q_off + r0) >> 5) * nsplit + split) * (size_t)map_words) : nullptr;
    // the first tile at or after t that is to be visited (ntiles: none)
    auto next_tile = [&](uint32_t t) -> uint32_t {
        if (!FILL || !mw)
            return t < ntiles ? t : ntiles;
        while (t < ntiles) {
            const uint32_t g = t >> map_shift;
            const uint32_t w = __builtin_amdgcn_readfirstlane(mw[g >> 5]) >> (g & 31);
            if (w & 1u)
                return t;
            t = (w ? g + (uint32_t)__ffs((int)w) - 1u : (g | 31u) + 1u) << map_shift; // the next set bit, or the next word
        }
        return ntiles;
    };
    // a column at or beyond c_end is not read (the lane reads the split's first row and drops it)
    auto fetch = [&](uint32_t t) {
        const size_t c = c_begin + ((size_t)t << 5) + m;
        load_row(X + (c < c_end ? c : c_begin) * (size_t)d, nxt);
    };
    uint32_t t = next_tile(0), bits = 0;
    if (t < ntiles)
        fetch(t);
    while (t < ntiles) {
        const size_t col = c_begin + ((size_t)t << 5) + m;
        const bool col_ok = col < c_end;
        to_i8(nxt, cur);
        const uint32_t tn = next_tile(t + 1);
        if (tn < ntiles)
            fetch(tn); // in flight behind this tile's MFMAs
        i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int xn = 0;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], cur[s], acc, 0, 0, 0);
            xn = exact_sq4(cur[s], xn);
        }
        xn += __shfl_xor(xn, 32);
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; r++)
            any |= (acc[r] << 1) - xn > gate[r];
        const bool hit = __ballot(any && col_ok) != 0; // wave-uniform
        if (hit) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const bool pass = col_ok && (acc[r] << 1) - xn > gate[r];
                const unsigned long long mask = __ballot(pass);
                const uint32_t half = kk ? (uint32_t)(mask >> 32) : (uint32_t)mask;
                if (FILL) {
                    const size_t o = (size_t)cnt[r] + __popc(half & ((1u << m) - 1u));
                    if (pass && o < out_cap) { // (o < out_cap always: the count form counted this very lane)
                        out_d[o] = (float)(qn_r[r] + xn - 2 * acc[r]);
                        out_l[o] = (long long)col;
                    }
                }
                cnt[r] += __popc(half);
            }
        }
        if (!FILL && mw) {
            const uint32_t g = t >> map_shift;
            bits |= hit ? 1u << (g & 31) : 0u;
            if (tn >= ntiles || (tn >> map_shift) >> 5 != g >> 5) { // the word is complete
                if (lane == 0)
                    mw[g >> 5] = bits;
                bits = 0;
            }
        }
        t = tn;
    }
    if (!FILL) {
        unsigned long long sum = 0;
        if (m == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
                if (r0 + row < nq)
                    slices[(q_off + r0 + row) * nsplit + split] = cnt[r];
                sum += cnt[r];
            }
        }
        sum += __shfl_xor(sum, 32);
        if (lane == 0 && sum)
            atomicAdd(total, sum);
    }
}

template <int NS>
hipError_t launch_exact_range_t(hipStream_t s, bool fill, dim3 grid, const uint8_t *Qp, const uint8_t *X, int nq, size_t nx, int d,
                                int thr, size_t cps, size_t q_off, uint32_t *slices, unsigned long long *total, uint32_t *map,
                                int map_shift, int map_words, float *out_d, long long *out_l, size_t out_cap)
{
    if (fill)
        hipLaunchKernelGGL((exact_range_kernel<NS, true>), grid, dim3(256), 0, s, Qp, X, nq, nx, d, thr, cps, q_off, slices, total,
                           map, map_shift, map_words, out_d, out_l, out_cap);
    else
        hipLaunchKernelGGL((exact_range_kernel<NS, false>), grid, dim3(256), 0, s, Qp, X, nq, nx, d, thr, cps, q_off, slices, total,
                           map, map_shift, map_words, out_d, out_l, out_cap);
    return hipGetLastError();
}

} // namespace

static size_t exact_range_cols_per_split(size_t nx, int nsplit)
{
    size_t cps = (nx + nsplit - 1) / nsplit;
    cps = (cps + 31) & ~(size_t)31;
    return cps ? cps : 32;
}

int exact_range_map_words(size_t nx, int nsplit, int map_shift)
{
    const size_t tiles = exact_range_cols_per_split(nx, nsplit) / 32;
    const size_t bits = (tiles + ((size_t)1 << map_shift) - 1) >> map_shift;
    return (int)((bits + 31) / 32);
}

hipError_t launch_exact_range(hipStream_t s, bool fill, const uint8_t *Qp, const uint8_t *X, size_t nq, size_t q_off, size_t nx,
                              int d, int thr, int nsplit, uint32_t *slices, unsigned long long *total, uint32_t *map,
                              int map_shift, float *dist, int64_t *labels, size_t out_cap)
{
    if (nq == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || thr < 0 || nq > 0x7fffffffull || nx >= 0xffffffffull || nsplit < 1 || nsplit > 64 ||
        (q_off & 31) || map_shift < 0 || map_shift > kExactRangeMaxShift)
        return hipErrorInvalidValue;
    const size_t cps = exact_range_cols_per_split(nx, nsplit);
    const int words = exact_range_map_words(nx, nsplit, map_shift);
    // query tile is the fast index, column split the slow one, as in launch_exact_t
    const dim3 grid((unsigned)((nq + 127) / 128), (unsigned)nsplit);
    long long *lab = reinterpret_cast<long long *>(labels);
#define IVFHNSW_EXACT_RANGE(NS) \
    launch_exact_range_t<NS>(s, fill, grid, Qp, X, (int)nq, nx, d, thr, cps, q_off, slices, total, map, map_shift, words, dist, lab, out_cap)
    switch ((d + 31) / 32) {
    case 1: return IVFHNSW_EXACT_RANGE(1);
    case 2: return IVFHNSW_EXACT_RANGE(2);
    case 3: return IVFHNSW_EXACT_RANGE(3);
    case 4: return IVFHNSW_EXACT_RANGE(4);
    case 5: return IVFHNSW_EXACT_RANGE(5);
    case 6: return IVFHNSW_EXACT_RANGE(6);
    case 7: return IVFHNSW_EXACT_RANGE(7);
    default: return IVFHNSW_EXACT_RANGE(8);
    }
#undef IVFHNSW_EXACT_RANGE
}

int exact_rows_per_block(int k) { return k <= 32 ? 128 : 64; }

int exact_splits_for(size_t nq, size_t nx, int k)
{
    // enough workgroups for two per CU; a split never shorter than 4096 columns
    const size_t rpb = (size_t)exact_rows_per_block(k);
    const size_t row_blocks = (nq + rpb - 1) / rpb;
    size_t s = (512 + row_blocks - 1) / row_blocks;
    const size_t max_s = (nx + 4095) / 4096;
    s = s > max_s ? max_s : s;
    s = s < 1 ? 1 : s;
    return (int)(s > 64 ? 64 : s);
}

// Qp: [nq][d] queries in the store's byte order (launch_rerank_permute); part: [nsplit][nq][k] u64 workspace
hipError_t launch_exact_search(hipStream_t s, const uint8_t *Qp, const uint8_t *X, size_t nq, size_t nx, int d, int k,
                               int nsplit, unsigned long long *part, float *dists, int64_t *labels)
{
    if (nq == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || k < 1 || k > 100 || nq > 0x7fffffffull || nx >= 0xffffffffull || nsplit < 1 ||
        nsplit > 64)
        return hipErrorInvalidValue;
    size_t cps = (nx + nsplit - 1) / nsplit;
    cps = (cps + 31) & ~(size_t)31;
    cps = cps ? cps : 32;
    hipError_t e;
    const int ns = (d + 31) / 32;
#define IVFHNSW_EXACT(NS)                                                                                     \
    (k <= 16   ? launch_exact_t<NS, 48, 4>(s, Qp, X, (int)nq, nx, d, k, nsplit, cps, part)                   \
     : k <= 32 ? launch_exact_t<NS, 64, 4>(s, Qp, X, (int)nq, nx, d, k, nsplit, cps, part)                   \
               : launch_exact_t<NS, 136, 2>(s, Qp, X, (int)nq, nx, d, k, nsplit, cps, part))
    switch (ns) {
    case 1: e = IVFHNSW_EXACT(1); break;
    case 2: e = IVFHNSW_EXACT(2); break;
    case 3: e = IVFHNSW_EXACT(3); break;
    case 4: e = IVFHNSW_EXACT(4); break;
    case 5: e = IVFHNSW_EXACT(5); break;
    case 6: e = IVFHNSW_EXACT(6); break;
    case 7: e = IVFHNSW_EXACT(7); break;
    default: e = IVFHNSW_EXACT(8); break;
    }
#undef IVFHNSW_EXACT
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(exact_merge_kernel, dim3((unsigned)nq), dim3(64), 0, s, part, nsplit, (int)nq, k, dists,
                       reinterpret_cast<long long *>(labels));
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
