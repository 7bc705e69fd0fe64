// The float16 base store (ivfhnsw_gpu_upload_base_f16) and its exact brute-force search on the f16 matrix cores
// (ivfhnsw_gpu_exact_search_f16).
//
// The store: every float32 value rounded to half (round to nearest even), rows permuted as the uint8 store's are
// (kernels_rerank.hip: lane t of a quad owns dims 8j + 2t, 8j + 2t + 1 as the d/4 contiguous halves [t d/4, (t + 1) d/4)), and
// beside the rows one float32 per row: the squared norm of the ROUNDED row.
//
// Arithmetic of the search, q^ and x^ the rounded vectors:
//     dist(q, x) = (|q^|^2 + |x^|^2) - 2 q^.x^        two rounded float32 operations, 2 * dot is exact
//     q^.x^      = a chain of v_mfma_f32_32x32x16_f16 over the d/16 steps of a row, float32 accumulation
// The queries go through the store's permutation once per call, so whatever contraction order the instruction gives the
// eight halves of a lane, it gives the same one to both operands; only the C/D map is relied on (sweep_steps.h mfma32_row).
// Where every value is an integer (or the same power of two times one) and every partial sum stays below 2^24 each
// operation is exact in any order and the result is the integer distance.
//
// Shape: wave w of a workgroup owns the 32 query rows [32w, 32w + 32) of the workgroup's strip for the whole sweep, operand
// A resident in d/16 x 4 registers.  Operand B is staged ONCE PER WORKGROUP: a tile of 32 columns is 32 rows of 2d bytes,
// contiguous in the store; the workgroup's threads copy it in 16-byte pieces into one of TWO LDS tiles while the waves
// multiply the other, the global loads of tile t + 1 in flight in registers behind the MFMAs of tile t, one barrier per
// tile.  An LDS row is padded by 16 bytes: its stride in words is 4 (d/8 + 1), four times an odd number, so the sixteen
// lanes of a ds_read_b128 pass fall on sixteen distinct groups of four banks.  A column's norm comes from the table, one
// float per column lane per tile.  The common tile (none of the wave's 32 x 32 distances is a candidate) costs one
// multiply-subtract and one compare per accumulator register against a per-row gate; selection and merge are
// sweep_steps.h's with float keys, as in kernels_knn.hip: columns arrive in increasing order, so ties go to the lower label
// by the strict '<' alone.
#include "sweep_steps.h"

#include <float.h>
#include <math.h>

namespace ivfhnsw_gpu_impl {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- upload -------------------------------------------------------------------------------------------------------------
// *flag |= 1 where a value of rows [count] at src_stride floats is NaN or does not round to a finite half: 65520 is the
// midpoint between the largest half, 65504, and 2^16, and rounds to even -- to infinity.
__global__ __launch_bounds__(256) void f16_check_kernel(const float *__restrict__ src, size_t src_stride, size_t count, int d,
                                                        uint32_t *__restrict__ flag)
{
    const size_t total = count * (size_t)d;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / (size_t)d;
        bad |= !(fabsf(src[r * src_stride + (i - r * (size_t)d)]) < 65520.f);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0)
        atomicOr(flag, 1u);
}

// One lane per (row, quad lane t): the lane's d/4 halves, two to a word, and its share of the norm; the quad adds the four
// shares.  The norm is that of the rounded values: fmaf chains of d/8 terms, then three additions.
// GATHER (the queries of a strip plan): row r comes from row row_src[r] of src, a negative entry -- the
// padding of a strip -- from row 0; the arithmetic is the same text, so a gathered row is the row the plain form makes.
template <bool GATHER>
__global__ __launch_bounds__(256) void f16_store_kernel(const float *__restrict__ src, size_t src_stride, _Float16 *__restrict__ dst,
                                                        float *__restrict__ norms, size_t count, int d,
                                                        const int32_t *__restrict__ row_src)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t r = i >> 2;
    const int t = (int)(i & 3);
    const bool ok = r < count; // (the four lanes of a quad agree)
    size_t from = ok ? r : 0;
    if constexpr (GATHER)
        from = (size_t)max(row_src[from], 0);
    const float *row = src + from * src_stride + 2 * t;
    uint32_t *out = reinterpret_cast<uint32_t *>(dst + (ok ? r : 0) * (size_t)d + t * (d >> 2));
    float alo = 0.f, ahi = 0.f;
    for (int j = 0; j < (d >> 3); j++) {
        const _Float16 h0 = (_Float16)row[8 * j], h1 = (_Float16)row[8 * j + 1];
        if (ok)
            out[j] = (uint32_t)__builtin_bit_cast(unsigned short, h0) | ((uint32_t)__builtin_bit_cast(unsigned short, h1) << 16);
        const float f0 = (float)h0, f1 = (float)h1;
        alo = __fmaf_rn(f0, f0, alo);
        ahi = __fmaf_rn(f1, f1, ahi);
    }
    float s = __fadd_rn(alo, ahi);
    s = __fadd_rn(s, __shfl_xor(s, 1));
    s = __fadd_rn(s, __shfl_xor(s, 2));
    if (ok && t == 0)
        norms[r] = s;
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------
// What the common tile compares against.  A distance is a candidate when
//     dist = fl(fl(qn + xn) - 2 dot) < thr,
// and the tile's cheap test is fl(2 dot - xn) > gate with gate = qn - thr lowered by a margin that covers the three
// roundings: each is at most 2^-24 of its result.  For a candidate the results are bounded by the row's own numbers --
// |dist| <= |thr| or so, and xn <= (sqrt(qn) + sqrt(dist))^2 <= 2 (qn + dist) by Cauchy-Schwarz, so qn + xn and |2 dot - xn|
// stay below 3 (qn + |thr|) -- which makes the sum of the three at most 2^-22 (qn + |thr|).  The margin is sixteen times
// that: the dot product's own rounding bends the Cauchy-Schwarz step a little, and a tile that passes the cheap test in
// vain costs only the exact test behind it.  thr = FLT_MAX (fewer than k keys yet) gives -inf: every tile passes.
// thr = -inf marks a row that is no query (beyond nq): nothing passes, ever.
// The range search (exact_range_f16_kernel) sets the gate ONCE from a thr that is the caller's radius: any float, small,
// zero or negative.  The argument holds as it stands.  A returned distance is never far below zero -- it is within
// (d + 3) 2^-23 (|q^| + |x^|)^2 of a real squared distance, and where it is negative x^ is nearly q^, so |dist| < 2^-12 qn --
// hence |dist| <= |thr| + 2^-12 qn whatever the sign of thr, which is the "or so" above.  The gate's own two subtractions
// round as well, each by at most 2^-24 (qn + |thr|): with them the roundings sum to less than 1.6 * 2^-22 (qn + |thr|), a
// tenth of the margin, so it is not widened.  thr = +inf gives -inf as FLT_MAX does; a query whose norm is not finite
// gives a NaN gate, which nothing passes, and its distances are inf or NaN, which are below no radius.
__device__ __forceinline__ float f16_gate(float qn, float thr)
{
    if (thr == -INFINITY)
        return INFINITY;
    return __fsub_rn(__fsub_rn(qn, thr), __fmul_rn(0x1p-18f, __fadd_rn(qn, fabsf(thr))));
}

// What a wave of the per-wave sweep (exact_f16_rows_kernel) does with a multiplied tile: acc[r] = q^.x^ of row
// mfma32_row(r, kk) and the lane's column, whose norm is xn_col and whose label is `label`; col_ok: the lane has a column.
// The common tile costs the cheap test; behind it the exact test, the append, the compaction of the rows that could
// overflow and the new gates -- the steps of exact_f16_kernel's loop in its arithmetic, operation for operation.  That
// kernel keeps them in its own body: called from there, this function costs its plain instantiations 6 to 17 registers
// and, at d = 96 and d = 192, a wave of occupancy (the compiler's report).
template <int CAP>
__device__ __forceinline__ void f16_select(const f32x16 &acc, float xn_col, bool col_ok, uint32_t label, const float (&qn_r)[16],
                                           float (&gate)[16], unsigned long long *buf, uint32_t *cnt, float *thr_s, int k, int lane)
{
    const int m = lane & 31, kk = lane >> 5;
    bool any = false;
#pragma unroll
    for (int r = 0; r < 16; r++)
        any |= __fsub_rn(__fmul_rn(2.0f, acc[r]), xn_col) > gate[r];
    if (__ballot(any && col_ok)) { // wave-uniform: rare once the thresholds have settled
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float dist = __fsub_rn(__fadd_rn(qn_r[r], xn_col), __fmul_rn(2.0f, acc[r]));
            const int row = mfma32_row(r, kk);
            const bool pass = col_ok && dist < thr_s[row];
            const unsigned long long mask = __ballot(pass);
            if (mask)
                row_append<CAP>(buf, cnt, row, pass, mask, dist, label, m, kk);
        }
        rows_compact<CAP>(buf, cnt, thr_s, k, lane);
#pragma unroll
        for (int r = 0; r < 16; r++)
            gate[r] = f16_gate(qn_r[r], thr_s[mfma32_row(r, kk)]);
    }
}

// ND = d / 16, the MFMA steps of a row; CAP = keys of a row's candidate buffer (a row is compacted when it holds more than
// CAP - 32); WAVES = 32-row strips per workgroup.  Qh [nq][d] the queries as the store holds its rows, qn [nq] their norms;
// X [nx][d], xn [nx] the store.
// SP: F16Rows is the plain call.  F16DenseStrips (base tags): Qh, qn are the nq = 32 * bound rows of a strip
// plan, and workgroup i owns the strips [WAVES i, WAVES i + WAVES) of the plan's Dense range -- the untagged queries, which
// sweep the whole store and so share its staging.  A workgroup beyond the range leaves before the first barrier; a wave
// beyond it in a workgroup that stays stages and meets every barrier, multiplies nothing and writes nothing
// (exact_range_f16_kernel's `active`); a padding row of a strip holds the threshold of a row beyond nq.
struct F16Rows {
    static constexpr bool kStrips = false;
};
struct F16DenseStrips {
    static constexpr bool kStrips = true;
    StripPlan sp;
};

template <int ND, int CAP, int WAVES, class SP>
__global__ __launch_bounds__(64 * WAVES) void exact_f16_kernel(const _Float16 *__restrict__ Qh, const float *__restrict__ qn,
                                                               const _Float16 *__restrict__ X, const float *__restrict__ xn,
                                                               int nq, size_t nx, int k, size_t cols_per_split,
                                                               unsigned long long *__restrict__ out_keys, SP sp)
{
    constexpr int D = 16 * ND, T = 64 * WAVES;
    constexpr int ROWB = 2 * D + 16;        // bytes of a tile's row in LDS: the row and its padding
    constexpr int TILEB = 32 * ROWB;
    constexpr int PPR = D / 8;              // 16-byte pieces of a row,
    constexpr int NPIECE = 32 * PPR;        // ... of a tile,
    constexpr int NP = (NPIECE + T - 1) / T; // ... of a thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *s_tile = smem;                                                              // [2][TILEB]
    unsigned long long *s_buf = reinterpret_cast<unsigned long long *>(smem + 2 * TILEB);       // [WAVES][32][CAP]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_buf + WAVES * 32 * CAP);                   // [WAVES][32]
    float *s_thr = reinterpret_cast<float *>(s_cnt + WAVES * 32);                               // [WAVES][32]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    int r0 = blockIdx.x * (32 * WAVES) + wave * 32;
    bool active = true; // wave-uniform
    if constexpr (SP::kStrips) {
        const uint32_t s0 = sp.sp.hdr->lay.range[kSweepColsDense][0] + blockIdx.x * WAVES, s1 = sp.sp.hdr->lay.range[kSweepColsDense][1];
        if (s0 >= s1)
            return;
        active = s0 + wave < s1;
        r0 = (int)((active ? s0 + wave : s0) << 5);
    }
    // (the same for every wave of the workgroup: all of them meet at every barrier below)
    const size_t c_begin = (size_t)blockIdx.y * cols_per_split < nx ? (size_t)blockIdx.y * cols_per_split : nx;
    const size_t c_end = c_begin + cols_per_split < nx ? c_begin + cols_per_split : nx;
    unsigned long long *buf = s_buf + (size_t)wave * 32 * CAP;
    uint32_t *cnt = s_cnt + wave * 32;
    float *thr_s = s_thr + wave * 32;

    // operand A: lane (m, kk) holds for step s the stored halves [16 s + 8 kk, + 8) of query row r0 + m (a row beyond nq
    // repeats the last one and is never a candidate)
    f16x8 a[ND];
    {
        const _Float16 *qr = Qh + (size_t)min(r0 + m, nq - 1) * D + 8 * kk;
#pragma unroll
        for (int s = 0; s < ND; s++)
            a[s] = *reinterpret_cast<const f16x8 *>(qr + 16 * s);
    }
    if (lane < 32) {
        bool is_query = r0 + lane < nq;
        if constexpr (SP::kStrips)
            is_query = active && sp.sp.strip_rows[r0 + lane] >= 0;
        cnt[lane] = 0;
        thr_s[lane] = is_query ? FLT_MAX : -INFINITY;
    }
    __builtin_amdgcn_wave_barrier();
    float qn_r[16], gate[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = mfma32_row(r, kk);
        qn_r[r] = qn[min(r0 + row, nq - 1)];
        gate[r] = f16_gate(qn_r[r], thr_s[row]);
    }

    // staging: thread tid takes the pieces tid, tid + T, ... of a tile, piece p = 16 bytes at byte 16 p of the tile in the
    // store, which is byte 16 (p % PPR) of tile row p / PPR.  A row at or beyond c_end is not read: its pieces are zeros.
    uint4 pre[NP];
    float pre_n = 0.f;
    auto fetch = [&](size_t c0) {
        const unsigned char *src = reinterpret_cast<const unsigned char *>(X) + c0 * (size_t)(2 * D);
        const int rows_in = c_end - c0 < 32 ? (int)(c_end - c0) : 32;
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int p = tid + i * T;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if ((NPIECE % T == 0 || p < NPIECE) && p / PPR < rows_in)
                v = *reinterpret_cast<const uint4 *>(src + 16 * (size_t)p);
            pre[i] = v;
        }
        pre_n = c0 + m < c_end ? xn[c0 + m] : 0.f;
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int p = tid + i * T;
            if (NPIECE % T == 0 || p < NPIECE)
                *reinterpret_cast<uint4 *>(s_tile + b * TILEB + (p / PPR) * ROWB + 16 * (p % PPR)) = pre[i];
        }
    };

    float xn_cur = 0.f;
    if (c_begin < c_end) {
        fetch(c_begin);
        stash(0);
        xn_cur = pre_n;
    }
    __syncthreads();
    int b = 0;
    for (size_t c0 = c_begin; c0 < c_end; c0 += 32, b ^= 1) {
        const bool more = c0 + 32 < c_end;
        if (more)
            fetch(c0 + 32); // in flight behind this tile's MFMAs
        if (active) {
            const unsigned char *bt = s_tile + b * TILEB + m * ROWB + 16 * kk;
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < ND; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], *reinterpret_cast<const f16x8 *>(bt + 32 * s), acc, 0, 0, 0);
            const size_t col = c0 + m;
            const bool col_ok = col < c_end;
            bool any = false;
#pragma unroll
            for (int r = 0; r < 16; r++)
                any |= __fsub_rn(__fmul_rn(2.0f, acc[r]), xn_cur) > gate[r];
            if (__ballot(any && col_ok)) { // wave-uniform: rare once the thresholds have settled
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float dist = __fsub_rn(__fadd_rn(qn_r[r], xn_cur), __fmul_rn(2.0f, acc[r]));
                    const int row = mfma32_row(r, kk);
                    const bool pass = col_ok && dist < thr_s[row];
                    const unsigned long long mask = __ballot(pass);
                    if (mask)
                        row_append<CAP>(buf, cnt, row, pass, mask, dist, (uint32_t)col, m, kk);
                }
                rows_compact<CAP>(buf, cnt, thr_s, k, lane);
#pragma unroll
                for (int r = 0; r < 16; r++)
                    gate[r] = f16_gate(qn_r[r], thr_s[mfma32_row(r, kk)]);
            }
        }
        if (more)
            stash(b ^ 1); // the tile every wave left at the last barrier
        xn_cur = pre_n;
        __syncthreads();
    }

    // out: [split][nq][k] keys
    if (active)
        rows_write_out<CAP>(buf, cnt, k, lane, nq - r0, out_keys, (size_t)blockIdx.y * nq + r0);
}

__global__ __launch_bounds__(64) void exact_f16_merge_kernel(const unsigned long long *__restrict__ part, int nsplit, int nq, int k,
                                                             float *__restrict__ dists, long long *__restrict__ labels)
{
    sweep_merge(
        part, nsplit, nq, k,
        [&](size_t o, unsigned long long key) {
            labels[o] = (long long)(uint32_t)key;
            dists[o] = orderable_f32((uint32_t)(key >> 32));
        },
        [&](size_t o) { // the store has fewer than k rows
            labels[o] = -1ll;
            dists[o] = FLT_MAX;
        });
}

// sp: F16Rows{} -- the nq queries in their order -- or F16DenseStrips{plan}: nq = the plan's rows, the grid covers every strip
// the plan can have and the workgroups beyond its Dense range leave at once
template <int ND, int CAP, int WAVES, class SP>
hipError_t launch_exact_f16_t(hipStream_t s, const _Float16 *Qh, const float *qn, const _Float16 *X, const float *xn, int nq,
                              size_t nx, int k, int nsplit, size_t cols_per_split, unsigned long long *part, SP sp)
{
    const size_t shm = exact_f16_lds_bytes(16 * ND, k);
    constexpr auto kern = exact_f16_kernel<ND, CAP, WAVES, SP>;
    if (hipError_t e = dyn_lds<kern>(shm); e != hipSuccess)
        return e;
    // query tile is the fast index, column split the slow one: the workgroups that run together stream the same columns
    hipLaunchKernelGGL(kern, dim3((unsigned)((nq + 32 * WAVES - 1) / (32 * WAVES)), (unsigned)nsplit), dim3(64 * WAVES), shm, s,
                       Qh, qn, X, xn, nq, nx, k, cols_per_split, part, sp);
    return hipGetLastError();
}

// ---- the tagged strips (ivfhnsw_gpu_exact_search_f16_tags) -----------------------------------------------
// An Indirect strip of a tag plan sweeps its tag's row list, and the strips of a workgroup sweep different lists: there is no
// tile to share, so a strip is a wave, there is no barrier and no LDS tile, and a wave without a strip, or whose split of a
// short list is empty, leaves at once (the merge reads only the splits that have columns).  Operand A is resident as in
// exact_f16_kernel.  For a tile of 32 columns lane (m, kk) reads rows[c0 + m] -- ascending, so the row number is the
// column's label -- and takes its operand B straight from the store: piece s is the 16 bytes at row * 2d + 32 s + 16 kk,
// the address pattern exact_f16_kernel reads from its LDS row; the store's quad permutation lays a row out in MFMA order,
// and over the ND steps the two lanes of a column consume the row's 2d contiguous bytes whole.  The column's norm is
// xn[row].  In flight behind the MFMAs of tile t: the row numbers of tile t + 2, the norms and the first NPRE pieces of
// tile t + 1 (two register buffers, the loop unrolled by two so that nothing is copied).  NPRE = ND up to d = 128; beyond
// it half the pieces, the other half loaded when their tile begins and in flight behind the MFMAs of its first half: 1.5 ND
// pieces live instead of 2 ND, which is what keeps ND = 16 within the registers of two waves per SIMD.
// A column at or beyond c_end is not read -- its pieces are zeros -- and never passes.
template <int ND, int CAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void exact_f16_rows_kernel(const _Float16 *__restrict__ Qh, const float *__restrict__ qn,
                                                                    const _Float16 *__restrict__ X, const float *__restrict__ xn,
                                                                    int nrows, int k, unsigned long long *__restrict__ out_keys,
                                                                    StripPlan sp)
{
    constexpr int D = 16 * ND;
    constexpr int NPRE = ND <= 8 ? ND : (ND + 1) / 2, NLATE = ND - NPRE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *s_buf = reinterpret_cast<unsigned long long *>(smem); // [WAVES][32][CAP]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_buf + WAVES * 32 * CAP);  // [WAVES][32]
    float *s_thr = reinterpret_cast<float *>(s_cnt + WAVES * 32);             // [WAVES][32]

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    const uint32_t strip = sp.hdr->lay.range[kSweepColsIndirect][0] + blockIdx.x * WAVES + wave;
    if (strip >= sp.hdr->lay.range[kSweepColsIndirect][1])
        return;
    const StripCols e = sp.strip_cols[strip];
    size_t c_begin, c_end;
    sweep_split_cut(e.nx, (int)gridDim.y, (int)blockIdx.y, &c_begin, &c_end);
    if (c_begin >= c_end)
        return;
    const uint32_t *__restrict__ rows = e.data;
    const int r0 = (int)(strip << 5); // (strip < the plan's bound: every row of it exists in Qh, qn and strip_rows)
    unsigned long long *buf = s_buf + (size_t)wave * 32 * CAP;
    uint32_t *cnt = s_cnt + wave * 32;
    float *thr_s = s_thr + wave * 32;

    f16x8 a[ND];
    {
        const _Float16 *qr = Qh + (size_t)(r0 + m) * D + 8 * kk;
#pragma unroll
        for (int s = 0; s < ND; s++)
            a[s] = *reinterpret_cast<const f16x8 *>(qr + 16 * s);
    }
    if (lane < 32) {
        cnt[lane] = 0;
        thr_s[lane] = sp.strip_rows[r0 + lane] >= 0 ? FLT_MAX : -INFINITY;
    }
    __builtin_amdgcn_wave_barrier();
    float qn_r[16], gate[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = mfma32_row(r, kk);
        qn_r[r] = qn[r0 + row];
        gate[r] = f16_gate(qn_r[r], thr_s[row]);
    }

    const unsigned char *xb = reinterpret_cast<const unsigned char *>(X) + 16 * kk;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    // the row number of the lane's column of the tile that begins at c0
    auto ids = [&](size_t c0) -> uint32_t { return c0 + m < c_end ? rows[c0 + m] : 0u; };
    // pieces [first, first + N) of store row `row` into w; ok: the lane has a column
    auto pieces = [&](uint32_t row, bool ok, int first, auto &w) {
        constexpr int N = (int)(sizeof(w) / sizeof(w[0]));
        const unsigned char *p = xb + (size_t)row * (2 * D) + 32 * first;
#pragma unroll
        for (int s = 0; s < N; s++)
            w[s] = zero;
        if (ok) {
#pragma unroll
            for (int s = 0; s < N; s++)
                w[s] = *reinterpret_cast<const f16x8 *>(p + 32 * s);
        }
    };
    // The tile at c0: `cur`, n_cur = its first NPRE pieces and its norms, id_cur its row numbers.  Starts the loads of tile
    // c0 + 32 (row numbers id_nxt) into nxt, n_nxt and of the row numbers of tile c0 + 64 into id_ahead.
    auto tile = [&](size_t c0, const f16x8 (&cur)[NPRE], float n_cur, uint32_t id_cur, f16x8 (&nxt)[NPRE], float &n_nxt, uint32_t id_nxt,
                    uint32_t &id_ahead) {
        const bool col_ok = c0 + m < c_end;
        f16x8 late[NLATE > 0 ? NLATE : 1];
        if constexpr (NLATE > 0)
            pieces(id_cur, col_ok, NPRE, late);
        if (c0 + 32 < c_end) { // in flight behind this tile's MFMAs
            const bool ok = c0 + 32 + m < c_end;
            pieces(id_nxt, ok, 0, nxt);
            n_nxt = ok ? xn[id_nxt] : 0.f;
        }
        if (c0 + 64 < c_end)
            id_ahead = ids(c0 + 64);
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NPRE; s++)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], cur[s], acc, 0, 0, 0);
        if constexpr (NLATE > 0) {
#pragma unroll
            for (int s = 0; s < NLATE; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[NPRE + s], late[s], acc, 0, 0, 0);
        }
        f16_select<CAP>(acc, n_cur, col_ok, id_cur, qn_r, gate, buf, cnt, thr_s, k, lane);
    };

    f16x8 b0[NPRE], b1[NPRE];
    float n0, n1 = 0.f;
    uint32_t id0 = ids(c_begin), id1 = 0, id_ahead = 0;
    pieces(id0, c_begin + m < c_end, 0, b0);
    n0 = c_begin + m < c_end ? xn[id0] : 0.f;
    if (c_begin + 32 < c_end)
        id1 = ids(c_begin + 32);
    for (size_t c0 = c_begin;;) {
        tile(c0, b0, n0, id0, b1, n1, id1, id_ahead);
        if ((c0 += 32) >= c_end)
            break;
        id0 = id_ahead;
        tile(c0, b1, n1, id1, b0, n0, id0, id_ahead);
        if ((c0 += 32) >= c_end)
            break;
        id1 = id_ahead;
    }

    // out: [split][plan row][k] keys, every row of the strip (a padding row holds nothing)
    rows_write_out<CAP>(buf, cnt, k, lane, 32, out_keys, (size_t)blockIdx.y * nrows + r0);
}

// The merge under a tag plan, one wavefront per plan row (exact_merge_strips_kernel with float keys): the row of a query
// goes to the query's place in the caller's order, padding rows and strips beyond the plan's are dropped.  part
// [split][nrows][k]; a Dense strip wrote ns_dense splits, an Indirect one the splits of ns_ind that have columns of its list.
__global__ __launch_bounds__(64) void exact_f16_merge_strips_kernel(const unsigned long long *__restrict__ part, int ns_dense,
                                                                    int ns_ind, int nrows, int k, float *__restrict__ dists,
                                                                    long long *__restrict__ labels, StripPlan sp)
{
    const uint32_t row = blockIdx.x, strip = row >> 5;
    if (strip >= sp.hdr->lay.nstrips)
        return;
    const int q = sp.strip_rows[row];
    if (q < 0)
        return;
    int ns = ns_dense;
    if (strip >= sp.hdr->lay.range[kSweepColsIndirect][0]) {
        const size_t nx = sp.strip_cols[strip].nx, cps = sweep_cols_per_split(nx, ns_ind);
        ns = (int)min((size_t)ns_ind, (nx + cps - 1) / cps);
    }
    sweep_merge_row(
        part, ns, nrows, k, (int)row, q,
        [&](size_t o, unsigned long long key) {
            labels[o] = (long long)(uint32_t)key;
            dists[o] = orderable_f32((uint32_t)(key >> 32));
        },
        [&](size_t o) { // fewer than k rows carry the query's tag
            labels[o] = -1ll;
            dists[o] = FLT_MAX;
        });
}

template <int ND, int CAP, int WAVES>
hipError_t launch_exact_f16_rows_t(hipStream_t s, const _Float16 *Qh, const float *qn, const _Float16 *X, const float *xn, size_t bound,
                                   int k, int nsplit, unsigned long long *part, const StripPlan &sp)
{
    const size_t shm = (size_t)WAVES * 32 * CAP * sizeof(unsigned long long) + (size_t)WAVES * 32 * (sizeof(uint32_t) + sizeof(float));
    constexpr auto kern = exact_f16_rows_kernel<ND, CAP, WAVES>;
    if (hipError_t e = dyn_lds<kern>(shm); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)((bound + WAVES - 1) / WAVES), (unsigned)nsplit), dim3(64 * WAVES), shm, s, Qh, qn, X, xn,
                       (int)(bound * 32), k, part, sp);
    return hipGetLastError();
}

// ---- the windowed strips (ivfhnsw_gpu_exact_search_f16_values) -------------------------------------------
// A windowed strip of a value plan sweeps a span of the holder's rows in (value, row) order, and every strip row counts only
// the columns of ITS OWN window win[32 strip + row] = [wa, wb) of the span.  The sweep is exact_f16_rows_kernel's -- a strip a
// wave, no barrier, no LDS tile, operand A resident, operand B straight from the store through the span's row numbers in
// MFMA order, the same prefetch depths -- with three things of its own.
//   Windows in lanes.  Lanes m and m + 32 hold row m's window.  Whether a tile of 32 columns is LIVE -- some window meets
//   it -- is one ballot over (c0, wa, wb): it depends on nothing that is loaded.  The pipeline therefore aims at live tiles
//   only, as exact_range_f16_rows_kernel's aims at visited ones: t is the tile being multiplied, tn the next live one (its
//   norms and pieces are requested now), ta the live one after it (its row numbers are).  next_tile decides before anything
//   of a tile is requested: a dead tile costs no row number, norm, piece or MFMA.  It steps while tiles are live -- one
//   ballot -- and at the first dead tile JUMPS: every lane whose window ends beyond the tile offers the tile its window
//   starts in, a wave minimum (five exchanges) takes the nearest.  A gap costs one reduction however long it is.
//   The two tests.  The cheap test counts an accumulator register only where its row's live bit is set; a tile inside
//   every non-empty window (`all`, a second ballot) takes the unwindowed test.  A padding row and a row whose window is
//   empty hold the threshold -inf and so the gate +inf, for good.  The exact test, behind the cheap one, reads the row's
//   window from its lane and rejects the columns of an edge tile outside it.
//   Arrival order.  Columns come in (value, row) order, not label order, so `<` alone no longer sends a tie to the lower
//   label.  Admission is dist <= thr; compaction, write-out and merge rank whole (distance bits, label) keys, which are
//   distinct, so of equal distances the lower label stays.  The cheap test is `>=`: f16_gate's margin is 2^-18 (qn + |thr|),
//   which is zero for a zero query whose k-th distance is zero, and 2 dot - xn > qn - thr would then drop dist == thr.
//   The buffer bound is unchanged by `<=`: a row enters a tile with at most CAP - 32 keys (one with more was compacted to
//   min(n, k) <= CAP - 32 keys behind the tile before: k <= 16 / 32 / 100 against CAP - 32 = 16 / 32 / 104), and a tile
//   appends at most its 32 columns.
// A split of the span without a live tile still writes its (empty) rows: the merge reads every split that has columns.
template <int ND, int CAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void exact_f16_windows_kernel(const _Float16 *__restrict__ Qh, const float *__restrict__ qn,
                                                                       const _Float16 *__restrict__ X, const float *__restrict__ xn,
                                                                       int nrows, int k, unsigned long long *__restrict__ out_keys,
                                                                       StripPlan sp, const StripWin *__restrict__ win)
{
    constexpr int D = 16 * ND;
    constexpr int NPRE = ND <= 8 ? ND : (ND + 1) / 2, NLATE = ND - NPRE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *s_buf = reinterpret_cast<unsigned long long *>(smem); // [WAVES][32][CAP]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_buf + WAVES * 32 * CAP);  // [WAVES][32]
    float *s_thr = reinterpret_cast<float *>(s_cnt + WAVES * 32);             // [WAVES][32]

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    const uint32_t strip = sp.hdr->lay.range[kSweepColsIndirect][0] + blockIdx.x * WAVES + wave;
    if (strip >= sp.hdr->lay.range[kSweepColsIndirect][1])
        return;
    const StripCols e = sp.strip_cols[strip];
    size_t cb, ce;
    sweep_split_cut(e.nx, (int)gridDim.y, (int)blockIdx.y, &cb, &ce);
    if (cb >= ce)
        return;
    const uint32_t c_begin = (uint32_t)cb, c_end = (uint32_t)ce; // (columns of a span: below the rows of the store)
    const uint32_t ntiles = (c_end - c_begin + 31u) >> 5;
    const uint32_t *__restrict__ rows = e.data;
    const int r0 = (int)(strip << 5); // (strip < the plan's bound: every row of it exists in Qh, qn, strip_rows and win)
    unsigned long long *buf = s_buf + (size_t)wave * 32 * CAP;
    uint32_t *cnt = s_cnt + wave * 32;
    float *thr_s = s_thr + wave * 32;

    f16x8 a[ND];
    {
        const _Float16 *qr = Qh + (size_t)(r0 + m) * D + 8 * kk;
#pragma unroll
        for (int s = 0; s < ND; s++)
            a[s] = *reinterpret_cast<const f16x8 *>(qr + 16 * s);
    }
    // the window of row m, in the span's columns; bit m of `empty`: row m has none
    const StripWin w = win[r0 + m];
    const uint32_t wa = w.a, wb = w.b;
    const uint32_t empty = (uint32_t)__ballot(wa >= wb);
    if (lane < 32) {
        cnt[lane] = 0;
        thr_s[lane] = sp.strip_rows[r0 + lane] >= 0 && wa < wb ? FLT_MAX : -INFINITY;
    }
    __builtin_amdgcn_wave_barrier();
    float qn_r[16], gate[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = mfma32_row(r, kk);
        qn_r[r] = qn[r0 + row];
        gate[r] = f16_gate(qn_r[r], thr_s[row]);
    }

    // the first column of tile t; does the lane's window meet the tile that begins at c0 (an empty window meets none; the
    // launch keeps columns below 2^32 - 64)
    auto col0 = [&](uint32_t t) -> uint32_t { return c_begin + (t << 5); };
    auto meets = [&](uint32_t c0) -> bool { return wa < c0 + 32u && wb > c0; };
    // the first live tile at or after t (ntiles: none); wave-uniform, from the windows alone
    auto next_tile = [&](uint32_t t) -> uint32_t {
        if (t >= ntiles)
            return ntiles;
        const uint32_t c0 = col0(t);
        if (__ballot(meets(c0)))
            return t;
        // dead: the tile in which the nearest window that ends beyond c0 begins (it begins beyond the tile, or it would meet it)
        uint32_t tt = wa < wb && wb > c0 ? ((wa > c0 ? wa : c0) - c_begin) >> 5 : ~0u;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) // (lanes m and m + 32 hold the same window: each half finds the minimum)
            tt = min(tt, (uint32_t)__shfl_xor((int)tt, o));
        tt = __builtin_amdgcn_readfirstlane(tt);
        return tt < ntiles ? tt : ntiles;
    };

    const unsigned char *xb = reinterpret_cast<const unsigned char *>(X) + 16 * kk;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    // the row number of the lane's column of tile t
    auto ids = [&](uint32_t t) -> uint32_t { return col0(t) + m < c_end ? rows[col0(t) + m] : 0u; };
    // pieces [first, first + N) of store row `row` into w; ok: the lane has a column
    auto pieces = [&](uint32_t row, bool ok, int first, auto &w) {
        constexpr int N = (int)(sizeof(w) / sizeof(w[0]));
        const unsigned char *p = xb + (size_t)row * (2 * D) + 32 * first;
#pragma unroll
        for (int s = 0; s < N; s++)
            w[s] = zero;
        if (ok) {
#pragma unroll
            for (int s = 0; s < N; s++)
                w[s] = *reinterpret_cast<const f16x8 *>(p + 32 * s);
        }
    };
    // Tile t: `cur`, n_cur = its first NPRE pieces and its norms, id_cur its row numbers.  Starts the loads of tile tn (row
    // numbers id_nxt) into nxt, n_nxt and of the row numbers of tile ta into id_ahead.
    auto tile = [&](uint32_t t, const f16x8 (&cur)[NPRE], float n_cur, uint32_t id_cur, uint32_t tn, f16x8 (&nxt)[NPRE], float &n_nxt,
                    uint32_t id_nxt, uint32_t ta, uint32_t &id_ahead) {
        const uint32_t c0 = col0(t), col = c0 + m;
        const bool col_ok = col < c_end;
        f16x8 late[NLATE > 0 ? NLATE : 1];
        if constexpr (NLATE > 0)
            pieces(id_cur, col_ok, NPRE, late);
        if (tn < ntiles) { // in flight behind this tile's MFMAs
            const bool ok = col0(tn) + m < c_end;
            pieces(id_nxt, ok, 0, nxt);
            n_nxt = ok ? xn[id_nxt] : 0.f;
        }
        if (ta < ntiles)
            id_ahead = ids(ta);
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NPRE; s++)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], cur[s], acc, 0, 0, 0);
        if constexpr (NLATE > 0) {
#pragma unroll
            for (int s = 0; s < NLATE; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[NPRE + s], late[s], acc, 0, 0, 0);
        }
        // the cheap test: inside every non-empty window the unwindowed one, else a register counts where its row is live
        const bool all = ((uint32_t)__ballot(wa <= c0 && wb >= c0 + 32u) | empty) == ~0u; // wave-uniform
        bool any = false;
        if (all) {
#pragma unroll
            for (int r = 0; r < 16; r++)
                any |= __fsub_rn(__fmul_rn(2.0f, acc[r]), n_cur) >= gate[r];
        } else {
            const uint32_t lv = (uint32_t)__ballot(meets(c0)) >> (4 * kk); // bit (r & 3) + 8 (r >> 2): register r's row is live
            uint32_t bits = 0;
#pragma unroll
            for (int r = 0; r < 16; r++)
                bits |= __fsub_rn(__fmul_rn(2.0f, acc[r]), n_cur) >= gate[r] ? 1u << ((r & 3) + 8 * (r >> 2)) : 0u;
            any = (bits & lv) != 0u;
        }
        if (__ballot(any && col_ok)) { // wave-uniform: rare once the thresholds have settled
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float dist = __fsub_rn(__fadd_rn(qn_r[r], n_cur), __fmul_rn(2.0f, acc[r]));
                const int row = mfma32_row(r, kk);
                const uint32_t ra = (uint32_t)__shfl((int)wa, row), rb = (uint32_t)__shfl((int)wb, row); // (every lane: read from another)
                const bool pass = col_ok && col >= ra && col < rb && dist <= thr_s[row];
                const unsigned long long mask = __ballot(pass);
                if (mask)
                    row_append<CAP>(buf, cnt, row, pass, mask, dist, id_cur, m, kk);
            }
            rows_compact<CAP>(buf, cnt, thr_s, k, lane);
#pragma unroll
            for (int r = 0; r < 16; r++)
                gate[r] = f16_gate(qn_r[r], thr_s[mfma32_row(r, kk)]);
        }
    };

    uint32_t t = next_tile(0);
    if (t < ntiles) {
        uint32_t tn = next_tile(t + 1), ta;
        f16x8 b0[NPRE], b1[NPRE];
        float n0, n1 = 0.f;
        uint32_t id0 = ids(t), id1 = 0, id_ahead = 0;
        pieces(id0, col0(t) + m < c_end, 0, b0);
        n0 = col0(t) + m < c_end ? xn[id0] : 0.f;
        if (tn < ntiles)
            id1 = ids(tn);
        for (;;) {
            ta = next_tile(tn + 1);
            tile(t, b0, n0, id0, tn, b1, n1, id1, ta, id_ahead);
            if (tn >= ntiles)
                break;
            t = tn, tn = ta, id0 = id_ahead;
            ta = next_tile(tn + 1);
            tile(t, b1, n1, id1, tn, b0, n0, id0, ta, id_ahead);
            if (tn >= ntiles)
                break;
            t = tn, tn = ta, id1 = id_ahead;
        }
    }

    // out: [split][plan row][k] keys, every row of the strip (a padding row holds nothing)
    rows_write_out<CAP>(buf, cnt, k, lane, 32, out_keys, (size_t)blockIdx.y * nrows + r0);
}

// part_rows: the rows of a split of `part` where the table holds more than this plan's; 0 = bound * 32
template <int ND, int CAP, int WAVES>
hipError_t launch_exact_f16_windows_t(hipStream_t s, const _Float16 *Qh, const float *qn, const _Float16 *X, const float *xn,
                                      size_t bound, int k, int nsplit, unsigned long long *part, const StripPlan &sp, const StripWin *win,
                                      size_t part_rows = 0)
{
    const size_t shm = (size_t)WAVES * 32 * CAP * sizeof(unsigned long long) + (size_t)WAVES * 32 * (sizeof(uint32_t) + sizeof(float));
    constexpr auto kern = exact_f16_windows_kernel<ND, CAP, WAVES>;
    if (hipError_t e = dyn_lds<kern>(shm); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)((bound + WAVES - 1) / WAVES), (unsigned)nsplit), dim3(64 * WAVES), shm, s, Qh, qn, X, xn,
                       (int)(part_rows ? part_rows : bound * 32), k, part, sp, win);
    return hipGetLastError();
}

// ---- the gated strips (ivfhnsw_gpu_exact_search_f16_tags_values) -----------------------------------------
// A tagged query with an interval of base values sweeps its tag's row list, as exact_f16_rows_kernel does, and counts only the
// columns whose VALUE lies in its interval.  The sweep is that kernel's -- a strip a wave, no barrier, no LDS tile, operand A
// resident, operand B straight from the store through the list in MFMA order, the NPRE / NLATE piece split -- with four
// things of its own.
//   Intervals in lanes, envelope in scalars.  Lanes m and m + 32 hold strip row m's interval as value_math.h's (lo, span,
//   live).  Once per strip two wave reductions give the envelope [LO, HI] over the rows that are queries and have lo <= hi;
//   a padding row and a row with lo > hi hold the threshold -inf and so the gate +inf, for good.  The tag plan orders a
//   tag's queries by lo (launch_tag_strip_plan's minor keys), so that the envelope of a strip is tight.
//   A value stage.  Whether a tile is LIVE -- some column's value lies in the envelope -- depends on loaded data: 4 bytes of
//   row number and 4 bytes of value per column.  The pipeline is three deep: behind the MFMAs of tile t are in flight the
//   row numbers of tile t + 3, the values of tile t + 2 (through the row numbers requested a tile ago) and, decided by one
//   ballot over the values requested a tile ago, the norms and the first NPRE pieces of tile t + 1 -- only if it is live.
//   A dead tile costs its row numbers and values: no norm, no piece, no MFMA.  There is nothing to jump over, as the
//   windows kernel does: the sweep steps tile by tile over 8 bytes per column.  In a live tile a column outside the
//   envelope is not read either: its pieces are zeros and it never passes, so under shuffled values the sweep moves the
//   rows of the envelope only.  The registers in flight alternate between two sets with the loop unrolled by two, so that
//   none is copied before it has arrived.
//   The two tests.  The cheap test is the rows kernel's over the columns inside the envelope.  The exact test, behind the
//   wave-uniform ballot, judges every (row, column) by tag_value_math.h's rule with the row's interval read from its lane.
//   The list ascends in row number, so `<` alone keeps ties on the lower label.
// vals null: the holder has no values, every row reads as 0xffffffff (value_math.h's keep).  A split of a list without a
// live tile still writes its (empty) rows: the merge reads every split that has columns.
template <int CAP>
__device__ __forceinline__ void f16_select_gated(const f32x16 &acc, float xn_col, bool col_in, uint32_t label, uint32_t wv, uint32_t wt,
                                                 uint32_t keep, uint32_t lo, uint32_t span, uint32_t live, const float (&qn_r)[16],
                                                 float (&gate)[16], unsigned long long *buf, uint32_t *cnt, float *thr_s, int k, int lane)
{
    const int m = lane & 31, kk = lane >> 5;
    bool any = false;
#pragma unroll
    for (int r = 0; r < 16; r++)
        any |= __fsub_rn(__fmul_rn(2.0f, acc[r]), xn_col) > gate[r];
    if (__ballot(any && col_in)) { // wave-uniform: rare once the thresholds have settled
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float dist = __fsub_rn(__fadd_rn(qn_r[r], xn_col), __fmul_rn(2.0f, acc[r]));
            const int row = mfma32_row(r, kk);
            // (every lane: read from another.)  The column carries the list's tag wt, which is the tag of every query of the strip.
            const uint32_t rlo = (uint32_t)__shfl((int)lo, row), rspan = (uint32_t)__shfl((int)span, row), rlive = (uint32_t)__shfl((int)live, row);
            const bool pass = col_in && tag_value_pass(wt, wv, wt, keep, rlo, rspan, rlive) && dist < thr_s[row];
            const unsigned long long mask = __ballot(pass);
            if (mask)
                row_append<CAP>(buf, cnt, row, pass, mask, dist, label, m, kk);
        }
        rows_compact<CAP>(buf, cnt, thr_s, k, lane);
#pragma unroll
        for (int r = 0; r < 16; r++)
            gate[r] = f16_gate(qn_r[r], thr_s[mfma32_row(r, kk)]);
    }
}

// Qh, qn, out_keys: at the tag plan's first row; nrows: the rows of a split of the partial table.  qtags, qranges: the
// chunk's tags and intervals in the caller's order, read through the plan's strip_rows.
template <int ND, int CAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void exact_f16_gated_kernel(const _Float16 *__restrict__ Qh, const float *__restrict__ qn,
                                                                     const _Float16 *__restrict__ X, const float *__restrict__ xn,
                                                                     int nrows, int k, unsigned long long *__restrict__ out_keys,
                                                                     StripPlan sp, const uint16_t *__restrict__ qtags,
                                                                     const uint32_t *__restrict__ qranges, const uint32_t *__restrict__ vals)
{
    constexpr int D = 16 * ND;
    constexpr int NPRE = ND <= 8 ? ND : (ND + 1) / 2, NLATE = ND - NPRE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *s_buf = reinterpret_cast<unsigned long long *>(smem); // [WAVES][32][CAP]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_buf + WAVES * 32 * CAP);  // [WAVES][32]
    float *s_thr = reinterpret_cast<float *>(s_cnt + WAVES * 32);             // [WAVES][32]

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    const uint32_t strip = sp.hdr->lay.range[kSweepColsIndirect][0] + blockIdx.x * WAVES + wave;
    if (strip >= sp.hdr->lay.range[kSweepColsIndirect][1])
        return;
    const StripCols e = sp.strip_cols[strip];
    size_t c_begin, c_end;
    sweep_split_cut(e.nx, (int)gridDim.y, (int)blockIdx.y, &c_begin, &c_end);
    if (c_begin >= c_end)
        return;
    const uint32_t *__restrict__ rows = e.data;
    const int r0 = (int)(strip << 5); // (strip < the plan's bound: every row of it exists in Qh, qn and strip_rows)
    unsigned long long *buf = s_buf + (size_t)wave * 32 * CAP;
    uint32_t *cnt = s_cnt + wave * 32;
    float *thr_s = s_thr + wave * 32;

    f16x8 a[ND];
    {
        const _Float16 *qr = Qh + (size_t)(r0 + m) * D + 8 * kk;
#pragma unroll
        for (int s = 0; s < ND; s++)
            a[s] = *reinterpret_cast<const f16x8 *>(qr + 16 * s);
    }
    // the interval of row m; valid: the row is a query and its interval is not empty.  The envelope of the valid rows.
    const int q_m = sp.strip_rows[r0 + m];
    const ValueFill f = value_fill(q_m >= 0 ? qranges[2 * (size_t)q_m] : 1u, q_m >= 0 ? qranges[2 * (size_t)q_m + 1] : 0u, vals != nullptr);
    const bool valid = q_m >= 0 && f.live;
    uint32_t elo = valid ? f.lo : ~0u, ehi = valid ? f.lo + f.span : 0u;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { // (lanes m and m + 32 hold the same interval: each half finds the envelope)
        elo = min(elo, (uint32_t)__shfl_xor((int)elo, o));
        ehi = max(ehi, (uint32_t)__shfl_xor((int)ehi, o));
    }
    const uint32_t LO = __builtin_amdgcn_readfirstlane(elo), HI = __builtin_amdgcn_readfirstlane(ehi);
    const uint32_t wt = qtags[sp.strip_rows[r0]]; // the list's tag (row 0 of a strip is a query)
    if (lane < 32) {
        cnt[lane] = 0;
        thr_s[lane] = valid ? FLT_MAX : -INFINITY;
    }
    __builtin_amdgcn_wave_barrier();
    float qn_r[16], gate[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = mfma32_row(r, kk);
        qn_r[r] = qn[r0 + row];
        gate[r] = f16_gate(qn_r[r], thr_s[row]);
    }

    if (LO <= HI) { // (else no row of the strip can find anything)
        const unsigned char *xb = reinterpret_cast<const unsigned char *>(X) + 16 * kk;
        const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t *__restrict__ vp = vals ? vals : rows; // (without values: element 0 of a readable array, ignored)
        // the row number of the lane's column of the tile that begins at c0; the value word of that row; is it in the envelope
        auto ids = [&](size_t c0) -> uint32_t { return c0 + m < c_end ? rows[c0 + m] : 0u; };
        auto val = [&](size_t c0, uint32_t id) -> uint32_t { return c0 + m < c_end ? vp[value_index(id, f.keep)] : 0u; };
        auto in_env = [&](size_t c0, uint32_t w) -> bool {
            const uint32_t v = w | ~f.keep;
            return c0 + m < c_end && LO <= v && v <= HI;
        };
        // pieces [first, first + N) of store row `row` into w; ok: the lane has a column that is read
        auto pieces = [&](uint32_t row, bool ok, int first, auto &w) {
            constexpr int N = (int)(sizeof(w) / sizeof(w[0]));
            const unsigned char *p = xb + (size_t)row * (2 * D) + 32 * first;
#pragma unroll
            for (int s = 0; s < N; s++)
                w[s] = zero;
            if (ok) {
#pragma unroll
                for (int s = 0; s < N; s++)
                    w[s] = *reinterpret_cast<const f16x8 *>(p + 32 * s);
            }
        };
        // The tile at c0: id_c its row numbers, w_c its values, live_c whether it is live, and if so `cur`, n_cur its first NPRE
        // pieces and its norms; id_n the row numbers of tile c0 + 32.  w_in: the values of tile c0 + 32, id_in: the row numbers
        // of tile c0 + 64, both requested a tile ago.  Starts the loads of tile c0 + 32 into nxt, n_nxt if that tile is live, of
        // the values of tile c0 + 64 into w_out and of the row numbers of tile c0 + 96 into id_out.
        uint32_t id_c = ids(c_begin), id_n = 0, w_c;
        bool live_c; // wave-uniform
        auto tile = [&](size_t c0, const f16x8 (&cur)[NPRE], float n_cur, f16x8 (&nxt)[NPRE], float &n_nxt, uint32_t w_in, uint32_t id_in,
                        uint32_t &w_out, uint32_t &id_out) {
            const bool in_c = in_env(c0, w_c);
            f16x8 late[NLATE > 0 ? NLATE : 1];
            if constexpr (NLATE > 0) {
                if (live_c)
                    pieces(id_c, in_c, NPRE, late);
            }
            bool live_n = false;
            if (c0 + 32 < c_end) { // in flight behind this tile's MFMAs
                const bool in_n = in_env(c0 + 32, w_in);
                live_n = __ballot(in_n) != 0;
                if (live_n) {
                    pieces(id_n, in_n, 0, nxt);
                    n_nxt = in_n ? xn[id_n] : 0.f;
                }
            }
            if (c0 + 64 < c_end)
                w_out = val(c0 + 64, id_in);
            if (c0 + 96 < c_end)
                id_out = ids(c0 + 96);
            if (live_c) {
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < NPRE; s++)
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], cur[s], acc, 0, 0, 0);
                if constexpr (NLATE > 0) {
#pragma unroll
                    for (int s = 0; s < NLATE; s++)
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[NPRE + s], late[s], acc, 0, 0, 0);
                }
                f16_select_gated<CAP>(acc, n_cur, in_c, id_c, w_c, wt, f.keep, f.lo, f.span, f.live, qn_r, gate, buf, cnt, thr_s, k, lane);
            }
            id_c = id_n, w_c = w_in, live_c = live_n, id_n = id_in; // (all arrived: none was requested in this tile)
        };

        f16x8 b0[NPRE], b1[NPRE];
        float n0 = 0.f, n1 = 0.f;
        uint32_t id_a = 0, id_b = 0, w_a = 0, w_b = 0;
        if (c_begin + 32 < c_end)
            id_n = ids(c_begin + 32);
        if (c_begin + 64 < c_end)
            id_b = ids(c_begin + 64);
        w_c = val(c_begin, id_c);
        if (c_begin + 32 < c_end)
            w_b = val(c_begin + 32, id_n);
        {
            const bool in0 = in_env(c_begin, w_c);
            live_c = __ballot(in0) != 0;
            if (live_c) {
                pieces(id_c, in0, 0, b0);
                n0 = in0 ? xn[id_c] : 0.f;
            }
        }
        for (size_t c0 = c_begin;;) {
            tile(c0, b0, n0, b1, n1, w_b, id_b, w_a, id_a);
            if ((c0 += 32) >= c_end)
                break;
            tile(c0, b1, n1, b0, n0, w_a, id_a, w_b, id_b);
            if ((c0 += 32) >= c_end)
                break;
        }
    }

    // out: [split][row of the table][k] keys, every row of the strip (a padding row holds nothing)
    rows_write_out<CAP>(buf, cnt, k, lane, 32, out_keys, (size_t)blockIdx.y * nrows + r0);
}

template <int ND, int CAP, int WAVES>
hipError_t launch_exact_f16_gated_t(hipStream_t s, const _Float16 *Qh, const float *qn, const _Float16 *X, const float *xn, size_t bound,
                                    size_t part_rows, int k, int nsplit, unsigned long long *part, const StripPlan &sp, const uint16_t *qtags,
                                    const uint32_t *qranges, const uint32_t *vals)
{
    const size_t shm = (size_t)WAVES * 32 * CAP * sizeof(unsigned long long) + (size_t)WAVES * 32 * (sizeof(uint32_t) + sizeof(float));
    constexpr auto kern = exact_f16_gated_kernel<ND, CAP, WAVES>;
    if (hipError_t e = dyn_lds<kern>(shm); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)((bound + WAVES - 1) / WAVES), (unsigned)nsplit), dim3(64 * WAVES), shm, s, Qh, qn, X, xn,
                       (int)part_rows, k, part, sp, qtags, qranges, vals);
    return hipGetLastError();
}

// the minor keys of the tag plan and the intervals of the value plan of a chunk of a _tags_values call: a tagged query is
// ordered inside its tag by its lo and gets the empty interval (1, 0) -- no strip of the value plan; an untagged one keeps
// its interval there
__global__ __launch_bounds__(256) void f16_tags_values_split_kernel(const uint16_t *__restrict__ qtags, const uint32_t *__restrict__ qr, size_t m,
                                                                    uint32_t *__restrict__ lo_keys, uint32_t *__restrict__ vranges)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m)
        return;
    const bool untagged = qtags[q] == kRowTagNone;
    lo_keys[q] = untagged ? 0u : qr[2 * q];
    vranges[2 * q] = untagged ? qr[2 * q] : 1u;
    vranges[2 * q + 1] = untagged ? qr[2 * q + 1] : 0u;
}

// The merge of a _tags_values chunk, one wavefront per row of the partial table [split][rows_v + rows_t][k]: rows [0, rows_v)
// are the value plan's (spv: the untagged queries, Dense under ns_dense, windowed under ns_win), the rest the tag plan's
// (spt), of which only the Indirect strips count (under ns_tag) -- its Dense strips hold the untagged queries, which the
// value plan answers.  sides: bit 0 the value plan was swept, bit 1 the tag plan.
__global__ __launch_bounds__(64) void exact_f16_merge_two_kernel(const unsigned long long *__restrict__ part, int ns_dense, int ns_win,
                                                                 int ns_tag, int rows_v, int nrows, int k, float *__restrict__ dists,
                                                                 long long *__restrict__ labels, StripPlan spv, StripPlan spt, unsigned sides)
{
    const bool tagside = (int)blockIdx.x >= rows_v;
    if (!(sides >> (tagside ? 1 : 0) & 1u))
        return;
    const StripPlan &sp = tagside ? spt : spv;
    const uint32_t row = tagside ? blockIdx.x - rows_v : blockIdx.x, strip = row >> 5;
    if (strip >= sp.hdr->lay.nstrips)
        return;
    const bool indirect = strip >= sp.hdr->lay.range[kSweepColsIndirect][0];
    if (tagside && !indirect)
        return;
    const int q = sp.strip_rows[row];
    if (q < 0)
        return;
    int ns = ns_dense;
    if (indirect) {
        const int nsi = tagside ? ns_tag : ns_win;
        const size_t nx = sp.strip_cols[strip].nx, cps = sweep_cols_per_split(nx, nsi);
        ns = (int)min((size_t)nsi, (nx + cps - 1) / cps);
    }
    sweep_merge_row(
        part, ns, nrows, k, (int)blockIdx.x, q,
        [&](size_t o, unsigned long long key) {
            labels[o] = (long long)(uint32_t)key;
            dists[o] = orderable_f32((uint32_t)(key >> 32));
        },
        [&](size_t o) { // fewer than k rows pass for the query
            labels[o] = -1ll;
            dists[o] = FLT_MAX;
        });
}

// f(int_c<ND>()) for ND = d / 16 = 1 .. 16; any other d is refused
template <class F> hipError_t by_f16_steps(int d, F &&f)
{
    switch (d / 16) {
#define IVFHNSW_F16_STEP(N) case N: return f(int_c<N>());
        IVFHNSW_F16_STEP(1) IVFHNSW_F16_STEP(2) IVFHNSW_F16_STEP(3) IVFHNSW_F16_STEP(4) IVFHNSW_F16_STEP(5) IVFHNSW_F16_STEP(6)
        IVFHNSW_F16_STEP(7) IVFHNSW_F16_STEP(8) IVFHNSW_F16_STEP(9) IVFHNSW_F16_STEP(10) IVFHNSW_F16_STEP(11) IVFHNSW_F16_STEP(12)
        IVFHNSW_F16_STEP(13) IVFHNSW_F16_STEP(14) IVFHNSW_F16_STEP(15) IVFHNSW_F16_STEP(16)
#undef IVFHNSW_F16_STEP
    default: return hipErrorInvalidValue;
    }
}

// ---- the range search (ivfhnsw_gpu_exact_range_search_f16) -------------------------------------------------
// The strip and the staging of exact_f16_kernel -- 4 waves of 32 query rows, operand A resident, operand B copied once per
// workgroup into two padded LDS tiles, the next tile's global loads in flight behind this tile's MFMAs, one barrier per
// tile -- with the fixed gate and the two forms of exact_range_kernel (kernels_exact.hip): nothing is selected, so the two
// tiles are all the LDS there is, and a lane keeps the counters or cursors of its 16 accumulator rows in registers.
//   dist = fl(fl(qn + xn) - 2 acc), the k-search's; a row passes iff dist < radius; the cheap test is f16_gate(qn, radius).
//   count (FILL = false): slices[(q_off + row) * nsplit + split] = the columns of the split that pass, *total += their sum.
//   fill (FILL = true): the cursor of a row starts at its slice's prefix; a passing lane writes (dist, col) at the cursor +
//       the passing lanes of its half below it.  Tiles come in increasing order: ascending label within and across splits.
// The tile map.  The count form records, as exact_range_kernel does and in its layout, per WAVE one bit per 2^map_shift
// tiles: did any of the wave's rows pass in them.  The int8 fill form lets each wave skip by its own bits, because each
// wave loads its own B.  Here B is staged by the workgroup behind a barrier, so a tile is skipped by all four waves or by
// none: the fill form visits a tile iff the OR of the bit over the workgroup's waves is set.  Every thread forms that OR
// itself from the (at most four) waves' words, which are the same addresses for the whole workgroup, so the decision is
// uniform without any exchange, and it is made before the tile is fetched: a skipped tile is neither loaded, staged nor
// multiplied and costs no barrier.  The prefetch asks for the next VISITED tile (next_tile), one step ahead.
// A wave whose 32 rows all lie beyond nq stages and meets every barrier, multiplies nothing, writes no map word, slice or
// total -- and its map words, which need not even exist (the map has ceil(nq / 32) strips), are never read: the OR runs
// over the waves with a row below nq only.
// SP: F16Rows is the plain call.  F16RangeDenseStrips (base tags): Qh, qn are the nq = 32 * bound rows of a
// strip plan and workgroup i owns the strips [4 i, 4 i + 4) of the plan's Dense range, as in exact_f16_kernel: a workgroup
// beyond the range leaves before the first barrier, a wave beyond it in a workgroup that stays is not `active`, and the OR
// of the map runs over the waves that own a strip.  Slices and cursors are the QUERY's (strip_rows), in a table slice_w
// splits wide; the map words the plan strip's, map_stride words a strip.
struct F16RangeDenseStrips {
    static constexpr bool kStrips = true;
    StripPlan sp;
    int slice_w;
    uint32_t map_stride;
};

template <int ND, bool FILL, class SP>
__global__ __launch_bounds__(256) void exact_range_f16_kernel(const _Float16 *__restrict__ Qh, const float *__restrict__ qn,
                                                              const _Float16 *__restrict__ X, const float *__restrict__ xn, int nq,
                                                              size_t nx, float radius, size_t q_off,
                                                              uint32_t *__restrict__ slices, unsigned long long *__restrict__ total,
                                                              uint32_t *__restrict__ map, int map_shift, int map_words,
                                                              float *__restrict__ out_d, long long *__restrict__ out_l, size_t out_cap,
                                                              SP sp)
{
    constexpr int D = 16 * ND, T = 256;
    constexpr int ROWB = 2 * D + 16; // bytes of a tile's row in LDS: the row and its padding
    constexpr int TILEB = 32 * ROWB;
    constexpr int PPR = D / 8;               // 16-byte pieces of a row,
    constexpr int NPIECE = 32 * PPR;         // ... of a tile,
    constexpr int NP = (NPIECE + T - 1) / T; // ... of a thread
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[2 * TILEB];

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    // the workgroup's first strip and the strips it owns: of the call's rows, or of the plan's Dense range
    uint32_t s0 = blockIdx.x * 4, s1 = (uint32_t)((nq + 31) >> 5);
    if constexpr (SP::kStrips) {
        s0 += sp.sp.hdr->lay.range[kSweepColsDense][0];
        s1 = sp.sp.hdr->lay.range[kSweepColsDense][1];
        if (s0 >= s1)
            return;
    }
    const int wg_r0 = (int)(s0 << 5), r0 = SP::kStrips ? wg_r0 + (s0 + wave < s1 ? wave : 0) * 32 : wg_r0 + wave * 32;
    const bool active = SP::kStrips ? s0 + wave < s1 : r0 < nq; // wave-uniform; the workgroup's first wave always is
    const int nsplit = gridDim.y, split = blockIdx.y;
    // the slice of row `row` of the plan or of the call (under a plan: of the query the row holds, padding rows of query 0)
    auto slice_of = [&](int row) -> size_t {
        if constexpr (SP::kStrips)
            return (q_off + (size_t)max(sp.sp.strip_rows[row], 0)) * sp.slice_w + split;
        else
            return (q_off + row) * nsplit + split;
    };
    // (the same for every wave of the workgroup: all of them meet at every barrier below)
    size_t c_begin, c_end;
    sweep_split_cut(nx, nsplit, split, &c_begin, &c_end);
    const uint32_t ntiles = (uint32_t)((c_end - c_begin + 31) >> 5);

    f16x8 a[ND];
    {
        const _Float16 *qr = Qh + (size_t)min(r0 + m, nq - 1) * D + 8 * kk;
#pragma unroll
        for (int s = 0; s < ND; s++)
            a[s] = *reinterpret_cast<const f16x8 *>(qr + 16 * s);
    }
    float qn_r[16], gate[16];
    uint32_t cnt[16], in_rows = 0; // bit r: accumulator row r is a query
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = r0 + mfma32_row(r, kk);
        bool in = row < nq;
        if constexpr (SP::kStrips)
            in = active && sp.sp.strip_rows[row] >= 0;
        in_rows |= in ? 1u << r : 0u;
        qn_r[r] = qn[min(row, nq - 1)];
        gate[r] = f16_gate(qn_r[r], in ? radius : -INFINITY);
        cnt[r] = FILL && in ? slices[slice_of(row)] : 0u;
    }

    // The map words: this wave's own (count), and the OR over the workgroup's waves with a row below nq (fill).
    const size_t wg_strip = SP::kStrips ? (size_t)(wg_r0 >> 5) : (q_off + wg_r0) >> 5;
    const int wg_waves = SP::kStrips ? (int)min(s1 - s0, 4u) : nq - wg_r0 >= 128 ? 4 : (nq - wg_r0 + 31) >> 5;
    // the words of wave v of the workgroup in this split
    auto words_of = [&](int v) -> uint32_t * {
        if constexpr (SP::kStrips)
            return map + (sp.sp.map_strip0 + wg_strip + v) * (size_t)sp.map_stride + (size_t)split * map_words;
        else
            return map + ((wg_strip + v) * nsplit + split) * (size_t)map_words;
    };
    uint32_t *mw = map ? words_of(wave) : nullptr;
    uint32_t or_at = ~0u, or_word = 0; // the last word formed: a word covers 32 << map_shift tiles
    auto wg_word = [&](uint32_t w) -> uint32_t {
        if (w != or_at) {
            or_at = w;
            or_word = 0;
            for (int v = 0; v < wg_waves; v++)
                or_word |= words_of(v)[w];
        }
        return or_word;
    };
    // the first tile at or after t that is visited (ntiles or beyond: none); workgroup-uniform
    auto next_tile = [&](uint32_t t) -> uint32_t {
        if (!FILL || !map)
            return t;
        while (t < ntiles) {
            const uint32_t g = t >> map_shift;
            const uint32_t w = wg_word(g >> 5) >> (g & 31);
            if (w & 1u)
                return t;
            t = (w ? g + (uint32_t)__ffs((int)w) - 1u : (g | 31u) + 1u) << map_shift; // the next set bit, or the next word
        }
        return ntiles;
    };

    // staging, as in exact_f16_kernel: thread tid takes the pieces tid, tid + T, ... of a tile; a row at or beyond c_end is
    // not read, its pieces are zeros
    uint4 pre[NP];
    float pre_n = 0.f;
    auto fetch = [&](size_t c0) {
        const unsigned char *src = reinterpret_cast<const unsigned char *>(X) + c0 * (size_t)(2 * D);
        const int rows_in = c_end - c0 < 32 ? (int)(c_end - c0) : 32;
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int p = tid + i * T;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if ((NPIECE % T == 0 || p < NPIECE) && p / PPR < rows_in)
                v = *reinterpret_cast<const uint4 *>(src + 16 * (size_t)p);
            pre[i] = v;
        }
        pre_n = c0 + m < c_end ? xn[c0 + m] : 0.f;
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int p = tid + i * T;
            if (NPIECE % T == 0 || p < NPIECE)
                *reinterpret_cast<uint4 *>(s_tile + b * TILEB + (p / PPR) * ROWB + 16 * (p % PPR)) = pre[i];
        }
    };

    uint32_t t = next_tile(0), bits = 0;
    float xn_cur = 0.f;
    if (t < ntiles) {
        fetch(c_begin + ((size_t)t << 5));
        stash(0);
        xn_cur = pre_n;
    }
    __syncthreads();
    for (int b = 0; t < ntiles; b ^= 1) {
        const uint32_t tn = next_tile(t + 1);
        if (tn < ntiles)
            fetch(c_begin + ((size_t)tn << 5)); // in flight behind this tile's MFMAs
        bool hit = false;
        if (active) {
            const unsigned char *bt = s_tile + b * TILEB + m * ROWB + 16 * kk;
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < ND; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], *reinterpret_cast<const f16x8 *>(bt + 32 * s), acc, 0, 0, 0);
            const size_t col = c_begin + ((size_t)t << 5) + m;
            const bool col_ok = col < c_end;
            bool any = false;
#pragma unroll
            for (int r = 0; r < 16; r++)
                any |= __fsub_rn(__fmul_rn(2.0f, acc[r]), xn_cur) > gate[r];
            if (__ballot(any && col_ok)) { // wave-uniform
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float dist = __fsub_rn(__fadd_rn(qn_r[r], xn_cur), __fmul_rn(2.0f, acc[r]));
                    const bool pass = col_ok && (in_rows >> r & 1u) && dist < radius;
                    const unsigned long long mask = __ballot(pass);
                    const uint32_t half = kk ? (uint32_t)(mask >> 32) : (uint32_t)mask;
                    hit |= mask != 0;
                    if (FILL) {
                        const size_t o = (size_t)cnt[r] + __popc(half & ((1u << m) - 1u));
                        if (pass && o < out_cap) { // (o < out_cap always: the count form counted this very lane)
                            out_d[o] = dist;
                            out_l[o] = (long long)col;
                        }
                    }
                    cnt[r] += __popc(half);
                }
            }
        }
        if (!FILL && mw && active) {
            const uint32_t g = t >> map_shift;
            bits |= hit ? 1u << (g & 31) : 0u;
            if (tn >= ntiles || (tn >> map_shift) >> 5 != g >> 5) { // the word is complete
                if (lane == 0)
                    mw[g >> 5] = bits;
                bits = 0;
            }
        }
        if (tn < ntiles)
            stash(b ^ 1); // the tile every wave left at the last barrier
        xn_cur = pre_n;
        __syncthreads();
        t = tn;
    }
    if (!FILL && active) {
        unsigned long long sum = 0;
        if (m == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (in_rows >> r & 1u) {
                    // (the plain call's index in its own words: through slice_of it costs the count form 10 to 25 VGPRs
                    // in this unit's build, which the Makefile compiles without packed float32 operations)
                    if constexpr (SP::kStrips)
                        slices[slice_of(r0 + mfma32_row(r, kk))] = cnt[r];
                    else
                        slices[(q_off + r0 + mfma32_row(r, kk)) * nsplit + split] = cnt[r];
                }
                sum += cnt[r];
            }
        }
        sum += __shfl_xor(sum, 32);
        if (lane == 0 && sum)
            atomicAdd(total, sum);
    }
}

// ---- the tagged strips of the range search (ivfhnsw_gpu_exact_range_search_f16_tags) -------------------------
// exact_f16_rows_kernel's sweep of a row list -- a strip is a wave, operand A resident, operand B straight from the store in
// MFMA order, row numbers two tiles ahead, norms and the first NPRE pieces one tile ahead, the late pieces behind the first
// MFMAs of their own tile -- with the fixed gate and the two forms of exact_range_f16_kernel, whose arithmetic it repeats
// operation for operation.  Nothing is selected: no candidate buffers, no LDS, no barrier; occupancy is the registers'.
// Slices and cursors are the QUERY's (strip_rows) in a table slice_w splits wide, so lims and results come out in the
// caller's order; the label is the row number, the list ascends, so results ascend within and across splits.
// The tile map, per WAVE: each wave loads its own B, so the fill form skips by the strip's OWN bits (as the int8 fill form
// does), words map + (map_strip0 + strip) * map_stride + split * map_words.  The pipeline aims at VISITED tiles: t is the
// tile being multiplied, tn the next visited one (its pieces and norms are requested now), ta the one after (its row
// numbers are).  next_tile decides before anything of a tile is requested; a skipped tile is neither loaded nor
// multiplied.  In the count form, and without a map, next_tile(t) == t: the loop is exact_f16_rows_kernel's.
// A wave without a strip, or whose split of a short list is empty, leaves at once in both forms: no slice (the memset left
// it zero), no map word (the fill form's wave leaves too), no total.
template <int ND, bool FILL>
__global__ __launch_bounds__(256) void exact_range_f16_rows_kernel(const _Float16 *__restrict__ Qh, const float *__restrict__ qn,
                                                                   const _Float16 *__restrict__ X, const float *__restrict__ xn,
                                                                   float radius, size_t q_off, int slice_w,
                                                                   uint32_t *__restrict__ slices, unsigned long long *__restrict__ total,
                                                                   uint32_t *__restrict__ map, int map_shift, int map_words,
                                                                   uint32_t map_stride, float *__restrict__ out_d,
                                                                   long long *__restrict__ out_l, size_t out_cap, StripPlan sp)
{
    constexpr int D = 16 * ND;
    constexpr int NPRE = ND <= 8 ? ND : (ND + 1) / 2, NLATE = ND - NPRE;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    const uint32_t strip = sp.hdr->lay.range[kSweepColsIndirect][0] + blockIdx.x * 4 + wave;
    if (strip >= sp.hdr->lay.range[kSweepColsIndirect][1])
        return;
    const StripCols e = sp.strip_cols[strip];
    const int split = blockIdx.y;
    size_t c_begin, c_end;
    sweep_split_cut(e.nx, (int)gridDim.y, split, &c_begin, &c_end);
    if (c_begin >= c_end)
        return;
    const uint32_t ntiles = (uint32_t)((c_end - c_begin + 31) >> 5);
    const uint32_t *__restrict__ rows = e.data;
    const int r0 = (int)(strip << 5); // (strip < the plan's bound: every row of it exists in Qh, qn and strip_rows)

    f16x8 a[ND];
    {
        const _Float16 *qr = Qh + (size_t)(r0 + m) * D + 8 * kk;
#pragma unroll
        for (int s = 0; s < ND; s++)
            a[s] = *reinterpret_cast<const f16x8 *>(qr + 16 * s);
    }
    // the slice of strip row `row`: its query's (a padding row: query 0's, never touched)
    auto slice_of = [&](int row) -> size_t { return (q_off + (size_t)max(sp.strip_rows[r0 + row], 0)) * slice_w + split; };
    float qn_r[16], gate[16];
    uint32_t cnt[16], in_rows = 0; // bit r: accumulator row r is a query
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = mfma32_row(r, kk);
        const bool in = sp.strip_rows[r0 + row] >= 0;
        in_rows |= in ? 1u << r : 0u;
        qn_r[r] = qn[r0 + row];
        gate[r] = f16_gate(qn_r[r], in ? radius : -INFINITY);
        cnt[r] = FILL && in ? slices[slice_of(row)] : 0u;
    }

    uint32_t *mw = map ? map + (size_t)(sp.map_strip0 + strip) * map_stride + (size_t)split * map_words : nullptr;
    // the first tile at or after t that is visited (ntiles or beyond: none); wave-uniform
    auto next_tile = [&](uint32_t t) -> uint32_t {
        if (!FILL || !mw)
            return t;
        while (t < ntiles) {
            const uint32_t g = t >> map_shift;
            const uint32_t w = __builtin_amdgcn_readfirstlane(mw[g >> 5]) >> (g & 31);
            if (w & 1u)
                return t;
            t = (w ? g + (uint32_t)__ffs((int)w) - 1u : (g | 31u) + 1u) << map_shift; // the next set bit, or the next word
        }
        return ntiles;
    };

    const unsigned char *xb = reinterpret_cast<const unsigned char *>(X) + 16 * kk;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    // the lane's column of tile t, whether it has one, and its row number
    auto col_of = [&](uint32_t t) -> size_t { return c_begin + ((size_t)t << 5) + m; };
    auto ids = [&](uint32_t t) -> uint32_t { return col_of(t) < c_end ? rows[col_of(t)] : 0u; };
    // pieces [first, first + N) of store row `row` into w; ok: the lane has a column
    auto pieces = [&](uint32_t row, bool ok, int first, auto &w) {
        constexpr int N = (int)(sizeof(w) / sizeof(w[0]));
        const unsigned char *p = xb + (size_t)row * (2 * D) + 32 * first;
#pragma unroll
        for (int s = 0; s < N; s++)
            w[s] = zero;
        if (ok) {
#pragma unroll
            for (int s = 0; s < N; s++)
                w[s] = *reinterpret_cast<const f16x8 *>(p + 32 * s);
        }
    };
    uint32_t bits = 0;
    // Tile t: `cur`, n_cur = its first NPRE pieces and its norms, id_cur its row numbers.  Starts the loads of tile tn (row
    // numbers id_nxt) into nxt, n_nxt and of the row numbers of tile ta into id_ahead.
    auto tile = [&](uint32_t t, const f16x8 (&cur)[NPRE], float n_cur, uint32_t id_cur, uint32_t tn, f16x8 (&nxt)[NPRE], float &n_nxt,
                    uint32_t id_nxt, uint32_t ta, uint32_t &id_ahead) {
        const bool col_ok = col_of(t) < c_end;
        f16x8 late[NLATE > 0 ? NLATE : 1];
        if constexpr (NLATE > 0)
            pieces(id_cur, col_ok, NPRE, late);
        if (tn < ntiles) { // in flight behind this tile's MFMAs
            const bool ok = col_of(tn) < c_end;
            pieces(id_nxt, ok, 0, nxt);
            n_nxt = ok ? xn[id_nxt] : 0.f;
        }
        if (ta < ntiles)
            id_ahead = ids(ta);
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NPRE; s++)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], cur[s], acc, 0, 0, 0);
        if constexpr (NLATE > 0) {
#pragma unroll
            for (int s = 0; s < NLATE; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[NPRE + s], late[s], acc, 0, 0, 0);
        }
        bool any = false, hit = false;
#pragma unroll
        for (int r = 0; r < 16; r++)
            any |= __fsub_rn(__fmul_rn(2.0f, acc[r]), n_cur) > gate[r];
        if (__ballot(any && col_ok)) { // wave-uniform
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float dist = __fsub_rn(__fadd_rn(qn_r[r], n_cur), __fmul_rn(2.0f, acc[r]));
                const bool pass = col_ok && (in_rows >> r & 1u) && dist < radius;
                const unsigned long long mask = __ballot(pass);
                const uint32_t half = kk ? (uint32_t)(mask >> 32) : (uint32_t)mask;
                hit |= mask != 0;
                if (FILL) {
                    const size_t o = (size_t)cnt[r] + __popc(half & ((1u << m) - 1u));
                    if (pass && o < out_cap) { // (o < out_cap always: the count form counted this very lane)
                        out_d[o] = dist;
                        out_l[o] = (long long)id_cur;
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
    };

    uint32_t t = next_tile(0);
    if (t >= ntiles)
        return; // (fill: no tile of the split has a hit)
    uint32_t tn = next_tile(t + 1), ta;
    f16x8 b0[NPRE], b1[NPRE];
    float n0, n1 = 0.f;
    uint32_t id0 = ids(t), id1 = 0, id_ahead = 0;
    pieces(id0, col_of(t) < c_end, 0, b0);
    n0 = col_of(t) < c_end ? xn[id0] : 0.f;
    if (tn < ntiles)
        id1 = ids(tn);
    for (;;) {
        ta = tn < ntiles ? next_tile(tn + 1) : tn;
        tile(t, b0, n0, id0, tn, b1, n1, id1, ta, id_ahead);
        if (tn >= ntiles)
            break;
        t = tn, tn = ta, id0 = id_ahead;
        ta = tn < ntiles ? next_tile(tn + 1) : tn;
        tile(t, b1, n1, id1, tn, b0, n0, id0, ta, id_ahead);
        if (tn >= ntiles)
            break;
        t = tn, tn = ta, id1 = id_ahead;
    }

    if (!FILL) {
        unsigned long long sum = 0;
        if (m == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (in_rows >> r & 1u)
                    slices[slice_of(mfma32_row(r, kk))] = cnt[r];
                sum += cnt[r];
            }
        }
        sum += __shfl_xor(sum, 32);
        if (lane == 0 && sum)
            atomicAdd(total, sum);
    }
}

// ---- the windowed strips of the range search (ivfhnsw_gpu_exact_range_search_f16_values) --------------------
// A windowed strip of a value plan sweeps a span of the holder's rows in (value, row) order, every strip row counting only the
// columns of ITS OWN window win[32 strip + row] = [wa, wb) of the span, and returns every pair below the radius.  The sweep
// is a strip a wave, four strips a workgroup that share nothing: no barrier, no LDS, operand A resident, operand B straight
// from the store through the span's row numbers in MFMA order with exact_f16_rows_kernel's prefetch depths; the arithmetic,
// the fixed gate and the two forms are exact_range_f16_rows_kernel's, operation for operation, counters and cursors in
// registers.  Two skips meet here, and next_tile composes them before anything of a tile is requested:
//   the windows (exact_f16_windows_kernel's, in lanes m and m + 32): a tile no window meets is dead; next_live steps while
//   tiles are live -- one ballot -- and jumps a gap with one wave minimum.  Both forms skip by them.
//   the tile map: the count form records, in the map's layout, one bit per 2^map_shift tiles of the strip's own span by
//   the strip's OWN hits; the fill form visits a tile iff it is live AND its bit is set.  The count form visits every live
//   tile and writes a word when it leaves it, so the word of a live tile is always written -- and only such words are
//   read: the fill form asks the windows first, looks up the live tile's bit, and from an unset bit goes to the word's
//   next set bit (or the next word) and asks the windows again from there.  A word no live tile lies in is neither
//   written nor read; the groups of a written word that hold no live tile are zero.
// The cheap test counts an accumulator register only where its row's live bit is set (a tile inside every non-empty window
// takes the unwindowed test); the exact test reads the row's window from its lane and rejects the columns of an edge tile
// outside it.  A padding row and a row with an empty window hold the gate +inf for good and are no query (in_rows).
// The fill form writes at the cursors in arrival order -- (value, row), not label order: the host gathers the results by
// label afterwards (launch_range_by_label).  A wave without a strip, whose split of a short span is empty or holds no live
// tile leaves at once in both forms: no slice (the memset left it zero), no map word, no total.
template <int ND, bool FILL>
__global__ __launch_bounds__(256) void exact_range_f16_windows_kernel(const _Float16 *__restrict__ Qh, const float *__restrict__ qn,
                                                                      const _Float16 *__restrict__ X, const float *__restrict__ xn,
                                                                      float radius, size_t q_off, int slice_w,
                                                                      uint32_t *__restrict__ slices, unsigned long long *__restrict__ total,
                                                                      uint32_t *__restrict__ map, int map_shift, int map_words,
                                                                      uint32_t map_stride, float *__restrict__ out_d,
                                                                      long long *__restrict__ out_l, size_t out_cap, StripPlan sp,
                                                                      const StripWin *__restrict__ win)
{
    constexpr int D = 16 * ND;
    constexpr int NPRE = ND <= 8 ? ND : (ND + 1) / 2, NLATE = ND - NPRE;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    const uint32_t strip = sp.hdr->lay.range[kSweepColsIndirect][0] + blockIdx.x * 4 + wave;
    if (strip >= sp.hdr->lay.range[kSweepColsIndirect][1])
        return;
    const StripCols e = sp.strip_cols[strip];
    const int split = blockIdx.y;
    size_t cb, ce;
    sweep_split_cut(e.nx, (int)gridDim.y, split, &cb, &ce);
    if (cb >= ce)
        return;
    const uint32_t c_begin = (uint32_t)cb, c_end = (uint32_t)ce; // (columns of a span: below the rows of the store)
    const uint32_t ntiles = (c_end - c_begin + 31u) >> 5;
    const uint32_t *__restrict__ rows = e.data;
    const int r0 = (int)(strip << 5); // (strip < the plan's bound: every row of it exists in Qh, qn, strip_rows and win)

    // the window of row m, in the span's columns; bit m of `empty`: row m has none
    const StripWin w = win[r0 + m];
    const uint32_t wa = w.a, wb = w.b;
    const uint32_t empty = (uint32_t)__ballot(wa >= wb);
    // the first column of tile t; does the lane's window meet the tile that begins at c0 (an empty window meets none; the
    // launch keeps columns below 2^32 - 64)
    auto col0 = [&](uint32_t t) -> uint32_t { return c_begin + (t << 5); };
    auto meets = [&](uint32_t c0) -> bool { return wa < c0 + 32u && wb > c0; };
    // the first live tile at or after t (ntiles: none); wave-uniform, from the windows alone
    auto next_live = [&](uint32_t t) -> uint32_t {
        if (t >= ntiles)
            return ntiles;
        const uint32_t c0 = col0(t);
        if (__ballot(meets(c0)))
            return t;
        // dead: the tile in which the nearest window that ends beyond c0 begins (it begins beyond the tile, or it would meet it)
        uint32_t tt = wa < wb && wb > c0 ? ((wa > c0 ? wa : c0) - c_begin) >> 5 : ~0u;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) // (lanes m and m + 32 hold the same window: each half finds the minimum)
            tt = min(tt, (uint32_t)__shfl_xor((int)tt, o));
        tt = __builtin_amdgcn_readfirstlane(tt);
        return tt < ntiles ? tt : ntiles;
    };
    uint32_t *mw = map ? map + (size_t)(sp.map_strip0 + strip) * map_stride + (size_t)split * map_words : nullptr;
    // the first tile at or after t that is visited: live, and in the fill form under a map with its bit set (ntiles: none)
    auto next_tile = [&](uint32_t t) -> uint32_t {
        t = next_live(t);
        if (!FILL || !mw)
            return t;
        while (t < ntiles) {
            const uint32_t g = t >> map_shift;
            const uint32_t bw = __builtin_amdgcn_readfirstlane(mw[g >> 5]) >> (g & 31);
            if (bw & 1u)
                return t;
            // the next set bit of the word, or the next word; then the windows again
            t = next_live((bw ? g + (uint32_t)__ffs((int)bw) - 1u : (g | 31u) + 1u) << map_shift);
        }
        return ntiles;
    };
    uint32_t t = next_tile(0);
    if (t >= ntiles)
        return; // no window meets the split, or (fill) no live tile of it has a hit

    f16x8 a[ND];
    {
        const _Float16 *qr = Qh + (size_t)(r0 + m) * D + 8 * kk;
#pragma unroll
        for (int s = 0; s < ND; s++)
            a[s] = *reinterpret_cast<const f16x8 *>(qr + 16 * s);
    }
    // the slice of strip row `row`: its query's (a padding row: query 0's, never touched)
    auto slice_of = [&](int row) -> size_t { return (q_off + (size_t)max(sp.strip_rows[r0 + row], 0)) * slice_w + split; };
    float qn_r[16], gate[16];
    uint32_t cnt[16], in_rows = 0; // bit r: accumulator row r is a query with a window
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = mfma32_row(r, kk);
        const bool in = sp.strip_rows[r0 + row] >= 0 && !(empty >> row & 1u);
        in_rows |= in ? 1u << r : 0u;
        qn_r[r] = qn[r0 + row];
        gate[r] = f16_gate(qn_r[r], in ? radius : -INFINITY);
        cnt[r] = FILL && in ? slices[slice_of(row)] : 0u;
    }

    const unsigned char *xb = reinterpret_cast<const unsigned char *>(X) + 16 * kk;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    // the row number of the lane's column of tile t
    auto ids = [&](uint32_t t) -> uint32_t { return col0(t) + m < c_end ? rows[col0(t) + m] : 0u; };
    // pieces [first, first + N) of store row `row` into w; ok: the lane has a column
    auto pieces = [&](uint32_t row, bool ok, int first, auto &w) {
        constexpr int N = (int)(sizeof(w) / sizeof(w[0]));
        const unsigned char *p = xb + (size_t)row * (2 * D) + 32 * first;
#pragma unroll
        for (int s = 0; s < N; s++)
            w[s] = zero;
        if (ok) {
#pragma unroll
            for (int s = 0; s < N; s++)
                w[s] = *reinterpret_cast<const f16x8 *>(p + 32 * s);
        }
    };
    uint32_t bits = 0;
    // Tile t: `cur`, n_cur = its first NPRE pieces and its norms, id_cur its row numbers.  Starts the loads of tile tn (row
    // numbers id_nxt) into nxt, n_nxt and of the row numbers of tile ta into id_ahead.
    auto tile = [&](uint32_t t, const f16x8 (&cur)[NPRE], float n_cur, uint32_t id_cur, uint32_t tn, f16x8 (&nxt)[NPRE], float &n_nxt,
                    uint32_t id_nxt, uint32_t ta, uint32_t &id_ahead) {
        const uint32_t c0 = col0(t), col = c0 + m;
        const bool col_ok = col < c_end;
        f16x8 late[NLATE > 0 ? NLATE : 1];
        if constexpr (NLATE > 0)
            pieces(id_cur, col_ok, NPRE, late);
        if (tn < ntiles) { // in flight behind this tile's MFMAs
            const bool ok = col0(tn) + m < c_end;
            pieces(id_nxt, ok, 0, nxt);
            n_nxt = ok ? xn[id_nxt] : 0.f;
        }
        if (ta < ntiles)
            id_ahead = ids(ta);
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NPRE; s++)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], cur[s], acc, 0, 0, 0);
        if constexpr (NLATE > 0) {
#pragma unroll
            for (int s = 0; s < NLATE; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[NPRE + s], late[s], acc, 0, 0, 0);
        }
        // the cheap test: inside every non-empty window the unwindowed one, else a register counts where its row is live
        const bool all = ((uint32_t)__ballot(wa <= c0 && wb >= c0 + 32u) | empty) == ~0u; // wave-uniform
        bool any = false, hit = false;
        if (all) {
#pragma unroll
            for (int r = 0; r < 16; r++)
                any |= __fsub_rn(__fmul_rn(2.0f, acc[r]), n_cur) > gate[r];
        } else {
            const uint32_t lv = (uint32_t)__ballot(meets(c0)) >> (4 * kk); // bit (r & 3) + 8 (r >> 2): register r's row is live
            uint32_t pb = 0;
#pragma unroll
            for (int r = 0; r < 16; r++)
                pb |= __fsub_rn(__fmul_rn(2.0f, acc[r]), n_cur) > gate[r] ? 1u << ((r & 3) + 8 * (r >> 2)) : 0u;
            any = (pb & lv) != 0u;
        }
        if (__ballot(any && col_ok)) { // wave-uniform
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float dist = __fsub_rn(__fadd_rn(qn_r[r], n_cur), __fmul_rn(2.0f, acc[r]));
                const int row = mfma32_row(r, kk);
                const uint32_t ra = (uint32_t)__shfl((int)wa, row), rb = (uint32_t)__shfl((int)wb, row); // (every lane: read from another)
                const bool pass = col_ok && (in_rows >> r & 1u) && col >= ra && col < rb && dist < radius;
                const unsigned long long mask = __ballot(pass);
                const uint32_t half = kk ? (uint32_t)(mask >> 32) : (uint32_t)mask;
                hit |= mask != 0;
                if (FILL) {
                    const size_t o = (size_t)cnt[r] + __popc(half & ((1u << m) - 1u));
                    if (pass && o < out_cap) { // (o < out_cap always: the count form counted this very lane)
                        out_d[o] = dist;
                        out_l[o] = (long long)id_cur;
                    }
                }
                cnt[r] += __popc(half);
            }
        }
        if (!FILL && mw) {
            const uint32_t g = t >> map_shift;
            bits |= hit ? 1u << (g & 31) : 0u;
            if (tn >= ntiles || (tn >> map_shift) >> 5 != g >> 5) { // the word is complete: no live tile of it is left
                if (lane == 0)
                    mw[g >> 5] = bits;
                bits = 0;
            }
        }
    };

    uint32_t tn = next_tile(t + 1), ta;
    f16x8 b0[NPRE], b1[NPRE];
    float n0, n1 = 0.f;
    uint32_t id0 = ids(t), id1 = 0, id_ahead = 0;
    pieces(id0, col0(t) + m < c_end, 0, b0);
    n0 = col0(t) + m < c_end ? xn[id0] : 0.f;
    if (tn < ntiles)
        id1 = ids(tn);
    for (;;) {
        ta = next_tile(tn + 1);
        tile(t, b0, n0, id0, tn, b1, n1, id1, ta, id_ahead);
        if (tn >= ntiles)
            break;
        t = tn, tn = ta, id0 = id_ahead;
        ta = next_tile(tn + 1);
        tile(t, b1, n1, id1, tn, b0, n0, id0, ta, id_ahead);
        if (tn >= ntiles)
            break;
        t = tn, tn = ta, id1 = id_ahead;
    }

    if (!FILL) {
        unsigned long long sum = 0;
        if (m == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (in_rows >> r & 1u)
                    slices[slice_of(mfma32_row(r, kk))] = cnt[r];
                sum += cnt[r];
            }
        }
        sum += __shfl_xor(sum, 32);
        if (lane == 0 && sum)
            atomicAdd(total, sum);
    }
}

} // namespace

size_t exact_f16_lds_bytes(int d, int k)
{
    const size_t waves = k <= 32 ? 4 : 2, cap = k <= 16 ? 48 : k <= 32 ? 64 : 136;
    return (size_t)2 * 32 * (2 * d + 16) + waves * 32 * cap * sizeof(unsigned long long) + waves * 32 * (sizeof(uint32_t) + sizeof(float));
}

hipError_t launch_f16_check(hipStream_t s, const float *src, size_t src_stride, size_t count, int d, uint32_t *flag)
{
    if (count == 0)
        return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((count * (size_t)d + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(f16_check_kernel, dim3(grid), dim3(256), 0, s, src, src_stride, count, d, flag);
    return hipGetLastError();
}

hipError_t launch_f16_store(hipStream_t s, const float *src, size_t src_stride, void *dst, float *norms, size_t count, int d)
{
    if (count == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || count > ((size_t)1 << 36))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_store_kernel<false>, dim3((unsigned)((count * 4 + 255) / 256)), dim3(256), 0, s, src, src_stride,
                       reinterpret_cast<_Float16 *>(dst), norms, count, d, (const int32_t *)nullptr);
    return hipGetLastError();
}

hipError_t launch_f16_store_rows(hipStream_t s, const float *src, size_t src_stride, void *dst, float *norms, size_t count, int d,
                                 const int32_t *row_src)
{
    if (count == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || count > ((size_t)1 << 36) || !row_src)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_store_kernel<true>, dim3((unsigned)((count * 4 + 255) / 256)), dim3(256), 0, s, src, src_stride,
                       reinterpret_cast<_Float16 *>(dst), norms, count, d, row_src);
    return hipGetLastError();
}

// Qh, qn: the queries as launch_f16_store leaves rows; part: [nsplit][nq][k] u64 workspace
hipError_t launch_exact_search_f16(hipStream_t s, const void *Qh, const float *qn, const void *X, const float *xn, size_t nq,
                                   size_t nx, int d, int k, int nsplit, unsigned long long *part, float *dists, int64_t *labels)
{
    if (nq == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || k < 1 || k > 100 || nq > 0x7fffffffull || nx == 0 || nx >= 0xffffffffull || nsplit < 1 ||
        nsplit > 64)
        return hipErrorInvalidValue;
    const size_t cps = sweep_cols_per_split(nx, nsplit);
    const _Float16 *q = reinterpret_cast<const _Float16 *>(Qh), *x = reinterpret_cast<const _Float16 *>(X);
    const hipError_t e = by_f16_steps(d, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        return k <= 16   ? launch_exact_f16_t<ND, 48, 4>(s, q, qn, x, xn, (int)nq, nx, k, nsplit, cps, part, F16Rows{})
               : k <= 32 ? launch_exact_f16_t<ND, 64, 4>(s, q, qn, x, xn, (int)nq, nx, k, nsplit, cps, part, F16Rows{})
                         : launch_exact_f16_t<ND, 136, 2>(s, q, qn, x, xn, (int)nq, nx, k, nsplit, cps, part, F16Rows{});
    });
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(exact_f16_merge_kernel, dim3((unsigned)nq), dim3(64), 0, s, part, nsplit, (int)nq, k, dists,
                       reinterpret_cast<long long *>(labels));
    return hipGetLastError();
}

// ... under a tag plan: Qh, qn [bound * 32] = the chunk's nq queries gathered by the plan
// (launch_f16_store_rows), part [max(ns_dense, ns_ind)][bound * 32][k]; the Dense strips by the staged kernel under ns_dense
// splits, the Indirect ones (forms bit kSweepColsIndirect) by the per-wave kernel under ns_ind; results in the caller's
// order, FLT_MAX / -1 for a query without a strip.  win (base values): sp is a value plan, its Indirect strips
// are windowed -- each row with its own window win[32 strip + row] of the strip's span -- and go to the windowed kernel
hipError_t launch_exact_search_f16_strips(hipStream_t s, const void *Qh, const float *qn, const void *X, const float *xn, size_t nq,
                                          size_t bound, size_t nx, int d, int k, int ns_dense, int ns_ind, unsigned long long *part,
                                          float *dists, int64_t *labels, const StripPlan &sp, unsigned forms, const StripWin *win)
{
    if (nq == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || k < 1 || k > 100 || bound == 0 || bound > (0x7fffffffull >> 5) || nx == 0 || nx >= 0xffffffffull ||
        ns_dense < 1 || ns_dense > 64 || ns_ind < 1 || ns_ind > 64 || !sp.hdr || !sp.strip_rows || !sp.strip_cols)
        return hipErrorInvalidValue;
    if (win && nx > 0xffffffffull - 64) // (the windowed kernel adds a tile's 32 columns to a column in 32 bits)
        return hipErrorInvalidValue;
    const int rows = (int)(bound * 32);
    if (hipError_t e = launch_exact_pad(s, dists, labels, nq * (size_t)k); e != hipSuccess)
        return e;
    const size_t cps = sweep_cols_per_split(nx, ns_dense);
    const _Float16 *q = reinterpret_cast<const _Float16 *>(Qh), *x = reinterpret_cast<const _Float16 *>(X);
    const bool indirect = forms >> kSweepColsIndirect & 1u;
    const hipError_t e = by_f16_steps(d, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        const F16DenseStrips ds{sp};
        hipError_t e = k <= 16   ? launch_exact_f16_t<ND, 48, 4>(s, q, qn, x, xn, rows, nx, k, ns_dense, cps, part, ds)
                       : k <= 32 ? launch_exact_f16_t<ND, 64, 4>(s, q, qn, x, xn, rows, nx, k, ns_dense, cps, part, ds)
                                 : launch_exact_f16_t<ND, 136, 2>(s, q, qn, x, xn, rows, nx, k, ns_dense, cps, part, ds);
        if (e != hipSuccess || !indirect)
            return e;
        if (win)
            return k <= 16   ? launch_exact_f16_windows_t<ND, 48, 4>(s, q, qn, x, xn, bound, k, ns_ind, part, sp, win)
                   : k <= 32 ? launch_exact_f16_windows_t<ND, 64, 4>(s, q, qn, x, xn, bound, k, ns_ind, part, sp, win)
                             : launch_exact_f16_windows_t<ND, 136, 2>(s, q, qn, x, xn, bound, k, ns_ind, part, sp, win);
        return k <= 16   ? launch_exact_f16_rows_t<ND, 48, 4>(s, q, qn, x, xn, bound, k, ns_ind, part, sp)
               : k <= 32 ? launch_exact_f16_rows_t<ND, 64, 4>(s, q, qn, x, xn, bound, k, ns_ind, part, sp)
                         : launch_exact_f16_rows_t<ND, 136, 2>(s, q, qn, x, xn, bound, k, ns_ind, part, sp);
    });
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(exact_f16_merge_strips_kernel, dim3((unsigned)rows), dim3(64), 0, s, part, ns_dense, ns_ind, rows, k, dists,
                       reinterpret_cast<long long *>(labels), sp);
    return hipGetLastError();
}

hipError_t launch_f16_tags_values_split(hipStream_t s, const uint16_t *d_tags, const uint32_t *d_ranges, size_t m, uint32_t *lo_keys,
                                        uint32_t *vranges)
{
    if (m == 0)
        return hipSuccess;
    if (!d_tags || !d_ranges || !lo_keys || !vranges)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_tags_values_split_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, d_tags, d_ranges, m, lo_keys, vranges);
    return hipGetLastError();
}

// ... under a tag AND an interval per query.  Qh, qn [(bound_v + bound_t) * 32]: the chunk's nq queries
// gathered by the value plan spv (its rows first) and by the tag plan spt; part [max of the splits][(bound_v + bound_t) * 32][k].
// spv (null: no untagged query, nothing of it is launched): the plan of the untagged queries' intervals with its windows
// win, Dense strips by the staged kernel under ns_dense, windowed ones (`windowed`: the holder has values) under ns_win.
// spt (null: nothing of it is launched): the tag plan, whose Indirect strips go to the gated kernel under ns_tag with the
// chunk's tags and intervals d_tags, d_ranges and the holder's values (null: none).  One merge; FLT_MAX / -1 for a query
// without a strip.
hipError_t launch_exact_search_f16_tags_values(hipStream_t s, const void *Qh, const float *qn, const void *X, const float *xn, size_t nq,
                                               size_t bound_v, size_t bound_t, size_t nx, int d, int k, int ns_dense, int ns_win, int ns_tag,
                                               unsigned long long *part, float *dists, int64_t *labels, const StripPlan *spv,
                                               const StripWin *win, bool windowed, const StripPlan *spt, const uint16_t *d_tags,
                                               const uint32_t *d_ranges, const uint32_t *vals)
{
    if (nq == 0)
        return hipSuccess;
    const size_t bound = bound_v + bound_t;
    if (d < 16 || d > 256 || (d & 15) || k < 1 || k > 100 || bound_v == 0 || bound_t == 0 || bound > (0x7fffffffull >> 5) || nx == 0 ||
        nx > 0xffffffffull - 64 || ns_dense < 1 || ns_dense > 64 || ns_win < 1 || ns_win > 64 || ns_tag < 1 || ns_tag > 64 ||
        (spv && (!spv->hdr || !spv->strip_rows || !spv->strip_cols || !win)) ||
        (spt && (!spt->hdr || !spt->strip_rows || !spt->strip_cols || !d_tags || !d_ranges)))
        return hipErrorInvalidValue;
    const int rows = (int)(bound * 32), rows_v = (int)(bound_v * 32);
    if (hipError_t e = launch_exact_pad(s, dists, labels, nq * (size_t)k); e != hipSuccess)
        return e;
    if (!spv && !spt)
        return hipSuccess;
    const size_t cps = sweep_cols_per_split(nx, ns_dense);
    const _Float16 *q = reinterpret_cast<const _Float16 *>(Qh), *x = reinterpret_cast<const _Float16 *>(X);
    const hipError_t e = by_f16_steps(d, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        hipError_t e = hipSuccess;
        if (spv) {
            const F16DenseStrips ds{*spv};
            e = k <= 16   ? launch_exact_f16_t<ND, 48, 4>(s, q, qn, x, xn, rows, nx, k, ns_dense, cps, part, ds)
                : k <= 32 ? launch_exact_f16_t<ND, 64, 4>(s, q, qn, x, xn, rows, nx, k, ns_dense, cps, part, ds)
                          : launch_exact_f16_t<ND, 136, 2>(s, q, qn, x, xn, rows, nx, k, ns_dense, cps, part, ds);
            if (e == hipSuccess && windowed)
                e = k <= 16   ? launch_exact_f16_windows_t<ND, 48, 4>(s, q, qn, x, xn, bound_v, k, ns_win, part, *spv, win, rows)
                    : k <= 32 ? launch_exact_f16_windows_t<ND, 64, 4>(s, q, qn, x, xn, bound_v, k, ns_win, part, *spv, win, rows)
                              : launch_exact_f16_windows_t<ND, 136, 2>(s, q, qn, x, xn, bound_v, k, ns_win, part, *spv, win, rows);
        }
        if (e != hipSuccess || !spt)
            return e;
        const _Float16 *qt = q + (size_t)rows_v * d;
        const float *qnt = qn + rows_v;
        unsigned long long *pt = part + (size_t)rows_v * k;
        return k <= 16   ? launch_exact_f16_gated_t<ND, 48, 4>(s, qt, qnt, x, xn, bound_t, rows, k, ns_tag, pt, *spt, d_tags, d_ranges, vals)
               : k <= 32 ? launch_exact_f16_gated_t<ND, 64, 4>(s, qt, qnt, x, xn, bound_t, rows, k, ns_tag, pt, *spt, d_tags, d_ranges, vals)
                         : launch_exact_f16_gated_t<ND, 136, 2>(s, qt, qnt, x, xn, bound_t, rows, k, ns_tag, pt, *spt, d_tags, d_ranges, vals);
    });
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(exact_f16_merge_two_kernel, dim3((unsigned)rows), dim3(64), 0, s, part, ns_dense, ns_win, ns_tag, rows_v, rows, k,
                       dists, reinterpret_cast<long long *>(labels), spv ? *spv : StripPlan{}, spt ? *spt : StripPlan{},
                       (spv ? 1u : 0u) | (spt ? 2u : 0u));
    return hipGetLastError();
}

size_t exact_range_f16_lds_bytes(int d) { return (size_t)2 * 32 * (2 * d + 16); }

// the argument checks of launch_exact_range (kernels_exact.hip); the radius is any float but NaN
hipError_t launch_exact_range_f16(hipStream_t s, bool fill, const void *Qh, const float *qn, const void *X, const float *xn, size_t nq,
                                  size_t q_off, size_t nx, int d, float radius, int nsplit, uint32_t *slices,
                                  unsigned long long *total, uint32_t *map, int map_shift, float *dist, int64_t *labels,
                                  size_t out_cap)
{
    if (nq == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || radius != radius || nq > 0x7fffffffull || nx >= 0xffffffffull || nsplit < 1 ||
        nsplit > 64 || (q_off & 31) || map_shift < 0 || map_shift > kExactRangeMaxShift)
        return hipErrorInvalidValue;
    const int words = sweep_map_words(nx, nsplit, map_shift);
    // query tile is the fast index, column split the slow one, as in launch_exact_f16_t
    const dim3 grid((unsigned)((nq + 127) / 128), (unsigned)nsplit);
    const _Float16 *q = reinterpret_cast<const _Float16 *>(Qh), *x = reinterpret_cast<const _Float16 *>(X);
    long long *lab = reinterpret_cast<long long *>(labels);
    return by_f16_steps(d, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        const auto kern = fill ? exact_range_f16_kernel<ND, true, F16Rows> : exact_range_f16_kernel<ND, false, F16Rows>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, q, qn, x, xn, (int)nq, nx, radius, q_off, slices, total, map, map_shift, words,
                           dist, lab, out_cap, F16Rows{});
        return hipGetLastError();
    });
}

// ... under a tag plan: Qh, qn [bound * 32] = the chunk's queries gathered by the plan, the chunk being
// queries [q_off, ...) of the call; nx = the rows of the store (the most columns any strip has).  The Dense strips by the
// staged kernel under ns_dense splits, the Indirect ones (forms bit kSweepColsIndirect) by the per-wave kernel under ns_ind;
// both grids cover every strip the plan can have, and what lies beyond a form's range leaves at once.  slices: one table
// max(ns_dense, ns_ind) splits wide, each form writes the splits it has.  map: exact_range_f16_strips_map_words words a strip.
// win (base values): sp is a value plan, its Indirect strips are windowed -- each row with its own window
// win[32 strip + row] of the strip's span -- and go to the windowed kernel, whose fill form writes in (value, row) order.
hipError_t launch_exact_range_f16_strips(hipStream_t s, bool fill, const void *Qh, const float *qn, const void *X, const float *xn,
                                         size_t bound, size_t q_off, size_t nx, int d, float radius, int ns_dense, int ns_ind,
                                         uint32_t *slices, unsigned long long *total, uint32_t *map, int map_shift, float *dist,
                                         int64_t *labels, size_t out_cap, const StripPlan &sp, unsigned forms, const StripWin *win)
{
    if (d < 16 || d > 256 || (d & 15) || radius != radius || bound == 0 || bound > (0x7fffffffull >> 5) || nx == 0 || nx >= 0xffffffffull ||
        ns_dense < 1 || ns_dense > 64 || ns_ind < 1 || ns_ind > 64 || map_shift < 0 || map_shift > kExactRangeMaxShift || !sp.hdr ||
        !sp.strip_rows || !sp.strip_cols)
        return hipErrorInvalidValue;
    if (win && nx > 0xffffffffull - 64) // (the windowed kernel adds a tile's 32 columns to a column in 32 bits)
        return hipErrorInvalidValue;
    const int slice_w = std::max(ns_dense, ns_ind);
    const uint32_t stride = (uint32_t)exact_range_f16_strips_map_words(nx, ns_dense, ns_ind, map_shift);
    const int w_dense = sweep_map_words(nx, ns_dense, map_shift), w_ind = sweep_map_words(nx, ns_ind, map_shift);
    const unsigned wgs = (unsigned)((bound + 3) / 4);
    const _Float16 *q = reinterpret_cast<const _Float16 *>(Qh), *x = reinterpret_cast<const _Float16 *>(X);
    long long *lab = reinterpret_cast<long long *>(labels);
    return by_f16_steps(d, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        const F16RangeDenseStrips ds{sp, slice_w, stride};
        const auto dense = fill ? exact_range_f16_kernel<ND, true, F16RangeDenseStrips> : exact_range_f16_kernel<ND, false, F16RangeDenseStrips>;
        hipLaunchKernelGGL(dense, dim3(wgs, (unsigned)ns_dense), dim3(256), 0, s, q, qn, x, xn, (int)(bound * 32), nx, radius, q_off, slices,
                           total, map, map_shift, w_dense, dist, lab, out_cap, ds);
        if (hipError_t e = hipGetLastError(); e != hipSuccess || !(forms >> kSweepColsIndirect & 1u))
            return e;
        if (win) {
            const auto wins = fill ? exact_range_f16_windows_kernel<ND, true> : exact_range_f16_windows_kernel<ND, false>;
            hipLaunchKernelGGL(wins, dim3(wgs, (unsigned)ns_ind), dim3(256), 0, s, q, qn, x, xn, radius, q_off, slice_w, slices, total, map,
                               map_shift, w_ind, stride, dist, lab, out_cap, sp, win);
            return hipGetLastError();
        }
        const auto rows = fill ? exact_range_f16_rows_kernel<ND, true> : exact_range_f16_rows_kernel<ND, false>;
        hipLaunchKernelGGL(rows, dim3(wgs, (unsigned)ns_ind), dim3(256), 0, s, q, qn, x, xn, radius, q_off, slice_w, slices, total, map,
                           map_shift, w_ind, stride, dist, lab, out_cap, sp);
        return hipGetLastError();
    });
}

} // namespace ivfhnsw_gpu_impl
