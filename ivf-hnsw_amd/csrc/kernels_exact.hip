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
// relied on (sweep_steps.h mfma32_row), the one knn_mfma_kernel uses.
//
// Shape: wave w of a workgroup owns the 32 query rows [32w, 32w + 32) of the workgroup's strip for the whole sweep and
// walks the columns of its split 32 at a time: the int8 strip of sweep_steps.h (I8Strip), which has the row load, the
// d % 32 == 16 tail rule and the tile product.  Selection is sweep_steps.h's too (row_append, rows_compact,
// rows_write_out), shared with kernels_knn.hip; here the key is (distance, label).  The common tile (no candidate in any
// of the wave's 32 x 32 distances) costs two vector instructions per accumulator register:
// 2 acc - |x'|^2 > |q'|^2 - threshold.
// LDS bounds the strip: 4 waves (128 rows) up to k = 32, 2 waves (64 rows) of 136 keys per row up to k = 100.
//
// The exact range search (ivfhnsw_gpu_exact_range_search) is the same strip with a fixed gate and no
// selection: exact_range_kernel, below the k-search.
//
// Under a base filter (ivfhnsw_gpu_set_base_filter) both kernels sweep through a column map, a template
// parameter (sweep_steps.h): ColsDense is the sweep described above and the only one without a filter; ColsMasked skips
// every tile of 32 rows in which no row passes; ColsIndirect sweeps the ascending list of passing rows instead of the store.
//
// With a base filter slot per query (ivfhnsw_gpu_exact_search_slots) the same two kernels run under
// ColsStrips<map>: the queries are laid out in slot-uniform strips of 32 rows (the plan: kernels_exact_filter.hip), a wave
// takes its strip's words or rows and column count from the holder's table (sweep_steps.h strip_open), one launch per form.
//
// With a base tag per query (ivfhnsw_gpu_exact_search_tags) the strips are tag-uniform and each carries its
// own entry (ColsStrips<map, true>): Dense for the untagged queries, Indirect over the tag's row list for the others.
//
// With an interval of row values per query (ivfhnsw_gpu_exact_search_values) the Indirect strips sweep a
// span of the holder's rows in (value, row) order and every strip row counts only its own window of it
// (ColsStrips<ColsIndirect, true, true>, RowWindows): columns arrive in value order, so the k-search admits ties at the
// k-th distance and the caller puts the range results in label order.
#include "sweep_steps.h"

#include <float.h>
#include <limits.h>

namespace ivfhnsw_gpu_impl {

namespace {

// NS = ceil(d / 32), the steps of 32 bytes a row is read in, CAP = keys of a row's candidate buffer (a row is
// compacted when it holds more than CAP - 32), WAVES = 32-row strips per workgroup.
// Qp: the queries in the store's byte order, [nq][d]; X: the store, [nx][d]; both 16-byte aligned, d % 16 == 0.
// CM: the column map (sweep_steps.h): ColsDense is the unfiltered sweep; under a base filter ColsMasked
// skips the tiles without a passing row, ColsIndirect sweeps the list of passing rows, nx = their number.
template <int NS, int CAP, int WAVES, class CM>
__global__ __launch_bounds__(64 * WAVES) void exact_mfma_kernel(const uint8_t *__restrict__ Qp, const uint8_t *__restrict__ X,
                                                                int nq, size_t nx, int d, int k, size_t cols_per_split,
                                                                unsigned long long *__restrict__ out_keys, CM cm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *s_buf = reinterpret_cast<unsigned long long *>(smem); // [WAVES][32][CAP]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_buf + WAVES * 32 * CAP);  // [WAVES][32]
    int *s_thr = reinterpret_cast<int *>(s_cnt + WAVES * 32);                  // [WAVES][32]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    // the wave's rows, map and columns: the call's, or under a strip plan its strip's
    int r0 = blockIdx.x * (32 * WAVES) + wave * 32;
    size_t c_begin, c_end;
    typename CM::Base bcm;
    if (!strip_open(cm, (int)gridDim.y, (int)blockIdx.y, nx, cols_per_split, r0, c_begin, c_end, bcm))
        return;
    unsigned long long *buf = s_buf + (size_t)wave * 32 * CAP;
    uint32_t *cnt = s_cnt + wave * 32;
    int *thr_s = s_thr + wave * 32;

    I8Strip<NS> st;
    st.setup(Qp, r0, lane, nq, d);
    // what the common tile compares against: dist < thr  <=>  2 dot - |x'|^2 > |q'|^2 - thr = gate
    // Under a windowed map columns do not arrive in label order, so a distance EQUAL to the k-th is admitted
    // too (dist <= thr: the gate one lower) and the keys, (distance, label), decide; the first threshold is then a number
    // above every distance (<= 256 * 255^2 < 2^24) from which thr + 1 and |q'|^2 - thr - 1 do not overflow.
    constexpr int kTie = CM::kWindowed ? 1 : 0, kThr0 = CM::kWindowed ? 1 << 30 : INT_MAX;
    int gate[16];
    RowWindows<CM> rw; // (a row without a window, the padding of a strip that is not full: a gate nothing passes)
    rw.setup(cm, r0, lane);
#pragma unroll
    for (int r = 0; r < 16; r++)
        gate[r] = rw.gate_of(r, st.qn_r[r] - kThr0 - kTie);
    if (lane < 32) {
        cnt[lane] = 0;
        thr_s[lane] = kThr0;
    }
    __builtin_amdgcn_wave_barrier();

    // The tiles of the split in turn -- under a column map the ones it visits: the prefetch goes to the next tile that will
    // be visited (ColsDense: c0 + 32, the loop as it was before there were column maps).
    ColCursor<typename CM::Base> cc;
    cc.setup(bcm, c_begin, c_end, (uint32_t)((c_end - c_begin + 31) >> 5), lane);
    size_t cn = cc.next_col(c_begin);
    if (cn < c_end) {
        cc.ids(cn);
        cc.shift();
        cc.fetch(st, X, cn, c_begin, c_end, d);
        if (CM::kIndirect && cn + 32 < c_end)
            cc.ids(cn + 32);
    }
    for (size_t c0 = cn; c0 < c_end; c0 = cn) {
        const size_t col = c0 + m;
        const bool col_ok = col < c_end && cc.lane_pass(m);
        st.take(); // a lane without a column scores a row it drops below
        cc.shift();
        cn = cc.next_col(c0 + 32);
        if (cn < c_end)
            cc.fetch(st, X, cn, c_begin, c_end, d); // in flight behind this tile's MFMAs
        if (CM::kIndirect && cn + 32 < c_end)
            cc.ids(cn + 32); // (Indirect visits every tile: the one after the next begins at cn + 32)
        if (!rw.tile(c0, kk))
            continue; // wave-uniform: no row's window meets the tile
        i32x16 acc;
        int xn;
        st.product(acc, xn);
        if (!__ballot(rw.any_pass(st, acc, xn, gate) && col_ok))
            continue; // wave-uniform: the common tile once the thresholds have settled
        const uint32_t label = (uint32_t)cc.label(col);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int dist = st.dist(acc, xn, r);
            const bool in = rw.row_counts(r, kk, col); // (every lane: a window is read from another lane)
            const bool pass = col_ok && dist < st.qn_r[r] - gate[r] && in;
            const unsigned long long mask = __ballot(pass);
            if (mask)
                row_append<CAP>(buf, cnt, mfma32_row(r, kk), pass, mask, dist, label, m, kk);
        }
        rows_compact<CAP>(buf, cnt, thr_s, k, lane);
#pragma unroll
        for (int r = 0; r < 16; r++)
            gate[r] = rw.gate_of(r, st.qn_r[r] - thr_s[mfma32_row(r, kk)] - kTie);
    }

    // out: [split][nq][k] keys
    rows_write_out<CAP>(buf, cnt, k, lane, nq - r0, out_keys, (size_t)blockIdx.y * nq + r0);
}

__global__ __launch_bounds__(64) void exact_merge_kernel(const unsigned long long *__restrict__ part, int nsplit, int nq, int k,
                                                         float *__restrict__ dists, long long *__restrict__ labels)
{
    sweep_merge(
        part, nsplit, nq, k,
        [&](size_t o, unsigned long long key) {
            labels[o] = (long long)(uint32_t)key;
            dists[o] = (float)(uint32_t)(key >> 32); // an integer below 2^24: exact
        },
        [&](size_t o) { // the store has fewer than k rows
            labels[o] = -1ll;
            dists[o] = FLT_MAX;
        });
}

template <int NS, int CAP, int WAVES, class CM>
hipError_t launch_exact_t(hipStream_t s, const uint8_t *Qp, const uint8_t *X, int nq, size_t nx, int d, int k, int nsplit,
                          size_t cols_per_split, unsigned long long *part, CM cm)
{
    const size_t shm = (size_t)WAVES * 32 * CAP * sizeof(unsigned long long) + (size_t)WAVES * 32 * (sizeof(uint32_t) + sizeof(int));
    constexpr auto kern = exact_mfma_kernel<NS, CAP, WAVES, CM>;
    if (hipError_t e = dyn_lds<kern>(shm); e != hipSuccess)
        return e;
    // query tile is the fast index, column split the slow one: the tiles that run together stream the same columns
    hipLaunchKernelGGL(kern, dim3((unsigned)((nq + 32 * WAVES - 1) / (32 * WAVES)), (unsigned)nsplit), dim3(64 * WAVES), shm,
                       s, Qp, X, nq, nx, d, k, cols_per_split, part, cm);
    return hipGetLastError();
}

// f(the column map of `cols` as its kernel argument): the one dispatch on the form
template <class F> hipError_t by_col_map(const SweepCols &cols, F &&f)
{
    switch (cols.form) {
    case kSweepColsDense: return f(ColsDense{});
    case kSweepColsMasked: return f(ColsMasked{cols.data});
    case kSweepColsIndirect: return f(ColsIndirect{cols.data});
    default: return hipErrorInvalidValue;
    }
}

// ... and under a strip plan: one launch per form in `forms` (bit f = form f), each over the plan's strips
// of that form.  A plan whose strips carry their own entries (base tags) has Dense and Indirect strips only.
template <bool OWN, class F> hipError_t by_strip_maps_of(const StripPlan &sp, unsigned forms, F &&f)
{
    hipError_t e = hipSuccess;
    if (e == hipSuccess && (forms >> kSweepColsDense & 1u))
        e = f(ColsStrips<ColsDense, OWN>{sp});
    if constexpr (!OWN)
        if (e == hipSuccess && (forms >> kSweepColsMasked & 1u))
            e = f(ColsStrips<ColsMasked>{sp});
    if (e == hipSuccess && (forms >> kSweepColsIndirect & 1u))
        e = f(ColsStrips<ColsIndirect, OWN>{sp});
    return e;
}
// win (base values): the plan's Indirect strips are windowed, each row with its own window
template <class F> hipError_t by_strip_maps(const StripPlan &sp, unsigned forms, const StripWin *win, F &&f)
{
    if (win) {
        if (!sp.strip_cols || (forms >> kSweepColsMasked & 1u))
            return hipErrorInvalidValue;
        hipError_t e = hipSuccess;
        if (forms >> kSweepColsDense & 1u)
            e = f(ColsStrips<ColsDense, true>{sp});
        if (e == hipSuccess && (forms >> kSweepColsIndirect & 1u))
            e = f(ColsStrips<ColsIndirect, true, true>{sp, win});
        return e;
    }
    if (sp.strip_cols)
        return (forms >> kSweepColsMasked & 1u) ? hipErrorInvalidValue : by_strip_maps_of<true>(sp, forms, f);
    return by_strip_maps_of<false>(sp, forms, f);
}

// the merge under a strip plan, one wavefront per strip row: the row of a query goes to the query's place in the caller's
// order, padding rows and strips beyond the plan's are dropped
__global__ __launch_bounds__(64) void exact_merge_strips_kernel(const unsigned long long *__restrict__ part, int nsplit, int nrows,
                                                                int k, float *__restrict__ dists, long long *__restrict__ labels,
                                                                StripPlan sp)
{
    const uint32_t row = blockIdx.x;
    if ((row >> 5) >= sp.hdr->lay.nstrips)
        return;
    const int q = sp.strip_rows[row];
    if (q < 0)
        return;
    sweep_merge_row(
        part, nsplit, nrows, k, (int)row, q,
        [&](size_t o, unsigned long long key) {
            labels[o] = (long long)(uint32_t)key;
            dists[o] = (float)(uint32_t)(key >> 32);
        },
        [&](size_t o) { // fewer than k rows pass the query's slot
            labels[o] = -1ll;
            dists[o] = FLT_MAX;
        });
}

// every result "nothing": what a query without a strip keeps
__global__ __launch_bounds__(256) void exact_pad_kernel(float *__restrict__ dists, long long *__restrict__ labels, size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        labels[i] = -1ll;
        dists[i] = FLT_MAX;
    }
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
// Under a column map (CM, as in exact_mfma_kernel) the tile map and the pass words compose: the count form visits the
// tiles with a passing row and sets map bits only for those, the fill form visits a tile iff its map bit is set and its
// pass word is not zero (a bit of a coarser map covers 2^map_shift tiles, some of which may be empty).
template <int NS, bool FILL, class CM>
__global__ __launch_bounds__(256) void exact_range_kernel(const uint8_t *__restrict__ Qp, const uint8_t *__restrict__ X, int nq,
                                                          size_t nx, int d, int thr, size_t cols_per_split, size_t q_off,
                                                          uint32_t *__restrict__ slices, unsigned long long *__restrict__ total,
                                                          uint32_t *__restrict__ map, int map_shift, int map_words,
                                                          float *__restrict__ out_d, long long *__restrict__ out_l,
                                                          size_t out_cap, CM cm)
{
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    int r0 = blockIdx.x * 128 + wave * 32;
    if (r0 >= nq)
        return; // no barrier anywhere below
    const int nsplit = gridDim.y, split = blockIdx.y;
    // the wave's rows, map and columns: the call's, or under a strip plan its strip's, whose rows are
    // queries of the call in any order (strip_row_query) -- slices and cursors are the QUERY's, the tile map the strip's
    size_t c_begin, c_end;
    typename CM::Base bcm;
    if (!strip_open(cm, nsplit, split, nx, cols_per_split, r0, c_begin, c_end, bcm))
        return;
    const uint32_t ntiles = (uint32_t)((c_end - c_begin + 31) >> 5);

    I8Strip<NS> st;
    st.setup(Qp, r0, lane, nq, d);
    // dist < thr  <=>  2 dot - |x'|^2 > |q'|^2 - thr = gate, set once (|q'|^2 <= 2^22: no overflow for any thr >= 0)
    int gate[16];
    uint32_t cnt[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        size_t qi;
        const bool in = strip_row_query(cm, r0, mfma32_row(r, kk), nq, q_off, &qi);
        gate[r] = in ? st.qn_r[r] - thr : INT_MAX;
        cnt[r] = FILL && in ? slices[qi * nsplit + split] : 0u;
    }

    size_t map_strip = (q_off + r0) >> 5;
    if constexpr (CM::kStrips)
        map_strip = cm.sp.map_strip0 + (size_t)(r0 >> 5);
    uint32_t *mw = map ? map + ((map_strip * nsplit + split) * (size_t)map_words) : nullptr;
    ColCursor<typename CM::Base> cc;
    cc.setup(bcm, c_begin, c_end, ntiles, lane);
    RowWindows<CM> rw;
    rw.setup(cm, r0, lane);
#pragma unroll
    for (int r = 0; r < 16; r++)
        gate[r] = rw.gate_of(r, gate[r]);
    // the first tile at or after t that is to be visited (ntiles: none): one with a passing row (cc.next) whose map bit is
    // set.  The map is read only at tiles with a passing row: those the count form visited, whose words it wrote.
    auto next_tile = [&](uint32_t t) -> uint32_t {
        for (;;) {
            t = cc.next(t, ntiles);
            if (!FILL || !mw || t >= ntiles)
                return t;
            const uint32_t g = t >> map_shift;
            const uint32_t w = __builtin_amdgcn_readfirstlane(mw[g >> 5]) >> (g & 31);
            if (w & 1u)
                return t;
            t = (w ? g + (uint32_t)__ffs((int)w) - 1u : (g | 31u) + 1u) << map_shift; // the next set bit, or the next word
        }
    };
    uint32_t t = next_tile(0), bits = 0;
    if (t < ntiles) {
        cc.ids(c_begin + ((size_t)t << 5));
        cc.shift();
        cc.fetch(st, X, c_begin + ((size_t)t << 5), c_begin, c_end, d);
        if constexpr (CM::kIndirect) {
            const uint32_t t1 = next_tile(t + 1);
            if (t1 < ntiles)
                cc.ids(c_begin + ((size_t)t1 << 5));
        }
    }
    while (t < ntiles) {
        const size_t col = c_begin + ((size_t)t << 5) + m;
        const bool col_ok = col < c_end && cc.lane_pass(m);
        st.take();
        cc.shift();
        const uint32_t tn = next_tile(t + 1);
        if (tn < ntiles)
            cc.fetch(st, X, c_begin + ((size_t)tn << 5), c_begin, c_end, d); // in flight behind this tile's MFMAs
        if constexpr (CM::kIndirect) { // the row numbers of the tile after the next
            const uint32_t tnn = tn < ntiles ? next_tile(tn + 1) : ntiles;
            if (tnn < ntiles)
                cc.ids(c_begin + ((size_t)tnn << 5));
        }
        i32x16 acc;
        int xn;
        bool hit = rw.tile(c_begin + ((size_t)t << 5), kk); // wave-uniform: does any row's window meet the tile
        if (hit) {
            st.product(acc, xn);
            hit = __ballot(rw.any_pass(st, acc, xn, gate) && col_ok) != 0; // wave-uniform
        }
        if (hit) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const bool in = rw.row_counts(r, kk, col); // (every lane: a window is read from another lane)
                const bool pass = col_ok && i8_gate_pass(acc[r], xn, gate[r]) && in;
                const unsigned long long mask = __ballot(pass);
                const uint32_t half = kk ? (uint32_t)(mask >> 32) : (uint32_t)mask;
                if (FILL) {
                    const size_t o = (size_t)cnt[r] + __popc(half & ((1u << m) - 1u));
                    if (pass && o < out_cap) { // (o < out_cap always: the count form counted this very lane)
                        out_d[o] = (float)st.dist(acc, xn, r);
                        out_l[o] = (long long)cc.label(col);
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
                size_t qi;
                if (strip_row_query(cm, r0, mfma32_row(r, kk), nq, q_off, &qi))
                    slices[qi * nsplit + split] = cnt[r];
                sum += cnt[r];
            }
        }
        sum += __shfl_xor(sum, 32);
        if (lane == 0 && sum)
            atomicAdd(total, sum);
    }
}

} // namespace

hipError_t launch_exact_range(hipStream_t s, bool fill, const uint8_t *Qp, const uint8_t *X, size_t nq, size_t q_off, size_t nx,
                              int d, int thr, int nsplit, uint32_t *slices, unsigned long long *total, uint32_t *map,
                              int map_shift, float *dist, int64_t *labels, size_t out_cap, const SweepCols &cols)
{
    if (nq == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || thr < 0 || nq > 0x7fffffffull || nx >= 0xffffffffull || nsplit < 1 || nsplit > 64 ||
        (q_off & 31) || map_shift < 0 || map_shift > kExactRangeMaxShift || (cols.form != kSweepColsDense && nx && !cols.data))
        return hipErrorInvalidValue;
    const size_t cps = sweep_cols_per_split(nx, nsplit);
    const int words = sweep_map_words(nx, nsplit, map_shift);
    // query tile is the fast index, column split the slow one, as in launch_exact_t
    const dim3 grid((unsigned)((nq + 127) / 128), (unsigned)nsplit);
    long long *lab = reinterpret_cast<long long *>(labels);
    return by_row_steps(d, [&](auto ns) {
        return by_col_map(cols, [&](auto cm) {
            using CM = decltype(cm);
            const auto kern = fill ? exact_range_kernel<decltype(ns)::value, true, CM> : exact_range_kernel<decltype(ns)::value, false, CM>;
            hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, Qp, X, (int)nq, nx, d, thr, cps, q_off, slices, total, map, map_shift,
                               words, dist, lab, out_cap, cm);
            return hipGetLastError();
        });
    });
}

// ... under a strip plan: Qp [bound * 32][d] = the chunk's queries gathered by the plan, the chunk being
// queries [q_off, ...) of the call; nx = the rows of the store (the most columns any strip has: the tile map's stride).
// One launch per form in `forms`, each sized by the bound: waves beyond the plan's strips of the form exit at once.
hipError_t launch_exact_range_strips(hipStream_t s, bool fill, const uint8_t *Qp, const uint8_t *X, size_t bound, size_t q_off,
                                     size_t nx, int d, int thr, int nsplit, uint32_t *slices, unsigned long long *total,
                                     uint32_t *map, int map_shift, float *dist, int64_t *labels, size_t out_cap,
                                     const StripPlan &sp, unsigned forms, const StripWin *win)
{
    if (d < 16 || d > 256 || (d & 15) || thr < 0 || bound == 0 || bound > (0x7fffffffull >> 5) || nx >= 0xffffffffull || nsplit < 1 ||
        nsplit > 64 || map_shift < 0 || map_shift > kExactRangeMaxShift || !sp.hdr || !sp.strip_rows || (!sp.strip_cols && (!sp.table || !sp.strip_slot)))
        return hipErrorInvalidValue;
    const int words = sweep_map_words(nx, nsplit, map_shift);
    const dim3 grid((unsigned)((bound + 3) / 4), (unsigned)nsplit);
    long long *lab = reinterpret_cast<long long *>(labels);
    return by_row_steps(d, [&](auto ns) {
        return by_strip_maps(sp, forms, win, [&](auto cm) {
            using CM = decltype(cm);
            const auto kern = fill ? exact_range_kernel<decltype(ns)::value, true, CM> : exact_range_kernel<decltype(ns)::value, false, CM>;
            hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, Qp, X, (int)(bound * 32), (size_t)0, d, thr, (size_t)0, q_off, slices, total,
                               map, map_shift, words, dist, lab, out_cap, cm);
            return hipGetLastError();
        });
    });
}

// Qp: [nq][d] queries in the store's byte order (launch_rerank_permute); part: [nsplit][nq][k] u64 workspace
hipError_t launch_exact_search(hipStream_t s, const uint8_t *Qp, const uint8_t *X, size_t nq, size_t nx, int d, int k,
                               int nsplit, unsigned long long *part, float *dists, int64_t *labels, const SweepCols &cols)
{
    if (nq == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || k < 1 || k > 100 || nq > 0x7fffffffull || nx >= 0xffffffffull || nsplit < 1 ||
        nsplit > 64 || (cols.form != kSweepColsDense && nx && !cols.data))
        return hipErrorInvalidValue;
    if (nx == 0) // no column at all (a filter nothing passes): no sweep, the merge of no tables writes the padding
        nsplit = 0;
    const size_t cps = sweep_cols_per_split(nx, nsplit ? nsplit : 1);
    const hipError_t e = nsplit == 0 ? hipSuccess : by_row_steps(d, [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        return by_col_map(cols, [&](auto cm) {
            return k <= 16   ? launch_exact_t<NS, 48, 4>(s, Qp, X, (int)nq, nx, d, k, nsplit, cps, part, cm)
                   : k <= 32 ? launch_exact_t<NS, 64, 4>(s, Qp, X, (int)nq, nx, d, k, nsplit, cps, part, cm)
                             : launch_exact_t<NS, 136, 2>(s, Qp, X, (int)nq, nx, d, k, nsplit, cps, part, cm);
        });
    });
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(exact_merge_kernel, dim3((unsigned)nq), dim3(64), 0, s, part, nsplit, (int)nq, k, dists,
                       reinterpret_cast<long long *>(labels));
    return hipGetLastError();
}

// ... under a strip plan: Qp [bound * 32][d] = the chunk's nq queries gathered by the plan, part
// [nsplit][bound * 32][k]; results in the caller's order, FLT_MAX / -1 for a query without a strip
hipError_t launch_exact_search_strips(hipStream_t s, const uint8_t *Qp, const uint8_t *X, size_t nq, size_t bound, int d, int k,
                                      int nsplit, unsigned long long *part, float *dists, int64_t *labels, const StripPlan &sp,
                                      unsigned forms, const StripWin *win)
{
    if (nq == 0)
        return hipSuccess;
    if (d < 16 || d > 256 || (d & 15) || k < 1 || k > 100 || bound == 0 || bound > (0x7fffffffull >> 5) || nsplit < 1 || nsplit > 64 ||
        !sp.hdr || !sp.strip_rows || (!sp.strip_cols && (!sp.table || !sp.strip_slot)))
        return hipErrorInvalidValue;
    const int rows = (int)(bound * 32);
    long long *lab = reinterpret_cast<long long *>(labels);
    hipLaunchKernelGGL(exact_pad_kernel, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, s, dists, lab, nq * (size_t)k);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    const hipError_t e = by_row_steps(d, [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        return by_strip_maps(sp, forms, win, [&](auto cm) {
            return k <= 16   ? launch_exact_t<NS, 48, 4>(s, Qp, X, rows, 0, d, k, nsplit, 0, part, cm)
                   : k <= 32 ? launch_exact_t<NS, 64, 4>(s, Qp, X, rows, 0, d, k, nsplit, 0, part, cm)
                             : launch_exact_t<NS, 136, 2>(s, Qp, X, rows, 0, d, k, nsplit, 0, part, cm);
        });
    });
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(exact_merge_strips_kernel, dim3((unsigned)rows), dim3(64), 0, s, part, nsplit, rows, k, dists, lab, sp);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
