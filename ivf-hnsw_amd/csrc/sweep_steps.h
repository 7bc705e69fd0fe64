// The steps the brute-force MFMA sweeps share, one copy each: the C/D row map, the selection of a row's k
// smallest keys through its LDS buffer (knn_mfma_kernel, exact_mfma_kernel), the int8 strip that reads the uint8 store
// (exact_mfma_kernel, exact_range_kernel), the column maps those two sweep under when the store has a base filter
// (ColsDense / ColsMasked / ColsIndirect, ColCursor; per 32-row strip under base filter slots, base tags and base values: ColsStrips, strip_open, RowWindows) and the merge of the splits' partial tables.  Control flow -- which tile comes
// next, what a tile without a candidate costs, what is done with a distance that passes -- stays in the kernels.  Host
// arithmetic (columns per split, split count): sweep_plan_math.h.
#pragma once

#include "ivfhnsw_kernels.h"
#include "device_common.h"

namespace ivfhnsw_gpu_impl {

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// a slot of a key table nothing was found for
constexpr unsigned long long kSweepKeyNone = ~0ull;

// C/D layout of the 32x32 MFMA: col = lane & 31, and accumulator register r of a lane with kk = lane >> 5 is row
__device__ __forceinline__ int mfma32_row(int r, int kk) { return (r & 3) + 8 * (r >> 2) + 4 * kk; }

// ---------------------------------------------------------------------------------------------------------------------
// Selection.  Every lane holds the running k-th distance of its 16 rows; a candidate below it (rare after the first
// tiles) goes to the row's LDS buffer, placed by a ballot; a row whose buffer could overflow in the next tile is
// compacted by its wave by rank (keys are unique: the column in the low word).  Columns arrive in increasing order, so
// among equal distances the lower column wins by the strict '<' alone.
// A wave's arrays: buf [32][CAP] keys, cnt [32] keys held, thr_s [32] the k-th distance (the type's maximum until a row
// holds k keys).  CAP = keys of a row's buffer; a row is compacted when it holds more than CAP - 32.

// A distance as the high word of a key, and back as the threshold its kernel compares distances with: float distances
// in their order-preserving form, the exact search's integers as they are.  Chosen by type at compile time: only a lane
// that appends, and the one lane that finds a row's k-th key, convert, which costs no register -- keeping the high word
// in LDS and converting on reload would be 16 conversions per lane after every tile with a candidate.
__device__ __forceinline__ uint32_t key_hi(float dist) { return f32_orderable(dist); }
__device__ __forceinline__ uint32_t key_hi(int dist) { return (uint32_t)dist; }
__device__ __forceinline__ void key_threshold(uint32_t hi, float &thr) { thr = orderable_f32(hi); }
__device__ __forceinline__ void key_threshold(uint32_t hi, int &thr) { thr = (int)hi; }

// The lanes of `row` that pass (mask = their ballot, not empty: the test is the kernel's, wave-uniform) append their
// (dist, col) keys in lane order = column order.
template <int CAP, class D>
__device__ __forceinline__ void row_append(unsigned long long *buf, uint32_t *cnt, int row, bool pass, unsigned long long mask,
                                           D dist, uint32_t col, int m, int kk)
{
    const uint32_t half = kk ? (uint32_t)(mask >> 32) : (uint32_t)mask;
    const uint32_t base = cnt[row];
    if (pass)
        buf[(size_t)row * CAP + base + __popc(half & ((1u << m) - 1u))] = ((unsigned long long)key_hi(dist) << 32) | col;
    if (m == 0 && half)
        cnt[row] = base + __popc(half);
}

// rank of up to NK keys per lane among the n keys of a row buffer (the number of smaller keys: all distinct), the k
// smallest written to dst in order
template <int NK>
__device__ __forceinline__ void rank_row(const unsigned long long *rb, int n, int k, int lane, unsigned long long *dst,
                                         bool in_place)
{
    unsigned long long key[NK];
    int rk[NK];
#pragma unroll
    for (int u = 0; u < NK; u++) {
        key[u] = lane + 64 * u < n ? rb[lane + 64 * u] : kSweepKeyNone;
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

// rows that could overflow in the next tile (32 more entries at most): keep their k smallest
template <int CAP, class T>
__device__ __forceinline__ void rows_compact(unsigned long long *buf, uint32_t *cnt, T *thr_s, int k, int lane)
{
    __builtin_amdgcn_wave_barrier();
    unsigned long long need = __ballot(lane < 32 && cnt[lane] > (uint32_t)(CAP - 32));
    while (need) {
        const int row = __ffsll((long long)need) - 1;
        need &= need - 1;
        const int n = (int)cnt[row];
        unsigned long long *rb = buf + (size_t)row * CAP;
        rank_row<(CAP + 63) / 64>(rb, n, k, lane, rb, true);
        if (lane == 0)
            cnt[row] = (uint32_t)min(n, k);
        __builtin_amdgcn_wave_barrier();
        if (lane == 0 && n >= k)
            key_threshold((uint32_t)(rb[k - 1] >> 32), thr_s[row]);
    }
    __builtin_amdgcn_wave_barrier();
}

// final order of the wave's first nrows rows (the others are beyond nq), then out: row i to out[(first + i) * k ..],
// k keys ascending, kSweepKeyNone beyond what was found
template <int CAP>
__device__ __forceinline__ void rows_write_out(const unsigned long long *buf, const uint32_t *cnt, int k, int lane, int nrows,
                                               unsigned long long *out, size_t first)
{
    __builtin_amdgcn_wave_barrier();
    for (int row = 0; row < min(nrows, 32); row++) {
        const int n = (int)cnt[row];
        unsigned long long *o = out + (first + row) * (size_t)k;
        rank_row<(CAP + 63) / 64>(buf + (size_t)row * CAP, n, k, lane, o, false);
        for (int i = n + lane; i < k; i += 64)
            o[i] = kSweepKeyNone;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The int8 strip.  A wave owns 32 query rows for the whole sweep (operand A: NS = ceil(d / 32) steps of 16 bytes per
// lane, in registers) and takes the columns 32 at a time.  Lane l loads bytes [32 s + 16 (l >> 5), + 16) of row
// c0 + (l & 31) for step s straight from the store -- the row norm comes from the same registers (v_dot4_i32_i8), so
// nothing is staged in LDS and the waves never meet at a barrier; the next tile's loads are in flight behind the
// current tile's MFMAs.  Rows are [.][d] bytes, 16-byte aligned, d % 16 == 0.

__device__ __forceinline__ int i8_sq4(const i32x4 &w, int acc)
{
    acc = __builtin_amdgcn_sdot4(w.x, w.x, acc, false);
    acc = __builtin_amdgcn_sdot4(w.y, w.y, acc, false);
    acc = __builtin_amdgcn_sdot4(w.z, w.z, acc, false);
    return __builtin_amdgcn_sdot4(w.w, w.w, acc, false);
}

// dist < thr  <=>  2 dot - |x'|^2 > |q'|^2 - thr = gate: what a tile costs per accumulator register when nothing passes
__device__ __forceinline__ bool i8_gate_pass(int acc_r, int xn, int gate_r) { return (acc_r << 1) - xn > gate_r; }

template <int NS> struct I8Strip {
    i32x4 a[NS], cur[NS], nxt[NS]; // operand A; the tile being multiplied; the raw bytes of the tile in flight
    int qn_r[16];                  // |q'|^2 of the 16 rows whose dot products this lane holds (mfma32_row)
    int m, kk;
    bool tail_in;

    // the 16 bytes of step s this lane owns.  Only the upper half of the last step can lie at or beyond byte d of the row
    // (d % 32 == 16): there the lane reads the row's first piece again, without a branch, and to_i8 replaces it by zeros
    // -- the upper half of the last step is zero in both operands and is never read (it would lie in the next row, or
    // past the store's end).
    __device__ __forceinline__ void load_row(const uint8_t *row, i32x4 (&w)[NS]) const
    {
#pragma unroll
        for (int s = 0; s < NS; s++)
            w[s] = *reinterpret_cast<const i32x4 *>(row + (s < NS - 1 || tail_in ? 32 * s + 16 * kk : 0));
    }
    // The XOR to i8 waits until the bytes are used, so that a tile's loads stay in flight behind the tile before it.
    __device__ __forceinline__ void to_i8(const i32x4 (&raw)[NS], i32x4 (&w)[NS]) const
    {
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const i32x4 zero = {0, 0, 0, 0};
            w[s] = s < NS - 1 || tail_in ? raw[s] ^ (int)0x80808080 : zero;
        }
    }

    // operand A and the norms of the wave's 32 query rows [r0, r0 + 32) of Qp [nq][d] (rows beyond nq repeat the last)
    __device__ __forceinline__ void setup(const uint8_t *Qp, int r0, int lane, int nq, int d)
    {
        m = lane & 31, kk = lane >> 5;
        tail_in = 32 * (NS - 1) + 16 * kk < d;
        load_row(Qp + (size_t)min(r0 + m, nq - 1) * d, nxt);
        to_i8(nxt, a);
        int qn = 0;
#pragma unroll
        for (int s = 0; s < NS; s++)
            qn = i8_sq4(a[s], qn);
        qn += __shfl_xor(qn, 32);
#pragma unroll
        for (int r = 0; r < 16; r++)
            qn_r[r] = __shfl(qn, mfma32_row(r, kk));
    }

    // start the loads of the tile whose first column is c0, of the split's columns [c_begin, c_end) of X [.][d]:
    // a column at or beyond c_end is not read (the lane reads the split's first row and drops it)
    __device__ __forceinline__ void fetch(const uint8_t *X, size_t c0, size_t c_begin, size_t c_end, int d)
    {
        const size_t c = c0 + m;
        fetch_row(X, c < c_end ? c : c_begin, d);
    }
    // ... of the tile in which this lane's column is row `row` of X (a gathered tile: ColCursor below)
    __device__ __forceinline__ void fetch_row(const uint8_t *X, size_t row, int d) { load_row(X + row * (size_t)d, nxt); }
    // the fetched tile becomes the current one; call before the next fetch
    __device__ __forceinline__ void take() { to_i8(nxt, cur); }

    // the current tile: acc[r] = q'.x' of row mfma32_row(r, kk) and the lane's column, xn = |x'|^2 of that column
    __device__ __forceinline__ void product(i32x16 &acc, int &xn) const
    {
        acc = i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        xn = 0;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], cur[s], acc, 0, 0, 0);
            xn = i8_sq4(cur[s], xn);
        }
        xn += __shfl_xor(xn, 32);
    }
    // does any of the lane's 16 distances pass its row's gate
    __device__ __forceinline__ bool any_pass(const i32x16 &acc, int xn, const int (&gate)[16]) const
    {
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; r++)
            any |= i8_gate_pass(acc[r], xn, gate[r]); // all terms far inside int32
        return any;
    }
    __device__ __forceinline__ int dist(const i32x16 &acc, int xn, int r) const { return qn_r[r] + xn - 2 * acc[r]; }
};

// ---------------------------------------------------------------------------------------------------------------------
// Column maps of the int8 sweeps: which store row a column of the sweep is, and which tiles of a split are
// visited at all.  A kernel takes the map as a template parameter and its last argument.
//   ColsDense     column c is row c, every tile is visited: the unfiltered sweep.
//   ColsMasked    column c is row c; words[w] has one pass bit per row of [32 w, 32 w + 32), bits at or beyond the store's
//                 end zero.  Splits begin at multiples of 32, so tile t of a split is word (c_begin >> 5) + t: a tile
//                 whose word is zero is neither fetched nor multiplied, in any other a lane counts only if its bit is set.
//   ColsIndirect  the sweep runs over the columns [0, npass) of rows[], the passing row numbers ascending: column c is
//                 row rows[c], which is also the label.  Ascending, so column order is still label order.
// Under a strip plan (base filter slots) the three take their words or rows and their nx per 32-row strip
// from the strip's table entry instead of the kernel's arguments: ColsStrips<map>, below.
struct ColsDense {
    static constexpr bool kMasked = false, kIndirect = false, kStrips = false, kWindowed = false;
    using Base = ColsDense;
    __device__ __forceinline__ void take(const uint32_t *) {}
};
struct ColsMasked {
    static constexpr bool kMasked = true, kIndirect = false, kStrips = false, kWindowed = false;
    using Base = ColsMasked;
    const uint32_t *words;
    __device__ __forceinline__ void take(const uint32_t *data) { words = data; }
};
struct ColsIndirect {
    static constexpr bool kMasked = false, kIndirect = true, kStrips = false, kWindowed = false;
    using Base = ColsIndirect;
    const uint32_t *rows;
    __device__ __forceinline__ void take(const uint32_t *data) { rows = data; }
};

// A column map per 32-row strip.  The launch of form B covers the strips [range[B][0], range[B][1]) of the chunk's plan
// (sweep_plan_math.h StripPlan): the wave whose strip of the launch is i owns strip range[B][0] + i, reads that strip's
// table entry once -- everything in it is wave-uniform -- and sweeps the entry's columns under B.  The rows of the strip
// are rows [32 strip, + 32) of the gathered queries; strip_rows says which of the call's queries each is.
// OWN: the strip's entry is its own, strip_cols[strip] (base tags, DESIGN.md 3.22: one bucket per tag among the chunk's
// queries, far more than a table of slots holds); else it is the slot table's, table[strip_slot[strip]].
// WIN (base values; Indirect, own entries): the strip's columns are a span of the holder's rows in (value,
// row) order that covers the windows of all its rows, and every strip row counts only the columns of ITS OWN window
// win[32 strip + row], relative to the span (RowWindows, below).  Columns then arrive in (value, row) order, not in label
// order: the k-search admits ties at the k-th distance (kTie) and the range results are put in label order afterwards.
template <class B, bool OWN = false, bool WIN = false> struct ColsStrips {
    static constexpr bool kMasked = B::kMasked, kIndirect = B::kIndirect, kStrips = true, kOwnEntries = OWN, kWindowed = false;
    using Base = B;
    StripPlan sp;
};
template <class B> struct ColsStrips<B, true, true> {
    static_assert(B::kIndirect, "a windowed strip sweeps a span of the holder's row order");
    static constexpr bool kMasked = false, kIndirect = true, kStrips = true, kOwnEntries = true, kWindowed = true;
    using Base = B;
    StripPlan sp;
    const StripWin *win;
};

// What the wave whose first row is r0 sweeps in split `split` of nsplit: the map, the first row and the columns
// [c_begin, c_end).  Without strips they are the kernel's own (cps = its columns per split); with strips r0 counts the
// launch's strips and everything comes from the strip's table entry -- false: the launch has no such strip, the wave exits
// (no barrier anywhere in these kernels).
template <class CM>
__device__ __forceinline__ bool strip_open(const CM &cm, int nsplit, int split, size_t nx, size_t cps, int &r0, size_t &c_begin,
                                           size_t &c_end, typename CM::Base &base)
{
    if constexpr (!CM::kStrips) {
        base = cm;
        c_begin = (size_t)split * cps < nx ? (size_t)split * cps : nx;
        c_end = c_begin + cps < nx ? c_begin + cps : nx;
        return true;
    } else {
        constexpr int f = CM::kMasked ? kSweepColsMasked : CM::kIndirect ? kSweepColsIndirect : kSweepColsDense;
        const uint32_t strip = __builtin_amdgcn_readfirstlane(cm.sp.hdr->lay.range[f][0] + (uint32_t)(r0 >> 5));
        if (strip >= cm.sp.hdr->lay.range[f][1])
            return false;
        StripCols e;
        if constexpr (CM::kOwnEntries)
            e = cm.sp.strip_cols[strip];
        else
            e = cm.sp.table[cm.sp.strip_slot[strip]];
        base.take(e.data);
        sweep_split_cut(e.nx, nsplit, split, &c_begin, &c_end);
        r0 = (int)(strip << 5);
        return true;
    }
}
// Is row `row` of the wave's strip a query (not: beyond nq; a padding row), and *qi = which of the call's, the chunk being
// queries [q_off, ...) of the call
template <class CM> __device__ __forceinline__ bool strip_row_query(const CM &cm, int r0, int row, int nq, size_t q_off, size_t *qi)
{
    if constexpr (CM::kStrips) {
        const int q = cm.sp.strip_rows[r0 + row];
        *qi = q_off + (size_t)max(q, 0);
        return q >= 0;
    } else {
        *qi = q_off + r0 + row;
        return r0 + row < nq;
    }
}

// The windows of a wave's 32 strip rows under a windowed map, two registers a lane: lanes m and m + 32 hold row m's window
// [wa, wb) in the strip's columns.  Per tile of columns [c0, c0 + 32) one ballot gives `live`, bit m = row m's window
// meets the tile -- wave-uniform, so a tile no window meets (the gap between two windows of a strip) is dropped before it
// is multiplied, and the tile's cheap test counts a row only where its bit is set; the exact test, column by column, is
// made behind the cheap test, where a row's window is read from its lane.  A row whose window is empty -- the padding rows
// of a strip that is not full -- never counts: gate_of() gives it a gate nothing passes, for good.  A tile inside the
// window of every row that has one (all == true) then takes the unwindowed cheap test.  Without kWindowed nothing here is
// live.
template <class CM> struct RowWindows {
    uint32_t wa = 0, wb = 0; // the window of row lane & 31
    uint32_t lv = 0;         // the live bits of the rows this lane holds: bit (r & 3) + 8 (r >> 2) = accumulator register r
    uint32_t dead = 0;       // ... and, in the same places, the rows whose window is empty
    uint32_t empty = 0;      // bit m = row m's window is empty (wave-uniform)
    bool all = true;

    __device__ __forceinline__ void setup(const CM &cm, int r0, int lane)
    {
        if constexpr (CM::kWindowed) {
            const StripWin w = cm.win[r0 + (lane & 31)];
            wa = w.a;
            wb = w.b;
            empty = (uint32_t)__ballot(wa >= wb);
            dead = empty >> (4 * (lane >> 5));
        }
    }
    // the gate of accumulator register r's row: g, or for a row without a window one that no distance passes
    __device__ __forceinline__ int gate_of(int r, int g) const
    {
        if constexpr (CM::kWindowed)
            return (dead >> ((r & 3) + 8 * (r >> 2))) & 1u ? 0x7fffffff : g;
        else
            return g;
    }
    // false: no row of the wave counts any column of the tile
    __device__ __forceinline__ bool tile(size_t c0, int kk)
    {
        if constexpr (CM::kWindowed) {
            const uint32_t t0 = (uint32_t)c0;
            const bool meets = wa < t0 + 32u && wb > t0; // (an empty window meets nothing; columns are below 2^32 - 32)
            const uint32_t live = (uint32_t)__ballot(meets);
            all = ((uint32_t)__ballot(wa <= t0 && wb >= t0 + 32u) | empty) == 0xffffffffu;
            lv = live >> (4 * kk);
            return live != 0u;
        } else {
            return true;
        }
    }
    // the cheap test of a tile: does any of the lane's 16 distances pass its row's gate, in a row whose window meets the tile
    template <int NS> __device__ __forceinline__ bool any_pass(const I8Strip<NS> &st, const i32x16 &acc, int xn, const int (&gate)[16]) const
    {
        if constexpr (CM::kWindowed) {
            if (all)
                return st.any_pass(acc, xn, gate);
            uint32_t any = 0;
#pragma unroll
            for (int r = 0; r < 16; r++)
                any |= i8_gate_pass(acc[r], xn, gate[r]) ? 1u << ((r & 3) + 8 * (r >> 2)) : 0u;
            return (any & lv) != 0u;
        } else {
            return st.any_pass(acc, xn, gate);
        }
    }
    // the exact test: does accumulator register r's row count column col
    __device__ __forceinline__ bool row_counts(int r, int kk, size_t col) const
    {
        if constexpr (CM::kWindowed) {
            const int row = mfma32_row(r, kk);
            const uint32_t a = __shfl(wa, row), b = __shfl(wb, row);
            return (uint32_t)col >= a && (uint32_t)col < b;
        } else {
            return true;
        }
    }
};

// A wave's place in its split's columns [c_begin, c_end) under a column map.  Everything below is wave-uniform except
// the row numbers; the members a map does not use are never live.
//   Masked: lane i holds the pass word of tile tbase + i (zero at or beyond ntiles), one load per 64 tiles; next() finds
//   the next tile with a set bit by a ballot and leaves its word in `word`.
//   Indirect: the row numbers of the lane's column are fetched one tile further ahead than the rows, so that the row
//   loads go out without waiting for them: `cur` belongs to the tile being multiplied (the label), `nxt` to the tile
//   whose rows are in flight, `ahead` to the one after it.  A lane at or beyond c_end takes the row of c_begin.
template <class CM> struct ColCursor {
    const uint32_t *p = nullptr; // Masked: the word of the split's tile 0; Indirect: the list
    size_t c_begin = 0, c_end = 0;
    uint32_t ntiles = 0;
    uint32_t tbase = 0, win = 0, word = 0;
    uint32_t cur = 0, nxt = 0, ahead = 0;
    int lane = 0;

    __device__ __forceinline__ void setup(const CM &cm, size_t c_begin_, size_t c_end_, uint32_t ntiles_, int lane_)
    {
        if constexpr (CM::kMasked) {
            lane = lane_;
            ntiles = ntiles_;
            c_begin = c_begin_;
            p = cm.words + (c_begin_ >> 5);
            win = (uint32_t)lane < ntiles ? p[lane] : 0u;
        }
        if constexpr (CM::kIndirect) {
            lane = lane_;
            c_begin = c_begin_;
            c_end = c_end_;
            p = cm.rows;
        }
    }
    // Masked: the first tile at or after t with a passing row (ntiles: none), its word left in `word`; else t itself
    __device__ __forceinline__ uint32_t next(uint32_t t, uint32_t ntiles_)
    {
        if constexpr (!CM::kMasked) {
            return t < ntiles_ ? t : ntiles_;
        } else {
            while (t < ntiles) {
                if (t - tbase >= 64u) {
                    tbase = t;
                    win = t + (uint32_t)lane < ntiles ? p[t + lane] : 0u;
                }
                const unsigned long long nz = __ballot(win != 0u) >> (t - tbase);
                if (nz) {
                    const uint32_t i = __builtin_amdgcn_readfirstlane(t - tbase + (uint32_t)__ffsll((long long)nz) - 1u);
                    word = __builtin_amdgcn_readlane(win, i);
                    return tbase + i;
                }
                t = tbase + 64u;
            }
            return ntiles;
        }
    }
    // the same in columns: the first column of the first tile at or after the one that begins at column c0 (c0 - c_begin a
    // multiple of 32) that is visited; at or beyond c_end: none
    __device__ __forceinline__ size_t next_col(size_t c0)
    {
        if constexpr (!CM::kMasked)
            return c0;
        else
            return c_begin + ((size_t)next((uint32_t)((c0 - c_begin) >> 5), ntiles) << 5);
    }
    // does the lane's column m of the tile next() returned last pass
    __device__ __forceinline__ bool lane_pass(int m) const
    {
        if constexpr (CM::kMasked)
            return (word >> m) & 1u;
        else
            return true;
    }
    // Indirect: start the load of the row numbers of the tile that begins at column c0 (c0 < c_end)
    __device__ __forceinline__ void ids(size_t c0)
    {
        if constexpr (CM::kIndirect) {
            const size_t c = c0 + (lane & 31);
            ahead = p[c < c_end ? c : c_begin];
        }
    }
    // Indirect: the row numbers move up one tile; call with the strip's take(), and once before the first fetch
    __device__ __forceinline__ void shift()
    {
        if constexpr (CM::kIndirect) {
            cur = nxt;
            nxt = ahead;
        }
    }
    // start the row loads of the tile that begins at column c0 of the split [cb, ce) (Indirect: its ids() and a shift()
    // came before)
    template <int NS>
    __device__ __forceinline__ void fetch(I8Strip<NS> &st, const uint8_t *X, size_t c0, size_t cb, size_t ce, int d) const
    {
        if constexpr (CM::kIndirect)
            st.fetch_row(X, nxt, d);
        else
            st.fetch(X, c0, cb, ce, d);
    }
    // the label of the lane's column col of the tile being multiplied
    __device__ __forceinline__ size_t label(size_t col) const
    {
        if constexpr (CM::kIndirect)
            return cur;
        else
            return col;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The merge of a split call, one wavefront per query: the k smallest of the splits' sorted partial tables part
// [nsplit][nq][k] (keys distinct: the low words differ).  A key's rank is the number of keys below it, summed over the
// tables; put(slot, key) stores a result, pad(slot) fills a slot nothing reached.
// sweep_merge_row: the same for the tables' row q whose results are the caller's row q_out (a strip plan's rows are not in
// the caller's order).
template <class Put, class Pad>
__device__ __forceinline__ void sweep_merge_row(const unsigned long long *__restrict__ part, int nsplit, int nq, int k, int q,
                                                int q_out, Put put, Pad pad)
{
    const int lane = threadIdx.x;
    const int total = nsplit * k;
    int found = 0;
    for (int i = lane; i < total; i += 64) {
        const int s = i / k, j = i - s * k;
        const unsigned long long key = part[((size_t)s * nq + q) * k + j];
        if (key == kSweepKeyNone)
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
        if (rank < k)
            put((size_t)q_out * k + rank, key);
    }
    // slots nothing reached: fewer than k candidates exist
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        found += __shfl_xor(found, o);
    for (int i = min(found, k) + lane; i < k; i += 64)
        pad((size_t)q_out * k + i);
}
template <class Put, class Pad>
__device__ __forceinline__ void sweep_merge(const unsigned long long *__restrict__ part, int nsplit, int nq, int k, Put put,
                                            Pad pad)
{
    sweep_merge_row(part, nsplit, nq, k, (int)blockIdx.x, (int)blockIdx.x, put, pad);
}

} // namespace ivfhnsw_gpu_impl
