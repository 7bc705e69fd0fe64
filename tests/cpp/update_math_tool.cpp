// Host check of csrc/update_math.h (tests/test_update_math_cpu.py builds it with the address and undefined-behaviour
// sanitizers): the 16-byte group copy against a plain serial copy (every head, several row widths, holes), whole updates
// -- IVFADC append, Grouping append, removal -- emulated tile by tile with the shared functions at tiles of 8 and of 2048
// rows against the naive result, list_of_row over runs of empty lists, and the workspace sizes against the largest index
// the emulation touches.  Includes nothing else of the library; exit status 0 = every check held.
#include "update_math.h"

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

using namespace ivfhnsw_gpu_impl;
typedef unsigned long long u64;
typedef std::vector<uint32_t> vec;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                printf("FAIL: " __VA_ARGS__); \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

// ---- the memory of copy_group_dwords / copy_group_bytes on the host: bounds-checked by the sanitizer (the vectors are
// exactly as long as the arrays), every store counted
template <class T> struct Mem {
    const std::vector<T> *src;
    std::vector<T> *dst;
    std::vector<int> *writes; // per destination element
    size_t dbase;             // index of group 0's first element; may lie up to 3 in front of the range
    std::vector<size_t> *runs; // groups that took the 16-byte load
    uint32_t load(size_t s) const { return (*src)[s]; }
    void load4(size_t s, uint32_t v[4]) const
    {
        for (int u = 0; u < 4; u++)
            v[u] = (*src)[s + u];
        runs->push_back(s);
    }
    void put(size_t d, T x) const
    {
        (*dst)[dbase + d] = x;
        (*writes)[dbase + d]++;
    }
    void store(size_t d, T x) const { put(d, x); }
    void store4(size_t d, const uint32_t v[4]) const // dwords
    {
        CHECK((dbase + d) % 4 == 0, "16-byte store at dword %zu", dbase + d);
        for (int u = 0; u < 4; u++)
            put(d + u, (T)v[u]);
    }
    void store4(size_t d, uint32_t w) const // bytes
    {
        CHECK((dbase + d) % 4 == 0, "dword store at byte %zu", dbase + d);
        for (int u = 0; u < 4; u++)
            put(d + u, (T)(w >> (8 * u)));
    }
};

// rows [0, rows) of q dwords to dst dwords [d0, d0 + rows * q) of an array of `len`, with the shared group copy; returns
// the number of 16-byte loads.  writes counts every store.
template <bool ALIGNED>
static size_t tile_copy_dwords(const vec &src, vec &dst, std::vector<int> &writes, const uint32_t *s_src, uint32_t rows, uint32_t q, u64 d0)
{
    std::vector<size_t> runs;
    const uint32_t ndw = rows * q, head = group_head<ALIGNED>(d0), ng = group_count(head, ndw);
    const Mem<uint32_t> m{&src, &dst, &writes, (size_t)(d0 - head), &runs};
    for (uint32_t gi = 0; gi < ng; gi++)
        copy_group_dwords<ALIGNED>(m, s_src, gi, head, ndw, q);
    return runs.size();
}
template <bool ALIGNED>
static void tile_copy_bytes(const std::vector<uint8_t> &src, std::vector<uint8_t> &dst, std::vector<int> &writes, const uint32_t *s_src,
                            uint32_t rows, u64 d0)
{
    const uint32_t head = group_head<ALIGNED>(d0), ng = group_count(head, rows);
    const Mem<uint8_t> m{&src, &dst, &writes, (size_t)(d0 - head), nullptr};
    for (uint32_t gi = 0; gi < ng; gi++)
        copy_group_bytes<ALIGNED>(m, s_src, gi, head, rows);
}

// ---- 1. the group decomposition against the serial copy
static void check_groups()
{
    const uint32_t qs[] = {1, 2, 3, 4, 7, 8};
    const uint32_t nsrc_rows = 100;
    for (uint32_t head = 0; head < 4; head++)
        for (uint32_t q : qs)
            for (uint32_t rows = 0; rows <= 40; rows++)
                for (int holes = 0; holes < 5; holes++)     // none, all, alternating, first only, last only
                    for (int layout = 0; layout < 3; layout++) { // sources consecutive, every other row, runs of five
                        vec s_src(rows); // exactly the tile's rows: the sanitizer sees a read of row `rows`
                        for (uint32_t j = 0; j < rows; j++) {
                            const bool hole = holes == 1 || (holes == 2 && (j & 1)) || (holes == 3 && j == 0) ||
                                              (holes == 4 && j + 1 == rows);
                            const uint32_t r = layout == 0 ? 3 + j : layout == 1 ? 2 * j + 1 : j + 7 * (j / 5);
                            s_src[j] = hole ? kSkip : r;
                        }
                        vec src(nsrc_rows * q);
                        for (size_t i = 0; i < src.size(); i++)
                            src[i] = 0x10000u + (uint32_t)i;
                        const u64 d0 = 8 + head; // the range starts at dword d0 of dst; dst ends with the range's last group
                        const uint32_t ndw = rows * q;
                        vec dst(d0 + ndw + 5, 0xdeadbeefu);
                        std::vector<int> writes(dst.size(), 0);
                        const size_t runs = head == 0 ? tile_copy_dwords<true>(src, dst, writes, s_src.data(), rows, q, d0)
                                                      : tile_copy_dwords<false>(src, dst, writes, s_src.data(), rows, q, d0);
                        size_t want_runs = 0;
                        for (size_t i = 0; i < dst.size(); i++) {
                            const bool in = i >= d0 && i < d0 + ndw;
                            CHECK(writes[i] == (in ? 1 : 0), "dwords head %u q %u rows %u holes %d: dword %zu written %d times",
                                  head, q, rows, holes, i, writes[i]);
                            if (!in)
                                continue;
                            const uint32_t e = (uint32_t)(i - d0), j = e / q, k = e % q;
                            const uint32_t want = s_src[j] == kSkip ? 0u : src[(size_t)s_src[j] * q + k];
                            CHECK(dst[i] == want, "dwords head %u q %u rows %u holes %d layout %d: element %u = %x, want %x", head, q,
                                  rows, holes, layout, e, dst[i], want);
                        }
                        // the 16-byte load: exactly the whole aligned groups whose four sources are present and consecutive
                        for (u64 g = (d0 + 3) / 4 * 4; g + 4 <= d0 + ndw; g += 4) {
                            bool run = true;
                            size_t first = 0;
                            for (int u = 0; u < 4; u++) {
                                const uint32_t e = (uint32_t)(g + u - d0), j = e / q, k = e % q;
                                const size_t s = (size_t)s_src[j] * q + k;
                                if (u == 0)
                                    first = s;
                                run = run && s_src[j] != kSkip && s == first + u;
                            }
                            want_runs += run;
                        }
                        CHECK(runs == want_runs, "dwords head %u q %u rows %u holes %d layout %d: %zu 16-byte loads, want %zu", head,
                              q, rows, holes, layout, runs, want_runs);
                        if (q != 1)
                            continue;
                        // the byte form: norm codes of the same rows
                        std::vector<uint8_t> bsrc(nsrc_rows * 8), bdst(d0 + rows + 5, 0xee);
                        for (size_t i = 0; i < bsrc.size(); i++)
                            bsrc[i] = (uint8_t)(i * 7 + 1);
                        std::vector<int> bw(bdst.size(), 0);
                        if (head == 0)
                            tile_copy_bytes<true>(bsrc, bdst, bw, s_src.data(), rows, d0);
                        else
                            tile_copy_bytes<false>(bsrc, bdst, bw, s_src.data(), rows, d0);
                        for (size_t i = 0; i < bdst.size(); i++) {
                            const bool in = i >= d0 && i < d0 + rows;
                            CHECK(bw[i] == (in ? 1 : 0), "bytes head %u rows %u holes %d: byte %zu written %d times", head, rows, holes,
                                  i, bw[i]);
                            if (in) {
                                const uint32_t sr = s_src[i - d0];
                                CHECK(bdst[i] == (sr == kSkip ? 0 : bsrc[sr]), "bytes head %u rows %u holes %d: byte %zu", head, rows,
                                      holes, i);
                            }
                        }
                    }
}

// ---- 2. whole updates.  An index: lists in CSR form, every row q dwords of code, an id and a norm code
struct Lists {
    std::vector<u64> goff;  // [nc + 1] global offsets
    vec loff;               // [nc] local offsets, kNotOwned = the list lives on another shard
    vec codes, ids;         // local rows
    std::vector<uint8_t> ncodes;
    uint32_t q;
    size_t n_local() const { return ids.size(); }
};
constexpr uint32_t kNotOwnedList = 0xffffffffu; // ivfhnsw_kernels.h's kNotOwned

static vec excl_scan(const vec &v) // [len] -> [len], the last slot = the total of the others when it holds 0
{
    vec out(v.size());
    uint32_t run = 0;
    for (size_t i = 0; i < v.size(); i++) {
        out[i] = run;
        run += v[i];
    }
    return out;
}

struct Batch {
    vec list, sub, ids, codes; // sub empty: IVFADC
    std::vector<uint8_t> ncodes;
};

// The append as the kernels run it, tile by tile of T rows: count, lens, scans, offsets, tile_first, merge, scatter.
// sizes: [nc * nsubc] sub-group sizes (Grouping), replaced by the new ones.  cached / searched count the tiles on either
// side of the prefix-cache limit.
static Lists emulate_append(const Lists &L, const Batch &b, uint32_t T, uint32_t nsubc, vec *sizes, int *cached, int *searched)
{
    const uint32_t nc = (uint32_t)L.loff.size(), q = L.q;
    const size_t n = b.list.size();
    const bool grouping = nsubc != 0;
    vec cnt(nc + 1, 0), own(nc + 1, 0), sizes2;
    if (grouping)
        sizes2 = *sizes;
    for (size_t i = 0; i < n; i++) {
        cnt[b.list[i]]++;
        if (grouping)
            sizes2[(size_t)b.list[i] * nsubc + b.sub[i]]++;
    }
    for (uint32_t c = 0; c < nc; c++)
        own[c] = L.loff[c] != kNotOwnedList ? (uint32_t)(L.goff[c + 1] - L.goff[c]) + cnt[c] : 0u;
    const vec nstart = excl_scan(cnt), lstart = excl_scan(own);
    Lists N;
    N.q = q;
    N.goff.resize(nc + 1);
    N.loff.resize(nc);
    for (uint32_t c = 0; c <= nc; c++) {
        N.goff[c] = L.goff[c] + nstart[c];
        if (c < nc)
            N.loff[c] = L.loff[c] == kNotOwnedList ? kNotOwnedList : lstart[c];
    }
    const uint32_t n_local2 = lstart[nc];
    N.codes.assign((size_t)n_local2 * q, 0xabababab);
    N.ids.assign(n_local2, 0xabababab);
    N.ncodes.assign(n_local2, 0xab);
    std::vector<int> wc(N.codes.size(), 0), wi(n_local2, 0), wn(n_local2, 0);
    // prefix sums of the touched lists
    vec pre_old, pre_new;
    if (grouping) {
        pre_old.assign((size_t)nc * nsubc, 0xcdcdcdcd);
        pre_new.assign((size_t)nc * nsubc, 0xcdcdcdcd);
        for (uint32_t c = 0; c < nc; c++) {
            if (nstart[c + 1] == nstart[c])
                continue;
            uint32_t ro = 0, rn = 0;
            for (uint32_t s = 0; s < nsubc; s++) {
                pre_old[(size_t)c * nsubc + s] = ro;
                pre_new[(size_t)c * nsubc + s] = rn;
                ro += (*sizes)[(size_t)c * nsubc + s];
                rn += sizes2[(size_t)c * nsubc + s];
            }
        }
    }
    const uint32_t ntiles = (uint32_t)update_tiles(n_local2, T);
    vec tile_first(append_tile_words(n_local2, T), 0);
    CHECK((size_t)ntiles + 1 <= tile_first.size(), "append T %u: tile_first[%u] touched, %zu words sized", T, ntiles, tile_first.size());
    for (uint32_t t = 0; n_local2 && t <= ntiles; t++)
        tile_first[t] = t == ntiles ? nc - 1 : list_of_row(lstart.data(), 0u, nc - 1, t * T);
    for (uint32_t t = 0; t < ntiles; t++) {
        const uint32_t r0 = t * T, rows = std::min(T, n_local2 - r0), lo = tile_first[t], hi = tile_first[t + 1];
        vec s_src(rows), s_pn(kPrefixCache, 0xefefefef), s_po(kPrefixCache, 0xefefefef);
        const uint32_t cw = grouping ? prefix_cache_words(lo, hi, nsubc) : 0u;
        for (uint32_t w = 0; w < cw; w++) {
            const uint32_t c = lo + w / nsubc;
            if (nstart[c + 1] != nstart[c]) {
                s_pn[w] = pre_new[(size_t)c * nsubc + w % nsubc];
                s_po[w] = pre_old[(size_t)c * nsubc + w % nsubc];
            }
        }
        if (grouping)
            (cw ? *cached : *searched)++;
        for (uint32_t j = 0; j < rows; j++) {
            const uint32_t r = r0 + j, c = list_of_row(lstart.data(), lo, hi, r), off = r - lstart[c];
            const uint32_t old_len = (uint32_t)(L.goff[c + 1] - L.goff[c]);
            if (!grouping || nstart[c + 1] == nstart[c])
                s_src[j] = list_source(off, old_len, L.loff[c]);
            else if (cw)
                s_src[j] = grouping_source(s_pn.data() + (c - lo) * nsubc, s_po.data() + (c - lo) * nsubc, nsubc, off, old_len, L.loff[c]);
            else
                s_src[j] = grouping_source(pre_new.data() + (size_t)c * nsubc, pre_old.data() + (size_t)c * nsubc, nsubc, off, old_len,
                                           L.loff[c]);
        }
        CHECK(((u64)r0 * q) % 4 == 0 || T % 4, "tile %u is not 16-byte aligned", t);
        if (T % 4 == 0) { // the merge's compile-time fact
            tile_copy_dwords<true>(L.codes, N.codes, wc, s_src.data(), rows, q, (u64)r0 * q);
            tile_copy_dwords<true>(L.ids, N.ids, wi, s_src.data(), rows, 1, r0);
            tile_copy_bytes<true>(L.ncodes, N.ncodes, wn, s_src.data(), rows, r0);
        }
    }
    for (size_t i = 0; i < wi.size(); i++)
        CHECK(wi[i] == 1 && wn[i] == 1, "append T %u: row %zu written %d / %d times by the merge", T, i, wi[i], wn[i]);
    for (size_t i = 0; i < wc.size(); i++)
        CHECK(wc[i] == 1, "append T %u: code dword %zu written %d times by the merge", T, i, wc[i]);
    // scatter: the batch sorted stably by (list, sub-group)
    std::vector<size_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](size_t x, size_t y) {
        if (b.list[x] != b.list[y])
            return b.list[x] < b.list[y];
        return grouping && b.sub[x] < b.sub[y];
    });
    for (size_t p = 0; p < n; p++) {
        const size_t i = perm[p];
        const uint32_t c = b.list[i];
        if (L.loff[c] == kNotOwnedList)
            continue;
        size_t row;
        if (grouping) {
            const size_t cs = (size_t)c * nsubc + b.sub[i];
            row = grouping_dest_row(lstart[c], pre_old[cs], (*sizes)[cs], p, nstart[c]);
        } else {
            row = append_dest_row(lstart[c], (uint32_t)(L.goff[c + 1] - L.goff[c]), p, nstart[c]);
        }
        CHECK(row < n_local2 && N.ids[row] == 0 && N.ncodes[row] == 0, "append T %u: batch row %zu lands on row %zu, not a hole", T, i, row);
        if (row >= n_local2)
            continue;
        for (uint32_t k = 0; k < q; k++)
            N.codes[row * q + k] = b.codes[i * q + k];
        N.ids[row] = b.ids[i];
        N.ncodes[row] = b.ncodes[i];
    }
    if (grouping)
        *sizes = sizes2;
    return N;
}

// the naive append: every owned list's old rows (Grouping: sub-group by sub-group) and its batch rows in arrival order
static Lists naive_append(const Lists &L, const Batch &b, uint32_t nsubc, const vec *sizes)
{
    const uint32_t nc = (uint32_t)L.loff.size(), q = L.q;
    Lists N;
    N.q = q;
    N.goff.assign(nc + 1, 0);
    N.loff.assign(nc, kNotOwnedList);
    auto push_old = [&](size_t r) {
        N.codes.insert(N.codes.end(), L.codes.begin() + r * q, L.codes.begin() + (r + 1) * q);
        N.ids.push_back(L.ids[r]);
        N.ncodes.push_back(L.ncodes[r]);
    };
    auto push_new = [&](size_t i) {
        N.codes.insert(N.codes.end(), b.codes.begin() + i * q, b.codes.begin() + (i + 1) * q);
        N.ids.push_back(b.ids[i]);
        N.ncodes.push_back(b.ncodes[i]);
    };
    for (uint32_t c = 0; c < nc; c++) {
        u64 len = L.goff[c + 1] - L.goff[c];
        const bool owned = L.loff[c] != kNotOwnedList;
        if (owned)
            N.loff[c] = (uint32_t)N.ids.size();
        if (owned && !nsubc)
            for (u64 r = 0; r < len; r++)
                push_old(L.loff[c] + r);
        size_t at = owned ? L.loff[c] : 0;
        for (uint32_t s = 0; s < std::max(nsubc, 1u); s++) {
            if (owned && nsubc)
                for (uint32_t r = 0; r < (*sizes)[(size_t)c * nsubc + s]; r++)
                    push_old(at++);
            for (size_t i = 0; i < b.list.size(); i++)
                if (b.list[i] == c && (!nsubc || b.sub[i] == s)) {
                    len++;
                    if (owned)
                        push_new(i);
                }
        }
        N.goff[c + 1] = N.goff[c] + len;
    }
    return N;
}

static void check_same(const Lists &a, const Lists &b, const char *what, uint32_t T)
{
    CHECK(a.goff == b.goff, "%s T %u: global offsets differ", what, T);
    CHECK(a.loff == b.loff, "%s T %u: local offsets differ", what, T);
    CHECK(a.ids == b.ids, "%s T %u: ids differ", what, T);
    CHECK(a.ncodes == b.ncodes, "%s T %u: norm codes differ", what, T);
    CHECK(a.codes == b.codes, "%s T %u: codes differ", what, T);
}

static Lists random_lists(std::mt19937 &rng, const vec &lens, uint32_t q, bool some_not_owned)
{
    const uint32_t nc = (uint32_t)lens.size();
    Lists L;
    L.q = q;
    L.goff.assign(nc + 1, 0);
    L.loff.assign(nc, 0);
    for (uint32_t c = 0; c < nc; c++) {
        L.goff[c + 1] = L.goff[c] + lens[c];
        const bool owned = !some_not_owned || c % 3 != 1;
        L.loff[c] = owned ? (uint32_t)L.ids.size() : kNotOwnedList;
        for (uint32_t r = 0; owned && r < lens[c]; r++) {
            L.ids.push_back(rng() | 1u); // never 0: a hole the scatter missed would show
            L.ncodes.push_back((uint8_t)(rng() | 1u));
            for (uint32_t k = 0; k < q; k++)
                L.codes.push_back(rng());
        }
    }
    return L;
}

static Batch random_batch(std::mt19937 &rng, size_t n, uint32_t q, uint32_t nsubc, const std::vector<uint32_t> &targets)
{
    Batch b;
    for (size_t i = 0; i < n; i++) {
        b.list.push_back(targets[rng() % targets.size()]);
        if (nsubc)
            b.sub.push_back(rng() % 3 ? rng() % nsubc : (nsubc - 1) * (rng() & 1)); // the ends often
        b.ids.push_back(rng() | 1u);
        b.ncodes.push_back((uint8_t)(rng() | 1u));
        for (uint32_t k = 0; k < q; k++)
            b.codes.push_back(rng());
    }
    return b;
}

static void check_appends(uint32_t T)
{
    std::mt19937 rng(T * 7919u + 1);
    const uint32_t qs[] = {1, 3, 4, 7};
    for (uint32_t q : qs) {
        // IVFADC: lists of every length around the tile (empty ones at the first, middle and last places), a batch into a
        // third of the lists, then one into the last list only, then one into a handle of empty lists; with and without
        // lists other shards own
        for (int sharded = 0; sharded < 2; sharded++) {
            vec lens = {0, 0, T / 2, 1, 0, 0, T + 3, T - 1, 0, 2 * T + 1, 5, 0};
            Lists L = random_lists(rng, lens, q, sharded);
            const std::vector<uint32_t> cases[] = {{0, 3, 4, 6, 10}, {11}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, {6}};
            for (const auto &targets : cases) {
                const Batch b = random_batch(rng, targets.size() == 1 ? T + 37 : 3 * T / 2 + 5, q, 0, targets);
                int c0 = 0, c1 = 0;
                const Lists N = emulate_append(L, b, T, 0, nullptr, &c0, &c1);
                check_same(N, naive_append(L, b, 0, nullptr), "append", T);
                L = N;
            }
            Lists E = random_lists(rng, vec(5, 0), q, false);
            const Batch b = random_batch(rng, 2 * T + 52, q, 0, {0, 2, 4});
            int c0 = 0, c1 = 0;
            check_same(emulate_append(E, b, T, 0, nullptr, &c0, &c1), naive_append(E, b, 0, nullptr), "append to empty", T);
        }
        // Grouping: nsubc 64 with long lists (few lists per tile: cached) and with short ones (searched), sub-groups of
        // size 0, untouched lists and sub-groups
        int cached = 0, searched = 0;
        for (int shape = 0; shape < 2; shape++) {
            const uint32_t nsubc = 64, nc = shape == 0 ? 4 : 3 * kPrefixCache / nsubc;
            vec sizes((size_t)nc * nsubc, 0), lens(nc, 0);
            for (uint32_t c = 0; c < nc; c++)
                for (uint32_t s = 0; s < nsubc; s++) {
                    const uint32_t per = shape == 0 ? T / 16 + 1 : std::max(1u, T / (2 * kPrefixCache / nsubc * nsubc));
                    const uint32_t sz = (rng() % 4 == 0 || c == 1) ? 0u : rng() % (2 * per + 1);
                    sizes[(size_t)c * nsubc + s] = sz;
                    lens[c] += sz;
                }
            Lists L = random_lists(rng, lens, q, false);
            std::vector<uint32_t> targets;
            for (uint32_t c = 0; c < nc; c++)
                if (c % 3 != 2) // every third list untouched; list 1 holds only empty sub-groups
                    targets.push_back(c);
            for (int round = 0; round < 2; round++) {
                const Batch b = random_batch(rng, T + T / 2 + 9, q, nsubc, targets);
                const vec old_sizes = sizes;
                const Lists N = emulate_append(L, b, T, nsubc, &sizes, &cached, &searched);
                check_same(N, naive_append(L, b, nsubc, &old_sizes), "grouping append", T);
                L = N;
            }
        }
        CHECK(T < 64 || (cached > 0 && searched > 0), "grouping T %u: %d tiles cached, %d searched: both sides of the limit wanted", T,
              cached, searched);
    }
}

// ---- removal, tile by tile of T rows: mask words of min(T, 64) rows, a tile's kept rows ranked, then compacted to the
// range that starts at the exclusive scan of the tiles' kept counts
static void check_removal(uint32_t T, size_t *max_mask_word)
{
    std::mt19937 rng(T * 104729u + 5);
    const uint32_t W = std::min(T, 64u), words = T / W;
    const uint32_t qs[] = {1, 3, 4, 7};
    for (uint32_t q : qs)
        for (int pattern = 0; pattern < 7; pattern++) {
            const uint32_t n_local = 5 * T + T / 3 + 1;
            Lists L = random_lists(rng, {T, 0, 2 * T + 7, n_local - 3 * T - 7}, q, false);
            std::vector<char> rm(n_local, 0);
            for (uint32_t r = 0; r < n_local; r++) {
                const uint32_t t = r / T, j = r % T;
                switch (pattern) {
                case 0: rm[r] = rng() % 3 == 0; break;            // scattered
                case 1: rm[r] = t == 1 || t == 2; break;          // two tiles keep nothing
                case 2: rm[r] = t != 0 && j == 0; break;          // the first tile keeps every row
                case 3: case 4: case 5:                           // the first tile keeps T - 3, T - 2, T - 1 rows: the next
                    rm[r] = t == 0 ? j < (uint32_t)(6 - pattern) : rng() % 5 == 0; // tile's range starts at head 1, 2, 3
                    break;
                default: rm[r] = 1;                               // every row
                }
            }
            const uint32_t ntiles = (uint32_t)update_tiles(n_local, T);
            std::vector<u64> mask(remove_mask_words(ntiles, T), 0);
            vec keep(ntiles + 1, 0);
            for (uint32_t r = 0; r < n_local; r++) {
                if (rm[r])
                    mask[r / W] |= 1ull << (r % W);
                else
                    keep[r / T]++;
            }
            if (pattern >= 3 && pattern <= 5 && T % 4 == 0)
                CHECK(keep[0] % 4 == (uint32_t)(pattern - 2), "removal pattern %d: first tile keeps %u", pattern, keep[0]);
            const vec kscan = excl_scan(keep);
            const uint32_t n2 = kscan[ntiles];
            Lists N;
            N.q = q;
            N.codes.assign((size_t)n2 * q, 0xabababab);
            N.ids.assign(n2, 0xabababab);
            N.ncodes.assign(n2, 0xab);
            std::vector<int> wc(N.codes.size(), 0), wi(n2, 0), wn(n2, 0);
            for (uint32_t t = 0; t < ntiles; t++) {
                vec pre(words + 1, 0);
                std::vector<u64> kept(words, 0);
                for (uint32_t w = 0; w < words; w++) {
                    const u64 rw = (u64)t * T + (u64)w * W;
                    if (rw < n_local) {
                        *max_mask_word = std::max(*max_mask_word, (size_t)t * words + w);
                        kept[w] = ~mask[(size_t)t * words + w] & (W == 64 ? ~0ull : (1ull << W) - 1);
                        if (n_local - rw < W)
                            kept[w] &= (1ull << (n_local - rw)) - 1;
                    }
                    pre[w + 1] = pre[w] + (uint32_t)__builtin_popcountll(kept[w]);
                }
                const uint32_t rows = pre[words];
                if (!rows)
                    continue;
                vec s_src(rows);
                for (uint32_t j = 0; j < T; j++)
                    if ((kept[j / W] >> (j % W)) & 1)
                        s_src[kept_rank(pre[j / W], kept[j / W], j % W)] = t * T + j;
                const u64 d0 = kscan[t];
                tile_copy_dwords<false>(L.codes, N.codes, wc, s_src.data(), rows, q, d0 * q);
                tile_copy_dwords<false>(L.ids, N.ids, wi, s_src.data(), rows, 1, d0);
                tile_copy_bytes<false>(L.ncodes, N.ncodes, wn, s_src.data(), rows, d0);
            }
            size_t at = 0;
            for (uint32_t r = 0; r < n_local; r++) {
                if (rm[r])
                    continue;
                bool same = N.ids[at] == L.ids[r] && N.ncodes[at] == L.ncodes[r] && wi[at] == 1 && wn[at] == 1;
                for (uint32_t k = 0; k < q; k++)
                    same = same && N.codes[at * q + k] == L.codes[(size_t)r * q + k] && wc[at * q + k] == 1;
                CHECK(same, "removal T %u q %u pattern %d: kept row %u is not row %zu of the result, written once", T, q, pattern, r, at);
                at++;
            }
            CHECK(at == n2, "removal T %u pattern %d: %zu rows kept, the scan says %u", T, pattern, at, n2);
        }
}

// ---- 3. list_of_row over starts with runs of equal values
static void check_list_of_row()
{
    const std::vector<vec> lens_cases = {{0, 0, 0, 5, 3, 1}, {4, 0, 0, 0, 2, 6}, {3, 2, 0, 0, 0}, {0, 0, 7, 0, 0, 1, 0, 0}, {1}, {0, 0, 3}};
    for (const vec &lens : lens_cases) {
        const uint32_t nc = (uint32_t)lens.size();
        vec start(nc + 1, 0);
        for (uint32_t c = 0; c < nc; c++)
            start[c + 1] = start[c] + lens[c];
        for (uint32_t r = 0; r < start[nc]; r++) {
            uint32_t want = 0; // the list that holds row r
            while (!(start[want] <= r && r < start[want + 1]))
                want++;
            CHECK(list_of_row(start.data(), 0u, nc - 1, r) == want, "list_of_row: row %u in list %u, want %u", r,
                  list_of_row(start.data(), 0u, nc - 1, r), want);
            // from inside a narrower range that holds it, as a tile searches
            for (uint32_t lo = 0; lo <= want; lo++)
                for (uint32_t hi = want; hi < nc; hi++)
                    if (start[lo] <= r)
                        CHECK(list_of_row(start.data(), lo, hi, r) == want, "list_of_row [%u, %u]: row %u", lo, hi, r);
        }
    }
}

// ---- 4. the remaining workspace sizes
static void check_sizes()
{
    for (size_t len : {(size_t)1, (size_t)kScanChunk - 1, (size_t)kScanChunk, (size_t)kScanChunk + 1, (size_t)1000003}) {
        // scan_reduce / scan_apply: array y of two, chunk x of nblk, writes part[y * nblk + x]
        const size_t nblk = (len + kScanChunk - 1) / kScanChunk;
        CHECK(append_scan_parts(len) == 2 * nblk && (nblk - 1) * kScanChunk < len, "append_scan_parts(%zu) = %zu", len,
              append_scan_parts(len));
    }
    for (size_t top : {(size_t)0, (size_t)1, (size_t)2, (size_t)255, (size_t)256, (size_t)993126, (size_t)0xfffffffeull}) {
        const int b = bits_of(top);
        CHECK(b >= 1 && b <= 32 && (b == 32 || top >> b == 0) && (b == 1 || top >> (b - 1)), "bits_of(%zu) = %d", top, b);
    }
    CHECK(update_tiles(0, 2048) == 0 && update_tiles(1, 2048) == 1 && update_tiles(2048, 2048) == 1 && update_tiles(2049, 2048) == 2,
          "update_tiles");
    CHECK(remove_mask_words(0, 2048) == 32 && remove_mask_words(3, 2048) == 96, "remove_mask_words");
}

int main()
{
    check_groups();
    check_list_of_row();
    for (uint32_t T : {8u, 2048u}) {
        size_t max_mask_word = 0;
        check_appends(T);
        check_removal(T, &max_mask_word);
        CHECK(max_mask_word < remove_mask_words(update_tiles(5 * T + T / 3 + 1, T), T), "T %u: mask word %zu touched", T, max_mask_word);
    }
    check_sizes();
    if (failures) {
        printf("update_math: %d checks failed\n", failures);
        return 1;
    }
    printf("update_math ok\n");
    return 0;
}
