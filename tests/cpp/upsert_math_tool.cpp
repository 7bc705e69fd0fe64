// Host check of the upsert's arithmetic in csrc/update_math.h (tests/test_upsert_cpu.py builds it with the address and
// undefined-behaviour sanitizers): a whole upsert -- removal mask, scans, the (source tile, list) segments of the fused
// compaction, the scatter of the batch -- emulated with the shared functions at tiles of 8 and of 2048 rows against a plain
// serial remove-then-append on random CSR lists, at rows of 1, 3, 4 and 7 dwords.  Every element of the new arrays must be
// written exactly once (the destinations of kept rows and batch rows are a permutation of [0, n_local2)) and hold what
// the serial result holds.  Includes nothing else of the library; exit status 0 = every check held.
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
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (failures++ < 20) {            \
                printf("FAIL: " __VA_ARGS__); \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

// the memory of copy_group_dwords / copy_group_bytes on the host: the vectors are exactly as long as the arrays, so the
// sanitizer checks the bounds; every store is counted
template <class T> struct Mem {
    const std::vector<T> *src;
    std::vector<T> *dst;
    std::vector<int> *writes;
    size_t dbase; // index of group 0's first element; may lie up to 3 in front of the range
    uint32_t load(size_t s) const { return (*src)[s]; }
    void load4(size_t s, uint32_t v[4]) const
    {
        for (int u = 0; u < 4; u++)
            v[u] = (*src)[s + u];
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

static void copy_dwords(const vec &src, vec &dst, std::vector<int> &writes, const uint32_t *s_src, uint32_t rows, uint32_t q, u64 d0)
{
    const uint32_t ndw = rows * q, head = group_head<false>(d0), ng = group_count(head, ndw);
    const Mem<uint32_t> m{&src, &dst, &writes, (size_t)(d0 - head)};
    for (uint32_t gi = 0; gi < ng; gi++)
        copy_group_dwords<false>(m, s_src, gi, head, ndw, q);
}
static void copy_bytes(const std::vector<uint8_t> &src, std::vector<uint8_t> &dst, std::vector<int> &writes, const uint32_t *s_src,
                       uint32_t rows, u64 d0)
{
    const uint32_t head = group_head<false>(d0), ng = group_count(head, rows);
    const Mem<uint8_t> m{&src, &dst, &writes, (size_t)(d0 - head)};
    for (uint32_t gi = 0; gi < ng; gi++)
        copy_group_bytes<false>(m, s_src, gi, head, rows);
}

struct Lists {
    uint32_t q = 1;
    std::vector<u64> goff; // [nc + 1]
    vec loff;              // [nc]
    vec codes, ids;        // [n * q], [n]
    std::vector<uint8_t> ncodes;
    uint32_t nc() const { return (uint32_t)loff.size(); }
    uint32_t n() const { return (uint32_t)ids.size(); }
};
struct Batch {
    vec list, ids, codes;
    std::vector<uint8_t> ncodes;
};

static vec excl_scan(const vec &v) // the last slot holds 0 on entry and the total on return
{
    vec s(v.size());
    uint32_t run = 0;
    for (size_t i = 0; i < v.size(); i++) {
        s[i] = run;
        run += v[i];
    }
    return s;
}

static Lists random_lists(std::mt19937 &rng, const vec &lens, uint32_t q)
{
    Lists L;
    L.q = q;
    L.goff.push_back(0);
    for (uint32_t len : lens) {
        L.loff.push_back((uint32_t)L.goff.back());
        L.goff.push_back(L.goff.back() + len);
    }
    const uint32_t n = (uint32_t)L.goff.back();
    L.ids.resize(n);
    L.ncodes.resize(n);
    L.codes.resize((size_t)n * q);
    for (uint32_t r = 0; r < n; r++) {
        L.ids[r] = r * 7 + 1;
        L.ncodes[r] = (uint8_t)rng();
    }
    for (uint32_t &x : L.codes)
        x = (uint32_t)rng();
    return L;
}

static Batch random_batch(std::mt19937 &rng, const vec &lists, uint32_t q)
{
    Batch b;
    b.list = lists;
    const size_t n = lists.size();
    b.ids.resize(n);
    b.ncodes.resize(n);
    b.codes.resize(n * q);
    for (size_t i = 0; i < n; i++) {
        b.ids[i] = 0x80000000u + (uint32_t)i;
        b.ncodes[i] = (uint8_t)rng();
    }
    for (uint32_t &x : b.codes)
        x = (uint32_t)rng();
    return b;
}

// the serial remove-then-append
static Lists naive(const Lists &L, const std::vector<char> &rm, const Batch &b)
{
    Lists N;
    N.q = L.q;
    N.goff.push_back(0);
    for (uint32_t c = 0; c < L.nc(); c++) {
        N.loff.push_back((uint32_t)N.goff.back());
        auto put = [&](uint32_t id, uint8_t nb, const uint32_t *code) {
            N.ids.push_back(id);
            N.ncodes.push_back(nb);
            N.codes.insert(N.codes.end(), code, code + L.q);
        };
        for (u64 r = L.goff[c]; r < L.goff[c + 1]; r++)
            if (!rm[r])
                put(L.ids[r], L.ncodes[r], L.codes.data() + r * L.q);
        for (size_t i = 0; i < b.list.size(); i++)
            if (b.list[i] == c)
                put(b.ids[i], b.ncodes[i], b.codes.data() + i * L.q);
        N.goff.push_back(N.ids.size());
    }
    return N;
}

// the upsert as the device runs it, tile by tile, with update_math.h
static void emulate(const Lists &L, const std::vector<char> &rm, const Batch &b, uint32_t T, const char *what)
{
    const uint32_t W = std::min(T, 64u), words = T / W, q = L.q, nc = L.nc(), n_local = L.n();
    uint32_t wshift = 0;
    while ((1u << wshift) < W)
        wshift++;
    const size_t n = b.list.size();
    // removal's mask, keep and rem; append's cnt
    const uint32_t ntiles = (uint32_t)update_tiles(n_local, T);
    std::vector<u64> mask(remove_mask_words(ntiles, T), 0);
    vec keep(ntiles + 1, 0), rem(nc + 1, 0), cnt(nc + 1, 0);
    for (uint32_t c = 0; c < nc; c++)
        for (u64 r = L.goff[c]; r < L.goff[c + 1]; r++) {
            if (rm[r]) {
                mask[r / W] |= 1ull << (r % W);
                rem[c]++;
            } else {
                keep[r / T]++;
            }
        }
    for (uint32_t c : b.list)
        cnt[c]++;
    const vec kscan = excl_scan(keep), rscan = excl_scan(rem), nstart = excl_scan(cnt);
    const uint32_t n2 = kscan[ntiles] + (uint32_t)n;
    // the batch sorted stably by list
    vec perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return b.list[x] < b.list[y]; });
    const Lists want = naive(L, rm, b);
    CHECK(want.n() == n2, "%s T %u q %u: %u rows expected, the scans say %u", what, T, q, want.n(), n2);
    for (uint32_t c = 0; c < nc; c++)
        CHECK(upsert_list_start(L.loff[c], rscan[c], nstart[c]) == want.loff[c], "%s T %u: new start of list %u", what, T, c);
    CHECK(L.goff[nc] - rscan[nc] + nstart[nc] == want.goff[nc], "%s T %u: new total", what, T);
    Lists N;
    N.q = q;
    N.codes.assign((size_t)n2 * q, 0xabababab);
    N.ids.assign(n2, 0xabababab);
    N.ncodes.assign(n2, 0xab);
    std::vector<int> wc(N.codes.size(), 0), wi(n2, 0), wn(n2, 0);
    // tile_first, then the fused compaction
    vec tile_first(ntiles + 1);
    for (uint32_t t = 0; t <= ntiles; t++)
        tile_first[t] = t == ntiles ? nc - 1 : list_of_row(L.loff.data(), 0u, nc - 1, t * T);
    size_t segments = 0;
    for (uint32_t t = 0; t < ntiles; t++) {
        vec pre(words + 1, 0);
        std::vector<u64> kept(words, 0);
        for (uint32_t w = 0; w < words; w++) {
            const u64 rw = (u64)t * T + (u64)w * W;
            if (rw < n_local) {
                kept[w] = ~mask[(size_t)t * words + w] & (W == 64 ? ~0ull : (1ull << W) - 1);
                if (n_local - rw < W)
                    kept[w] &= (1ull << (n_local - rw)) - 1;
            }
            pre[w + 1] = pre[w] + (uint32_t)__builtin_popcountll(kept[w]);
        }
        const uint32_t rows = pre[words];
        CHECK(rows == keep[t], "%s T %u: tile %u keeps %u, the mark said %u", what, T, t, rows, keep[t]);
        if (!rows)
            continue;
        vec s_src(rows);
        for (uint32_t j = 0; j < T; j++)
            if ((kept[j / W] >> (j % W)) & 1)
                s_src[kept_rank(pre[j / W], kept[j / W], j % W)] = t * T + j;
        const uint32_t a0 = t * T, r_end = std::min(a0 + T, n_local), hi = tile_first[t + 1];
        uint32_t lo = tile_first[t], a = a0, covered = 0;
        while (a < r_end) {
            const TileSegment seg = tile_segment(L.loff.data(), L.goff.data(), lo, hi, a, r_end);
            CHECK(seg.end > a && L.loff[seg.list] <= a && seg.end <= L.goff[seg.list + 1], "%s T %u: segment at row %u", what, T, a);
            if (seg.end <= a)
                break;
            const uint32_t j0 = kept_before(pre.data(), kept.data(), a - a0, wshift, words);
            const uint32_t j1 = kept_before(pre.data(), kept.data(), seg.end - a0, wshift, words);
            CHECK(j0 == covered && j1 >= j0 && j1 <= rows, "%s T %u: ranks %u..%u of tile %u", what, T, j0, j1, t);
            if (j1 > j0) {
                const u64 d0 = upsert_kept_dest(kscan[t], j0, nstart[seg.list]);
                copy_dwords(L.codes, N.codes, wc, s_src.data() + j0, j1 - j0, q, d0 * q);
                copy_dwords(L.ids, N.ids, wi, s_src.data() + j0, j1 - j0, 1, d0);
                copy_bytes(L.ncodes, N.ncodes, wn, s_src.data() + j0, j1 - j0, d0);
                segments++;
            }
            covered = j1;
            lo = seg.list;
            a = seg.end;
        }
        CHECK(covered == rows, "%s T %u: the segments of tile %u cover %u of %u kept rows", what, T, t, covered, rows);
    }
    // the scatter
    for (size_t p = 0; p < n; p++) {
        const uint32_t i = perm[p], c = b.list[i];
        const size_t row = upsert_batch_dest(L.loff[c], (uint32_t)(L.goff[c + 1] - L.goff[c]), rscan[c], rscan[c + 1], p, nstart[c]);
        CHECK(row < n2, "%s T %u: batch row %zu goes to %zu of %u", what, T, p, row, n2);
        if (row >= n2)
            continue;
        for (uint32_t k = 0; k < q; k++) {
            N.codes[row * q + k] = b.codes[(size_t)i * q + k];
            wc[row * q + k]++;
        }
        N.ids[row] = b.ids[i];
        wi[row]++;
        N.ncodes[row] = b.ncodes[i];
        wn[row]++;
    }
    // a permutation of [0, n2): every element written exactly once; and the serial result
    bool once = true;
    for (int x : wc)
        once = once && x == 1;
    for (uint32_t r = 0; r < n2; r++)
        once = once && wi[r] == 1 && wn[r] == 1;
    CHECK(once, "%s T %u q %u: some element of the new arrays is not written exactly once", what, T, q);
    CHECK(N.ids == want.ids && N.ncodes == want.ncodes && N.codes == want.codes, "%s T %u q %u: not the serial result (%zu segments)",
          what, T, q, segments);
}

static std::vector<char> remove_where(const Lists &L, const std::vector<int> &share_of_list, std::mt19937 &rng)
{
    // share_of_list[c]: 0 = nothing, 100 = every row, else one row in that many
    std::vector<char> rm(L.n(), 0);
    for (uint32_t c = 0; c < L.nc(); c++)
        for (u64 r = L.goff[c]; r < L.goff[c + 1]; r++) {
            const int s = share_of_list[c];
            rm[r] = s == 100 ? 1 : s == 0 ? 0 : rng() % s == 0;
        }
    return rm;
}

static void check_upserts(uint32_t T)
{
    std::mt19937 rng(T * 7919u + 3);
    const uint32_t qs[] = {1, 3, 4, 7};
    for (uint32_t q : qs) {
        { // scattered removals, a batch into every list; empty lists, a list over several tiles
            const vec lens = {T, 0, 2 * T + 7, 0, 0, T / 2 + 1, 3 * T + T / 3, 3, 0};
            const Lists L = random_lists(rng, lens, q);
            vec to;
            for (uint32_t i = 0; i < 3 * T + 5; i++)
                to.push_back(rng() % lens.size());
            emulate(L, remove_where(L, std::vector<int>(lens.size(), 3), rng), random_batch(rng, to, q), T, "scattered");
            // head offsets 1, 2, 3 of the first segment behind a batch's rows
            for (uint32_t extra = 1; extra <= 3; extra++) {
                vec few(extra, 0u);
                emulate(L, remove_where(L, std::vector<int>(lens.size(), 4), rng), random_batch(rng, few, q), T, "head");
            }
        }
        { // lists emptied entirely and refilled; empty lists that get rows
            const vec lens = {T + 3, 0, 2 * T, 5, 0, T - 1};
            const Lists L = random_lists(rng, lens, q);
            vec to;
            for (uint32_t i = 0; i < T + 9; i++)
                to.push_back(i % 3 == 0 ? 0u : i % 3 == 1 ? 1u : 2u);
            emulate(L, remove_where(L, {100, 0, 100, 100, 0, 2}, rng), random_batch(rng, to, q), T, "emptied and refilled");
            emulate(L, remove_where(L, {100, 100, 100, 100, 100, 100}, rng), random_batch(rng, to, q), T, "every row replaced");
        }
        { // tiles holding many lists
            vec lens;
            for (uint32_t c = 0; c < 3 * T; c++)
                lens.push_back(rng() % 4);
            const Lists L = random_lists(rng, lens, q);
            vec to;
            for (uint32_t i = 0; i < 2 * T; i++)
                to.push_back(rng() % lens.size());
            emulate(L, remove_where(L, std::vector<int>(lens.size(), 2), rng), random_batch(rng, to, q), T, "many lists per tile");
        }
        { // the batch touches only lists nothing is removed from / removals only from lists the batch does not touch
            const vec lens = {T / 2, T + 1, 0, 2 * T + 2, T / 4 + 1, 7};
            const Lists L = random_lists(rng, lens, q);
            vec to;
            for (uint32_t i = 0; i < T + 1; i++)
                to.push_back(3 + rng() % 3);
            emulate(L, remove_where(L, {2, 3, 0, 0, 0, 0}, rng), random_batch(rng, to, q), T, "batch beside the removals");
            emulate(L, remove_where(L, {0, 0, 0, 0, 0, 100}, rng), random_batch(rng, vec(T / 2 + 3, 0u), q), T, "removals beside the batch");
            emulate(L, remove_where(L, {0, 0, 0, 0, 0, 0}, rng), random_batch(rng, to, q), T, "nothing removed");
        }
        { // an index without codes
            const Lists L = random_lists(rng, {0, 0, 0}, q);
            emulate(L, {}, random_batch(rng, {2, 0, 2, 2, 0}, q), T, "empty index");
        }
    }
}

int main()
{
    check_upserts(8);
    check_upserts(2048);
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("upsert_math ok\n");
    return 0;
}
