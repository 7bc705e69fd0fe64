// Host check of csrc/walk_form.h (tests/test_walk_form_cpu.py builds it with the address and undefined-behaviour
// sanitizers as a stand-alone program): which instantiation of the walk a launch takes -- result-set class, visited-set
// tag width, filter form, shape, stamps build, dynamic LDS -- and that the dispatcher has an instantiation for every form
// the rule can produce and for no other.  The expectations are those of launch_coarse as it stood before the rule moved
// into the header, written out as numbers.
#include "walk_form.h"

#include <initializer_list>
#include <set>
#include <stdio.h>
#include <tuple>

using namespace ivfhnsw_gpu_impl;

static int failures = 0;

static void check(bool ok, const char *what, long a = 0, long b = 0)
{
    if (!ok) {
        printf("FAILED: %s (%ld, %ld)\n", what, a, b);
        failures++;
    }
}

static void expect(const char *what, WalkForm got, int d, int maxM)
{
    if (got.d != d || got.maxM != maxM) {
        printf("%s: got (%d, %d), want (%d, %d)\n", what, got.d, got.maxM, d, maxM);
        failures++;
    }
}

static WalkGraph graph(uint32_t n, int d, int maxM, int nb_rows, bool qrows, bool nbrows, bool unique, bool merge)
{
    const WalkGraph g = {n, d, maxM, nb_rows, qrows, nbrows, unique, merge};
    return g;
}

// The shape of a launch given what used to be walk_shape_for's arguments: a small graph and knobs that make the rule
// derive exactly this fmode, tagw and nch (checked), then the shape it picks.
static WalkForm shape_for(int d, int maxM, int nb_rows, int fmode, int tagw, int nch, bool shape_on)
{
    WalkKnobs k;
    k.shape_on = shape_on;
    k.force_bitmap = tagw == 0;
    k.force_tagw = tagw > 8 ? tagw : 0;
    const WalkForm f = walk_form_for(graph(2048, d, maxM, nb_rows, fmode >= 1, fmode >= 2, fmode == 3, true), 64 * nch, k);
    check(f.fmode == fmode && f.tagw == tagw && f.nch == (nch < 1 ? 1 : nch), "shape_for's inputs", f.fmode, f.tagw);
    return f;
}

struct Seen {
    int nch, tagw, fmode, d, maxM;
    bool stamps, merge;
};

static bool dispatch(const WalkForm &f, Seen *seen)
{
    return with_walk_form(f, [&](auto nch, auto tagw, auto fmode, auto stamps, auto d, auto maxm, auto merge) {
        *seen = {decltype(nch)::value,  decltype(tagw)::value,   decltype(fmode)::value, decltype(d)::value,
                 decltype(maxm)::value, decltype(stamps)::value, decltype(merge)::value};
    });
}

int main()
{
    const WalkKnobs none;
    // ---- walk_shape_tool.cpp's expectations
    // the cases of tests/test_gpu_walk_shape.py: d 128 / maxM 32 at ef 40, 33 (nch 1) and 80 (nch 2), both filter forms
    for (int nch = 1; nch <= 2; nch++)
        for (int fmode = 2; fmode <= 3; fmode++)
            for (int tagw : {8, 10, 12, 16}) {
                expect("d 128, maxM 32", shape_for(128, 32, 32, fmode, tagw, nch, true), 128, 32);
                expect("d 96 (DEEP)", shape_for(96, 32, 32, fmode, tagw, nch, true), 96, 32);
                expect("the knob at 0", shape_for(128, 32, 32, fmode, tagw, nch, false), 0, 0);
                expect("maxM 16", shape_for(128, 16, 32, fmode, tagw, nch, true), 0, 0);
                expect("d 64", shape_for(64, 32, 32, fmode, tagw, nch, true), 0, 0);
                expect("maxM 64", shape_for(128, 64, 64, fmode, tagw, nch, true), 0, 0);
                expect("a record of 64 rows", shape_for(128, 32, 64, fmode, tagw, nch, true), 0, 0);
                expect("d 112", shape_for(112, 32, 32, fmode, tagw, nch, true), 0, 0);
            }
    // forms that have no shaped instantiation: no filter, the gather form, the global bitmap, larger result sets
    expect("fmode 0", shape_for(128, 32, 32, 0, 10, 2, true), 0, 0);
    expect("fmode 1", shape_for(128, 32, 32, 1, 10, 2, true), 0, 0);
    expect("bitmap only", shape_for(128, 32, 32, 2, 0, 2, true), 0, 0);
    for (int nch : {3, 4, 8, 16})
        expect("nch > 2", shape_for(128, 32, 32, 3, 10, nch, true), 0, 0);
    expect("nch 0", shape_for(128, 32, 32, 3, 10, 0, true), 0, 0);
    // the bench's graphs: 993 127 and 2^17 nodes, d 128, maxM 32, ef 80 and 100
    const WalkGraph g1b = graph(993127, 128, 32, 32, true, true, true, true);
    const WalkGraph g100m = graph(131072, 128, 32, 32, true, true, false, true);
    expect("1B", walk_form_for(g1b, 80, none), 128, 32);
    expect("100M", walk_form_for(g100m, 80, none), 128, 32);

    // ---- tag width by n, no knobs: each boundary on both sides
    const struct {
        uint32_t n;
        int tagw, nbuckets;
    } by_n[] = {{1, 8, 1008},         {257040, 8, 1008},    {257041, 10, 1040},   {1063920, 10, 1040},   {1063921, 12, 1008},
                {4127760, 12, 1008},  {4127761, 16, 1008},  {66059280, 16, 1008}, {66059281, 0, 0},      {0x7fffffffu, 0, 0}};
    for (const auto &c : by_n) {
        const WalkForm f = walk_form_for(graph(c.n, 128, 32, 32, true, true, true, true), 80, none);
        check(f.tagw == c.tagw && f.nbuckets == c.nbuckets, "tag width by n", c.n, f.tagw);
        WalkKnobs k;
        k.force_bitmap = true;
        check(walk_form_for(graph(c.n, 128, 32, 32, true, true, true, true), 80, k).tagw == 0, "forced bitmap", c.n);
    }
    check(walk_vis_buckets(8) == 1008 && walk_vis_buckets(10) == 1040 && walk_vis_buckets(12) == 1008 && walk_vis_buckets(16) == 1008,
          "walk_vis_buckets");
    // forced widths
    const struct {
        uint32_t n;
        int force, tagw;
    } forced[] = {{2048, 10, 10},    {2048, 12, 12},    {2048, 16, 16},    {2048, 9, 8},       {500000, 12, 12},  {500000, 16, 16},
                  {500000, 10, 10},  {1063921, 10, 12}, {4127761, 10, 16}, {4127761, 12, 16},  {1063921, 16, 16}, {66059281, 10, 0},
                  {66059281, 12, 0}, {66059281, 16, 0}};
    for (const auto &c : forced) {
        WalkKnobs k;
        k.force_tagw = (c.force == 10 || c.force == 12 || c.force == 16) ? c.force : 0; // as the knob is parsed
        const WalkForm f = walk_form_for(graph(c.n, 128, 32, 32, true, true, true, true), 80, k);
        check(f.tagw == c.tagw && f.nbuckets == (c.tagw == 0 ? 0 : c.tagw == 10 ? 1040 : 1008), "forced tag width", c.n, c.force);
    }

    // ---- filter form, in this order
    for (int bits = 0; bits < 16; bits++) {
        const bool qrows = bits & 1, nbrows = bits & 2, unique = bits & 4, bitmap = bits & 8;
        WalkKnobs k;
        k.force_bitmap = bitmap;
        const int want = nbrows ? (unique && !bitmap ? 3 : 2) : qrows ? 1 : 0;
        check(walk_form_for(graph(2048, 128, 32, 32, qrows, nbrows, unique, true), 80, k).fmode == want, "filter form", bits);
    }

    // ---- nch classes and slots
    const struct {
        int ef, nch;
    } by_ef[] = {{1, 1}, {64, 1}, {65, 2}, {128, 2}, {129, 3}, {192, 3}, {193, 4}, {256, 4}, {257, 8}, {512, 8}, {513, 16}, {1024, 16}};
    for (const auto &c : by_ef) {
        check(walk_form_for(g1b, c.ef, none).nch == c.nch, "nch class", c.ef);
        check(walk_redo_form(g1b, c.ef).nch == c.nch, "nch class of the redo launch", c.ef);
        check(walk_nch_for(c.ef) == c.nch, "walk_nch_for", c.ef);
        check(coarse_slots_for(c.ef) == (c.ef <= 512 ? 4096 : 3072), "coarse_slots_for", c.ef);
    }

    // ---- the bench's graphs
    {
        const WalkForm f = walk_form_for(g1b, 80, none);
        check(f.nch == 2 && f.tagw == 10 && f.nbuckets == 1040 && f.fmode == 3 && f.d == 128 && f.maxM == 32 && f.merge && !f.stamps,
              "1B at ef 80");
        check(f.lds_bytes == 10048 && f.lds_bytes == 512 + 512 + (64 + 24) * 8 + 1040 * 8, "1B at ef 80: LDS", (long)f.lds_bytes);
        const WalkForm f100 = walk_form_for(g1b, 100, none);
        check(f100.nch == 2 && f100.tagw == 10 && f100.nbuckets == 1040 && f100.fmode == 3 && f100.d == 128 && f100.maxM == 32 &&
                  f100.merge && !f100.stamps,
              "1B at ef 100");
        check(f100.lds_bytes == 10208, "1B at ef 100: LDS", (long)f100.lds_bytes);
        const WalkForm s = walk_form_for(g100m, 80, none);
        check(s.nch == 2 && s.tagw == 8 && s.nbuckets == 1008 && s.fmode == 2 && s.d == 128 && s.maxM == 32 && s.merge, "100M at ef 80");
        check(s.lds_bytes == 9792 && s.lds_bytes == 512 + 512 + 704 + 8064, "100M at ef 80: LDS", (long)s.lds_bytes);
        const WalkForm q = walk_form_for(graph(131072, 128, 32, 0, true, false, false, true), 80, none);
        check(q.fmode == 1 && q.d == 0 && q.maxM == 0, "gather form");
        // the query twice (floats, and in byte-row units): 1024 + 512 + 704 + 8064
        check(q.lds_bytes == 10304 && q.lds_bytes == 2 * 512 + 512 + 704 + 8064, "gather form: LDS", (long)q.lds_bytes);
        // beyond ef 256 the tail is no merge buffer: 64 entries
        for (const WalkGraph &g : {g1b, g100m}) {
            const WalkForm big = walk_form_for(g, 300, none);
            check(big.lds_bytes == 512 + 512 + 512 + (size_t)big.nbuckets * 8, "ef 300: LDS", (long)big.lds_bytes);
            check(walk_redo_form(g, 300).lds_bytes == 512 + 512 + 512, "ef 300: LDS of the redo launch");
        }
        check(walk_form_for(g1b, 256, none).lds_bytes == 512 + 512 + (256 + 8) * 8 + 8320, "ef 256: LDS");
        check(walk_form_for(g1b, 56, none).lds_bytes == 512 + 512 + 512 + 8320, "ef 56: LDS");
        check(walk_form_for(g1b, 57, none).lds_bytes == 512 + 512 + 520 + 8320, "ef 57: LDS");
        const WalkForm r = walk_redo_form(g1b, 80);
        check(r.nch == 2 && r.tagw == 0 && r.nbuckets == 0 && r.fmode == 0 && r.d == 0 && r.maxM == 0 && !r.stamps, "redo form");
        check(r.lds_bytes == 1728 && r.lds_bytes == 512 + 512 + 704, "redo form: LDS", (long)r.lds_bytes);
    }

    // ---- late-visit default
    check(!walk_late_visit_default(257040) && walk_late_visit_default(257041) && !walk_late_visit_default(0), "late-visit default");

    // ---- the stamps rule
    {
        WalkKnobs k;
        k.stamps = true;
        // tagw 8 with fmode 2: always the generic stamps build
        WalkForm f = walk_form_for(g100m, 80, k);
        check(f.stamps && f.tagw == 8 && f.fmode == 2 && f.d == 0 && f.maxM == 0 && f.merge, "stamps: tagw 8, fmode 2");
        check(f.lds_bytes == 9792, "stamps: tagw 8, fmode 2: LDS");
        // tagw 10 with fmode 3: the shaped stamps build only for d 128 with merge
        f = walk_form_for(g1b, 80, k);
        check(f.stamps && f.tagw == 10 && f.fmode == 3 && f.d == 128 && f.maxM == 32 && f.merge, "stamps: tagw 10, fmode 3, d 128");
        f = walk_form_for(graph(993127, 128, 32, 32, true, true, true, false), 80, k);
        check(f.stamps && f.d == 0 && f.maxM == 0 && f.merge, "stamps: tagw 10, fmode 3, d 128, no merge");
        f = walk_form_for(graph(993127, 96, 32, 32, true, true, true, true), 80, k);
        check(f.stamps && f.d == 0 && f.maxM == 0, "stamps: tagw 10, fmode 3, d 96");
        k.shape_on = false;
        f = walk_form_for(g1b, 80, k);
        check(f.stamps && f.d == 0 && f.maxM == 0, "stamps: tagw 10, fmode 3, shape off");
        k.shape_on = true;
        // only nch 2, only those two forms
        check(!walk_form_for(g1b, 64, k).stamps && !walk_form_for(g1b, 129, k).stamps, "stamps: nch 2 only");
        check(!walk_form_for(graph(131072, 128, 32, 32, true, true, true, true), 80, k).stamps, "stamps: tagw 8 with fmode 3");
        check(!walk_form_for(graph(993127, 128, 32, 32, true, true, false, true), 80, k).stamps, "stamps: tagw 10 with fmode 2");
        check(!walk_form_for(graph(993127, 128, 32, 0, true, false, false, true), 80, k).stamps, "stamps: gather form");
        check(!walk_form_for(graph(2000000, 128, 32, 32, true, true, true, true), 80, k).stamps, "stamps: tagw 12");
        check(!walk_form_for(g1b, 80, none).stamps, "stamps: knob off");
    }

    // ---- the dispatcher: an instantiation for every form the rule can produce, handed the form's own values
    std::set<std::tuple<int, int, int, int, int, bool, bool>> distinct;
    long swept = 0;
    for (uint32_t n : {2048u, 131072u, 257040u, 257041u, 993127u, 1063920u, 1063921u, 4127760u, 4127761u, 66059280u, 66059281u})
        for (int d : {64, 96, 112, 128, 256})
            for (int shape = 0; shape < 4; shape++)
                for (int bits = 0; bits < 16; bits++)
                    for (int ef : {1, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 1024})
                        for (int kb = 0; kb < 32; kb++) {
                            const int maxM = shape == 0 ? 16 : shape == 3 ? 64 : 32, nb_rows = shape < 2 ? 32 : 64;
                            WalkKnobs k;
                            k.force_bitmap = kb & 1;
                            k.shape_on = !(kb & 2);
                            k.stamps = kb & 4;
                            k.force_tagw = (kb >> 3) == 0 ? 0 : (kb >> 3) == 1 ? 10 : (kb >> 3) == 2 ? 12 : 16;
                            const WalkForm f = walk_form_for(graph(n, d, maxM, nb_rows, bits & 1, bits & 2, bits & 4, bits & 8), ef, k);
                            Seen s = {};
                            const bool ok = dispatch(f, &s);
                            if (!ok || s.nch != f.nch || s.tagw != f.tagw || s.fmode != f.fmode || s.d != f.d || s.maxM != f.maxM ||
                                s.stamps != f.stamps || s.merge != f.merge || f.nbuckets != (f.tagw ? walk_vis_buckets(f.tagw) : 0)) {
                                if (failures < 20)
                                    printf("dispatch: n %u d %d maxM %d nb_rows %d bits %d ef %d knobs %d: %s\n", n, d, maxM, nb_rows, bits,
                                           ef, kb, ok ? "other constants than the form's fields" : "no instantiation");
                                failures++;
                            }
                            distinct.insert(std::make_tuple(s.nch, s.tagw, s.fmode, s.d, s.maxM, s.stamps, s.merge));
                            swept++;
                        }
    // 6 nch classes x (5 tag widths x 4 filter forms - 1) generic, 2 x 4 x 2 x 2 x 2 shaped, 3 stamps builds: the rule
    // reaches every instantiation the dispatcher lists
    check(distinct.size() == 6 * 19 + 64 + 3, "instantiations reached by the sweep", (long)distinct.size(), swept);

    // forms that cannot occur have none
    {
        Seen s;
        const WalkForm hot = walk_form_for(g1b, 80, none);
        check(dispatch(hot, &s), "the hot form");
        WalkForm f = walk_form_for(graph(2048, 128, 32, 32, true, true, true, true), 300, none); // generic: nch 8, tagw 8, fmode 3
        check(dispatch(f, &s), "a generic form");
        f.tagw = 0;
        f.nbuckets = 0;
        check(!dispatch(f, &s), "fmode 3 with tagw 0");
        f = hot, f.nch = 3;
        check(!dispatch(f, &s), "shaped with nch 3");
        f = hot, f.nch = 5;
        check(!dispatch(f, &s), "nch 5");
        f = hot, f.maxM = 0;
        check(!dispatch(f, &s), "d without maxM");
        f = hot, f.d = 64;
        check(!dispatch(f, &s), "shaped with d 64");
        f = hot, f.fmode = 1;
        check(!dispatch(f, &s), "shaped with the gather form");
        f = hot, f.tagw = 9;
        check(!dispatch(f, &s), "tagw 9");
        f = hot, f.nbuckets = 1008;
        check(!dispatch(f, &s), "tagw 10 with 1008 buckets");
        f = hot, f.d = f.maxM = 0, f.merge = false;
        check(!dispatch(f, &s), "generic with MERGE = false");
        f = hot, f.stamps = true, f.nch = 1;
        check(!dispatch(f, &s), "stamps with nch 1");
        f = hot, f.stamps = true, f.d = 96;
        check(!dispatch(f, &s), "stamps with d 96");
    }
    for (int nch = 0; nch <= 17; nch++) {
        int got = -1, got4 = -1;
        const bool is_class = nch == 1 || nch == 2 || nch == 3 || nch == 4 || nch == 8 || nch == 16;
        check(with_walk_nch(nch, [&](auto n) { got = decltype(n)::value; }) == is_class && got == (is_class ? nch : -1), "with_walk_nch", nch);
        check(with_walk_nch<4>(nch, [&](auto n) { got4 = decltype(n)::value; }) == (is_class && nch <= 4) &&
                  got4 == (is_class && nch <= 4 ? nch : -1),
              "with_walk_nch<4>", nch);
    }

    if (failures) {
        printf("walk_form: %d checks failed\n", failures);
        return 1;
    }
    printf("walk_form ok (%ld forms swept, %zu instantiations)\n", swept, distinct.size());
    return 0;
}
