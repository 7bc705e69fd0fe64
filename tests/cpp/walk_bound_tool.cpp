// Host check of csrc/walk_bound.h (tests/test_walk_bound_cpu.py builds it with the address and undefined-behaviour
// sanitizers as a stand-alone program): for many (query, row) pairs the walk filter's lower bound, computed by the header's
// own functions with both square roots pushed one ulp UP, must not exceed the float distance in the reference's summation
// order (eight accumulators, unfused, summed left to right).  The tables are quantised as build_byte_rows does it, the
// query is prepared as the kernel's prologue does it (floats, so host and device agree bit for bit up to the order of
// three per-query sums that carry their own 10^-3 margins).  Also: the 9-bit error code never under-states a row's error
// and leaves the 23-bit norm alone.
#include "walk_bound.h"

#include <algorithm>
#include <random>
#include <stdio.h>
#include <vector>

using namespace ivfhnsw_gpu_impl;

static long failures = 0, pairs = 0, rejected_tight = 0, rejected_wide = 0;

static void check(bool ok, const char *what, double a = 0, double b = 0)
{
    if (!ok) {
        if (failures < 20)
            printf("FAILED: %s (%.9g, %.9g)\n", what, a, b);
        failures++;
    }
}

struct UpSqrt { // v_sqrt_f32 at its worst: one ulp above the correctly rounded root
    float operator()(float v) const { return nextafterf(sqrtf(v), INFINITY); }
};

// hnswalg.cpp's distance: 8 accumulators over blocks of 16 floats, multiply then add, accumulators summed left to right
static float l2_ref(const float *x, const float *y, int d)
{
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < d; j++) {
        const volatile float t = x[j] - y[j];
        const volatile float p = t * t;
        a[j & 7] = a[j & 7] + p;
    }
    volatile float r = a[0] + a[1];
    for (int i = 2; i < 8; i++)
        r = r + a[i];
    return r;
}

struct Table {
    int n = 0, d = 0;
    std::vector<float> x;
    std::vector<uint8_t> c;       // [n][d]
    std::vector<uint32_t> entry;  // norm | code << 23
    std::vector<double> err_raw;  // measured, in byte-row units
    float lo = 0.f, step = 1.f, errc = 0.f, unit = 0.f;
};

// capi_upload.cpp, build_byte_rows + build_nbrows_kernel's packing
static void quantise(Table &t)
{
    const size_t n = t.n, d = t.d;
    float lo = t.x[0], hi = t.x[0];
    for (float v : t.x)
        lo = std::min(lo, v), hi = std::max(hi, v);
    const float step = (float)(((double)hi - (double)lo) / 255.0);
    check(step > 0.f && std::isfinite(1.f / step), "table has a usable range");
    t.lo = lo, t.step = step;
    t.c.resize(n * d), t.entry.resize(n), t.err_raw.resize(n);
    std::vector<double> e2s(n);
    double worst = 0.0;
    for (size_t r = 0; r < n; r++) {
        double e2 = 0.0;
        uint32_t norm = 0;
        for (size_t j = 0; j < d; j++) {
            const double v = t.x[r * d + j];
            double c = std::nearbyint((v - (double)lo) / (double)step);
            c = std::min(255.0, std::max(0.0, c));
            t.c[r * d + j] = (uint8_t)c;
            norm += (uint32_t)c * (uint32_t)c;
            const double e = v - ((double)lo + (double)step * c);
            e2 += e * e;
        }
        e2s[r] = e2;
        t.err_raw[r] = std::sqrt(e2) / (double)step;
        worst = std::max(worst, e2);
        t.entry[r] = norm;
    }
    const double errc = walk_err_round_up(worst, (double)step);
    float errc_f = (float)errc;
    if ((double)errc_f < errc)
        errc_f = nextafterf(errc_f, INFINITY);
    t.errc = errc_f;
    t.unit = walk_err_unit(errc_f);
    for (size_t r = 0; r < n; r++) {
        const double er = walk_err_round_up(e2s[r], (double)step);
        const uint32_t code = walk_err_code(er, t.unit);
        check(code <= kWalkErrCodes && (double)code * (double)t.unit >= er, "a table row's code covers its error", er, code);
        const uint32_t norm = t.entry[r];
        t.entry[r] = walk_norm_pack(norm, code);
        check(walk_norm_of(t.entry[r]) == norm && (t.entry[r] >> kWalkNormBits) == code, "pack / unpack", norm, code);
    }
}

struct Query { // the kernel's per-query values (hnsw_walk_kernel's prologue)
    int Q[128], xl[128], xh[128];
    int q16_w, x_const;
    float slack_query, slack_q, bonus;
};

static void prepare(const Table &t, const float *q, Query &p)
{
    float qp_sq = 0.f, dq_sq = 0.f, bonus = 0.f;
    long s_hh = 0, s_hl = 0, s_ll = 0, s_xh = 0;
    for (int j = 0; j < 128; j++) {
        const float vp = j < t.d ? (q[j] - t.lo) / t.step : 0.f;
        if (j < t.d)
            qp_sq = fmaf(vp, vp, qp_sq);
        const float fh = fminf(255.f, fmaxf(0.f, floorf(vp)));
        const float fl = fminf(255.f, fmaxf(0.f, rintf((vp - fh) * 256.f)));
        const float qin = fh + fl * 0.00390625f;
        const bool below = vp < 0.f, above = vp >= 256.f;
        const float e = (below || above) ? 0.f : vp - qin;
        dq_sq = fmaf(e, e, dq_sq);
        const float out = (below || above) ? fabsf(vp - qin) : 0.f;
        bonus = fmaf(out, out, bonus);
        const int x = (int)fminf(255.f, floorf(2.f * out));
        const int hi = (int)fh, lo = (int)fl;
        s_hh += hi * hi, s_hl += hi * lo, s_ll += lo * lo;
        p.Q[j] = 256 * hi + lo;
        p.xl[j] = below ? x : 0;
        p.xh[j] = above ? x : 0;
        s_xh += p.xh[j];
    }
    const long w = 128 * s_hh + s_hl + (s_ll >> 9);
    check(w >= 0 && w < (1l << 31), "q16_w fits an int", (double)w);
    p.q16_w = (int)w;
    p.x_const = (int)(255 * s_xh);
    p.slack_query = 3.9e-6f * sqrtf(qp_sq);
    p.slack_q = 1.001f * sqrtf(dq_sq);
    p.bonus = 0.999f * bonus;
}

// every query against every row: the three combinations of margins and slack the kernel's forms use
static void sweep(const char *what, const Table &t, const std::vector<float> &queries, float worst_scale = 1.f)
{
    const int d = t.d, nq = (int)(queries.size() / d);
    long viol = 0;
    std::vector<float> dref(t.n);
    for (int qi = 0; qi < nq; qi++) {
        const float *q = queries.data() + (size_t)qi * d;
        Query p;
        prepare(t, q, p);
        for (int r = 0; r < t.n; r++)
            dref[r] = l2_ref(q, t.x.data() + (size_t)r * d, d);
        // what a full result set's maximum might be: the 80th smallest distance
        std::vector<float> s(dref);
        const size_t kth = std::min<size_t>(79, s.size() - 1);
        std::nth_element(s.begin(), s.begin() + kth, s.end());
        const float worst = s[kth] * worst_scale;
        for (int r = 0; r < t.n; r++) {
            const uint8_t *c = t.c.data() + (size_t)r * d;
            long qc = 0, xs = 0;
            for (int j = 0; j < d; j++) {
                qc += (long)p.Q[j] * c[j];
                xs += (long)(p.xl[j] - p.xh[j]) * c[j];
            }
            const long w = 128l * walk_norm_of(t.entry[r]) - qc + p.q16_w, x = xs + p.x_const;
            check(w >= 0 && w < (1l << 31) && x >= 0 && x < (1l << 31), "the integer sums fit an int", (double)w, (double)x);
            const float slack_row = walk_row_slack(t.entry[r], t.unit, p.slack_query), slack_tab = t.errc + p.slack_query;
            check((double)slack_row >= t.err_raw[r] + (double)p.slack_query / 32.0, "decoded slack covers the row's error",
                  slack_row, t.err_raw[r]);
            check(slack_row <= slack_tab * 1.000001f, "a row's slack is not above the table's", slack_row, slack_tab);
            const float lb3 = walk_lb_int<true>((int)w, (int)x, p.slack_q, p.bonus, slack_row, t.step, UpSqrt());  // FMODE 3 shaped
            const float lb2 = walk_lb_int<true>((int)w, (int)x, p.slack_q, p.bonus, slack_tab, t.step, UpSqrt());  // FMODE 2 shaped
            const float lbg = walk_lb_int<false>((int)w, (int)x, p.slack_q, p.bonus, slack_row, t.step, UpSqrt()); // FMODE 3 generic
            const float lbo = walk_lb_int<false>((int)w, (int)x, p.slack_q, p.bonus, slack_tab, t.step, UpSqrt()); // as it was
            if (lb3 > dref[r] || lb2 > dref[r] || lbg > dref[r] || lbo > dref[r]) {
                if (viol++ < 5)
                    printf("%s: query %d row %d: lb %.9g / %.9g / %.9g / %.9g above the distance %.9g\n", what, qi, r, lb3, lb2, lbg,
                           lbo, dref[r]);
            }
            rejected_tight += lb3 > worst;
            rejected_wide += lbo > worst;
            pairs++;
        }
    }
    failures += viol;
}

// the gather form's half of the header: float sums of d terms, margins 1 - 2^-10
static void sweep_gather(const Table &t, const std::vector<float> &queries)
{
    const int d = t.d, nq = (int)(queries.size() / d);
    for (int qi = 0; qi < nq; qi++) {
        const float *q = queries.data() + (size_t)qi * d;
        std::vector<float> qp(d);
        float qp_sq = 0.f;
        for (int j = 0; j < d; j++) {
            qp[j] = (q[j] - t.lo) / t.step;
            qp_sq = fmaf(qp[j], qp[j], qp_sq);
        }
        const float slack = t.errc + 3.9e-6f * sqrtf(qp_sq);
        for (int r = 0; r < t.n; r++) {
            float S = 0.f;
            for (int j = 0; j < d; j++) {
                const float e = qp[j] - (float)t.c[(size_t)r * d + j];
                S = fmaf(e, e, S);
            }
            const float lb = walk_lb_of_root<false>(UpSqrt()(S), slack, t.step);
            check(!(lb > l2_ref(q, t.x.data() + (size_t)r * d, d)), "gather form", lb);
            pairs++;
        }
    }
}

static std::mt19937_64 rng(20240521);
static float uni(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); }

static float ulps(float v, int k)
{
    for (; k > 0; k--)
        v = nextafterf(v, INFINITY);
    for (; k < 0; k++)
        v = nextafterf(v, -INFINITY);
    return v;
}

enum Kind { RANDOM, EXACT, OUTLIERS, NEAR };

static Table make_table(Kind kind, int n, int d)
{
    Table t;
    t.n = n, t.d = d;
    t.x.resize((size_t)n * d);
    std::normal_distribution<float> gauss(0.f, 1.f);
    for (int r = 0; r < n; r++)
        for (int j = 0; j < d; j++) {
            float &v = t.x[(size_t)r * d + j];
            switch (kind) {
            case RANDOM: // SIFT-like magnitudes, not on any grid
                v = fabsf(gauss(rng)) * 40.f + uni(0.f, 3.f);
                break;
            case EXACT: // integers 0..255: with lo = 0 and step = 1 every row is its own byte row
            case NEAR:
                v = (float)(int)std::min(255.f, fabsf(gauss(rng)) * 45.f);
                break;
            case OUTLIERS: // 1 % of the rows half a step off in every component, the rest exact
                v = (float)(int)std::min(254.f, fabsf(gauss(rng)) * 45.f) + (r % 100 == 7 ? 0.5f : 0.f);
                break;
            }
        }
    if (kind != RANDOM) { // pin the range to [0, 255]
        t.x[0] = 0.f;
        t.x[1] = 255.f;
    }
    if (kind == NEAR) // runs of rows a few ulps apart in one component, and exact duplicates
        for (int r = 8; r + 8 <= n; r += 16)
            for (int k = 1; k < 8; k++) {
                std::copy(t.x.begin() + (size_t)r * d, t.x.begin() + (size_t)(r + 1) * d, t.x.begin() + (size_t)(r + k) * d);
                const int j = (r + k) % d;
                if (k < 6) {
                    float &v = t.x[(size_t)(r + k) * d + j];
                    v = v == 0.f ? ulps(1.f, k - 3) : ulps(v, k - 3);
                }
            }
    quantise(t);
    return t;
}

static std::vector<float> make_queries(const Table &t, int nq)
{
    const int d = t.d;
    std::vector<float> q((size_t)nq * d);
    std::normal_distribution<float> gauss(0.f, 1.f);
    for (int i = 0; i < nq; i++) {
        float *v = q.data() + (size_t)i * d;
        const float *row = t.x.data() + (size_t)(rng() % t.n) * d;
        const int kind = i % 8;
        for (int j = 0; j < d; j++) {
            switch (kind) {
            case 0: // a table row itself: distance zero to it, and to its duplicates
                v[j] = row[j];
                break;
            case 1: // the rounded image of a point near a row: lo + step * byte, in floats
                v[j] = t.lo + t.step * (float)(int)std::min(255.f, std::max(0.f, rintf((row[j] + gauss(rng) - t.lo) / t.step)));
                break;
            case 2: // a row, a few ulps off in every component
                v[j] = ulps(row[j], (int)(rng() % 7) - 3);
                break;
            case 3: // near a row
                v[j] = row[j] + gauss(rng) * 4.f;
                break;
            case 4: // far below the byte range in some components
                v[j] = (rng() % 4 == 0) ? t.lo - uni(0.f, 600.f) * t.step : row[j] + gauss(rng) * 10.f;
                break;
            case 5: // far above it
                v[j] = (rng() % 4 == 0) ? t.lo + (255.f + uni(0.f, 900.f)) * t.step : row[j] + gauss(rng) * 10.f;
                break;
            case 6: // outside on both sides, every component
                v[j] = (rng() & 1) ? t.lo - uni(0.f, 300.f) * t.step : t.lo + (255.f + uni(0.f, 300.f)) * t.step;
                break;
            default: // unrelated to any row
                v[j] = fabsf(gauss(rng)) * 40.f * t.step + t.lo;
                break;
            }
        }
    }
    return q;
}

static void check_codes()
{
    // the norm field survives its largest value under the largest code
    const uint32_t top = 128u * 255u * 255u;
    check(top <= kWalkNormMask, "128 * 255^2 fits 23 bits", top);
    check(walk_norm_of(walk_norm_pack(top, kWalkErrCodes)) == top && (walk_norm_pack(top, kWalkErrCodes) >> kWalkNormBits) == kWalkErrCodes,
          "largest norm under the largest code");
    check(walk_norm_of(walk_norm_pack(0, kWalkErrCodes)) == 0 && walk_norm_of(walk_norm_pack(top, 0)) == top, "pack corners");
    std::vector<float> errcs = {1e-6f, 1.0000001e-6f, 3.6f, 3.5999999f, 511.f, 510.99997f, 1e-3f, 0.75f, 1e4f, 1e-30f, 3e38f / 600.f};
    for (int i = 0; i < 2000; i++)
        errcs.push_back(expf(uni(-14.f, 12.f)));
    for (float errc : errcs) {
        const float unit = walk_err_unit(errc);
        check((double)unit * 511.0 >= (double)errc && unit > 0.f, "511 units reach errc", unit, errc);
        check((double)unit <= (double)errc / 511.0 * (1.0 + 3e-7) + 2e-45, "unit is errc / 511 rounded up, no more", unit, errc);
        std::vector<double> errs = {0.0, (double)errc, (double)nextafterf(errc, 0.f), (double)errc * 0.5, 5e-324, (double)unit,
                                    (double)nextafterf(unit, INFINITY), (double)nextafterf(unit, 0.f)};
        for (int k = 0; k <= 511; k += 7) {
            errs.push_back((double)k * (double)unit);
            errs.push_back(nextafter((double)k * (double)unit, INFINITY));
            errs.push_back(nextafter((double)k * (double)unit, 0.0));
        }
        for (int k = 0; k < 50; k++)
            errs.push_back((double)errc * (double)uni(0.f, 1.f));
        for (double e : errs) {
            if (e > (double)errc)
                continue;
            const uint32_t code = walk_err_code(e, unit);
            check(code <= kWalkErrCodes, "code fits 9 bits", code, e);
            check((double)code * (double)unit >= e, "decoded error is not below the row's", (double)code * unit, e);
            check(code == 0 || (double)(code - 1) * (double)unit < e, "the smallest such code", code, e);
            check(e > 0.0 || code == 0, "no error, no code", code);
            // the kernel's decode: one fma with the query's term; nothing of the ERROR is lost beyond the fma's rounding,
            // which the (1 + 10^-6) of walk_err_round_up holds sixteen times over
            const float sq = 3.9e-6f * uni(0.f, 3000.f);
            const float got = walk_row_slack(walk_norm_pack(12345u, code), unit, sq);
            check((double)got >= ((double)code * (double)unit + (double)sq) * (1.0 - 6e-8), "decode rounds once", got, e);
        }
        // err_row == q_errc, as the tables meet it (the row that set the maximum)
        check(walk_err_code((double)errc, unit) <= kWalkErrCodes && (double)walk_err_code((double)errc, unit) * unit >= (double)errc,
              "the worst row's own code", errc);
    }
    // the rounded-up error holds the decode's one rounding with room: (1 + 1e-6) against 2^-24
    for (double raw : {0.0, 1e-9, 0.3, 3.6, 1e3})
        check(walk_err_round_up(raw * raw, 1.0) * (1.0 - 6e-8) >= raw, "round-up margin", raw);
}

int main()
{
    check_codes();
    for (int d : {16, 96, 128})
        for (Kind kind : {RANDOM, EXACT, OUTLIERS, NEAR}) {
            const Table t = make_table(kind, 2048, d);
            if (kind == EXACT || kind == NEAR) // (the near-duplicates are a few ulps off the grid)
                check(t.lo == 0.f && t.step == 1.f && t.errc <= (kind == EXACT ? 1.1e-6f : 1e-4f), "byte-exact table", t.step, t.errc);
            if (kind == OUTLIERS)
                check(t.errc > 0.49f * sqrtf((float)d) && walk_err_code(walk_err_round_up(0.0, 1.0), t.unit) == 1,
                      "outlier table: exact rows carry the smallest code", t.errc);
            const char *names[] = {"random", "exact", "outliers", "near-duplicates"};
            sweep(names[kind], t, make_queries(t, 416));
        }
    // the gather form's margins on float sums, d up to 2048
    for (int d : {144, 2048}) {
        const Table t = make_table(RANDOM, 256, d);
        sweep_gather(t, make_queries(t, 64));
    }
    check(pairs >= 10000000, "at least 10^7 pairs", (double)pairs);
    if (failures) {
        printf("walk_bound: %ld checks failed\n", failures);
        return 1;
    }
    printf("walk_bound ok (%ld pairs; rows above the 80th distance: %ld with per-row slack and sized margins, %ld as before)\n", pairs,
           rejected_tight, rejected_wide);
    return 0;
}
