// The arithmetic of the walk's exact rejection filter (kernels_hnsw.hip), from the integer sums of a byte row to the
// lower bound `lb` that is compared with the result set's maximum; the per-row slack carried in the norm table; and
// the margins that make the bound safe.  No HIP in it: the kernel and the host check (tests/cpp/walk_bound_tool.cpp)
// compile the same functions, the square root being the caller's (v_sqrt_f32 there, an adversarial one here).
//
// WHAT IS BOUNDED.  The reference's distance d_ref(q, x): float, eight accumulators, unfused multiply-add, the
// accumulators summed left to right (device_common.h, l2_ref_order).  A row is dropped when lb > max(result set), which
// is only right if lb <= d_ref.  With x ~ lo + step * c (c the byte row), q' = (q - lo) / step and
// err = ||x - (lo + step * c)|| / step,
//     ||q - x|| >= step * (||q' - c|| - err)                                                        (reals)
// and in the neighbour-row forms, with q' = q_in + q_out (clamped and rounded to 1/256 steps: Q; what the clamp cut off),
//     ||q_in - c|| >= ||Q/256 - c|| - ||q_in - Q/256||                                              -> m1
//     ||q' - c||^2 >= m1^2 + XL.c + XH.(255 - c) + ||q_out||^2                                      -> m2
//     lb = (step * (sqrt(m2) - slack))^2,  slack = err + 2^-18 ||q'||                               -> m, lb
// The term 2^-18 ||q'|| covers the rounding of q' itself (two operations per component, <= 2^-23 ||q'||, times 32).
//
// THE MARGINS, integer form with d <= 128 (u = 2^-24, one rounding to nearest; every factor sits BEFORE the next
// subtraction, because a relative error of a minuend is not one of the difference):
//   site 1, k1, on the first root:  128 ||Q/256 - c||^2 is exact in integers (< 2^31; the floor of Q.Q only lowers it)
//       int -> float            1 u on the radicand, 0.5 u on the root
//       v_sqrt_f32, 1 ulp       2 u
//       the product with k1     1 u                                   sum 3.5 u;  k1 = 1 - 2^-19 = 1 - 32 u  (9 x)
//     then  m1 = root * k1 - slack_q  rounds once more (1 u of m1, carried to site 3).
//   site 2, k2, on the clamp's cross term (an exact integer >= 0):
//       int -> float            1 u                                   sum 1 u;    k2 = 1 - 2^-20 = 1 - 16 u  (16 x)
//     then  t = x * k2 + bonus  rounds once (1 u of t; bonus is the caller's 0.999 ||q_out||^2).
//   site 3, k3, on the second root:  m2 = fma(m1, m1, t)
//       m1 (1 u) squared        2 u  }  on the radicand, together at most 3 u: 1.5 u on the root
//       t, and the fma          1 u + 1 u }
//       v_sqrt_f32              2 u
//       the product with k3     1 u                                   sum 4.5 u;  k3 = 1 - 2^-18 = 1 - 64 u  (14 x)
//   site 4, k4, on lb:
//       root * k3 - slack       1 u
//       times step              1 u        -> m, 2 u; squared 4 u
//       m * m, and times k4     2 u
//       the REFERENCE's own rounding downwards: a term passes one subtraction (2 u on its square), one product,
//       at most 15 additions in its accumulator (d / 8 = 16 terms, the first onto zero) and 7 in the final sum:
//                               25 u                                  sum 31 u;   k4 = 1 - 2^-16 = 1 - 256 u (8.2 x)
//   Each factor leaves at least 8 x its site's worst case, the generosity the constants below had over their own case.
//   (Squares that underflow in the reference lose less than 2^-126 each; the surplus of the 2^-18 ||q'|| term, 31 / 32 of
//   it, is above that for every query the byte rows can tell from zero.)
// EVERY OTHER FORM keeps 1 - 2^-10 at all four sites: the gather form sums d <= 2048 float terms on both sides
// ((d + 2) u each), and a generic instantiation does not know its d at compile time.
//
// THE PER-ROW SLACK.  The norm table's entries are ||c||^2 <= 128 * 255^2 < 2^23; the nine bits above carry the row's own
// error as a code E = walk_err_code(err_row, unit), unit = walk_err_unit(errc) >= errc / 511 with errc the table-wide
// maximum, so that E <= 511 and E * unit >= err_row, exactly (a 9-bit by 24-bit product).  err_row as encoded already
// stands (1 + 10^-6) above the measured error, 16 u: the one rounding of fma(E, unit, 2^-18 ||q'||) is inside it.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WALK_BOUND_HD __host__ __device__ __forceinline__
#else
#define WALK_BOUND_HD inline
#endif

namespace ivfhnsw_gpu_impl {

constexpr float kWalkMarginWide = 0.9990234375f; // 1 - 2^-10

// TIGHT: the integer form of the filter on rows of d <= 128 known at compile time
template <bool TIGHT>
struct WalkMargins {
    static constexpr float k1 = TIGHT ? 0.99999809265136719f : kWalkMarginWide; // 1 - 2^-19
    static constexpr float k2 = TIGHT ? 0.99999904632568359f : kWalkMarginWide; // 1 - 2^-20
    static constexpr float k3 = TIGHT ? 0.99999618530273438f : kWalkMarginWide; // 1 - 2^-18
    static constexpr float k4 = TIGHT ? 0.99998474121093750f : kWalkMarginWide; // 1 - 2^-16
};

constexpr uint32_t kWalkNormBits = 23, kWalkNormMask = (1u << kWalkNormBits) - 1u, kWalkErrCodes = 511;

// ---- the norm table's entry: ||c||^2 below, the row's error code above
WALK_BOUND_HD uint32_t walk_norm_pack(uint32_t norm, uint32_t code) { return norm | (code << kWalkNormBits); }
WALK_BOUND_HD uint32_t walk_norm_of(uint32_t entry) { return entry & kWalkNormMask; }
// this row's slack: its own error, plus the query's term (2^-18 ||q'||)
WALK_BOUND_HD float walk_row_slack(uint32_t entry, float unit, float slack_query)
{
    return fmaf((float)(entry >> kWalkNormBits), unit, slack_query);
}

// errc / 511, rounded up (errc: the table-wide error, itself rounded up)
inline float walk_err_unit(float errc)
{
    const double u = (double)errc / (double)kWalkErrCodes;
    float f = (float)u;
    while ((double)f * (double)kWalkErrCodes < (double)errc)
        f = nextafterf(f, INFINITY);
    return f;
}

// the smallest E with E * unit >= err_row (0 <= err_row <= errc, so E <= 511; clamped for a caller that breaks that)
inline uint32_t walk_err_code(double err_row, float unit)
{
    if (!(err_row > 0.0))
        return 0;
    double e = ceil(err_row / (double)unit);
    if (!(e < (double)kWalkErrCodes))
        return kWalkErrCodes;
    uint32_t code = (uint32_t)e;
    while (code < kWalkErrCodes && (double)code * (double)unit < err_row)
        code++;
    return code;
}

// a row's error as the table keeps it: the measured one (double) in byte-row units, rounded up
inline double walk_err_round_up(double err2, double step) { return sqrt(err2) / step * (1.0 + 1e-6) + 1e-6; }

// ---- the bound
// from the bound on ||q' - c|| (before its margin) to lb; also the whole of the gather form, whose `root` is
// sqrt(sum (q' - c)^2) in floats
template <bool TIGHT>
WALK_BOUND_HD float walk_lb_of_root(float root, float slack, float step)
{
    const float m = fmaxf(0.f, root * WalkMargins<TIGHT>::k3 - slack) * step;
    return m * m * WalkMargins<TIGHT>::k4;
}

// integer form.  w = 128 ||c||^2 - Q.c + floor(128 Q.Q / 65536) >= 0 (so w / 128 ~ ||Q/256 - c||^2), x = XL.c + XH.(255 - c);
// slack_q >= ||q_in - Q/256||, bonus <= ||q_out||^2, both the caller's per-query values.
template <bool TIGHT, class Sqrt>
WALK_BOUND_HD float walk_lb_int(int w, int x, float slack_q, float bonus, float slack, float step, Sqrt root)
{
    const float m1 = fmaxf(0.f, root((float)w * 0.0078125f) * WalkMargins<TIGHT>::k1 - slack_q);
    const float m2 = fmaf(m1, m1, fmaf((float)x, WalkMargins<TIGHT>::k2, bonus));
    return walk_lb_of_root<TIGHT>(root(m2), slack, step);
}

} // namespace ivfhnsw_gpu_impl
