"""numpy helpers of the float16 base store's value-domain tests (tests/test_gpu_base_f16_widths.py,
tests/test_gpu_base_f16_values.py): numpy's own round to nearest even, the float64 distance between the
rounded operands with the documented bound, the selection and the range cut of a matrix of float32 BITS -- so that one call
of the device can be held to another bit for bit where no integer restatement exists -- and the makers of the data those
tests search.  tests/test_exact_f16_ref_cpu.py pins every function here to a brute-force loop."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def rounded(x):
    """x as float16, numpy's round to nearest even (a value of 65520 or more in magnitude becomes infinite)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def truth(x, q):
    """(D, tol) [nq, n] float64: the squared distance between the ROUNDED operands, and the bound the header gives for the
    float32 value the store returns for the pair, (d + 3) 2^-23 (|q^| + |x^|)^2."""
    xh, qh = rounded(x).astype(np.float64), rounded(q).astype(np.float64)
    d = xh.shape[1]
    xn, qn = (xh * xh).sum(1), (qh * qh).sum(1)
    D = qn[:, None] + xn[None, :] - 2.0 * (qh @ xh.T)
    tol = (d + 3) * 2.0 ** -23 * (np.sqrt(qn)[:, None] + np.sqrt(xn)[None, :]) ** 2
    return D, tol


def matrix_of(lims, dist, labels, n):
    """[nq, n] float32 of a range result: entry (q, l) is the distance returned for the pair, NaN where none was."""
    nq = len(lims) - 1
    B = np.full((nq, n), np.nan, np.float32)
    qi = np.repeat(np.arange(nq), np.diff(np.asarray(lims).astype(np.int64)))
    B[qi, np.asarray(labels, np.int64)] = dist
    return B


def topk_of_bits(B, k, mask=None):
    """(distances f32 [nq, k], labels i64 [nq, k]): the k smallest entries of each row of B by (value, label), padded with
    FLT_MAX / -1.  mask [nq, n] bool: the entries a row may select (None: all).  A NaN is never selected."""
    B = np.asarray(B, np.float32)
    nq, n = B.shape
    ok = ~np.isnan(B)
    if mask is not None:
        ok &= np.asarray(mask, bool)
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        idx = np.flatnonzero(ok[i])  # ascending label, and the sort is stable: equal values stay in that order
        best = idx[np.argsort(B[i, idx], kind="stable")][:k]
        out_d[i, :best.size] = B[i, best]
        out_l[i, :best.size] = best
    return out_d, out_l


def range_of_bits(B, radius, mask=None):
    """(lims u64 [nq + 1], distances f32 [total], labels i64 [total]): per row the entries with B < float32(radius),
    strictly, in ascending label; mask as in topk_of_bits.  A NaN is below no radius."""
    B = np.asarray(B, np.float32)
    with np.errstate(invalid="ignore"):
        hit = B < np.float32(radius)
    if mask is not None:
        hit &= np.asarray(mask, bool)
    lims = np.zeros(B.shape[0] + 1, np.uint64)
    lims[1:] = np.cumsum(hit.sum(1), dtype=np.uint64)
    q, lab = np.nonzero(hit)  # row major: by row, then ascending label
    return lims, B[q, lab], lab.astype(np.int64)


# ---- data ------------------------------------------------------------------------------------------------------------
def offset_rows(seed, n, d, centre, spread):
    """float32 [n, d]: centre + spread * standard normal.  With spread far below centre every distance is small against the
    norms, which is where the sweep's cheap gate and the sign of a returned distance are decided by roundings."""
    rng = np.random.default_rng(seed)
    return (np.float32(centre) + np.float32(spread) * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)


def scaled_ints(seed, n, d, log2_scale):
    """(ints uint8 [n, d] in 0..127, rows float32 = ints * 2^log2_scale): one power of two times an integer, the case the
    header calls exact.  At log2_scale = -24 every nonzero value is a subnormal half."""
    ints = np.random.default_rng(seed).integers(0, 128, (n, d), dtype=np.uint8)
    return ints, np.ldexp(ints.astype(np.float32), log2_scale).astype(np.float32)


def edge_values():
    """float32 [m]: where a rounding to half can go wrong.  Every value is exact in float32 and below 65520 in magnitude."""
    f = np.float32
    u, s = 2.0 ** -10, 2.0 ** -24  # the spacing of the halves in [1, 2), and of the subnormal halves
    v = [
        # ties between neighbouring normal halves: to the even mantissa, which lies below, then above; and their neighbours
        1 + u / 2, 1 + 3 * u / 2, -(1 + u / 2), -(1 + 3 * u / 2), 2049.0, 2051.0,
        np.nextafter(f(1 + u / 2), f(2)), np.nextafter(f(1 + u / 2), f(0)),
        # ties between neighbouring subnormal halves: 2.5 -> 2, 3.5 -> 4, 1.5 -> 2 units, and the neighbours of one
        2.5 * s, 3.5 * s, 1.5 * s, -2.5 * s, np.nextafter(f(2.5 * s), f(1)), np.nextafter(f(2.5 * s), f(0)),
        # the top: the last float32 that rounds to 65504, and 65504 itself
        np.nextafter(f(65520), f(0)), -np.nextafter(f(65520), f(0)), 65504.0, -65504.0, 65519.0,
        # zero and the bottom: the least subnormal, the tie to zero and the float just above it
        0.0, -0.0, s, -s, s / 2, -s / 2, np.nextafter(f(s / 2), f(1)), np.nextafter(f(s / 2), f(0)),
        # the least normal half, the largest subnormal, and the tie between them (to the normal: its mantissa is even)
        2.0 ** -14, 2.0 ** -14 - s, 2.0 ** -14 - s / 2,
    ]
    out = np.array(v, np.float64)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)
