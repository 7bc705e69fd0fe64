"""tests/exact_f16_ref.py against brute-force loops on small inputs: the rounding against a search of all 63 488 finite
halves, the float64 truth against a loop over pairs, the selection and the range cut of a bit matrix against sorted Python
tuples -- with ties, negative values, a NaN entry, a masked row of fewer than k members and a radius that sits on an entry."""
import math

import numpy as np

import exact_f16_ref as fr

F = np.float32


# ---- rounding -----------------------------------------------------------------------------------------------------------
def _nearest_half(v):
    """The finite half nearest to v by a search of them all, a tie to the even bit pattern; None where v rounds beyond."""
    halves = np.arange(1 << 16, dtype=np.uint16)
    vals = halves.view(np.float16).astype(np.float64)
    fin = np.isfinite(vals)
    halves, vals = halves[fin], vals[fin]
    if abs(v) >= 65520:
        return None
    err = np.abs(vals - float(v))
    near = halves[err == err.min()]
    near = near[(near & 0x8000) == (0x8000 if math.copysign(1.0, float(v)) < 0 else 0)]  # (+0 and -0 are both nearest to 0)
    assert 1 <= near.size <= 2
    return int(near[0] if near.size == 1 else near[near % 2 == 0][0])


def test_edge_values_round_as_the_search_of_all_halves_says():
    ev = fr.edge_values()
    assert ev.dtype == np.float32 and (np.abs(ev) < 65520).all()
    got = fr.rounded(ev).view(np.uint16)
    for v, h in zip(ev, got):
        assert int(h) == _nearest_half(v), (float(v), hex(int(h)))
    # what the vector is there for, value by value
    r = {float(v): float(h) for v, h in zip(ev.astype(np.float64), fr.rounded(ev).astype(np.float64))}
    u, s = 2.0 ** -10, 2.0 ** -24
    assert r[1 + u / 2] == 1.0 and r[1 + 3 * u / 2] == 1 + 2 * u          # a tie down, a tie up
    assert r[2049.0] == 2048.0 and r[2051.0] == 2052.0
    assert r[2.5 * s] == 2 * s and r[3.5 * s] == 4 * s and r[1.5 * s] == 2 * s
    assert r[float(np.nextafter(F(65520), F(0)))] == 65504.0 and r[65519.0] == 65504.0
    assert r[s / 2] == 0.0 and r[float(np.nextafter(F(s / 2), F(1)))] == s
    assert r[2.0 ** -14 - s / 2] == 2.0 ** -14 and r[2.0 ** -14 - s] == 2.0 ** -14 - s
    signs = np.signbit(fr.rounded(ev))
    assert np.array_equal(signs, np.signbit(ev))                           # -0.0 and -2^-25 keep their sign
    assert np.isinf(fr.rounded(np.array([65520.0, -1e6], F))).all()


def test_random_values_round_as_the_search_of_all_halves_says():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.standard_normal(40, dtype=F) * F(3), rng.standard_normal(20, dtype=F) * F(2.0 ** -16),
                        rng.standard_normal(20, dtype=F) * F(20000)])
    for x, h in zip(v, fr.rounded(v).view(np.uint16)):
        assert int(h) == _nearest_half(x)


# ---- the float64 truth ------------------------------------------------------------------------------------------------
def test_truth_is_the_distance_of_the_rounded_vectors():
    x, q = fr.offset_rows(2, 7, 16, 30.0, 0.05), fr.offset_rows(3, 3, 16, 30.0, 0.05)
    D, tol = fr.truth(x, q)
    for i in range(3):
        for j in range(7):
            a = [float(np.float16(v)) for v in q[i]]
            b = [float(np.float16(v)) for v in x[j]]
            want = math.fsum((s - t) ** 2 for s, t in zip(a, b))
            na, nb = math.sqrt(math.fsum(s * s for s in a)), math.sqrt(math.fsum(t * t for t in b))
            assert abs(D[i, j] - want) <= 1e-9 * (na + nb) ** 2
            assert math.isclose(tol[i, j], 19 * 2.0 ** -23 * (na + nb) ** 2, rel_tol=1e-12)
    assert (D < 1.0).all() and (tol > 0.1).all()  # the regime: distances far below the norms


def test_the_makers():
    ints, rows = fr.scaled_ints(4, 5, 16, -24)
    assert ints.dtype == np.uint8 and ints.max() < 128 and rows.dtype == np.float32
    assert np.array_equal(rows.astype(np.float64) * 2.0 ** 24, ints.astype(np.float64))
    h = fr.rounded(rows)
    assert np.array_equal(h.astype(np.float64), rows.astype(np.float64))     # exact as halves,
    assert ((h.view(np.uint16) & 0x7c00) == 0).all()                         # ... and every one a subnormal (or zero)
    bi, big = fr.scaled_ints(4, 5, 16, 9)
    assert np.array_equal(bi, ints) and np.array_equal(big, ints.astype(np.float32) * 512)
    assert np.array_equal(fr.rounded(big).astype(np.float32), big) and 127 * 512 < 65504
    r = fr.offset_rows(5, 1000, 16, 2000.0, 1.0)
    assert r.dtype == np.float32 and abs(float(r.mean()) - 2000.0) < 0.1 and 0.9 < float(r.std()) < 1.1
    assert np.array_equal(r, fr.offset_rows(5, 1000, 16, 2000.0, 1.0))


# ---- the bit matrix -----------------------------------------------------------------------------------------------------
def _bits():
    """5 x 40 float32 of few distinct values (many ties), some negative, one NaN, and a mask whose row 3 has 4 members."""
    rng = np.random.default_rng(6)
    B = (rng.integers(-3, 9, (5, 40)).astype(F) * F(0.25)).astype(F)
    B[1, 7] = np.nan
    B[2, :] = F(1.5)  # one value throughout: the order is the labels'
    mask = rng.random((5, 40)) < 0.6
    mask[3] = False
    mask[3, [2, 11, 12, 39]] = True
    mask[1, 7] = True
    return B, mask


def _loop_topk(B, k, mask):
    out_d, out_l = np.full((B.shape[0], k), fr.FLT_MAX, F), np.full((B.shape[0], k), -1, np.int64)
    for i in range(B.shape[0]):
        keys = sorted((float(B[i, j]), j) for j in range(B.shape[1]) if not math.isnan(B[i, j]) and (mask is None or mask[i, j]))
        for s, (v, j) in enumerate(keys[:k]):
            out_d[i, s], out_l[i, s] = v, j
    return out_d, out_l


def _loop_range(B, radius, mask):
    lims, d, l = [0], [], []
    for i in range(B.shape[0]):
        for j in range(B.shape[1]):
            if (mask is None or mask[i, j]) and float(B[i, j]) < float(F(radius)):
                d.append(B[i, j])
                l.append(j)
        lims.append(len(d))
    return np.array(lims, np.uint64), np.array(d, F), np.array(l, np.int64)


def test_topk_of_bits_against_sorted_tuples():
    B, mask = _bits()
    for m in (None, mask):
        for k in (1, 5, 39, 40, 64):
            got, want = fr.topk_of_bits(B, k, m), _loop_topk(B, k, m)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    d, l = fr.topk_of_bits(B, 40, None)
    assert l[1, 39] == -1 and 7 not in l[1] and d[1, 39] == fr.FLT_MAX      # the NaN is never selected
    assert np.array_equal(l[2], np.arange(40))                              # equal values in ascending label
    d, l = fr.topk_of_bits(B, 5, mask)
    assert sorted(l[3, :4]) == [2, 11, 12, 39] and l[3, 4] == -1            # fewer than k members: padded
    assert (np.diff(fr.topk_of_bits(B, 5)[0], axis=1) >= 0).all() and fr.topk_of_bits(B, 5)[0].min() < 0


def test_range_of_bits_against_a_loop():
    B, mask = _bits()
    assert (B == F(0.5)).any()
    for m in (None, mask):
        for radius in (0.5, 0.75, 0.0, -0.5, float(np.nextafter(F(-0.75), F(np.inf))), -np.inf, np.inf, 1.5, 1.5000001):
            got, want = fr.range_of_bits(B, radius, m), _loop_range(B, radius, m)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    lims, d, l = fr.range_of_bits(B, 0.5)
    assert (d < F(0.5)).all() and lims[-1] == (B < F(0.5)).sum()            # strictly: the entries ON the radius stay out
    assert fr.range_of_bits(B, 1.5)[0][3] - fr.range_of_bits(B, 1.5)[0][2] == 0
    assert fr.range_of_bits(B, np.inf)[0][-1] == B.size - 1                 # everything but the NaN
    assert fr.range_of_bits(B, -np.inf)[0][-1] == 0


def test_matrix_of_inverts_range_of_bits():
    B, mask = _bits()
    lims, d, l = fr.range_of_bits(B, np.inf, mask)
    M = fr.matrix_of(lims, d, l, 40)
    keep = mask & ~np.isnan(B)
    assert np.array_equal(np.isnan(M), ~keep) and np.array_equal(M[keep].view(np.uint32), B[keep].view(np.uint32))
