"""numpy restatement of the reconstruction contract, ROTATED space, for IVFADC and Grouping corpora of
synth.make_corpus().  Every step is one float32 operation on float32 operands, so the result is the device's bit for bit.

Resident row r = position r of the corpus' ids / codes / norm_codes arrays (upload order)."""
import numpy as np

EMPTY_BITS = np.uint32(0x7FC00000)


def quantizer_vectors(c):
    """V: the vectors the quantizer holds at search time (rotated when the corpus has OPQ)."""
    return np.ascontiguousarray(c["graph"].vectors, np.float32)


def row_lists(offsets, rows):
    """The list of every row: the last c with offsets[c] <= r (empty lists are skipped)."""
    off = np.asarray(offsets).astype(np.int64)
    return (np.searchsorted(off, np.asarray(rows, np.int64), side="right") - 1).astype(np.int64)


def row_subgroups(offsets, subgroup_sizes, rows):
    """(list, sub-group) of every row of a Grouping index: the sub-groups of a list lie end to end."""
    rows = np.asarray(rows, np.int64)
    lst = row_lists(offsets, rows)
    pos = rows - np.asarray(offsets).astype(np.int64)[lst]
    ends = np.cumsum(np.asarray(subgroup_sizes).astype(np.int64), axis=1)[lst]   # [n, nsubc]
    sub = (pos[:, None] >= ends).sum(1)
    return lst, np.minimum(sub, ends.shape[1] - 1)


def anchors(c, rows):
    """float32 [n, d]: V[c], or for Grouping V[c] + alpha[c] * (V[nn[c][s]] + (-1 * V[c]))."""
    V = quantizer_vectors(c)
    if not c["nsubc"]:
        return V[row_lists(c["offsets"], rows)]
    lst, sub = row_subgroups(c["offsets"], c["subgroup_sizes"], rows)
    vc = V[lst]
    vn = V[np.asarray(c["nn_centroid_idxs"])[lst, sub]]
    alpha = np.asarray(c["alphas"], np.float32)[lst][:, None]
    cv = vn + np.float32(-1.0) * vc
    return (vc + alpha * cv).astype(np.float32)


def decode(c, rows):
    """float32 [n, d]: the code words of the rows' codes."""
    cb = np.asarray(c["pq_centroids"], np.float32)
    codes = np.asarray(c["codes"])[np.asarray(rows, np.int64)]
    M, _, dsub = cb.shape
    out = np.empty((len(codes), M * dsub), np.float32)
    for m in range(M):
        out[:, m * dsub:(m + 1) * dsub] = cb[m][codes[:, m]]
    return out


def recon_rotated(c, rows=None):
    """float32 [n, d] of the given resident rows (all of them by default); a row of -1 is an empty slot."""
    n_local = len(c["ids"])
    rows = np.arange(n_local, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).ravel()
    ok = rows >= 0
    safe = np.where(ok, rows, 0)
    out = np.empty((len(rows), c["d"]), np.float32)
    if n_local:
        out[:] = anchors(c, safe) + decode(c, safe)
    out.view(np.uint32)[~ok] = EMPTY_BITS
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
