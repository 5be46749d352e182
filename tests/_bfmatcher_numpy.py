"""NumPy stand-in for ``cv2.BFMatcher`` (test code only; the package never imports it).

It implements the matching contract of INTEGRATION.md (how OpenCV 4.x ``batchDistance`` / ``BFMatcher`` behave as
read from their documentation and source, not checked against cv2, which is not installed):

* NORM_L2: d = float32(sqrt(s)) correctly rounded, s = sum (a - b)^2 exact in int64 for integer-valued rows (the
  float64 GEMM of integers below 2^53 is exact), else float64 then rounded;
* NORM_HAMMING: popcount(a ^ b) over uint8 rows, as a float;
* neighbours ordered by (d, train index); crossCheck keeps mutual nearest neighbours only (ties to the lower index
  in both directions), knnMatch then gives [] for the other queries.
"""
import numpy as np

NORM_L2 = 4
NORM_HAMMING = 6
_BLOCK = 512


class DMatch:
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx, trainIdx, distance):
        self.queryIdx = int(queryIdx)
        self.trainIdx = int(trainIdx)
        self.imgIdx = 0
        self.distance = float(distance)

    def __repr__(self):
        return "DMatch(%d, %d, %r)" % (self.queryIdx, self.trainIdx, self.distance)


def sqrt_rn_f32(s):
    """float32(sqrt(s)) correctly rounded for non-negative integers s < 2^53 (array)."""
    s = np.asarray(s, dtype=np.float64)
    d = np.sqrt(s).astype(np.float32)
    bits = d.view(np.uint32)
    pred = np.where(bits > 0, bits - 1, 0).astype(np.uint32).view(np.float32).astype(np.float64)
    succ = (bits + 1).astype(np.uint32).view(np.float32).astype(np.float64)
    dd = d.astype(np.float64)
    mlo, mhi = 0.5 * (pred + dd), 0.5 * (dd + succ)
    out = np.where((s < mlo * mlo) & (s > 0), pred, np.where(s > mhi * mhi, succ, dd))
    return out.astype(np.float32)


def _is_integer_rows(a):
    return a.dtype.kind in "ui" or (np.all(np.isfinite(a)) and np.array_equal(a, np.round(a)))


def distances(norm, query, train):
    """(Q, T) float32 distances of the contract."""
    q = np.asarray(query); t = np.asarray(train)
    if norm == NORM_HAMMING:
        qb = np.unpackbits(q.astype(np.uint8), axis=1).astype(np.float64)
        tb = np.unpackbits(t.astype(np.uint8), axis=1).astype(np.float64)
        h = qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2.0 * (qb @ tb.T)
        return h.astype(np.float32)
    qf = q.astype(np.float64); tf = t.astype(np.float64)
    if _is_integer_rows(q) and _is_integer_rows(t):
        s = (qf * qf).sum(1)[:, None] + (tf * tf).sum(1)[None, :] - 2.0 * (qf @ tf.T)
        return sqrt_rn_f32(np.rint(s))
    diff = qf[:, None, :] - tf[None, :, :]
    return np.sqrt((diff * diff).sum(-1)).astype(np.float32)


def _keys(d, idx_axis):
    """uint64 (d bits << 32 | index along idx_axis): one min orders by (d, index)."""
    hi = d.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)
    shape = [1, 1]
    shape[idx_axis] = d.shape[idx_axis]
    return hi | np.arange(d.shape[idx_axis], dtype=np.uint64).reshape(shape)


def neighbours(norm, query, train, k=2, col_best=False):
    """Per query the k best (train index, distance) by (d, index) -- index -1 / inf when T < k -- and, with col_best,
    the best query index of every train column.  Computed in query blocks."""
    query = np.asarray(query); train = np.asarray(train)
    nq, nt = query.shape[0], train.shape[0]
    idx = np.full((nq, k), -1, dtype=np.int64)
    dist = np.full((nq, k), np.inf, dtype=np.float32)
    cbest = np.full(nt, np.iinfo(np.uint64).max, dtype=np.uint64)
    for q0 in range(0, nq, _BLOCK):
        d = distances(norm, query[q0:q0 + _BLOCK], train)
        keys = _keys(d, 1)
        for j in range(min(k, nt)):
            m = keys.argmin(1)
            idx[q0:q0 + d.shape[0], j] = m
            dist[q0:q0 + d.shape[0], j] = d[np.arange(d.shape[0]), m]
            keys[np.arange(d.shape[0]), m] = np.iinfo(np.uint64).max
        if col_best and nt:
            ck = (d.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
                np.arange(q0, q0 + d.shape[0], dtype=np.uint64)[:, None]
            cbest = np.minimum(cbest, ck.min(0))
    cb = (cbest & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return idx, dist, cb


class BFMatcher:
    def __init__(self, normType=NORM_L2, crossCheck=False):
        self.normType = normType
        self.crossCheck = bool(crossCheck)

    def _mutual(self, query, train):
        idx, dist, cb = neighbours(self.normType, query, train, k=1, col_best=True)
        q = np.arange(idx.shape[0])
        ok = (idx[:, 0] >= 0) & (cb[np.maximum(idx[:, 0], 0)] == q)
        return idx[:, 0], dist[:, 0], ok

    def knnMatch(self, queryDescriptors, trainDescriptors, k=2):
        if self.crossCheck:
            if k != 1:
                raise ValueError("crossCheck needs k == 1")
            b, d, ok = self._mutual(queryDescriptors, trainDescriptors)
            return [[DMatch(i, b[i], d[i])] if ok[i] else [] for i in range(b.shape[0])]
        idx, dist, _ = neighbours(self.normType, queryDescriptors, trainDescriptors, k=k)
        return [tuple(DMatch(i, idx[i, j], dist[i, j]) for j in range(k) if idx[i, j] >= 0) for i in range(idx.shape[0])]

    def match(self, queryDescriptors, trainDescriptors):
        if self.crossCheck:
            b, d, ok = self._mutual(queryDescriptors, trainDescriptors)
            return [DMatch(i, b[i], d[i]) for i in np.flatnonzero(ok)]
        idx, dist, _ = neighbours(self.normType, queryDescriptors, trainDescriptors, k=1)
        return [DMatch(i, idx[i, 0], dist[i, 0]) for i in range(idx.shape[0]) if idx[i, 0] >= 0]
