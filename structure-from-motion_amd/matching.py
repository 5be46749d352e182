"""Host side of ``KeyTracker.__extend_list`` (key_tracker.py:213-317): from the per-query neighbours the device
returns (``native.match``) to the ``KeyTrack.table`` writes, in NumPy, with no Python loop per match.

The steps and the reference lines they replace:

* ``filter_matches`` -- the ``if item`` filter and ``__process_knn_result`` (key_tracker.py:254-271, 337-344): the ratio
  test ``d0 / d1 < 0.7`` in Python floats, crossCheck (only mutual nearest neighbours), or plain 1-NN;
* ``dedup_kept`` -- the duplicate-train-index loop (key_tracker.py:272-291) in closed form (quirk Q14);
* ``table_writes`` -- the inlier filter and the writes (key_tracker.py:301-314), truncated to the number of
  fundamental-matrix inliers when there is one (quirk Q15).
"""
import numpy as np

RATIO = 0.7                   # key_tracker.py:10


def match_mode(is_knn_match, is_cross_check):
    """The device mode of one configuration: knnMatch k = 2 (ratio test), mutual (crossCheck, k = 1 or match()), or 1-NN."""
    from . import native
    if is_cross_check:
        return native.MATCH_MUTUAL
    return native.MATCH_KNN2 if is_knn_match else native.MATCH_NN1


def filter_matches(best_idx, best_dist, second_idx, second_dist, mutual, is_knn_match, is_cross_check):
    """The match list of one (new view, reference view) pair as three arrays in query order:
    (query index, train index, float32 distance).

    Raises what the reference raises (quirk Q16): ``IndexError`` for k = 2 against a reference with a single descriptor
    (``item[1]``), ``ZeroDivisionError`` when a second-best distance is 0 -- at the first query that hits either."""
    best_idx = np.asarray(best_idx); best_dist = np.asarray(best_dist, dtype=np.float32)
    nq = best_idx.shape[0]
    if is_cross_check:
        keep = np.asarray(mutual, dtype=bool) & (best_idx >= 0)          # non-mutual queries give [] (crossCheck), dropped
    elif is_knn_match:
        second_idx = np.asarray(second_idx); second_dist = np.asarray(second_dist, dtype=np.float32)
        if nq:
            no_second = second_idx < 0
            zero = (~no_second) & (second_dist == 0)
            bad = np.flatnonzero(no_second | zero)
            if bad.shape[0]:
                if no_second[bad[0]]:
                    raise IndexError("tuple index out of range")         # item[1] of a one-element knnMatch result
                raise ZeroDivisionError("float division by zero")        # item[0].distance / item[1].distance
        # Python floats: float64 division of the float32 distances
        keep = (best_dist.astype(np.float64) / second_dist.astype(np.float64)) < RATIO if nq else np.zeros(0, dtype=bool)
    else:
        keep = best_idx >= 0
    q = np.flatnonzero(keep)
    return q, best_idx[q].astype(np.int64), best_dist[q]


def filter_guided(best_idx, best_dist, second_dist, mutual, ratio=RATIO):
    """The match list of one (reference view, query view) pair after a guided match (``native.match_guided``), as
    (query index, train index) in query order: query ``i`` is kept iff it has a best neighbour, is mutual, and either has
    no second neighbour (``second_dist`` = inf: the gate left one candidate) or ``float64(d0) < ratio * float64(d1)``.
    A zero second distance keeps nothing for that query and raises nothing; ``filter_matches`` and its quirks
    (Q14 - Q16) are not involved."""
    best_idx = np.asarray(best_idx)
    d0 = np.asarray(best_dist, dtype=np.float32).astype(np.float64)
    d1 = np.asarray(second_dist, dtype=np.float32).astype(np.float64)
    keep = (best_idx >= 0) & np.asarray(mutual, dtype=bool) & (np.isposinf(d1) | (d0 < float(ratio) * d1))
    q = np.flatnonzero(keep)
    return q, best_idx[q].astype(np.int64)


def dedup_kept(train_idx, dist):
    """Positions (into the filtered list) of the matches the duplicate loop of key_tracker.py:276-291 keeps, in the
    order of its output list.

    Quirk Q14: the output has one entry per distinct train index t, at p(t) = the rank of t's first appearance among
    the distinct train indices.  A later match i with train index t replaces that entry iff
    ``dist[i] < dist[p(t)]`` -- the FILTERED list's element at position p(t) (key_tracker.py:283), not the kept one --
    so the kept entry is the last later match of t with ``dist[i] < dist[p(t)]``, or t's first appearance."""
    train_idx = np.asarray(train_idx)
    dist = np.asarray(dist)
    n = train_idx.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    _uniq, first, inverse = np.unique(train_idx, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")          # distinct train indices by first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    pos = np.arange(n)
    thr = dist[rank[inverse]]                         # matches[p(t)].distance for every i
    cand = np.flatnonzero((pos > first[inverse]) & (dist < thr))
    kept = first.astype(np.int64)
    if cand.shape[0]:
        np.maximum.at(kept, inverse[cand], cand)      # the last replacing match wins
    return kept[order]


def table_writes(query_idx, train_idx, dist, n_inliers=None):
    """(query indices, train indices) the reference writes for one pair (key_tracker.py:301-314): the deduplicated
    list, cut to its first ``n_inliers`` entries when the fundamental-matrix inliers are used (quirk Q15: only their
    NUMBER matters; the train indices of the kept list are distinct, so ``ref_key_idx in inlier_ref_incides`` selects
    exactly that prefix)."""
    kept = dedup_kept(train_idx, dist)
    if n_inliers is not None:
        kept = kept[:int(n_inliers)]
    return np.asarray(query_idx)[kept], np.asarray(train_idx)[kept]


def dedup_matches(query_idx, train_idx, dist):
    """The deduplicated match list as (query, train, distance) arrays (what ``__build_key_match_arr`` reads)."""
    kept = dedup_kept(train_idx, dist)
    return np.asarray(query_idx)[kept], np.asarray(train_idx)[kept], np.asarray(dist)[kept]
