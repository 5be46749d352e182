"""The track-linking rule of include/sfm_hip.h (block "track linking") in plain NumPy / Python, and the cases the tests run.

The labels are reached by two routes that share nothing: a sequential union-find over the used matches in their given order,
and repeated minimum propagation over the edges to a fixed point.  A case is SETTLED iff both routes agree in every output;
tests/test_track_link_host.py asserts that every case is.  Everything after the labels (sizes, verdicts, numbering, the CSR) is
written once, from the rule's steps 3-5."""
import numpy as np

UNMATCHED, SHORT, CONFLICT = -1, -2, -3
OUTPUTS = ("key_track", "pt_ptr", "cam_idx", "key_idx", "summary", "label")


def global_ids(case):
    """(ga, gb, used) of every match: the global ids of its two keys and step 1's flag."""
    key_ptr = np.asarray(case["key_ptr"], dtype=np.int64)
    pair_views = np.asarray(case["pair_views"], dtype=np.int64).reshape(-1, 2)
    pair_ptr = np.asarray(case["pair_ptr"], dtype=np.int64)
    a, b = np.asarray(case["a"], dtype=np.int64), np.asarray(case["b"], dtype=np.int64)
    pair_of = np.repeat(np.arange(pair_views.shape[0]), np.diff(pair_ptr))
    ga, gb = key_ptr[pair_views[pair_of, 0]] + a, key_ptr[pair_views[pair_of, 1]] + b
    mask = case.get("mask")
    used = np.ones(a.size, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    return ga, gb, used


def labels_union_find(K, ga, gb):
    """Step 2 by a sequential union-find with full path compression; the root of a set is kept at its minimum."""
    parent = list(range(K))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for x, y in zip(ga.tolist(), gb.tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(g) for g in range(K)], dtype=np.int64).reshape(K)


def labels_propagation(K, ga, gb):
    """Step 2 by minimum propagation: every edge hands the smaller label of its ends to both, every key then takes the label
    of its label, until nothing changes."""
    label = np.arange(K, dtype=np.int64)
    while True:
        before = label.copy()
        low = np.minimum(label[ga], label[gb])
        np.minimum.at(label, ga, low)
        np.minimum.at(label, gb, low)
        label = label[label]
        if np.array_equal(label, before):
            return label


def judge(case, label):
    """Steps 3-5 from the labels."""
    key_ptr = np.asarray(case["key_ptr"], dtype=np.int64)
    V, K, min_len = key_ptr.size - 1, int(key_ptr[-1]), int(case.get("min_len", 2))
    _, _, used = global_ids(case)
    g = np.arange(K, dtype=np.int64)
    view = np.searchsorted(key_ptr, g, side="right") - 1
    size = np.bincount(label, minlength=K)[label] if K else np.zeros(0, dtype=np.int64)
    # two keys of one view in a component: equal (label, view) among the keys
    code = label * max(V, 1) + view
    order = np.argsort(code, kind="stable")
    twice = code[order][1:] == code[order][:-1]
    conflict_label = np.zeros(K, dtype=bool)
    conflict_label[label[order][1:][twice]] = True
    roots = g[(label == g) & (size >= 2)] if K else g
    conflict = conflict_label[roots] | (size[roots] > V)
    short = ~conflict & (size[roots] < min_len)
    kept = ~conflict & ~short
    verdict = np.full(K, UNMATCHED, dtype=np.int64)
    verdict[roots[conflict]] = CONFLICT
    verdict[roots[short]] = SHORT
    verdict[roots[kept]] = np.arange(int(kept.sum()))
    key_track = np.where(size >= 2, verdict[label], UNMATCHED) if K else verdict
    n_tracks = int(kept.sum())
    member = np.flatnonzero(key_track >= 0)                       # ascending global id
    by_track = member[np.argsort(key_track[member], kind="stable")]
    pt_ptr = np.concatenate(([0], np.cumsum(np.bincount(key_track[member], minlength=n_tracks)))).astype(np.int64)
    cam_idx, key_idx = view[by_track], by_track - key_ptr[view[by_track]]
    summary = np.array([int(used.sum()), roots.size, n_tracks, int(conflict.sum()), int(short.sum()), int(pt_ptr[-1]),
                        int(size[roots[kept]].max()) if n_tracks else 0, int(size.max()) if roots.size else 0], dtype=np.int64)
    return {"key_track": key_track.astype(np.int32), "pt_ptr": pt_ptr.astype(np.int32), "cam_idx": cam_idx.astype(np.int32),
            "key_idx": key_idx.astype(np.int32), "summary": summary, "label": label.astype(np.int32)}


def link(case, route="union_find"):
    ga, gb, used = global_ids(case)
    K = int(np.asarray(case["key_ptr"])[-1])
    labels = labels_union_find if route == "union_find" else labels_propagation
    return judge(case, labels(K, ga[used], gb[used]))


def same(x, y):
    return all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in OUTPUTS)


def settle(case):
    """The reference outputs of a case, or AssertionError if the two routes disagree."""
    u, p = link(case, "union_find"), link(case, "propagation")
    assert same(u, p), "the two routes disagree on %s" % case.get("name", "a case")
    return u


_settled = {}


def settled(name):
    """(case, reference outputs) of a named case, computed once and shared: callers must not write into either."""
    if name not in _settled:
        case = CASES[name][1]()
        case["name"] = name
        _settled[name] = (case, settle(case))
    return _settled[name]


# ---- case builders ------------------------------------------------------------------------------------------------------
def make_case(n_keys, pairs, min_len=2, mask=None):
    """n_keys per view; pairs: a list of ((i, j), [(a, b), ...])."""
    key_ptr = np.concatenate(([0], np.cumsum(np.asarray(n_keys, dtype=np.int64)))).astype(np.int32)
    pair_views = np.array([p for p, _ in pairs], dtype=np.int32).reshape(-1, 2)
    counts = [len(m) for _, m in pairs]
    pair_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    ab = np.array([x for _, m in pairs for x in m], dtype=np.int32).reshape(-1, 2)
    case = {"key_ptr": key_ptr, "pair_views": pair_views, "pair_ptr": pair_ptr, "a": np.ascontiguousarray(ab[:, 0]),
            "b": np.ascontiguousarray(ab[:, 1]), "mask": None if mask is None else np.asarray(mask, dtype=np.uint8), "min_len": min_len}
    return case


def through_views(V, order="ascending"):
    """Two keys per view; key 0 of every view is one track of length V over the pairs (v, v + 1), key 1 is matched between
    views 2 t and 2 t + 1 only.  `order` lists the pairs ascending, descending (every union hooks a fresh root: the chain of
    parents is V long before the flatten) or interleaved (even pairs first: V / 2 roots, then all of them hooked)."""
    idx = list(range(V - 1))
    if order == "descending":
        idx = idx[::-1]
    elif order == "interleaved":
        idx = idx[0::2] + idx[1::2][::-1]
    pairs = [((v, v + 1), [(0, 0)] + ([(1, 1)] if v % 2 == 0 else [])) for v in idx]
    return make_case([2] * V, pairs)


def scene(V, N, seed, see=0.5, pair_share=0.6, drop=0.2, false_share=0.0, extra=0.1, min_len=2, n_matches=None):
    """N scene points seen by random subsets of V views; every view's keys are the points it sees, shuffled, and a share of
    keys that see nothing.  A random set of pairs in random orientation; a match for a point both views see survives with
    1 - drop, so tracks fragment; a share of the matches gets a random key of the second view instead, so conflicts arise.
    n_matches cuts the list to exactly that many matches.  case["key_point"] is the scene point of every key (-1: none)."""
    rng = np.random.default_rng(seed)
    sees = rng.random((V, N)) < see
    key_of, key_point, n_keys = [], [], []
    for v in range(V):
        pts = np.flatnonzero(sees[v])
        n_extra = int(round(extra * pts.size))
        slot = rng.permutation(pts.size + n_extra)
        ko = np.full(N, -1, dtype=np.int64)
        ko[pts] = slot[:pts.size]
        kp = np.full(pts.size + n_extra, -1, dtype=np.int64)
        kp[slot[:pts.size]] = pts
        key_of.append(ko); key_point.append(kp); n_keys.append(pts.size + n_extra)
    pairs = []
    for i in range(V):
        for j in range(i + 1, V):
            if rng.random() >= pair_share:
                continue
            r, q = (i, j) if rng.random() < 0.5 else (j, i)
            both = np.flatnonzero(sees[r] & sees[q])
            both = rng.permutation(both[rng.random(both.size) >= drop])
            a, b = key_of[r][both], key_of[q][both].copy()
            wrong = rng.random(both.size) < false_share
            if n_keys[q]:
                b[wrong] = rng.integers(0, n_keys[q], int(wrong.sum()))
            pairs.append(((r, q), list(zip(a.tolist(), b.tolist()))))
    order = rng.permutation(len(pairs))
    pairs = [pairs[k] for k in order]
    if n_matches is not None:
        left, cut = n_matches, []
        for p, m in pairs:
            cut.append((p, m[:left]))
            left -= len(cut[-1][1])
        assert left == 0, "the scene has %d matches too few" % left
        pairs = cut
    case = make_case(n_keys, pairs, min_len=min_len)
    case["key_point"] = np.concatenate(key_point) if key_point else np.zeros(0, dtype=np.int64)
    return case


def two_view_tracks(K, n):
    """Two views of K keys in all (the first holds the odd one), n two-key tracks between them."""
    k0 = (K + 1) // 2
    return make_case([k0, K - k0], [((0, 1), [(k, k) for k in range(n)])])


def _conflict_by_counting():
    pairs = [((0, v), [(0, k) for k in range(500)]) for v in range(1, 10)] + [((1, 0), [(0, k) for k in range(500)])]
    return make_case([500] * 10, pairs)


def _duplicates():
    return make_case([3, 3, 3], [((0, 1), [(0, 0), (0, 0), (1, 2)]), ((0, 1), [(0, 0), (2, 1)]), ((1, 0), [(2, 1), (1, 2)]), ((1, 2), [(0, 0)])])


def _with(case, **changes):
    case = dict(case)
    case.update(changes)
    return case


def permuted(case, seed, matches=True, pairs=True, orientation=True):
    """The same match graph listed differently: matches shuffled inside their pairs, pairs shuffled, pairs turned round."""
    rng = np.random.default_rng(seed)
    pv, ptr = np.asarray(case["pair_views"]).reshape(-1, 2), np.asarray(case["pair_ptr"])
    mask = case.get("mask")
    blocks = []
    for p in range(pv.shape[0]):
        idx = np.arange(ptr[p], ptr[p + 1])
        if matches:
            idx = rng.permutation(idx)
        turn = orientation and rng.random() < 0.5
        a, b = (case["b"][idx], case["a"][idx]) if turn else (case["a"][idx], case["b"][idx])
        blocks.append(((int(pv[p, 1]), int(pv[p, 0])) if turn else (int(pv[p, 0]), int(pv[p, 1])), a, b, None if mask is None else mask[idx]))
    if pairs:
        blocks = [blocks[k] for k in rng.permutation(len(blocks))]
    out = dict(case)
    out["pair_views"] = np.array([blk[0] for blk in blocks], dtype=np.int32).reshape(-1, 2)
    out["pair_ptr"] = np.concatenate(([0], np.cumsum([blk[1].size for blk in blocks]))).astype(np.int64)
    out["a"] = np.concatenate([blk[1] for blk in blocks]).astype(np.int32) if blocks else case["a"]
    out["b"] = np.concatenate([blk[2] for blk in blocks]).astype(np.int32) if blocks else case["b"]
    if mask is not None:
        out["mask"] = np.concatenate([blk[3] for blk in blocks]).astype(np.uint8)
    return out


# name -> (what the case is there for, builder)
CASES = {
    "no_views": ("K = 0, P = 0, M = 0: every launch guarded", lambda: make_case([], [])),
    "no_keys": ("views and a pair, but K = 0", lambda: make_case([0, 0, 0], [((0, 1), [])])),
    "no_pairs": ("P = 0: every key unmatched", lambda: make_case([3, 2, 4], [])),
    "no_matches": ("pairs without matches: M = 0", lambda: make_case([3, 2, 4], [((0, 1), []), ((2, 1), [])])),
    "view_without_keys": ("a view without keys between views with keys: the view search must skip it",
                          lambda: make_case([2, 0, 3, 0], [((0, 2), [(0, 1), (1, 2)])])),
    "one_match": ("one match: one track of two", lambda: make_case([2, 2], [((1, 0), [(1, 0)])])),
    "all_masked": ("every match masked: used = 0", lambda: make_case([2, 2, 2], [((0, 1), [(0, 0), (1, 1)]), ((1, 2), [(0, 0)])], mask=[0, 0, 0])),
    "conflict_small": ("two keys of view 0 joined through views 1 and 2: a conflict of size 4 <= V = 5, next to a clean track",
                       lambda: make_case([2, 2, 2, 1, 1], [((0, 1), [(0, 0)]), ((1, 2), [(0, 0)]), ((2, 0), [(0, 1)]), ((3, 4), [(0, 0)]), ((1, 3), [(1, 0)])])),
    "conflict_by_counting": ("5 000 keys of 10 views in one component, every match at one root: union under contention, size > V",
                             _conflict_by_counting),
    "triangle": ("a consistent triangle of matches is no conflict", lambda: make_case([1, 1, 1], [((0, 1), [(0, 0)]), ((1, 2), [(0, 0)]), ((2, 0), [(0, 0)])])),
    "duplicates": ("duplicate matches, a pair listed twice and in both orientations", _duplicates),
    "mask_split": ("a masked match splits a track of four into two of two",
                   lambda: make_case([1, 1, 1, 1], [((0, 1), [(0, 0)]), ((1, 2), [(0, 0)]), ((2, 3), [(0, 0)])], mask=[1, 0, 1])),
    "chain_descending": ("pairs listed from the last down: every union hooks a fresh root", lambda: through_views(300, "descending")),
    "chain_interleaved": ("even pairs first, then the odd ones from the last down", lambda: through_views(300, "interleaved")),
    "m_1023": ("M = 1 023: the last block of the union grid is short", lambda: scene(6, 700, 31, n_matches=1023)),
    "m_1025": ("M = 1 025: one match into the next block", lambda: scene(6, 700, 32, n_matches=1025)),
    "m_65537": ("M = 65 537: past a full grid of 256 blocks", lambda: scene(14, 3000, 33, see=0.6, pair_share=0.9, drop=0.05, false_share=0.01, n_matches=65537)),
}
for _v in (63, 64, 65, 1023, 1025, 1100):
    CASES["through_%d" % _v] = ("a track through one key of each of %d views: %s" % (
        _v, "the wave boundary of the ordering" if _v < 100 else "the workgroup boundary of the ordering (1 024 members in LDS)"),
        lambda v=_v: through_views(v))
for _n in (1023, 1024, 1025, 2049):
    CASES["tracks_%d" % _n] = ("n_tracks = %d: the chunk boundary of the scan over the components" % _n, lambda n=_n: two_view_tracks(2 * n, n))
    CASES["keys_%d" % _n] = ("K = %d: the chunk boundary of the scan over the keys" % _n, lambda n=_n: two_view_tracks(n, n // 2 - 3))
for _f, _tag in ((0.0, "0"), (0.02, "2"), (0.10, "10")):
    CASES["scene_12_%s" % _tag] = ("12 views x 600 points, %s %% false matches" % _tag, lambda f=_f: scene(12, 600, 41, false_share=f))
    CASES["scene_70_%s" % _tag] = ("70 views x 3 000 points, tracks of about 8, %s %% false matches" % _tag,
                                   lambda f=_f: scene(70, 3000, 42, see=8.0 / 70, pair_share=0.35, drop=0.15, false_share=f))
for _m in (2, 3, 6):
    CASES["min_len_%d" % _m] = ("min_len = %d of V = 6: short tracks leave, conflicts stay conflicts" % _m,
                                lambda m=_m: scene(6, 300, 43, see=0.7, false_share=0.03, min_len=m))
