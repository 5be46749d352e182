"""The view-pair rule of include/sfm_hip.h (block "view pairs") in NumPy int64: the vocabulary (integer k-means from a
stratified start), the VLAD descriptor of a view (integer residual sums, integer square root), the scores (three float64
operations) with the k best partners of every view, and the sorted list of pairs.  Every function has a brute-force twin
(``*_brute``: Python loops over keys, a sort of all candidates, a double loop over the pairs) that the host tests compare it
with.  Also the synthetic band scene of the quality record."""
import math

import numpy as np

M64 = (1 << 64) - 1
MAX_WORDS, MAX_LEN, MAX_K = 1024, 131072, 64
CAP_DEFAULT, CAP_MAX = 1 << 20, 1 << 22
NEG_INF = -np.inf


# ---- the start ---------------------------------------------------------------------------------------------------------------
def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def train_rows(N, train_cap=0):
    """The rows of the concatenation that are trained on (Python integers: no overflow)."""
    cap = train_cap if train_cap else CAP_DEFAULT
    if N <= cap:
        return np.arange(N, dtype=np.int64)
    return np.array([j * N // cap for j in range(cap)], dtype=np.int64)


def init_rows(N, K, seed, train_cap=0):
    rows = train_rows(N, train_cap)
    T = rows.shape[0]
    out = np.zeros(K, dtype=np.int64)
    for w in range(K):
        lo, hi = w * T // K, (w + 1) * T // K
        out[w] = rows[lo + mix((seed * K + w) & M64) % (hi - lo)]
    return out


# ---- assignment ----------------------------------------------------------------------------------------------------------------
def sqdist(X, C):
    """s(x, c) for every row and word, int64.  The products go through float64 (exact: every sum stays below 2^53)."""
    Xf, Cf = X.astype(np.float64), C.astype(np.float64)
    dot = (Xf @ Cf.T).astype(np.int64)
    return (Xf * Xf).sum(1).astype(np.int64)[:, None] + (Cf * Cf).sum(1).astype(np.int64)[None, :] - 2 * dot


def assign(X, C):
    """a(j) = argmin_w (s, w) and s(x_j, c_a(j)); np.argmin takes the first minimum: the lower word."""
    if X.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    a, s = [], []
    for i in range(0, X.shape[0], 1 << 16):
        d = sqdist(X[i:i + (1 << 16)], C)
        ai = np.argmin(d, axis=1)
        a.append(ai)
        s.append(d[np.arange(d.shape[0]), ai])
    return np.concatenate(a).astype(np.int64), np.concatenate(s)


def assign_brute(X, C):
    a, s = np.zeros(X.shape[0], dtype=np.int64), np.zeros(X.shape[0], dtype=np.int64)
    for j in range(X.shape[0]):
        best = None
        for w in range(C.shape[0]):
            d = sum((int(x) - int(c)) ** 2 for x, c in zip(X[j], C[w]))
            if best is None or (d, w) < best:
                best = (d, w)
        s[j], a[j] = best
    return a, s


# ---- the vocabulary ------------------------------------------------------------------------------------------------------------
def _sums(X, a, K):
    S = np.zeros((K, X.shape[1]), dtype=np.int64)
    n = np.bincount(a, minlength=K).astype(np.int64)
    if X.shape[0]:                                           # the rows sorted by word, one segment sum per word that has rows
        order = np.argsort(a, kind="stable")
        first = np.concatenate(([0], np.cumsum(n)[:-1]))
        S[n > 0] = np.add.reduceat(X[order].astype(np.int64), first[n > 0], axis=0)
    return S, n


def _sums_brute(X, a, K):
    S, n = np.zeros((K, X.shape[1]), dtype=np.int64), np.zeros(K, dtype=np.int64)
    for j in range(X.shape[0]):
        n[a[j]] += 1
        for d in range(X.shape[1]):
            S[a[j], d] += int(X[j, d])
    return S, n


def train(X_all, K, iters, seed, train_cap=0, brute=False):
    """``words`` uint8 (K, D) and ``log`` int64 (iters + 1, 3) from the concatenation ``X_all`` (N, D) uint8."""
    N = X_all.shape[0]
    X = X_all[train_rows(N, train_cap)]
    assert X.shape[0] >= K
    C = X_all[init_rows(N, K, seed, train_cap)].astype(np.int64)
    fa, fs = (assign_brute, _sums_brute) if brute else (assign, _sums)
    log = np.zeros((iters + 1, 3), dtype=np.int64)
    for r in range(iters + 1):
        a, s = fa(X, C)
        S, n = fs(X, a, K)
        log[r, 0], log[r, 1] = s.sum(), (n == 0).sum()
        if r == iters:
            break
        new = C.copy()
        has = n > 0
        new[has] = (2 * S[has] + n[has, None]) // (2 * n[has, None])
        log[r, 2] = np.any(new != C, axis=1).sum()
        C = new
    return C.astype(np.uint8), log


# ---- the descriptor of a view -----------------------------------------------------------------------------------------------------
def isqrt(v):
    """The exact floor square root of non-negative int64."""
    v = np.asarray(v, dtype=np.int64)
    s = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    s = np.where(s * s > v, s - 1, s)
    return np.where((s + 1) * (s + 1) <= v, s + 1, s)


def describe(C, views, brute=False):
    """desc int8 (V, K D), norm2 int64 (V,), word_count int32 (V, K), assign int32 (keys,), residual int32 (V, K D)."""
    C = C.astype(np.int64)
    K, D = C.shape
    V = len(views)
    desc, res = np.zeros((V, K * D), dtype=np.int8), np.zeros((V, K * D), dtype=np.int32)
    norm2, count, assigned = np.zeros(V, dtype=np.int64), np.zeros((V, K), dtype=np.int32), []
    for v, X in enumerate(views):
        X = np.asarray(X).reshape(-1, D)
        if brute:
            a, _ = assign_brute(X, C)
            r = np.zeros((K, D), dtype=np.int64)
            n = np.zeros(K, dtype=np.int64)
            for i in range(X.shape[0]):
                n[a[i]] += 1
                for d in range(D):
                    r[a[i], d] += int(X[i, d]) - int(C[a[i], d])
            q = np.zeros((K, D), dtype=np.int64)
            for w in range(K):
                for d in range(D):
                    q[w, d] = (1 if r[w, d] >= 0 else -1) * min(math.isqrt(abs(int(r[w, d]))), 127)
        else:
            a, _ = assign(X, C)
            S, n = _sums(X, a, K)
            r = S - n[:, None] * C
            q = np.sign(r) * np.minimum(isqrt(np.abs(r)), 127)
        desc[v], res[v], count[v], norm2[v] = q.reshape(-1), r.reshape(-1), n, (q * q).sum()
        assigned.append(a)
    return dict(desc=desc, norm2=norm2, word_count=count, assign=np.concatenate(assigned).astype(np.int32) if V else np.zeros(0, np.int32),
                residual=res)


# ---- scores, neighbours, pairs ------------------------------------------------------------------------------------------------
def score(dot, na, nb):
    """(double)dot / sqrt((double)na * (double)nb): three correctly rounded float64 operations."""
    with np.errstate(divide="ignore", invalid="ignore"):
        f = lambda x: np.asarray(x, dtype=np.float64)
        return f(dot) / np.sqrt(f(na) * f(nb))


def neighbours(dot, norm2, k, min_score):
    V = dot.shape[0]
    nbr, nbr_score = np.full((V, k), -1, dtype=np.int32), np.full((V, k), NEG_INF)
    idx = np.arange(V)
    for a in range(V):
        if norm2[a] <= 0:
            continue
        ok = (idx != a) & (norm2 > 0)
        sc = np.full(V, NEG_INF)
        sc[ok] = score(dot[a, ok], norm2[a], norm2[ok])
        ok &= sc >= min_score
        cand = idx[ok]
        order = cand[np.lexsort((cand, -sc[cand]))][:k]
        nbr[a, :order.shape[0]], nbr_score[a, :order.shape[0]] = order, sc[order]
    return nbr, nbr_score


def neighbours_brute(desc, norm2, k, min_score):
    V = desc.shape[0]
    nbr, nbr_score = np.full((V, k), -1, dtype=np.int32), np.full((V, k), NEG_INF)
    for a in range(V):
        cands = []
        for b in range(V):
            if b == a or norm2[a] <= 0 or norm2[b] <= 0:
                continue
            dot = sum(int(x) * int(y) for x, y in zip(desc[a], desc[b]))
            sc = float(dot) / math.sqrt(float(int(norm2[a])) * float(int(norm2[b])))
            if sc >= min_score:
                cands.append((-sc, b))
        for j, (neg, b) in enumerate(sorted(cands)[:k]):
            nbr[a, j], nbr_score[a, j] = b, -neg
    return nbr, nbr_score


def listing(nbr, V, mutual, sequential):
    """The listed pairs a < b in lexicographic order with their `how` bits."""
    lists = [set(int(x) for x in row if x >= 0) for row in nbr]
    pairs, how = [], []
    for a in range(V):
        partners = set(b for b in lists[a] if b > a) | set(b for b in range(a + 1, V) if a in lists[b])
        partners |= set(range(a + 1, min(V - 1, a + sequential) + 1))
        for b in sorted(partners):
            h = (1 if b in lists[a] else 0) | (2 if a in lists[b] else 0) | (4 if b - a <= sequential else 0)
            if (h & 4) or ((h & 3) == 3 if mutual else (h & 3) != 0):
                pairs.append((a, b)); how.append(h)
    return np.array(pairs, dtype=np.int32).reshape(-1, 2), np.array(how, dtype=np.int32)


def listing_brute(nbr, V, mutual, sequential):
    pairs, how = [], []
    for a in range(V):
        for b in range(a + 1, V):
            fwd, bwd, seq = b in list(nbr[a]), a in list(nbr[b]), b - a <= sequential
            if seq or ((fwd and bwd) if mutual else (fwd or bwd)):
                pairs.append((a, b)); how.append(int(fwd) + 2 * int(bwd) + 4 * int(seq))
    return np.array(pairs, dtype=np.int32).reshape(-1, 2), np.array(how, dtype=np.int32)


def pairs(desc, norm2, k, min_score=NEG_INF, mutual=False, sequential=0, brute=False):
    """Everything sfm_view_pairs returns, uncapped: nbr, nbr_score, pairs, how, pair_score, dot, n_pairs."""
    desc = np.asarray(desc, dtype=np.int8)
    norm2 = np.asarray(norm2, dtype=np.int64)
    V = desc.shape[0]
    d64 = desc.astype(np.float64)                            # exact: |dot| < 2^31
    dot = (d64 @ d64.T).astype(np.int64)
    if brute:
        nbr, nbr_score = neighbours_brute(desc, norm2, k, min_score)
        pr, how = listing_brute(nbr, V, bool(mutual), int(sequential))
    else:
        nbr, nbr_score = neighbours(dot, norm2, k, min_score)
        pr, how = listing(nbr, V, bool(mutual), int(sequential))
    ps = np.full(pr.shape[0], NEG_INF)
    for i, (a, b) in enumerate(pr):
        if norm2[a] > 0 and norm2[b] > 0:
            ps[i] = score(dot[a, b], norm2[a], norm2[b])
    return dict(nbr=nbr, nbr_score=nbr_score, pairs=pr, how=how, pair_score=ps, dot=dot.astype(np.int32), n_pairs=pr.shape[0])


def select(views, K, iters, seed, k, min_score=NEG_INF, mutual=False, sequential=0, train_cap=0, words=None):
    """The three steps in a row, as ``processors.select_pairs`` drives them."""
    X_all = np.concatenate([np.asarray(v).reshape(-1, views[0].shape[1]) for v in views])
    log = None
    if words is None:
        words, log = train(X_all, K, iters, seed, train_cap)
    d = describe(words, views)
    p = pairs(d["desc"], d["norm2"], k, min_score, mutual, sequential)
    return words, log, d, p


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the band scene of the quality record ---------------------------------------------------------------------------------------
def _landmark_descriptors(rng, n, D):
    d = np.abs(rng.standard_normal((n, D)))
    d[rng.random((n, D)) < 0.3] = 0.0
    d *= 512.0 / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    return np.minimum(d, 255.0)


def band_scene(V, seed, per_view=600, D=128, reach=1.5, p_seen=0.8, noise=15.0):
    """Views 0 .. V - 1 on a band: per_view * V landmarks at positions uniform in [0, V); view a sees a landmark within `reach`
    of a with probability p_seen; an observation adds N(0, noise) per dimension and is rounded to uint8; each view adds half
    as many unrelated keys again; its rows are shuffled.  Returns the list of uint8 (n_a, D) arrays."""
    rng = np.random.default_rng(seed)
    n_land = per_view * V
    pos = rng.uniform(0.0, V, n_land)
    land = _landmark_descriptors(rng, n_land, D)
    views = []
    for a in range(V):
        seen = np.nonzero((np.abs(pos - a) <= reach) & (rng.random(n_land) < p_seen))[0]
        base = np.vstack((land[seen], _landmark_descriptors(rng, seen.shape[0] // 2, D)))
        obs = np.clip(np.rint(base + rng.normal(0.0, noise, base.shape)), 0, 255).astype(np.uint8)
        views.append(obs[rng.permutation(obs.shape[0])])
    return views
