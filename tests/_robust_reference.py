"""Float64 NumPy reference of the robust losses of the resident bundle adjustment (sfm_ba_set_loss).

One iteration is the oracle's damped Gauss-Newton step on the reweighted problem: ``oracle.obs_terms_vec`` gives r, Jp, Jx
of every observation, each is multiplied by sqrt(w(s)), s = |r|^2 / delta^2, and the oracle's own ``ba_reduced_system``
builds [S | rhs] and the back-substitution pieces from the scaled terms (IRLS; no second-order correction)."""
import importlib

import numpy as np

LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY = 0, 1, 2


def _oracle():
    return importlib.import_module("sfm_oracle")


def loss_terms(kind, delta, r):
    """(s, w, rho), each (M,), of residuals r (M, 2).  LOSS_NONE: s = |r|^2, w = 1, rho = s (delta ignored)."""
    e = np.sum(np.square(np.asarray(r, dtype=np.float64)), axis=1)
    if kind == LOSS_NONE:
        return e, np.ones_like(e), e.copy()
    s = e / (delta * delta)
    if kind == LOSS_HUBER:
        big = s > 1.0
        root = np.sqrt(np.where(big, s, 1.0))
        return s, np.where(big, 1.0 / root, 1.0), np.where(big, 2.0 * root - 1.0, s)
    if kind == LOSS_CAUCHY:
        return s, 1.0 / (1.0 + s), np.log1p(s)
    raise ValueError("unknown loss %r" % (kind,))


def cost(kind, delta, r):
    """The minimised cost: delta^2 sum rho(s), or sum |r|^2 without a loss."""
    rho = loss_terms(kind, delta, r)[2]
    return float(np.sum(rho)) * (1.0 if kind == LOSS_NONE else delta * delta)


def state_cost(cams, pts, cam_idx, pt_idx, uv, kind, delta):
    r = _oracle().obs_terms_vec(np.asarray(cams, dtype=np.float64).reshape(-1, 7), np.asarray(pts, dtype=np.float64),
                                cam_idx, pt_idx, uv)[0]
    return cost(kind, delta, r)


def reduced_system(cams, pts, cam_idx, pt_idx, uv, lam, kind, delta, quirks=None):
    """``oracle.ba_reduced_system`` on the sqrt(w)-scaled terms; the dict also holds ``cost`` (of the unscaled
    residuals) and ``w``."""
    oracle = _oracle()
    quirks = oracle.QUIRKS_REFERENCE if quirks is None else quirks
    plain = oracle.obs_terms_vec
    seen = {}

    def scaled(*args, **kwargs):
        r, jp, jx = plain(*args, **kwargs)
        _s, w, _rho = loss_terms(kind, delta, r)
        seen["cost"], seen["w"] = cost(kind, delta, r), w
        if kind == LOSS_NONE:
            return r, jp, jx
        sw = np.sqrt(w)
        return r * sw[:, None], jp * sw[:, None, None], jx * sw[:, None, None]

    oracle.obs_terms_vec = scaled
    try:
        t = oracle.ba_reduced_system(cams, pts, cam_idx, pt_idx, uv, lam, quirks)
    finally:
        oracle.obs_terms_vec = plain
    t.update(seen)
    return t


def ba_robust(cams, pts, cam_idx, pt_idx, uv, lam, iters, kind, delta, trace=None):
    """``oracle.ba_sparse`` with the loss: (cams (V, 7), pts (3, N), costs (iters,)), costs[i] the minimised cost at the
    linearisation point of iteration i.  ``trace`` collects the state after every iteration."""
    cams = np.array(cams, dtype=np.float64, copy=True).reshape(-1, 7)
    pts = np.array(pts, dtype=np.float64, copy=True)
    nv = cams.shape[0]
    costs = np.zeros(iters)
    for it in range(iters):
        t = reduced_system(cams, pts, cam_idx, pt_idx, uv, lam, kind, delta)
        costs[it] = t["cost"]
        delta_p = (np.linalg.inv(t["S"]) @ t["rhs"]).reshape(nv, 7)
        cams = cams + delta_p
        cams[:, 3:7] /= np.sqrt(np.sum(np.square(cams[:, 3:7]), axis=1))[:, None]
        btd = np.zeros_like(t["ex"])
        np.add.at(btd, pt_idx, np.einsum('mij,mi->mj', t["W"], delta_p[cam_idx]))
        pts = pts + np.einsum('pij,pj->pi', t["D_inv"], t["ex"] - btd).T
        if trace is not None:
            trace.append((cams.copy(), pts.copy()))
    return cams, pts, costs


_RUNS = {}


def cached_run(name, cams, pts, cam_idx, pt_idx, uv, lam, iters, kind, delta):
    """``ba_robust`` computed once per ``name`` and left unchanged: (cams, pts, costs)."""
    if name not in _RUNS:
        out = ba_robust(cams, pts, cam_idx, pt_idx, uv, lam, iters, kind, delta)
        for a in out:
            a.setflags(write=False)
        _RUNS[name] = out
    return _RUNS[name]
