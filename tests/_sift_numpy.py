"""NumPy stand-in for ``cv2.SIFT_create().detectAndCompute(img, None)`` (test code only; the package never imports it).

It restates OpenCV 4.6's SIFT with its ``SIFT_create()`` defaults (nfeatures=0, nOctaveLayers=3,
contrastThreshold=0.04, edgeThreshold=10, sigma=1.6, CV_32F descriptors) as read from OpenCV's source and
documentation.  It was NOT checked against cv2, which is not installed; INTEGRATION.md ('SIFT detection') lists the
contract and where it departs from cv2 on purpose.  Every floating-point step is written out so that the HIP kernels
of csrc/sfm_sift.hip can repeat it:

* float32 everywhere, every product and sum rounded on its own (NumPy never fuses a multiply-add);
* the separable blur accumulates the taps from the leftmost one up, the row pass before the column pass;
* the 3x3 refinement solve is Gaussian elimination with partial pivoting, scalar by scalar (``_solve3``);
* transcendental functions (exp, atan2 in degrees, cos, sin, exp2) are evaluated in float64 and rounded to float32
  (``precise=True``, the contract; cv2 uses ``fastAtan2``), or in float32 (``precise=False``, a second valid
  stand-in whose distance from the first sizes the tolerances of the GPU tests);
* histogram bins are summed in sample order.
"""
import numpy as np

F32 = np.float32
FLT_EPSILON = F32(np.finfo(np.float32).eps)
IMG_BORDER = 5
MAX_INTERP_STEPS = 5
ORI_HIST_BINS = 36
DESCR_WIDTH = 4
DESCR_HIST_BINS = 8
INT_MAX_3 = F32(2147483647 // 3)


class Params:
    def __init__(self, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6):
        if int(n_octave_layers) < 1 or int(n_octave_layers) > 16:
            raise ValueError("n_octave_layers must be in [1, 16]")
        if not (contrast_threshold >= 0) or not (edge_threshold > 0) or not (sigma > 0):
            raise ValueError("bad SIFT parameters")
        self.L = int(n_octave_layers)
        self.contrast = float(contrast_threshold)
        self.edge = float(edge_threshold)
        self.sigma = float(sigma)


# ---- image preparation -----------------------------------------------------------------------------------------
def to_gray(img):
    """(H, W) uint8 as is; (H, W, 3) uint8 is BGR -> cvtColor's fixed-point rule.  Returns float32 in [0, 255]."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.size == 0 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError("SIFT input must be a non-empty (H, W) or (H, W, 3) uint8 image, got %s %s" % (a.dtype, a.shape))
    if a.ndim == 3:
        b, g, r = (a[..., i].astype(np.int32) for i in range(3))
        a = (1868 * b + 9617 * g + 4899 * r + 8192) >> 14
    return a.astype(F32)


def upsample2(g):
    """x2 bilinear with half-pixel centres: weights 0.75 / 0.25, border replicated; along x, then along y."""
    def along(a, axis):
        n = a.shape[axis]
        i = np.arange(n)
        lo, hi = np.take(a, np.maximum(i - 1, 0), axis), np.take(a, np.minimum(i + 1, n - 1), axis)
        even = F32(0.75) * a + F32(0.25) * lo
        odd = F32(0.75) * a + F32(0.25) * hi
        out = np.stack((even, odd), axis=axis + 1)
        shape = list(a.shape)
        shape[axis] = 2 * n
        return out.reshape(shape)
    return along(along(g, 1), 0)


def octave_count(h, w):
    """cvRound(log2(min side of the x2 base image) - 2) - firstOctave (rint: half to even)."""
    return int(np.rint(np.log2(float(min(2 * h, 2 * w))) - 2)) + 1


def gaussian_kernel(sigma):
    """ksize = rint(8 sigma + 1) | 1 taps; float64 weights, normalised, rounded to float32."""
    ksize = int(np.rint(sigma * 8 + 1)) | 1
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    t = np.exp((-0.5 / (sigma * sigma)) * x * x)
    total = 0.0
    for v in t:                                        # sequential, as the library sums them
        total += v
    return (t * (1.0 / total)).astype(F32)


def reflect101(idx, n):
    idx = np.array(idx, dtype=np.int64)
    if n == 1:
        return np.zeros_like(idx)
    while True:
        lo, hi = idx < 0, idx >= n
        if not (lo.any() or hi.any()):
            return idx
        idx = np.where(lo, -idx, idx)
        idx = np.where(idx >= n, 2 * n - 2 - idx, idx)


def blur(img, sigma):
    w = gaussian_kernel(sigma)
    r = len(w) // 2
    h, wd = img.shape
    tmp = None
    cols = np.arange(wd)
    for t in range(len(w)):
        p = w[t] * img[:, reflect101(cols + t - r, wd)]
        tmp = p if tmp is None else tmp + p
    out = None
    rows = np.arange(h)
    for t in range(len(w)):
        p = w[t] * tmp[reflect101(rows + t - r, h), :]
        out = p if out is None else out + p
    return out


def level_sigmas(p):
    """sig[0] = sigma, sig[i] = sqrt((k^i sigma)^2 - (k^(i-1) sigma)^2), k = 2^(1/L) (float64)."""
    k = 2.0 ** (1.0 / p.L)
    sig = [p.sigma]
    for i in range(1, p.L + 3):
        prev = k ** (i - 1) * p.sigma
        tot = prev * k
        sig.append(float(np.sqrt(tot * tot - prev * prev)))
    return sig


def base_sigma(p):
    s = F32(p.sigma)
    return float(np.sqrt(max(s * s - F32(0.5) * F32(0.5) * F32(4), F32(0.01))))


def _down(img):
    """resize to (rows / 2, cols / 2) with INTER_NEAREST: pixel (2y, 2x), a trailing odd row / column dropped."""
    h, w = img.shape
    return img[0:2 * (h // 2):2, 0:2 * (w // 2):2].copy()


def build_pyramid(gray, p):
    h, w = gray.shape
    n_oct = octave_count(h, w)
    if n_oct <= 0:
        return [], []
    sig = level_sigmas(p)
    gauss = []
    for o in range(n_oct):
        lev = [blur(upsample2(gray), base_sigma(p)) if o == 0 else _down(gauss[o - 1][p.L])]
        for i in range(1, p.L + 3):
            lev.append(blur(lev[i - 1], sig[i]))
        gauss.append(lev)
    dog = [[g[i + 1] - g[i] for i in range(p.L + 2)] for g in gauss]
    return gauss, dog


# ---- extrema and refinement ------------------------------------------------------------------------------------
def _solve3(a, b):
    """H x = b for a batch: Gaussian elimination with partial pivoting, float32, one rounding per operation.
    a: (n, 3, 3), b: (n, 3).  Returns (x, ok); a zero pivot gives ok = False and x = 0 (cv::Matx::solve's zeros)."""
    a = a.astype(F32).copy()
    b = b.astype(F32).copy()
    n = a.shape[0]
    ar = np.arange(n)
    piv = np.zeros(n, dtype=np.int64)
    piv = np.where(np.abs(a[:, 1, 0]) > np.abs(a[ar, piv, 0]), 1, piv)
    piv = np.where(np.abs(a[:, 2, 0]) > np.abs(a[ar, piv, 0]), 2, piv)

    def swap(r0, r1, mask):
        ra, rb = a[ar, r0].copy(), a[ar, r1].copy()
        ba, bb = b[ar, r0].copy(), b[ar, r1].copy()
        a[ar, r0] = np.where(mask[:, None], rb, ra)
        a[ar, r1] = np.where(mask[:, None], ra, rb)
        b[ar, r0] = np.where(mask, bb, ba)
        b[ar, r1] = np.where(mask, ba, bb)

    swap(np.zeros(n, dtype=np.int64), piv, piv != 0)
    ok = a[:, 0, 0] != 0
    d0 = np.where(ok, a[:, 0, 0], F32(1))
    for r in (1, 2):
        f = a[:, r, 0] / d0
        a[:, r, 1] = a[:, r, 1] - f * a[:, 0, 1]
        a[:, r, 2] = a[:, r, 2] - f * a[:, 0, 2]
        b[:, r] = b[:, r] - f * b[:, 0]
    swap(np.ones(n, dtype=np.int64), np.full(n, 2), np.abs(a[:, 2, 1]) > np.abs(a[:, 1, 1]))
    ok &= a[:, 1, 1] != 0
    d1 = np.where(a[:, 1, 1] != 0, a[:, 1, 1], F32(1))
    f = a[:, 2, 1] / d1
    a[:, 2, 2] = a[:, 2, 2] - f * a[:, 1, 2]
    b[:, 2] = b[:, 2] - f * b[:, 1]
    ok &= a[:, 2, 2] != 0
    d2 = np.where(a[:, 2, 2] != 0, a[:, 2, 2], F32(1))
    x2 = b[:, 2] / d2
    x1 = (b[:, 1] - a[:, 1, 2] * x2) / d1
    x0 = ((b[:, 0] - a[:, 0, 1] * x1) - a[:, 0, 2] * x2) / d0
    x = np.stack((x0, x1, x2), axis=1)
    return np.where(ok[:, None], x, F32(0)), ok


def _derivs(dg, lay, r, c):
    """dD, the Hessian and the centre value at integer (layer, r, c) of one octave's DoG stack dg (L+2, h, w)."""
    img_scale = F32(1) / F32(255)
    deriv_scale = img_scale * F32(0.5)
    cross_scale = img_scale * F32(0.25)
    at = lambda dl, dr, dc: dg[lay + dl, r + dr, c + dc]
    dD = np.stack(((at(0, 0, 1) - at(0, 0, -1)) * deriv_scale,
                   (at(0, 1, 0) - at(0, -1, 0)) * deriv_scale,
                   (at(1, 0, 0) - at(-1, 0, 0)) * deriv_scale), axis=1)
    v = at(0, 0, 0)
    v2 = v * F32(2)
    dxx = (at(0, 0, 1) + at(0, 0, -1) - v2) * img_scale
    dyy = (at(0, 1, 0) + at(0, -1, 0) - v2) * img_scale
    dss = (at(1, 0, 0) + at(-1, 0, 0) - v2) * img_scale
    dxy = (at(0, 1, 1) - at(0, 1, -1) - at(0, -1, 1) + at(0, -1, -1)) * cross_scale
    dxs = (at(1, 0, 1) - at(1, 0, -1) - at(-1, 0, 1) + at(-1, 0, -1)) * cross_scale
    dys = (at(1, 1, 0) - at(1, -1, 0) - at(-1, 1, 0) + at(-1, -1, 0)) * cross_scale
    hess = np.stack((np.stack((dxx, dxy, dxs), 1), np.stack((dxy, dyy, dys), 1), np.stack((dxs, dys, dss), 1)), 1)
    return dD, hess, v, dxx, dyy, dxy


def find_candidates(dog, p):
    """Scan layers 1..L of every octave (5-pixel border): pre-threshold, then 26-neighbour max / min.
    Returns (o, layer, r, c) int arrays and the margins of the three decisions."""
    thr = F32(np.floor(0.5 * p.contrast / p.L * 255))
    out = []
    for o, dg in enumerate(dog):
        st = np.stack(dg)
        h, w = st.shape[1:]
        if h <= 2 * IMG_BORDER or w <= 2 * IMG_BORDER:
            continue
        for lay in range(1, p.L + 1):
            ctr = st[lay, IMG_BORDER:h - IMG_BORDER, IMG_BORDER:w - IMG_BORDER]
            nmax = np.full(ctr.shape, -np.inf, dtype=F32)
            nmin = np.full(ctr.shape, np.inf, dtype=F32)
            for dl in (-1, 0, 1):
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        if dl == dr == dc == 0:
                            continue
                        nb = st[lay + dl, IMG_BORDER + dr:h - IMG_BORDER + dr, IMG_BORDER + dc:w - IMG_BORDER + dc]
                        nmax = np.maximum(nmax, nb)
                        nmin = np.minimum(nmin, nb)
            hit = (np.abs(ctr) > thr) & (((ctr > 0) & (ctr >= nmax)) | ((ctr < 0) & (ctr <= nmin)))
            rr, cc = np.nonzero(hit)
            v = ctr[rr, cc]
            out.append((np.full(len(rr), o), np.full(len(rr), lay), rr + IMG_BORDER, cc + IMG_BORDER,
                        np.abs(v) - thr, np.where(v > 0, v - nmax[rr, cc], nmin[rr, cc] - v)))
    if not out:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, np.zeros(0, F32), np.zeros(0, F32)
    return tuple(np.concatenate(x) for x in zip(*out))


def refine(dog, p, o, lay, r, c):
    """adjustLocalExtrema for every candidate of one octave.  Returns a dict of kept keypoints (pyramid octave o)."""
    L = p.L
    st = np.stack(dog[o])
    h, w = st.shape[1:]
    n = len(r)
    r, c, lay = r.copy(), c.copy(), lay.copy()
    alive = np.ones(n, dtype=bool)
    done = np.zeros(n, dtype=bool)
    x = np.zeros((n, 3), dtype=F32)
    step_margin = np.full(n, np.inf, dtype=F32)
    half = F32(0.5)
    for _ in range(MAX_INTERP_STEPS):
        act = np.nonzero(alive & ~done)[0]
        if len(act) == 0:
            break
        dD, hess, _, _, _, _ = _derivs(st, lay[act], r[act], c[act])
        sol, _ = _solve3(hess, dD)
        xa = -sol                                       # (xc, xr, xi)
        x[act] = xa
        ax = np.abs(xa)
        conv = (ax < half).all(axis=1)
        step_margin[act] = half - ax.max(axis=1)
        done[act[conv]] = True
        go = act[~conv]
        big = (np.abs(xa[~conv]) > INT_MAX_3).any(axis=1)
        alive[go[big]] = False
        go = go[~big]
        xg = x[go]
        c[go] += np.rint(xg[:, 0]).astype(np.int64)
        r[go] += np.rint(xg[:, 1]).astype(np.int64)
        lay[go] += np.rint(xg[:, 2]).astype(np.int64)
        bad = ((lay[go] < 1) | (lay[go] > L) | (c[go] < IMG_BORDER) | (c[go] >= w - IMG_BORDER)
               | (r[go] < IMG_BORDER) | (r[go] >= h - IMG_BORDER))
        alive[go[bad]] = False
    keep = np.nonzero(alive & done)[0]
    dD, _, v, dxx, dyy, dxy = _derivs(st, lay[keep], r[keep], c[keep])
    xk = x[keep]
    t = dD[:, 0] * xk[:, 0] + dD[:, 1] * xk[:, 1] + dD[:, 2] * xk[:, 2]
    contr = v * (F32(1) / F32(255)) + t * half
    contr_margin = np.abs(contr) * F32(L) - F32(p.contrast)
    tr = dxx + dyy
    det = dxx * dyy - dxy * dxy
    edge = F32(p.edge)
    edge_margin = np.where(det <= 0, np.minimum(det, F32(0)) - F32(1),
                           (edge + F32(1)) * (edge + F32(1)) * det - tr * tr * edge)
    ok = (contr_margin >= 0) & (det > 0) & ~(tr * tr * edge >= (edge + F32(1)) * (edge + F32(1)) * det)
    sel = keep[ok]
    xs = x[sel]
    scale = F32(1 << o)
    arg = (lay[sel].astype(F32) + xs[:, 2]) / F32(L)
    size = F32(p.sigma) * np.exp2(arg.astype(np.float64)).astype(F32) * scale * F32(2)
    octave = (o + (lay[sel] << 8) + (np.rint((xs[:, 2].astype(np.float64) + 0.5) * 255).astype(np.int64) << 16))
    return dict(o=np.full(len(sel), o), layer=lay[sel], r=r[sel], c=c[sel], xc=xs[:, 0], xr=xs[:, 1], xi=xs[:, 2],
                x=(c[sel].astype(F32) + xs[:, 0]) * scale, y=(r[sel].astype(F32) + xs[:, 1]) * scale, size=size,
                response=np.abs(contr[ok]), octave=octave.astype(np.int32), step_margin=step_margin[sel],
                contrast_margin=contr_margin[ok], edge_margin=edge_margin[ok],
                rejected_contrast_margin=contr_margin[~ok], rejected_edge_margin=edge_margin[~ok])


# ---- orientation -----------------------------------------------------------------------------------------------
def _exp(a, precise):
    return np.exp(a.astype(np.float64)).astype(F32) if precise else np.exp(a.astype(F32))


def _atan2_deg(y, x, precise):
    """Exact atan2 in degrees in [0, 360) (cv2 uses fastAtan2: a documented deviation)."""
    if precise:
        d = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64)))
        d = np.where(d < 0, d + 360.0, d).astype(F32)
    else:
        d = np.arctan2(y.astype(F32), x.astype(F32)) * F32(180 / np.pi)
        d = np.where(d < 0, d + F32(360), d).astype(F32)
    return np.where(d >= F32(360), F32(0), d)


def _trig(a, precise):
    if precise:
        a64 = a.astype(np.float64)
        return np.cos(a64).astype(F32), np.sin(a64).astype(F32)
    return np.cos(a.astype(F32)), np.sin(a.astype(F32))


def orientations(gauss, kp, p, precise=True, chunk=256):
    """calcOrientationHist + the peak search, for every refined keypoint.  Returns (parent index, angle) arrays and
    per keypoint the smallest relative margin of its peak decisions."""
    n = ORI_HIST_BINS
    n_kp = len(kp["x"])
    parents, angles = [], []
    margin = np.full(n_kp, np.inf, dtype=np.float64)
    scl = kp["size"] * F32(0.5) / np.array([F32(1 << int(o)) for o in kp["o"]], dtype=F32).reshape(-1)
    radius = np.rint(F32(4.5) * scl).astype(np.int64)
    sig = F32(1.5) * scl
    expf_scale = F32(-1) / (F32(2) * sig * sig)
    for s0 in range(0, n_kp, chunk):
        idx = np.arange(s0, min(n_kp, s0 + chunk))
        R = int(radius[idx].max()) if len(idx) else 0
        ii, jj = np.meshgrid(np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
        ii, jj = ii.ravel(), jj.ravel()                  # sample order: i outer, j inner
        hist = np.zeros((len(idx), n), dtype=F32)
        for g, k in enumerate(idx):
            img = gauss[kp["o"][k]][kp["layer"][k]]
            h, w = img.shape
            rad = radius[k]
            y = kp["r"][k] + ii
            x = kp["c"][k] + jj
            m = (np.abs(ii) <= rad) & (np.abs(jj) <= rad) & (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
            y, x, si, sj = y[m], x[m], ii[m], jj[m]
            dx = img[y, x + 1] - img[y, x - 1]
            dy = img[y - 1, x] - img[y + 1, x]
            wgt = _exp((si * si + sj * sj).astype(F32) * expf_scale[k], precise)
            ori = _atan2_deg(dy, dx, precise)
            mag = np.sqrt(dx * dx + dy * dy)
            b = np.rint(F32(n / 360.0) * ori).astype(np.int64)
            b = np.where(b >= n, b - n, b)
            b = np.where(b < 0, b + n, b)
            np.add.at(hist[g], b, wgt * mag)
        t = hist
        sm = ((np.roll(t, 2, 1) + np.roll(t, -2, 1)) * F32(1 / 16.0) + (np.roll(t, 1, 1) + np.roll(t, -1, 1)) * F32(4 / 16.0)
              + t * F32(6 / 16.0))
        omax = sm.max(axis=1)
        thr = (omax * F32(0.8)).astype(F32)
        hl, hr = np.roll(sm, 1, 1), np.roll(sm, -1, 1)
        peak = (sm > hl) & (sm > hr) & (sm >= thr[:, None])
        # margin of every bin's peak decision, relative to the histogram's maximum: a peak is as far from losing its
        # status as its weakest test; a non-peak is as far from becoming one as its most clearly failed test
        m = np.stack(((sm - hl), (sm - hr), (sm - thr[:, None]))).astype(np.float64)
        fail = np.stack((m[0] <= 0, m[1] <= 0, m[2] < 0))
        bin_margin = np.where(peak, m.min(axis=0), np.where(fail, -m, -np.inf).max(axis=0))
        margin[idx] = bin_margin.min(axis=1) / np.where(omax > 0, omax, 1).astype(np.float64)
        gk, jb = np.nonzero(peak)                         # keypoint-major, bin order
        l_, r_ = hl[gk, jb], hr[gk, jb]
        binf = jb.astype(F32) + F32(0.5) * (l_ - r_) / (l_ - F32(2) * sm[gk, jb] + r_)
        binf = np.where(binf < 0, F32(n) + binf, np.where(binf >= n, binf - F32(n), binf)).astype(F32)
        ang = F32(360) - F32(360.0 / n) * binf
        ang = np.where(np.abs(ang - F32(360)) < FLT_EPSILON, F32(0), ang)
        parents.append(idx[gk])
        angles.append(ang.astype(F32))
    if not parents:
        return np.zeros(0, dtype=np.int64), np.zeros(0, F32), margin
    return np.concatenate(parents), np.concatenate(angles), margin


# ---- order, duplicates and the firstOctave fixup ------------------------------------------------------------------
def sort_dedup(x, y, size, angle, response, octave):
    """KeyPoint_LessThan (x, y asc; size desc; angle asc; response desc; octave desc; stable), then
    removeDuplicatedSorted on (x, y, size, angle).  Returns the kept indices in order."""
    order = np.lexsort((-octave.astype(np.int64), -response.astype(np.float64), angle, -size.astype(np.float64), y, x))
    keep = []
    prev = None
    for i in order:
        key = (x[i], y[i], size[i], angle[i])
        if prev is not None and key == prev:
            continue
        keep.append(i)
        prev = key
    return np.array(keep, dtype=np.int64)


def unpack_octave(octave):
    """unpackOctave: (octave, layer, scale) of a packed cv2 octave field."""
    octave = np.asarray(octave, dtype=np.int64)
    o = octave & 255
    o = np.where(o < 128, o, o | -128)
    layer = (octave >> 8) & 255
    scale = np.where(o >= 0, 1.0 / np.exp2(np.maximum(o, 0)), np.exp2(np.maximum(-o, 0))).astype(F32)
    return o, layer, scale


# ---- descriptors -----------------------------------------------------------------------------------------------
def descriptors(gauss, p, x, y, size, angle, octave, precise=True):
    """calcDescriptors / calcSIFTDescriptor for the final (fixed-up) keypoints.  Returns (n, 128) float32 integers."""
    d, n = DESCR_WIDTH, DESCR_HIST_BINS
    o, layer, scale = unpack_octave(octave)
    out = np.zeros((len(x), d * d * n), dtype=F32)
    for k in range(len(x)):
        img = gauss[int(o[k]) + 1][int(layer[k])]
        h, w = img.shape
        ptx, pty = x[k] * scale[k], y[k] * scale[k]
        scl = size[k] * scale[k] * F32(0.5)
        ori = F32(360) - angle[k]
        if abs(ori - F32(360)) < FLT_EPSILON:
            ori = F32(0)
        px, py = int(np.rint(ptx)), int(np.rint(pty))
        cos_t, sin_t = _trig(np.array([ori * F32(np.pi / 180)], dtype=F32), precise)
        cos_t, sin_t = cos_t[0], sin_t[0]
        bins_per_rad = F32(n / 360.0)
        exp_scale = F32(-1) / (F32(d * d) * F32(0.5))
        hist_width = F32(3) * scl
        radius = int(np.rint(hist_width * F32(1.4142135623730951) * F32(d + 1) * F32(0.5)))
        radius = min(radius, int(np.sqrt(float(w) * w + float(h) * h)))
        cos_t = cos_t / hist_width
        sin_t = sin_t / hist_width
        ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
        ii, jj = ii.ravel(), jj.ravel()
        fi, fj = ii.astype(F32), jj.astype(F32)
        c_rot = fj * cos_t - fi * sin_t
        r_rot = fj * sin_t + fi * cos_t
        rbin = r_rot + F32(d // 2) - F32(0.5)
        cbin = c_rot + F32(d // 2) - F32(0.5)
        rr, cc = py + ii, px + jj
        m = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (rr > 0) & (rr < h - 1) & (cc > 0) & (cc < w - 1)
        rr, cc, rbin, cbin, c_rot, r_rot = rr[m], cc[m], rbin[m], cbin[m], c_rot[m], r_rot[m]
        dx = img[rr, cc + 1] - img[rr, cc - 1]
        dy = img[rr - 1, cc] - img[rr + 1, cc]
        wgt = _exp((c_rot * c_rot + r_rot * r_rot) * exp_scale, precise)
        ori_s = _atan2_deg(dy, dx, precise)
        mag = np.sqrt(dx * dx + dy * dy)
        obin = (ori_s - ori) * bins_per_rad
        mag = mag * wgt
        r0, c0, o0 = np.floor(rbin).astype(np.int64), np.floor(cbin).astype(np.int64), np.floor(obin).astype(np.int64)
        rbin = rbin - r0.astype(F32)
        cbin = cbin - c0.astype(F32)
        obin = obin - o0.astype(F32)
        o0 = np.where(o0 < 0, o0 + n, o0)
        o0 = np.where(o0 >= n, o0 - n, o0)
        v_r1 = mag * rbin; v_r0 = mag - v_r1
        v_rc11 = v_r1 * cbin; v_rc10 = v_r1 - v_rc11
        v_rc01 = v_r0 * cbin; v_rc00 = v_r0 - v_rc01
        v111 = v_rc11 * obin; v110 = v_rc11 - v111
        v101 = v_rc10 * obin; v100 = v_rc10 - v101
        v011 = v_rc01 * obin; v010 = v_rc01 - v011
        v001 = v_rc00 * obin; v000 = v_rc00 - v001
        idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0
        hist = np.zeros((d + 2) * (d + 2) * (n + 2), dtype=F32)
        offs = (0, 1, n + 2, n + 3, (d + 2) * (n + 2), (d + 2) * (n + 2) + 1, (d + 3) * (n + 2), (d + 3) * (n + 2) + 1)
        vals = (v000, v001, v010, v011, v100, v101, v110, v111)
        # the eight bins of one sample are distinct, so every bin receives its contributions in sample order
        allidx = np.stack([idx + o_ for o_ in offs], axis=1).ravel()
        allval = np.stack(vals, axis=1).ravel()
        np.add.at(hist, allidx, allval)
        hist = hist.reshape(d + 2, d + 2, n + 2)
        dst = np.zeros((d, d, n), dtype=F32)
        for i in range(d):
            for j in range(d):
                hb = hist[i + 1, j + 1].copy()
                hb[0] = hb[0] + hb[n]
                hb[1] = hb[1] + hb[n + 1]
                dst[i, j] = hb[:n]
        out[k] = dst.ravel()
    # normalise, clamp at 0.2 |d|, renormalise to 512 / max(|d|, FLT_EPSILON), saturate_cast<uchar>; the squared norms
    # are sequential float32 sums over the 128 elements (add.accumulate does not pair)
    nrm2 = np.add.accumulate(out * out, axis=1, dtype=F32)[:, -1] if len(out) else np.zeros(0, F32)
    thr = np.sqrt(nrm2) * F32(0.2)
    out = np.minimum(out, thr[:, None])
    nrm2 = np.add.accumulate(out * out, axis=1, dtype=F32)[:, -1] if len(out) else np.zeros(0, F32)
    nrm2 = F32(512) / np.maximum(np.sqrt(nrm2), FLT_EPSILON)
    return np.clip(np.rint(out * nrm2[:, None]), 0, 255).astype(F32)


# ---- the whole detector ----------------------------------------------------------------------------------------
def detect(img, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, precise=True,
           with_descriptors=True):
    """detectAndCompute(img, None).  Returns a dict: x, y, size, angle, response, octave (final, fixed up),
    descriptors (n, 128) float32, and the intermediates: gauss / dog (lists per octave), pre (the refined keypoints
    before orientation, in pyramid coordinates), cand (the candidate margins) and ori_margin (per pre keypoint)."""
    p = Params(n_octave_layers, contrast_threshold, edge_threshold, sigma)
    gray = to_gray(img)
    gauss, dog = build_pyramid(gray, p)
    co, cl, cr, cc, thr_m, nb_m = find_candidates(dog, p)
    parts = [refine(dog, p, o, cl[co == o], cr[co == o], cc[co == o]) for o in range(len(dog)) if (co == o).any()]
    keys = ("o", "layer", "r", "c", "xc", "xr", "xi", "x", "y", "size", "response", "octave", "step_margin",
            "contrast_margin", "edge_margin")
    pre = {k: (np.concatenate([pp[k] for pp in parts]) if parts else np.zeros(0)) for k in keys}
    for k in ("o", "layer", "r", "c"):
        pre[k] = pre[k].astype(np.int64)
    for k in ("x", "y", "size", "response", "xc", "xr", "xi"):
        pre[k] = pre[k].astype(F32)
    pre["octave"] = pre["octave"].astype(np.int32)
    par, ang, ori_margin = orientations(gauss, pre, p, precise)
    x, y, size, resp, octv = (pre[k][par] for k in ("x", "y", "size", "response", "octave"))
    keep = sort_dedup(x, y, size, ang, resp, octv)
    x, y, size, ang, resp, octv, par = x[keep], y[keep], size[keep], ang[keep], resp[keep], octv[keep], par[keep]
    octv = ((octv & ~255) | ((octv - 1) & 255)).astype(np.int32)
    x, y, size = x * F32(0.5), y * F32(0.5), size * F32(0.5)
    desc = descriptors(gauss, p, x, y, size, ang, octv, precise) if with_descriptors else None
    return dict(x=x, y=y, size=size, angle=ang, response=resp, octave=octv, descriptors=desc, parent=par,
                gauss=gauss, dog=dog, pre=pre, ori_margin=ori_margin,
                cand=dict(o=co, layer=cl, r=cr, c=cc, threshold_margin=thr_m, neighbour_margin=nb_m))
