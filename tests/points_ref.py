"""The point Kalman filter of the reference (src/utils/kalman/kalman_2d_point.rs) as a dense f32 numpy model, vectorised over points.
TEST INFRASTRUCTURE: what similari_amd/csrc/sa_kalman_point.h and the point bank are compared with, bit for bit.

Arrays are mean [..., 4] and cov [..., 4, 4] (any leading shape); only the matrix indices are looped over, so every f32 operation
happens in nalgebra's order: a product C = A B is, per element, the k-ascending sum seeded by the first product; the gain is
solve_lower_triangular on the UN-factorised projected covariance (the reference's quirk); the distance goes through a 2 x 2 Cholesky
factor.  tests/test_points_ref.py pins this file to the oracle's box filter, which the reference's known-answer tests pin."""
import numpy as np

f32 = np.float32
PW, VW = f32(1.0) / f32(20.0), f32(1.0) / f32(160.0)
CHI2_2, CHI2_5, UPPER = f32(5.9915), f32(11.070), f32(100.0)
F = np.eye(4, dtype=f32)
F[0, 2] = F[1, 3] = 1
H = np.eye(2, 4, dtype=f32)


def _a(x):
    return np.asarray(x, f32)


def matmul(A, B):
    """[..., m, k] x [..., k, n]: element (i, j) = A[i][0] B[0][j], then A[i][k] B[k][j] + acc for k = 1 .. (no fused multiply-add)."""
    A, B = _a(A), _a(B)
    m, kk, n = A.shape[-2], A.shape[-1], B.shape[-1]
    lead = np.broadcast_shapes(A.shape[:-2], B.shape[:-2])
    C = np.empty(lead + (m, n), f32)
    for i in range(m):
        for j in range(n):
            acc = A[..., i, 0] * B[..., 0, j]
            for k in range(1, kk):
                acc = A[..., i, k] * B[..., k, j] + acc
            C[..., i, j] = acc
    return C


def _t(A):
    return np.swapaxes(A, -1, -2)


def _diag(vals, lead):
    D = np.zeros(lead + (len(vals), len(vals)), f32)
    for i, v in enumerate(vals):
        D[..., i, i] = v
    return D


def initiate(z, pw=PW, vw=VW):
    """z [..., 2] -> (mean, cov)"""
    z, pw, vw = _a(z), f32(pw), f32(vw)
    mean = np.zeros(z.shape[:-1] + (4,), f32)
    mean[..., 0], mean[..., 1] = z[..., 0], z[..., 1]
    sp, sv = f32(2.0) * pw, f32(10.0) * vw
    return mean, _diag([sp * sp, sp * sp, sv * sv, sv * sv], z.shape[:-1])


def predict(mean, cov, pw=PW, vw=VW):
    mean, cov, pw, vw = _a(mean), _a(cov), f32(pw), f32(vw)
    m = matmul(F, mean[..., None])[..., 0]
    c = matmul(matmul(F, cov), F.T) + _diag([pw * pw, pw * pw, vw * vw, vw * vw], cov.shape[:-2])
    return m, c


def project(mean, cov, pw=PW):
    mean, cov, pw = _a(mean), _a(cov), f32(pw)
    pm = matmul(H, mean[..., None])[..., 0]
    pc = matmul(matmul(H, cov), H.T) + _diag([pw * pw, pw * pw], cov.shape[:-2])
    return pm, pc


def solve_lower(L, B):
    """nalgebra's column-oriented forward substitution, column by column of B [..., d, n]; reads the lower triangle of L only."""
    X = np.array(B, f32)
    d = L.shape[-1]
    for c in range(X.shape[-1]):
        for i in range(d):
            coeff = X[..., i, c] / L[..., i, i]
            X[..., i, c] = coeff
            nc = -coeff
            for r in range(i + 1, d):
                X[..., r, c] = nc * L[..., r, i] + X[..., r, c]
    return X


def update(mean, cov, z, pw=PW):
    mean, cov, z = _a(mean), _a(cov), _a(z)
    with np.errstate(all="ignore"):
        pm, pc = project(mean, cov, pw)
        B = _t(matmul(cov, H.T))
        G = solve_lower(pc, B)
        innov = (z - pm)[..., None, :]
        m = mean + matmul(innov, G)[..., 0, :]
        c = cov - matmul(matmul(_t(G), pc), G)
    return m, c


def distance(mean, cov, z, pw=PW):
    """d^2 [...]; NaN where a Cholesky pivot fails."""
    mean, cov, z = _a(mean), _a(cov), _a(z)
    with np.errstate(all="ignore"):
        pm, pc = project(mean, cov, pw)
        r = z - pm
        p00, p10, p11 = pc[..., 0, 0], pc[..., 1, 0], pc[..., 1, 1]
        bad0 = (p00 == 0) | ~(p00 >= 0)
        l00 = np.sqrt(np.where(bad0, f32(1), p00))
        l10 = p10 / l00
        d1 = (-l10) * l10 + p11
        bad1 = (d1 == 0) | ~(d1 >= 0)
        l11 = np.sqrt(np.where(bad1, f32(1), d1))
        y0 = r[..., 0] / l00
        y1 = ((-y0) * l10 + r[..., 1]) / l11
        d2 = y0 * y0 + y1 * y1
    return np.where(bad0 | bad1, f32(np.nan), d2).astype(f32)


def cost(d2, inverted):
    d2 = _a(d2)
    with np.errstate(invalid="ignore"):
        if not inverted:
            return np.where(d2 > CHI2_2, UPPER, d2).astype(f32)
        return np.where(d2 > CHI2_5, f32(0), UPPER - d2).astype(f32)


def present_of(pts, min_score=0.0, mask=None):
    """pts [..., comps] -> bool [...]: finite x and y, score >= min_score where there is one, and the mask."""
    pts = _a(pts)
    ok = np.isfinite(pts[..., 0]) & np.isfinite(pts[..., 1])
    if pts.shape[-1] == 3:
        with np.errstate(invalid="ignore"):
            ok &= pts[..., 2] >= f32(min_score)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return ok


class Bank:
    """The states of a set of point vectors with presence handled as include/similari_points.h says: has [...], mean [..., 4],
    cov [..., 4, 4].  Every call takes z [..., 2] and present [...] for the whole set."""

    def __init__(self, shape, pw=PW, vw=VW):
        self.pw, self.vw = f32(pw), f32(vw)
        self.has = np.zeros(shape, bool)
        self.mean = np.full(tuple(shape) + (4,), np.nan, f32)
        self.cov = np.full(tuple(shape) + (4, 4), np.nan, f32)

    def _put(self, sel, m, c):
        self.mean[sel], self.cov[sel] = m[sel], c[sel]

    def initiate(self, z, present):
        m, c = initiate(z, self.pw, self.vw)
        self._put(present, m, c)
        self.has |= present

    def predict(self):
        with np.errstate(all="ignore"):
            m, c = predict(self.mean, self.cov, self.pw, self.vw)
        self._put(self.has, m, c)
        return self.xy()

    def update(self, z, present):
        m, c = update(self.mean, self.cov, np.where(present[..., None], z, f32(0)), self.pw)
        self._put(self.has & present, m, c)
        return self.xy()

    def distance(self, z, present, mode=0):
        d = distance(self.mean, self.cov, np.where(present[..., None], z, f32(0)), self.pw)
        if mode:
            d = cost(d, mode == 2)
        return np.where(self.has & present, d, f32(np.nan)).astype(f32)

    def step(self, z, present):
        self.initiate(z, present & ~self.has)
        self.predict()
        return self.update(z, present)

    def xy(self):
        return np.where(self.has[..., None], self.mean[..., :2], f32(np.nan)).astype(f32)
