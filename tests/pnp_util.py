"""Float64 numpy restatement of the batched PnP-RANSAC solver (nerfmatch_amd/csrc/pnp.hip), the yardstick of tests/test_pnp_*.py.

Written from the papers, one hypothesis at a time, with none of the kernel's structure:
  * sampling: the counter-based hash of include/nerfmatch_amd.h (lowbias32 finaliser chained over seed, hypothesis, slot, attempt);
  * minimal solver: Lambda Twist (Persson & Nordberg, ECCV 2018): the two quadrics D1, D2 in the depths (l1, l2, l3), one real root g of
    the cubic det(D1 + g D2) = 0, the degenerate conic D1 + g D2 split into its two lines (adjugate method, Richter-Gebert,
    "Perspectives on Projective Geometry", sec. 11.1), a quadratic in tau = l3 / l2 per line, Gauss-Newton on the three distance
    constraints, R = Y X^-1;
  * scoring: positive depth and squared pixel residual <= thr^2;
  * refinement: Levenberg-Marquardt on the reprojection error of the inlier set, which is re-evaluated at every step.

Every validity decision that a rounding error could flip (the triangle's area, the cubic's discriminant, the line split's pivot, the
quadratic's discriminant, the signs of tau / l1 / the fourth point's depth) sets `flag` when it falls within FLOOR_BAND of its floor:
a flagged sample is one on which two correct implementations may disagree about whether a hypothesis exists.
"""
import math

import numpy as np

AREA_FLOOR = 1e-8    # sin^2 of the angle at x1 of the sample triangle below which there is no hypothesis (angle < 1e-4 rad)
FLOOR_BAND = 1e-6    # relative distance to a decision boundary inside which the restatement flags the sample as degenerate
GN_ITERS = 5
LM_LAMBDA0, LM_LAMBDA_MIN, LM_LAMBDA_MAX = 1e-3, 1e-9, 1e9
MAX_ATTEMPTS = 64


# ------------------------------------------------------------------------------------------------------------- hash and sampling
def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def hash4(seed, h, slot, attempt):
    v = mix32((seed & 0xFFFFFFFF) ^ 0x9E3779B9)
    v = mix32(v + h)
    v = mix32(v + slot)
    return mix32(v + attempt)


def sample_indices(seed, h, n):
    """Four distinct indices in [0, n), n >= 4: slot s takes hash4(seed, h, s, attempt) % n, a duplicate of an earlier slot bumps
    `attempt`; after MAX_ATTEMPTS the smallest unused index."""
    idx = []
    for slot in range(4):
        attempt = 0
        while True:
            if attempt >= MAX_ATTEMPTS:
                i = min(j for j in range(n) if j not in idx)
                break
            i = hash4(seed, h, slot, attempt) % n
            if i not in idx:
                break
            attempt += 1
        idx.append(i)
    return idx


# ------------------------------------------------------------------------------------------------------------- P3P (Lambda Twist)
def _adj_sym(A):
    """Adjugate of a symmetric 3 x 3 matrix."""
    a, b, c, d, e, f = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
    return np.array([[d * f - e * e, c * e - b * f, b * e - c * d],
                     [c * e - b * f, a * f - c * c, b * c - a * e],
                     [b * e - c * d, b * c - a * e, a * d - b * b]])


def _near(value, scale):
    return abs(value) <= FLOOR_BAND * abs(scale)


def p3p(y, x):
    """y (3,3): unit bearing vectors (rows), x (3,3): the 3-D points.  -> (list of (R, t) with l_i y_i = R x_i + t, l_i > 0; flag)."""
    flag = False
    d12, d13, d23 = x[0] - x[1], x[0] - x[2], x[1] - x[2]
    a12, a13, a23 = d12 @ d12, d13 @ d13, d23 @ d23
    cr = np.cross(d12, d13)
    area2 = cr @ cr
    flag |= _near(area2 - AREA_FLOOR * a12 * a13, 16 * AREA_FLOOR * a12 * a13)
    if not area2 > AREA_FLOOR * a12 * a13:
        return [], flag
    b12, b13, b23 = y[0] @ y[1], y[0] @ y[2], y[1] @ y[2]
    D1 = np.array([[a23, -a23 * b12, 0.0], [-a23 * b12, a23 - a12, a12 * b23], [0.0, a12 * b23, -a12]])
    D2 = np.array([[a23, 0.0, -a23 * b13], [0.0, -a13, a13 * b23], [-a23 * b13, a13 * b23, a23 - a13]])
    A1, A2 = _adj_sym(D1), _adj_sym(D2)
    c3, c0 = np.linalg.det(D2), np.linalg.det(D1)
    c1, c2 = float(np.sum(A1 * D2)), float(np.sum(D1 * A2))
    with np.errstate(all="ignore"):
        a, b, c = c2 / c3, c1 / c3, c0 / c3
        q, r = (a * a - 3 * b) / 9, (2 * a * a * a - 9 * a * b + 27 * c) / 54
        disc = r * r - q * q * q
        flag |= _near(disc, max(r * r, abs(q * q * q)))
        if disc < 0:
            g = -2 * math.sqrt(q) * math.cos(math.acos(max(-1.0, min(1.0, r / math.sqrt(q * q * q)))) / 3) - a / 3
        else:
            A = -math.copysign(np.cbrt(abs(r) + math.sqrt(disc)), r) if np.isfinite(disc) else float("nan")
            g = A + (q / A if A != 0 else 0.0) - a / 3
        for _ in range(2):
            f, fp = ((g + a) * g + b) * g + c, (3 * g + 2 * a) * g + b
            if fp != 0:
                g -= f / fp
    if not np.isfinite(g):
        return [], True
    D0 = D1 + g * D2
    B = -_adj_sym(D0)
    i = int(np.argmax(np.diag(B)))
    flag |= _near(B[i, i], np.sum(D0 * D0))
    if not B[i, i] > 0:
        return [], flag
    p = B[:, i] / math.sqrt(B[i, i])
    C = D0 + np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])
    j, k = divmod(int(np.argmax(np.abs(C))), 3)
    sols = []
    for v in (C[j, :], C[:, k]):
        flag |= _near(v[0], np.linalg.norm(v))
        if v[0] == 0:
            continue
        w0, w1 = -v[1] / v[0], -v[2] / v[0]
        qa = a23 * w1 * w1 - a12
        qb = a23 * (2 * w0 * w1 - 2 * b12 * w1) + 2 * a12 * b23
        qc = a23 * (w0 * w0 - 2 * b12 * w0 + 1) - a12
        dq = qb * qb - 4 * qa * qc
        flag |= _near(dq, qb * qb + abs(4 * qa * qc))
        if not dq >= 0:
            continue
        qq = -0.5 * (qb + math.copysign(math.sqrt(dq), qb))
        with np.errstate(all="ignore"):
            taus = (np.float64(qq) / qa, np.float64(qc) / qq)
        for tau in taus:
            if not (np.isfinite(tau) and tau > 0):
                flag |= bool(np.isfinite(tau)) and abs(tau) < FLOOR_BAND
                continue
            flag |= abs(tau) < FLOOR_BAND
            l2 = math.sqrt(a23 / (tau * (tau - 2 * b23) + 1))
            lam = np.array([(w0 + w1 * tau) * l2, l2, tau * l2])
            flag |= _near(lam[0], l2)
            if not lam[0] > 0:
                continue
            for _ in range(GN_ITERS):
                l1, l2, l3 = lam
                res = np.array([l1 * l1 + l2 * l2 - 2 * b12 * l1 * l2 - a12, l1 * l1 + l3 * l3 - 2 * b13 * l1 * l3 - a13,
                                l2 * l2 + l3 * l3 - 2 * b23 * l2 * l3 - a23])
                J = np.array([[2 * l1 - 2 * b12 * l2, 2 * l2 - 2 * b12 * l1, 0.0], [2 * l1 - 2 * b13 * l3, 0.0, 2 * l3 - 2 * b13 * l1],
                              [0.0, 2 * l2 - 2 * b23 * l3, 2 * l3 - 2 * b23 * l2]])
                if np.linalg.det(J) == 0:
                    break
                lam = lam - np.linalg.solve(J, res)
            flag |= bool(np.min(np.abs(lam)) < FLOOR_BAND * np.max(np.abs(lam)))
            if not (np.all(np.isfinite(lam)) and np.all(lam > 0)):
                continue
            e1, e2 = lam[0] * y[0] - lam[1] * y[1], lam[1] * y[1] - lam[2] * y[2]
            Y = np.stack([e1, e2, np.cross(e1, e2)], axis=1)
            X = np.stack([d12, d23, np.cross(d12, d23)], axis=1)
            R = Y @ np.linalg.inv(X)
            sols.append((R, lam[0] * y[0] - R @ x[0]))
    return sols, flag


def bearings(pt2d, K):
    yn = (pt2d[:, 1] - K[1, 2]) / K[1, 1]
    xn = (pt2d[:, 0] - K[0, 2] - K[0, 1] * yn) / K[0, 0]
    y = np.stack([xn, yn, np.ones_like(xn)], axis=1)
    return y / np.linalg.norm(y, axis=1, keepdims=True)


def project(K, R, t, X):
    """-> pixels (n, 2), depth (n,)"""
    Xc = X @ R.T + t
    with np.errstate(all="ignore"):
        xn, yn = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        return np.stack([K[0, 0] * xn + K[0, 1] * yn + K[0, 2], K[1, 1] * yn + K[1, 2]], axis=1), Xc[:, 2]


def hypothesis(pt2d, pt3d, K, idx):
    """The hypothesis of a four-index sample: P = K [R | t] (3 x 4, float64; the kernel stores it rounded to float32) of the P3P root of
    the first three points that reprojects the fourth best, among the roots that put it in front of the camera.  -> (P | None, flag)."""
    pt2d, pt3d, K = np.asarray(pt2d, np.float64), np.asarray(pt3d, np.float64), np.asarray(K, np.float64)
    i3 = list(idx[:3])
    sols, flag = p3p(bearings(pt2d[i3], K), pt3d[i3])
    best, best_err = None, float("inf")
    errs = []
    for R, t in sols:
        pix, z = project(K, R, t, pt3d[idx[3]:idx[3] + 1])
        flag |= abs(z[0]) < FLOOR_BAND * (abs(t[2]) + 1.0)
        if not z[0] > 0:
            continue
        err = float(np.sum((pix[0] - pt2d[idx[3]]) ** 2))
        errs.append(err)
        if err < best_err:
            best, best_err = (R, t), err
    if best is None:
        return None, flag
    P = K @ np.concatenate([best[0], best[1][:, None]], axis=1)
    if not np.all(np.isfinite(P.astype(np.float32))):
        return None, True
    return P, flag


def residuals_P(P, pt2d, pt3d):
    """Pixel residual norms (inf behind the camera) of the points under the 3 x 4 projection P, in float64."""
    P = np.asarray(P, np.float64)
    h = np.asarray(pt3d, np.float64) @ P[:, :3].T + P[:, 3]
    with np.errstate(all="ignore"):
        d = np.stack([h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]], axis=1) - np.asarray(pt2d, np.float64)
        r = np.sqrt(np.sum(d * d, axis=1))
    return np.where(h[:, 2] > 0, r, np.inf)


def win_key(count, h):
    return (int(count) << 32) | (0xFFFFFFFF - int(h))


# ------------------------------------------------------------------------------------------------------------- refinement
def pose_from_P(P, K, dtype=np.float64):
    """[R | t] = K^-1 P with K upper triangular, the rows of R made orthonormal by Gram-Schmidt (row 0, row 1, their cross product)."""
    P, K = np.asarray(P, dtype), np.asarray(K, dtype)
    m2 = P[2]
    m1 = (P[1] - K[1, 2] * m2) / K[1, 1]
    m0 = (P[0] - K[0, 1] * m1 - K[0, 2] * m2) / K[0, 0]
    r0 = m0[:3] / np.linalg.norm(m0[:3])
    r1 = m1[:3] - (r0 @ m1[:3]) * r0
    r1 = r1 / np.linalg.norm(r1)
    R = np.stack([r0, r1, np.cross(r0, r1)])
    return R.astype(dtype), np.array([m0[3], m1[3], m2[3]], dtype)


def _rigid(R, t, X):
    """R X + t for the rows of X, as three scaled columns added in order (no BLAS: the same float32 bits on every machine)."""
    return X[:, 0:1] * R[:, 0] + X[:, 1:2] * R[:, 1] + X[:, 2:3] * R[:, 2] + t


def _mm(a, b):
    return np.einsum("ij,j...->i...", a, b)  # (numpy's own loops, no BLAS)


def so3_exp(w):
    dt = w.dtype
    th2 = float(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th2 < 1e-8:
        a, b = 1 - th2 / 6, 0.5 - th2 / 24
    else:
        th = math.sqrt(th2)
        a, b = math.sin(th) / th, (1 - math.cos(th)) / th2
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dt)
    return (np.eye(3, dtype=dt) + dt.type(a) * W + dt.type(b) * _mm(W, W)).astype(dt)


def _reproj(K, R, t, pt2d, pt3d):
    Xc = _rigid(R, t, pt3d)
    with np.errstate(all="ignore"):
        iz = 1 / Xc[:, 2]
        xn, yn = Xc[:, 0] * iz, Xc[:, 1] * iz
        r = np.stack([K[0, 0] * xn + K[0, 1] * yn + K[0, 2], K[1, 1] * yn + K[1, 2]], axis=1) - pt2d
    return Xc, iz, xn, yn, r


def inliers_Rt(K, R, t, pt2d, pt3d, thr):
    Xc, _, _, _, r = _reproj(K, R, t, pt2d, pt3d)
    e2 = np.sum(r * r, axis=1)
    return (Xc[:, 2] > 0) & (e2 <= thr * thr), e2


def lm_refine(R, t, pt2d, pt3d, K, thr, iters, dtype=np.float64):
    """`iters` Levenberg-Marquardt steps.  Each step: S = inliers at thr under the current pose; normal equations of the reprojection
    error over S for the update X_c <- exp(w) X_c + v; (H + lambda diag H) d = -g; the candidate is taken iff it has at least as many
    inliers as the current pose AND the cost of S (sum of squared residuals; inf if a member falls behind the camera) falls; lambda
    /= 10 on acceptance, *= 10 otherwise.  -> R, t, final inlier mask."""
    dt = np.dtype(dtype)
    R, t, K = np.asarray(R, dt), np.asarray(t, dt), np.asarray(K, dt)
    pt2d, pt3d, thr = np.asarray(pt2d, dt), np.asarray(pt3d, dt), dt.type(thr)
    lam = LM_LAMBDA0
    for _ in range(iters):
        S, e2 = inliers_Rt(K, R, t, pt2d, pt3d, thr)
        cnt, cost = int(S.sum()), float(np.sum(e2[S].astype(dt)))
        Xc, iz, xn, yn, r = _reproj(K, R, t, pt2d[S], pt3d[S])
        fx, sk, fy = K[0, 0], K[0, 1], K[1, 1]
        du = np.stack([fx * iz, sk * iz, -(fx * xn + sk * yn) * iz], axis=1)  # d u / d X_c
        dv = np.stack([np.zeros_like(iz), fy * iz, -fy * yn * iz], axis=1)
        # d X_c = -[X_c]x w + v  ->  row (a x X_c... ) : (d/dw) = X_c x a  for a row a of the projection Jacobian
        Ju = np.concatenate([np.cross(Xc, du), du], axis=1)
        Jv = np.concatenate([np.cross(Xc, dv), dv], axis=1)
        # summed row by row over the matches (a reduction over axis 0 adds the rows in order): no BLAS, so the float32 run that
        # measures LM_F32_VS_F64 gives the same numbers on every machine
        H = (Ju[:, :, None] * Ju[:, None, :] + Jv[:, :, None] * Jv[:, None, :]).sum(axis=0).astype(dt)
        g = (Ju * r[:, 0:1] + Jv * r[:, 1:2]).sum(axis=0).astype(dt)
        ok = False
        try:
            A = H + dt.type(lam) * np.diag(np.diag(H))
            if cnt >= 3 and np.all(np.isfinite(A)) and np.all(np.diag(A) > 0):
                L = np.linalg.cholesky(A)
                d = -np.linalg.solve(L.T, np.linalg.solve(L, g)).astype(dt)
                ok = bool(np.all(np.isfinite(d)))
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            E = so3_exp(d[:3])
            Rn, tn = _mm(E, R).astype(dt), (_mm(E, t) + d[3:]).astype(dt)
            Sn, e2n = inliers_Rt(K, Rn, tn, pt2d, pt3d, thr)
            Xn = _rigid(Rn, tn, pt3d[S])
            costn = float(np.sum(e2n[S].astype(dt))) if np.all(Xn[:, 2] > 0) else float("inf")
            ok = int(Sn.sum()) >= cnt and costn < cost
        if ok:
            R, t, lam = Rn, tn, max(lam / 10, LM_LAMBDA_MIN)
        else:
            lam = min(lam * 10, LM_LAMBDA_MAX)
    S, _ = inliers_Rt(K, R, t, pt2d, pt3d, thr)
    return R, t, S


# ------------------------------------------------------------------------------------------------------------- the whole solver
def solve(pt2d, pt3d, K, thr=1.0, n_hyps=64, refine_iters=10, seed=0, add_half_px=False, hyps=None):
    """One query.  -> dict(R, t, n_inliers, mask, win, hyp_P (list of 3x4 | None), hyp_flag, hyp_count).  `hyps`: hypothesis matrices to
    score and refine from instead of the restatement's own (the GPU's study output)."""
    pt2d, pt3d, K = np.asarray(pt2d, np.float64), np.asarray(pt3d, np.float64), np.asarray(K, np.float64)
    if add_half_px:
        pt2d = pt2d + 0.5
    n = len(pt2d)
    out = dict(R=np.eye(3), t=np.zeros(3), n_inliers=0, mask=np.zeros(n, bool), win=-1, hyp_P=[], hyp_flag=[], hyp_count=[])
    if n < 4:
        return out
    if hyps is None:
        for h in range(n_hyps):
            P, flag = hypothesis(pt2d, pt3d, K, sample_indices(seed, h, n))
            out["hyp_P"].append(None if P is None else P.astype(np.float32))
            out["hyp_flag"].append(flag)
    else:
        out["hyp_P"] = [None if not np.all(np.isfinite(P)) else np.asarray(P, np.float32) for P in hyps]
        out["hyp_flag"] = [False] * len(hyps)
    out["hyp_count"] = [0 if P is None else int(np.sum(residuals_P(P, pt2d, pt3d) <= thr)) for P in out["hyp_P"]]
    keys = [win_key(c, h) for h, c in enumerate(out["hyp_count"])]
    win = int(np.argmax(keys))
    if out["hyp_P"][win] is None or out["hyp_count"][win] < 4:
        out["n_inliers"] = out["hyp_count"][win] if out["hyp_P"][win] is not None else 0
        return out
    R, t = pose_from_P(out["hyp_P"][win], K)
    R, t, mask = lm_refine(R, t, pt2d, pt3d, K, thr, refine_iters)
    if int(mask.sum()) < 4:  # the refined pose keeps fewer than 4 inliers: no pose
        out.update(n_inliers=int(mask.sum()), win=win)
        return out
    out.update(R=R, t=t, mask=mask, n_inliers=int(mask.sum()), win=win)
    return out


# ------------------------------------------------------------------------------------------------------------- scenes
def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_scene(n, sigma=0.0, outlier_frac=0.0, seed=0, W=640, H=480):
    """n matches of a W x H camera (f about 500, a random world-to-camera pose): points at depth 2-10 that project inside the image,
    Gaussian pixel noise `sigma`, and a fraction of the pixels replaced by uniform draws over the image -- redrawn while within 3 px of
    the point's true projection, so that `inlier` (the complement of the replaced set) is the true inlier set at thresholds up to 3 px.
    float32 pt2d / pt3d / K, as the solver takes them; R, t float64."""
    rng = np.random.default_rng(seed)
    f = 500.0 + rng.uniform(-20, 20)
    K = np.array([[f, 0, W / 2 + rng.uniform(-5, 5)], [0, f * rng.uniform(0.98, 1.02), H / 2 + rng.uniform(-5, 5)], [0, 0, 1]])
    R, t = random_rotation(rng), rng.uniform(-1, 1, size=3)
    pix = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)
    z = rng.uniform(2, 10, n)
    Xc = np.stack([(pix[:, 0] - K[0, 2]) / K[0, 0] * z, (pix[:, 1] - K[1, 2]) / K[1, 1] * z, z], axis=1)
    X = ((Xc - t) @ R).astype(np.float32)  # R^T (Xc - t)
    K32 = K.astype(np.float32)
    true_pix, _ = project(K32.astype(np.float64), R, t, X.astype(np.float64))
    obs = true_pix + sigma * rng.normal(size=(n, 2))
    inlier = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    for i in rng.permutation(n)[:n_out]:
        while True:
            o = np.array([rng.uniform(0, W), rng.uniform(0, H)])
            if np.linalg.norm(o - true_pix[i]) > 3:
                break
        obs[i], inlier[i] = o, False
    return dict(pt2d=obs.astype(np.float32), pt3d=X, K=K32, R=R, t=t, inlier=inlier)


def pose_distance(R0, t0, R1, t1):
    """(rotation angle in degrees, translation distance) between two world-to-camera poses."""
    # |R1 - R0|_F = 2 sqrt(2) sin(angle / 2): unlike acos of the trace this resolves angles far below 1e-8 rad
    chord = np.linalg.norm(np.asarray(R1, np.float64) - np.asarray(R0, np.float64)) / (2 * math.sqrt(2))
    return math.degrees(2 * math.asin(min(1.0, chord))), float(np.linalg.norm(np.asarray(t0, np.float64) - np.asarray(t1, np.float64)))


def c2w_err(R_true, t_true, R, t):
    """(rotation deg, camera-centre distance) as utils.metrics.pose_err measures it on the camera-to-world poses."""
    c0, c1 = -np.asarray(R_true).T @ t_true, -np.asarray(R, np.float64).T @ np.asarray(t, np.float64)
    return pose_distance(R_true, 0 * c0, R, 0 * c1)[0], float(np.linalg.norm(c0 - c1))


# ------------------------------------------------------------------------------------------------------------- the two measured bounds
# Both come from this restatement alone (no kernel involved); tests/test_pnp_cpu.py re-measures them on the scenes of tests/test_pnp_gpu.py
# and fails if a recorded value drifts from what the functions below return.
HYP_RESIDUAL_F32_PX = 5.22e-3         # measure_hyp_rounding over HYP_RUNS of test_pnp_gpu.py (540 finite hypotheses of 576)
LM_F32_VS_F64 = (3.28e-6, 1.35e-7)    # measure_lm_f32_vs_f64 on the sigma = 0.5 px scene of pose_scenes(): (degrees, scene units)


def measure_hyp_rounding(scenes_and_hyps, seed):
    """Largest pixel residual of a restatement hypothesis' own three sample points after its K [R | t] is rounded to float32 (evaluated in
    float64).  scenes_and_hyps: [(scene, n_hyps)].  -> (max, all residual maxima, number of hypotheses, number flagged)."""
    worst, total, flagged = [], 0, 0
    for s, n_hyps in scenes_and_hyps:
        n = len(s["pt2d"])
        for h in range(n_hyps):
            idx = sample_indices(seed, h, n)
            P, flag = hypothesis(s["pt2d"], s["pt3d"], s["K"], idx)
            total += 1
            flagged += bool(flag)
            if P is not None:
                worst.append(float(residuals_P(P.astype(np.float32), s["pt2d"][idx[:3]], s["pt3d"][idx[:3]]).max()))
    return max(worst), np.array(worst), total, flagged


def measure_lm_f32_vs_f64(scene, n_hyps, seed, thr=1.0, iters=10):
    """pose_distance between lm_refine run in float32 and in float64 from the restatement's winning hypothesis of the scene."""
    out = solve(scene["pt2d"], scene["pt3d"], scene["K"], thr, n_hyps, 0, seed)
    P, K = out["hyp_P"][int(np.argmax([win_key(c, h) for h, c in enumerate(out["hyp_count"])]))], scene["K"].astype(np.float64)
    R64, t64, _ = lm_refine(*pose_from_P(P, K), scene["pt2d"], scene["pt3d"], K, thr, iters)
    R32, t32, _ = lm_refine(*pose_from_P(P, K, np.float32), scene["pt2d"], scene["pt3d"], K, thr, iters, np.float32)
    return pose_distance(R64, t64, R32, t32)
