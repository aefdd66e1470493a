"""NumPy restatement of the EXACT gradient of nlZ (gpak_grad_exact) and a line-for-line port of the driver that uses
it (Opt_Algs::ProjectedLBFGSOptimise, gp_ss_ak_amd/host/opt_algs.cpp).  TEST INFRASTRUCTURE, written independently of
the device code:

  nlZ(theta) = 1/2 y'(K + sn2 I)^-1 y + 1/2 log|K + sn2 I| + const
  d nlZ / d theta = 1/2 sum_ij W_ij dK_ij / d theta,   W = (K + sn2 I)^-1 - alpha alpha',  alpha = (K + sn2 I)^-1 y

Where the device accumulates parameter-independent moments over the pairs and contracts them on the host, this file
forms every dK / d theta as a full matrix (row slabs of it, to bound the memory at N = 8192) from the analytic
dA / d theta, and sums W o dK.  tests/test_exact_grad.py checks it against finite differences of the CPU checker's nlZ.

Parameter layout = gpak_grad_hyb's: the stationary children's blocks in order (ExpAns 8, Exp 2, RBF 3), bias, sn2.
"""
import math

import numpy as np

EXPANS, EXP, RBF = 0, 1, 2


def rotation(ax, ay, az):
    """Rot of Kernel.cpp:1399-1410 for the angles (AngleX, AngleY, AngleZ), rows top to bottom."""
    ca, sa, cb, sb, ct, st = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    return np.array([[ca * ct + sa * sb * st, -sa * ct + ca * sb * st, -cb * st],
                     [sa * cb, ca * cb, sb],
                     [ca * st - sa * sb * ct, -sa * st - ca * sb * ct, cb * ct]])


def rotation_derivatives(ax, ay, az):
    """d Rot / d AngleX, d AngleY, d AngleZ, each entry differentiated by hand from rotation()."""
    ca, sa, cb, sb, ct, st = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    dx = np.array([[-sa * ct + ca * sb * st, -ca * ct - sa * sb * st, 0.0],
                   [ca * cb, -sa * cb, 0.0],
                   [-sa * st - ca * sb * ct, -ca * st + sa * sb * ct, 0.0]])
    dy = np.array([[sa * cb * st, ca * cb * st, sb * st],
                   [-sa * sb, -ca * sb, cb],
                   [-sa * cb * ct, -ca * cb * ct, -sb * ct]])
    dz = np.array([[-ca * st + sa * sb * ct, sa * st + ca * sb * ct, -cb * ct],
                   [0.0, 0.0, 0.0],
                   [ca * ct + sa * sb * st, -sa * ct + ca * sb * st, -cb * st]])
    return dx, dy, dz


def expans_metric(p):
    """A = Rot diag(lam) Rot' and the six dA / d{AngleX, lam_x, AngleY, lam_y, AngleZ, lam_z} (parameter order)."""
    R = rotation(p[0], p[2], p[4])
    dR = rotation_derivatives(p[0], p[2], p[4])
    lam = np.diag([p[1], p[3], p[5]])
    A = R @ lam @ R.T
    dA = []
    for a in range(3):
        dA.append(dR[a] @ lam @ R.T + R @ lam @ dR[a].T)
        dA.append(np.outer(R[:, a], R[:, a]))
    return A, dA


def _term_blocks(kind, p, dcols, d):
    """For one stationary term on a slab of pairs: K block and the list of dK / dp blocks.  dcols[c] = x_ic - x_jc."""
    if kind == EXPANS:
        A, dA = expans_metric(p)
        A2 = A @ A
        D = sum(A2[a, b] * dcols[a] * dcols[b] for a in range(3) for b in range(3))
        if d == 4:
            D = D + (p[7] * dcols[3]) ** 2
        D = np.maximum(D, 0.0)
        sd = np.sqrt(D)
        e = np.exp(-sd)
        with np.errstate(divide="ignore", invalid="ignore"):
            dk = np.where(sd > 0.0, -e / (2.0 * sd), 0.0)
        var2 = p[6] * p[6]
        out = []
        for Ap in dA:
            C = A @ Ap + Ap @ A
            out.append(var2 * dk * sum(C[a, b] * dcols[a] * dcols[b] for a in range(3) for b in range(3)))
        out.append(2.0 * p[6] * e)
        out.append(var2 * dk * 2.0 * p[7] * dcols[3] ** 2 if d == 4 else np.zeros_like(e))
        return var2 * e, out
    d2 = sum(dcols[c] ** 2 for c in range(d)) / (p[0] * p[0])
    if kind == EXP:                                  # Sigma^2 exp(-sqrt(d2)), d2 = |x - x'|^2 / hyp^2
        sd = np.sqrt(d2)
        e = np.exp(-sd)
        with np.errstate(divide="ignore", invalid="ignore"):
            dk = np.where(sd > 0.0, -e / (2.0 * sd), 0.0)
        var2 = p[1] * p[1]
        return var2 * e, [var2 * dk * (-2.0 * d2 / p[0]), 2.0 * p[1] * e]
    e = np.exp(-0.5 * p[1] * d2)                     # Sigma^2 exp(-iw d2 / 2)
    var2 = p[2] * p[2]
    return var2 * e, [var2 * e * (-0.5 * p[1]) * (-2.0 * d2 / p[0]), var2 * e * (-0.5 * d2), 2.0 * p[2] * e]


def gram(X, terms, bias):
    X = np.asarray(X, dtype=float)
    N, d = X.shape
    dcols = [X[:, c][:, None] - X[:, c][None, :] for c in range(d)]
    K = np.full((N, N), float(bias))
    for kind, p in terms:
        K += _term_blocks(kind, [float(v) for v in p], dcols, d)[0]
    return K


def weights(K, y, sn2):
    """W = (K + sn2 I)^-1 - alpha alpha'."""
    N = K.shape[0]
    M = K + sn2 * np.eye(N)
    L = np.linalg.cholesky(M)
    Li = np.linalg.solve(L, np.eye(N))
    Minv = Li.T @ Li
    alpha = Minv @ np.asarray(y, dtype=float)
    return Minv - np.outer(alpha, alpha)


def grad_exact(X, y, terms, bias, sn2, W=None, slab=1024):
    """terms = [(kind, parameters in the reference's order)].  Returns the gradient, gpak_grad_hyb's layout."""
    X = np.asarray(X, dtype=float)
    N, d = X.shape
    terms = [(int(k), [float(v) for v in p]) for k, p in terms]
    if W is None:
        W = weights(gram(X, terms, bias), y, sn2)
    ng = sum({EXPANS: 8, EXP: 2, RBF: 3}[k] for k, _ in terms)
    g = np.zeros(ng + 2)
    for r0 in range(0, N, slab):
        r1 = min(N, r0 + slab)
        Ws = W[r0:r1]
        dcols = [X[r0:r1, c][:, None] - X[:, c][None, :] for c in range(d)]
        o = 0
        for kind, p in terms:
            for dK in _term_blocks(kind, p, dcols, d)[1]:
                g[o] += 0.5 * float(np.sum(Ws * dK))
                o += 1
    g[ng] = 0.5 * float(W.sum())            # dK / d bias = ones
    g[ng + 1] = 0.5 * float(np.trace(W))    # d(K + sn2 I) / d sn2 = I
    return g


# ---------------------------------------------------------------------------------------------------------------
# Opt_Algs::ProjectedLBFGSOptimise, line for line.  Reductions are left-to-right loops in Python floats so that the two
# round alike; exp / log go through the same libm.
# ---------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s += float(x) * float(y)
    return s


def projected_lbfgs(fun, grad, x0, is_angle, maxit, trace=None):
    """fun(x) -> objective (one factorisation); grad(x) -> exact gradient with respect to x at a point fun has just
    evaluated.  Returns (x, [kept objective after each iteration], evaluations).
    trace: optional list that receives (objective, evaluations so far, point) after every iteration."""
    n = len(x0)
    mem, maxls = 6, 12
    ang = [bool(a) for a in is_angle]
    lbz = [1e-4 if ang[i] else math.log(1e-4) for i in range(n)]
    ubz = [6.0 if ang[i] else math.log(6.0) for i in range(n)]
    x = [min(6.0, max(1e-4, float(v))) for v in x0]
    z = [x[i] if ang[i] else math.log(x[i]) for i in range(n)]
    f = float(fun(np.array(x)))
    nfev = 1
    G = grad(np.array(x))
    g = [float(G[i]) if ang[i] else x[i] * float(G[i]) for i in range(n)]
    S, Y = [], []

    def ginf():
        m = 0.0
        for v in g:
            m = max(m, abs(v))
        return m

    gamma = 1.0 / max(ginf(), 1.0)
    hist = []
    for it in range(1, maxit + 1):
        def project(d):
            for i in range(n):
                if (z[i] <= lbz[i] and d[i] < 0) or (z[i] >= ubz[i] and d[i] > 0):
                    d[i] = 0.0

        if not S:
            sc = 1.0 / max(ginf(), 1.0)
            d = [-g[i] * sc for i in range(n)]
        else:
            m = len(S)
            q = list(g)
            al = [0.0] * m
            for k in range(m - 1, -1, -1):
                al[k] = _dot(S[k], q) / _dot(S[k], Y[k])
                for i in range(n):
                    q[i] -= al[k] * Y[k][i]
            for i in range(n):
                q[i] *= gamma
            for k in range(m):
                b = _dot(Y[k], q) / _dot(S[k], Y[k])
                for i in range(n):
                    q[i] += S[k][i] * (al[k] - b)
            d = [-q[i] for i in range(n)]
        project(d)
        if _dot(g, d) >= 0:
            S, Y = [], []
            d = [-gamma * g[i] for i in range(n)]
            project(d)
        step, fn, ok = 1.0, f, False
        zn, xn = [0.0] * n, [0.0] * n
        for _ in range(maxls):
            for i in range(n):
                zn[i] = min(ubz[i], max(lbz[i], z[i] + step * d[i]))
                xn[i] = zn[i] if ang[i] else math.exp(zn[i])
            fn = float(fun(np.array(xn)))
            nfev += 1
            gs = 0.0
            for i in range(n):
                gs += g[i] * (zn[i] - z[i])
            if math.isfinite(fn) and fn <= f + 1e-4 * gs:
                ok = True
                break
            step *= 0.5
        if not ok:
            hist.append(f)
            if trace is not None:
                trace.append((f, nfev, np.array(x)))
            if not S:
                break
            S, Y = [], []
            continue
        G = grad(np.array(xn))
        gn = [float(G[i]) if ang[i] else xn[i] * float(G[i]) for i in range(n)]
        s = [zn[i] - z[i] for i in range(n)]
        y = [gn[i] - g[i] for i in range(n)]
        smax = 0.0
        for v in s:
            smax = max(smax, abs(v))
        sy = _dot(s, y)
        if sy > 1e-10 * math.sqrt(_dot(s, s)) * math.sqrt(_dot(y, y)):
            if len(S) == mem:
                S.pop(0)
                Y.pop(0)
            S.append(s)
            Y.append(y)
            gamma = sy / _dot(y, y)
        df = f - fn
        x, z, g, f = list(xn), list(zn), gn, fn
        hist.append(f)
        if trace is not None:
            trace.append((f, nfev, np.array(x)))
        if smax < 1e-7 or df < 1e-9 * abs(f):
            break
    return np.array(x), hist, nfev
