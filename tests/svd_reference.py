"""socp_svd_batch_dev / socp_singular_batch restated in numpy (helper of test_svd_cpu.py / test_gpu_svd_batch.py, not a test).

The one-sided Jacobi iteration on the ROWS of the matrix as include/socp_hip.h writes it down, one operation per rounding: numpy
multiplies, adds and takes square roots in separate IEEE roundings (no fused multiply-add), which is what the reference-order
flavour of the device kernel does.  Vectorised over the batch and over the disjoint pairs of a step; the sums run over i in a
Python loop, one rounded product added at a time."""
import numpy as np

F64 = np.float64
EPS = float(np.finfo(F64).eps)


def schedule(n):
    """The round-robin schedule: a list of m - 1 steps, each a list of pairs (p, q), p < q < n (phantom pairs left out)."""
    m = n + (n & 1)
    steps = []
    for s in range(m - 1):
        pairs = []
        for k in range(m // 2):
            if k == 0:
                a, b = m - 1, s
            else:
                a, b = (s + k) % (m - 1), (s - k + m - 1) % (m - 1)
            p, q = min(a, b), max(a, b)
            if q < n:
                pairs.append((p, q))
        steps.append(pairs)
    return steps


def seq_dot(X, Y):
    """sum_i X[..., i] Y[..., i]: from +0.0, one rounded product added at a time, i = 0 .. n-1."""
    acc = np.zeros(X.shape[:-1], dtype=F64)
    for prod in np.moveaxis(X * Y, -1, 0):                         # every product rounded on its own, then added in order
        acc = acc + prod
    return acc


def svd_batch(A, max_sweeps=60, want_vt=True):
    """A[B][n*n] column-major (or [B][n][n] holding the same memory: A[b][j][i] = entry (i, j)) -> dict(sigma[B][n], vt[B][n][n] or
    None, sweeps[B], info[B])."""
    A = np.asarray(A, dtype=F64)
    B = A.shape[0]
    n = int(round(np.sqrt(A[0].size))) if B else 1
    W = A.reshape(B, n, n).transpose(0, 2, 1).copy()              # W[b][p][i] = A[b][p + i n]: row p of the matrix
    tol = F64(n) * F64(EPS)
    info = np.zeros(B, dtype=np.int32)
    sweeps = np.zeros(B, dtype=np.int32)
    bad = ~np.all(np.isfinite(W.reshape(B, -1)), axis=1)
    info[bad] = 2
    live = ~bad                                                    # still iterating
    steps = [(np.array([p for p, _ in st], dtype=np.intp), np.array([q for _, q in st], dtype=np.intp)) for st in schedule(n) if st]
    with np.errstate(all="ignore"):
        for sweep in range(1, max_sweeps + 1):
            idx = np.nonzero(live)[0]
            if idx.size == 0:
                break
            Wl = W[idx]
            rotated = np.zeros(idx.size, dtype=bool)
            for P, Q in steps:
                wp, wq = Wl[:, P, :], Wl[:, Q, :]
                alpha, beta, gamma = seq_dot(np.stack([wp, wq, wp]), np.stack([wp, wq, wq]))
                skip = (gamma == 0.0) | (np.abs(gamma) <= (tol * np.sqrt(alpha)) * np.sqrt(beta))
                rot = ~skip
                if not rot.any():
                    continue
                zeta = (beta - alpha) / (2.0 * gamma)
                t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                c, s = c[..., None], s[..., None]
                np_ = c * wp - s * wq
                nq_ = s * wp + c * wq
                r3 = rot[..., None]
                Wl[:, P, :] = np.where(r3, np_, wp)
                Wl[:, Q, :] = np.where(r3, nq_, wq)
                rotated |= rot.any(axis=1)
            W[idx] = Wl
            sweeps[idx] = sweep
            live[idx[~rotated]] = False
        info[live] = 1
        sig = np.sqrt(seq_dot(W, W))                               # [B][n], by row
        # rank by counting: larger first, equal values by ascending row
        gt = sig[:, None, :] > sig[:, :, None]                     # [b][p][q]: sigma_q > sigma_p
        eq = (sig[:, None, :] == sig[:, :, None]) & (np.arange(n)[None, None, :] < np.arange(n)[None, :, None])
        rank = (gt | eq).sum(axis=2)
        sigma = np.full((B, n), np.nan)
        vt = np.full((B, n, n), np.nan) if want_vt else None
        for b in range(B):
            if bad[b]:
                continue
            sigma[b, rank[b]] = sig[b]
            if want_vt:
                V = np.where(sig[b][:, None] == 0.0, 0.0, W[b] / sig[b][:, None])
                big = np.argmax(np.abs(V), axis=1)                # the first among equals
                neg = V[np.arange(n), big] < 0.0
                V = np.where(neg[:, None], -V, V)
                vt[b, rank[b]] = V
    return dict(sigma=sigma, vt=vt, sweeps=sweeps, info=info)


def column_scale(J):
    """J[B][n*n] column-major -> (J scaled, colnorm[B][n]): colnorm_j = sqrt(sum_i J_ij^2) summed in order, a zero replaced by 1."""
    J = np.asarray(J, dtype=F64)
    B = J.shape[0]
    n = int(round(np.sqrt(J[0].size)))
    C = J.reshape(B, n, n)                                         # C[b][j] = column j
    with np.errstate(all="ignore"):
        norm = np.sqrt(seq_dot(C, C))
        norm = np.where(norm == 0.0, 1.0, norm)
        return (C / norm[:, :, None]).reshape(J.shape), norm


def singular_batch(J, scale=0, max_sweeps=60):
    """Steps 3 and 4 of socp_singular_batch on the Jacobians J[B][n*n] (column-major): dict(sigma, vmin, colnorm, sweeps, info)."""
    J = np.asarray(J, dtype=F64)
    B = J.shape[0]
    n = int(round(np.sqrt(J[0].size)))
    J = J.reshape(B, n * n)
    if scale:
        J, colnorm = column_scale(J)
    else:
        colnorm = np.ones((B, n))
    r = svd_batch(J, max_sweeps)
    return dict(sigma=r["sigma"], vmin=r["vt"][:, n - 1, :].copy(), colnorm=colnorm, sweeps=r["sweeps"], info=r["info"])


# ---- fixtures both test files share ---------------------------------------------------------------------------------------------

def colmajor(M):
    """A matrix M[i][j] (or a stack of them) as the column-major rows the call takes."""
    M = np.asarray(M, dtype=F64)
    return np.swapaxes(M, -1, -2).reshape(M.shape[:-2] + (-1,)).copy()


def graded(n, cond, seed):
    """U diag(s) V^T with s log-spaced from 1 down to 1 / cond and random orthogonal U, V (seeded)."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0.0, -np.log10(cond), n) if n > 1 else np.ones(1)
    return (U * s) @ V.T


CONDS = (2.0, 1e6, 1e12)
SIZES = (2, 3, 14, 15, 64, 65, 85, 127)


def graded_batch(n):
    """The three matrices of size n (cond 2, 1e6, 1e12), column-major rows."""
    return colmajor(np.array([graded(n, c, 1000 * n + k) for k, c in enumerate(CONDS)]))


def accuracy_ratios(A, sigma, vmin):
    """The three measured quantities of one column-major matrix against LAPACK, each divided by its unit (n eps sigma_max, the same,
    n eps): (max |sigma^ - sigma|, | ||A vmin||2 - sigma^_min |, | ||vmin||2 - 1 |)."""
    n = sigma.size
    M = np.asarray(A, dtype=F64).reshape(n, n).T
    ref = np.linalg.svd(M, compute_uv=False)
    unit = n * EPS * ref[0]
    return (float(np.max(np.abs(sigma - ref)) / unit), float(abs(np.linalg.norm(M @ vmin) - sigma[-1]) / unit),
            float(abs(np.linalg.norm(vmin) - 1.0) / (n * EPS)))


# c of the three bounds: 4 x the largest ratio measured with this restatement on graded_batch(n), n in SIZES, and on the oracle's
# Goddard and double-integrator Jacobians, rounded up (the figures are in test_svd_cpu.py's docstring)
C_BOUND = 3.0

MAX_SWEEPS = 60
_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def graded_reference(n):
    """(A[3][n*n], the restatement's result on it at MAX_SWEEPS), computed once."""
    def build():
        A = graded_batch(n)
        A.setflags(write=False)
        return A, svd_batch(A, MAX_SWEEPS)
    return cached(("graded", n), build)


def random_batch(n, B, seed=None):
    """B well-conditioned random matrices (standard normal entries), column-major rows."""
    rng = np.random.default_rng(77 * n + B if seed is None else seed)
    return rng.standard_normal((B, n * n))


def permuted_diagonal():
    """A 5 x 5 matrix with one entry per row and column, M[i][perm[i]] = d[i]; its hand-written decomposition (sigma, Vt)."""
    perm, d = [2, 0, 4, 1, 3], [-3.0, 0.5, 7.0, -0.25, 3.0]
    M = np.zeros((5, 5))
    for i in range(5):
        M[i, perm[i]] = d[i]
    # descending |d|, equal values by ascending row: rows 2 (7), 0 (3), 4 (3), 1 (0.5), 3 (0.25); every vector made positive
    order = [2, 0, 4, 1, 3]
    sigma = np.array([7.0, 3.0, 3.0, 0.5, 0.25])
    Vt = np.zeros((5, 5))
    for j, row in enumerate(order):
        Vt[j, perm[row]] = 1.0
    return colmajor(M)[None, :], sigma, Vt


def mixed_batch(n=14):
    """One batch of eight n x n matrices whose fates differ: 0, 1 healthy, 2 holds a NaN, 3 healthy, 4 holds an infinity, 5 the zero
    matrix, 6 two equal rows, 7 healthy.  With n = 14 they share one workgroup."""
    A = random_batch(n, 8, seed=4242).reshape(8, n, n)
    A[2, n // 2, 1] = np.nan
    A[4, 0, n - 1] = -np.inf
    A[5] = 0.0
    A[6, :, 3] = A[6, :, 9 % n]                                   # memory is [column][row]: rows 3 and 9 of the matrix are equal
    return A.reshape(8, n * n)
