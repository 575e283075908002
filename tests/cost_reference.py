"""The definition of socp_cost_batch restated in numpy (helper of test_cost_cpu.py / test_gpu_cost_batch.py, not a test).

The running cost is L(t, X) = H(t, X) - sum_k p_k f_k(t, X), carried as a quadrature variable q' = L through the fixed RK4 steps
the residual takes.  Every operation below is one IEEE double operation (numpy does not contract), in the order the
reference-order kernel performs it, so a result can be compared bit for bit.

`rhs(t, X)` and `ham(t, X)` are the model's right-hand side and Hamiltonian.  With X of shape [2d] and scalar t the functions
work on one trajectory; with X of shape [L][2d] and t of shape [L] on L trajectories at once (the arithmetic is element-wise, so
both forms give the same bits)."""
import numpy as np


def lagrangian(ham, d, t, Y, F):
    """H(t, Y) - s,  s = Y[d] F[0];  s = s + Y[d+k] F[k]  for k = 1 .. d-1."""
    s = Y[..., d] * F[..., 0]
    for k in range(1, d):
        s = s + Y[..., d + k] * F[..., k]
    return ham(t, Y) - s


def reference_step(rhs, ham, d, t, X, step, q):
    """One RK4 step of the state (odeTools.cpp:89-98, the association order of Lane::rk4) and of the quadrature: returns (X, q)."""
    col = (lambda a: a[..., None]) if np.ndim(X) == 2 else (lambda a: a)        # a per-trajectory scalar against its state row
    h2 = step / 2.0
    th = t + step / 2.0
    F1 = rhs(t, X)
    L1 = lagrangian(ham, d, t, X, F1)
    Y = X + col(h2) * F1
    F2 = rhs(th, Y)
    L2 = lagrangian(ham, d, th, Y, F2)
    Y = X + col(h2) * F2
    F3 = rhs(th, Y)
    L3 = lagrangian(ham, d, th, Y, F3)
    Y = X + col(step) * F3
    F4 = rhs(t + step, Y)
    L4 = lagrangian(ham, d, t + step, Y, F4)
    h6 = step / 6.0
    X = X + col(h6) * (F1 + (F4 + 2.0 * (F2 + F3)))
    q = q + h6 * (L1 + (L4 + 2.0 * (L2 + L3)))
    return X, q


def reference_cost(rhs, ham, d, t1, t2, X, N, after=None):
    """One segment: the loop of Lane::integrate (dt = (t2 - t1)/N, t accumulated by t += dt, last step clamped to t2 - t, no step
    when t2 <= t1 + dt/2) around reference_step, q = 0.0 at the start.  Returns (cost, X_end).  `after(t_before, step, X, q)` sees
    every step."""
    X = np.array(X, dtype=np.float64)
    t1, t2 = np.float64(t1), np.float64(t2)
    q = np.float64(0.0)
    dt = (t2 - t1) / N
    t = t1
    guard = N + 8
    while t < (t2 - dt / 2) and guard > 0:
        guard -= 1
        step = (t2 - t) if (t + dt > t2) else dt
        X, q = reference_step(rhs, ham, d, t, X, step, q)
        if after is not None:
            after(t, step, X, q)
        t += dt
    return q, X


def reference_cost_lanes(rhs, ham, d, t1, t2, X, N):
    """L segments in lock-step, for references whose evaluation is itself a batch: the same loop with every lane's own
    condition; `rhs(idx, t, X)` / `ham(idx, t, X)` receive the indices of the lanes that take the step.  Returns (cost[L], X_end[L][2d])."""
    X = np.array(X, dtype=np.float64)
    t1, t2 = np.array(t1, dtype=np.float64), np.array(t2, dtype=np.float64)
    q = np.zeros(len(X))
    dt = (t2 - t1) / N
    t = t1.copy()
    for _ in range(N + 8):
        idx = np.where(t < (t2 - dt / 2))[0]
        if len(idx) == 0:
            break
        ti, dti, tfi = t[idx], dt[idx], t2[idx]
        step = np.where(ti + dti > tfi, tfi - ti, dti)
        X[idx], q[idx] = reference_step(lambda tt, Y: rhs(idx, tt, Y), lambda tt, Y: ham(idx, tt, Y), d, ti, X[idx], step, q[idx])
        t[idx] = ti + dti
    return q, X
