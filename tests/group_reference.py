"""The definition of socp_group_batch (include/socp_hip.h) restated in numpy: greedy leader grouping of the rows of a table IN ROW
ORDER, in the float64 operations exactly as the header writes them -- fl(v - l), fl(rtol * |l|), fl(atol + .), an inclusive
comparison, no contraction (numpy rounds every operation).  The only reference of the grouping tests."""
import numpy as np

OVERFLOW, NOTFINITE, MASKED = -1, -2, -3


def near(v, L, atol, rtol):
    """v[n] against the leader rows L[G][n]: (near[G], max_i |fl(v_i - l_i)| [G]).  Element-wise float64 operations, one rounding each."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.abs(v - L)
        bound = atol + rtol * np.abs(L)
    return np.all(d <= bound, axis=1), d.max(axis=1)


def group_reference(V, n=None, mask=None, atol=0.0, rtol=1e-6, max_groups=1024):
    """dict(label[B], leader[max_groups] (-1 unused), count[max_groups] (0 unused), radius[max_groups] (0 unused), summary[4] =
    [G, overflow, non-finite, masked]) -- the full-length arrays the C entry points fill."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    B = V.shape[0]
    n = V.shape[1] if n is None else n
    label = np.zeros(B, dtype=np.int32)
    leader = np.full(max_groups, -1, dtype=np.int32)
    count = np.zeros(max_groups, dtype=np.int32)
    radius = np.zeros(max_groups)
    G = 0
    for b in range(B):
        if mask is not None and mask[b] == 0:
            label[b] = MASKED
            continue
        v = V[b, :n]
        if not np.all(np.isfinite(v)):
            label[b] = NOTFINITE
            continue
        ok, d = near(v, V[leader[:G], :n], atol, rtol)            # every leader so far; the FIRST near one takes the row
        if ok.any():
            g = int(np.argmax(ok))
            label[b] = g
            count[g] += 1
            radius[g] = max(radius[g], d[g])
        else:
            if G < max_groups:
                leader[G], label[b], count[G] = b, G, 1         # (the leader's own differences are +0)
                G += 1
            else:
                label[b] = OVERFLOW
    summary = np.array([G, np.sum(label == OVERFLOW), np.sum(label == NOTFINITE), np.sum(label == MASKED)], dtype=np.int32)
    return dict(label=label, leader=leader, count=count, radius=radius, summary=summary)
