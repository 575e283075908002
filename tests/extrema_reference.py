"""The definition of socp_extrema_batch restated in numpy (helper of test_extrema_cpu.py / test_gpu_extrema_batch.py, not a test).

A segment's rows are the rows socp_trace_batch keeps with stride = 1, in the trace's format [R][W] = t, X[S], u[NU], H, aux0, aux1.
The channels of a row are X[S], u[NU], H and the model's event channels g[EC] (the restatements of tests/events_reference.py,
evaluated on the row's X); the reduction runs over the rows IN ORDER with strict comparisons, one IEEE comparison per line of the
header's definition, so a result can be compared bit for bit:
    row 0:  vmin = vmax = v, tmin = tmax = t;    later:  if v < vmin: vmin, tmin = v, t;    if v > vmax: vmax, tmax = v, t
The first attainment wins, -0.0 never displaces +0.0, a NaN never displaces anything and a NaN in row 0 stays."""
import numpy as np

from events_reference import goddard_event, dint_event, covid_event

F64 = np.float64
CONTROL, HAMILTONIAN, EVENTS = 1, 2, 4
EVENT_FN = {"goddard": (goddard_event, 1), "dint": (dint_event, 1), "covid": (covid_event, 2)}

SENT = np.uint64(0x7FF8DEADBEEF0001)            # a NaN no kernel produces
SENT_I = np.int32(-559038737)
GUARD = 64


def u64(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def less(v, best):
    return v < best


def greater(v, best):
    return v > best


def reduce_rows(t, V, below=less, above=greater):
    """t[R], V[R][C] -> (vmin[C], vmax[C], tmin[C], tmax[C]): the sequential reduction, every channel on its own.
    below / above: the two comparisons (replaced by the wrong restatements of test_extrema_cpu.py)."""
    t, V = np.asarray(t, dtype=F64), np.asarray(V, dtype=F64)
    R, C = V.shape
    vmin, vmax = V[0].copy(), V[0].copy()
    tmin, tmax = np.full(C, t[0]), np.full(C, t[0])
    for k in range(1, R):
        for c in range(C):
            v = V[k, c]
            if below(v, vmin[c]):
                vmin[c], tmin[c] = v, t[k]
            if above(v, vmax[c]):
                vmax[c], tmax[c] = v, t[k]
    return vmin, vmax, tmin, tmax


def selected_columns(S, NU, EC, what):
    """Mask [C] of the channels `what` selects: the state always, u / H / g by its bits."""
    sel = np.zeros(S + NU + 1 + EC, dtype=bool)
    sel[:S] = True
    sel[S:S + NU] = bool(what & CONTROL)
    sel[S + NU] = bool(what & HAMILTONIAN)
    sel[S + NU + 1:] = bool(what & EVENTS)
    return sel


def count_bad(V, sel):
    """Rows in which at least one selected channel is not finite."""
    V = np.asarray(V, dtype=F64)
    return int(np.sum(~np.all(np.isfinite(V[:, sel]), axis=1)))


def channels_of_rows(rows, S, NU, event=None, EC=0, params=None):
    """Trace-format rows [R][W] -> (t[R], V[R][C]), C = S + NU + 1 + EC; event(params, X, c) restates channel c."""
    rows = np.asarray(rows, dtype=F64)
    g = np.array([[event(params, X, c) for c in range(EC)] for X in rows[:, 1:1 + S]], dtype=F64).reshape(len(rows), EC)
    return rows[:, 0].copy(), np.concatenate([rows[:, 1:1 + S + NU + 1], g], axis=1)


def reference_extrema(rows, S, NU, what, event=None, EC=0, params=None):
    """One segment: dict(vmin, vmax, tmin, tmax [C], sel [C], count, nbad) of its trace-format rows."""
    t, V = channels_of_rows(rows, S, NU, event, EC, params)
    sel = selected_columns(S, NU, EC, what)
    vmin, vmax, tmin, tmax = reduce_rows(t, V)
    return dict(vmin=vmin, vmax=vmax, tmin=tmin, tmax=tmax, sel=sel, count=len(t), nbad=count_bad(V, sel))


def reference_from_trace(rows, count, S, NU, what, event=None, EC=0, params=None):
    """What trace_batch(stride = 1) returned (rows[B][M][cap][W], count[B][M], every count <= cap) -> list [b][i] of
    reference_extrema; params: one packed parameter vector, or [B] of them (per-row blocks)."""
    B, M = count.shape
    assert count.max() <= rows.shape[2], "the trace's cap was too small for this comparison"
    per_row = params is not None and np.ndim(params) == 2
    return [[reference_extrema(rows[b, i, :count[b, i]], S, NU, what, event, EC, params[b] if per_row else params) for i in range(M)]
            for b in range(B)]


def sentinel(size):
    return np.full(size + GUARD, SENT, dtype=np.uint64).view(F64)


def sentinel_i(size):
    return np.full(size + GUARD, SENT_I, dtype=np.int32)


def pack_extrema(ref, times=(True, True), nbad=True):
    """What the entry points leave in guarded, sentinel-filled caller buffers: the six WHOLE buffers (vmin, vmax, tmin, tmax as
    uint64, count, nbad as int32), guard words included.  Columns of a group that is not selected, and a buffer that was not passed
    (times[0] / times[1] / nbad False), keep the sentinel."""
    B, M, C = len(ref), len(ref[0]), len(ref[0][0]["sel"])
    bufs = [np.full(B * M * C + GUARD, SENT, dtype=np.uint64) for _ in range(4)]
    cnt, bad = sentinel_i(B * M), sentinel_i(B * M)
    given = (True, True, times[0], times[1])
    for b in range(B):
        for i in range(M):
            r, T = ref[b][i], b * M + i
            for buf, key, on in zip(bufs, ("vmin", "vmax", "tmin", "tmax"), given):
                if on:
                    buf[T * C:(T + 1) * C][r["sel"]] = u64(r[key])[r["sel"]]
            cnt[T] = r["count"]
            if nbad:
                bad[T] = r["nbad"]
    return (*bufs, cnt, bad)
