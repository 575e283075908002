"""GPU: the batched exact sensitivities (socp_sensitivity_batch[_dev] / _blocks, capi.Context.sensitivity_batch) against
tests/sensitivity_reference.py -- the definition restated in Python on dual numbers, the parameter dual too.  Outputs live in
sentinel-filled buffers followed by 64 guard words and are compared WHOLE on integer views (the conventions of
test_gpu_exact_jacobian.py), so a store past a row or through a NULL Gp shows, and so does the sign of a zero.  Every output is
bit-equal to the restatement, in both flavours (the kernels are one object without contraction, the elimination runs in reference
order); the one exception is the payload of a NaN that arithmetic produced, so NaNs other than the sentinel are compared as NaN.
The inputs are tests/sensitivity_cases.py (N = 10 steps or less).  A reference is computed once and shared read-only.  Without the
feature every test fails at the missing symbol."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sensitivity_cases as sc
import sensitivity_reference as sr
from tangent_reference import DIR_PARAM, DIR_TIME, DIR_XNODE
from test_gpu_jacobi_batch import SENT, SENT_I, GUARD, DP, IP, sentinel, sentinel_i, views, canon, plugin_path   # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGIN_IDS = {"osc1d": ("osc1d_sensitivity", 1007), "osc1d_exact_jacobian": ("osc1d_exact_jacobian", 1005)}
_REF = {}


def context(c, variant="exact"):
    from socp_amd import capi
    if c["model"] in PLUGIN_IDS:
        name, ident = PLUGIN_IDS[c["model"]]
        capi.plugin_load(plugin_path(name))
        ctx = capi.Context(ident, nparams=1)
    else:
        ctx = capi.Context({"goddard": capi.MODEL_GODDARD, "dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[c["model"]])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(np.array(c["params"]))
    ctx.set_step_number(c["N"])
    if any(c["sw"]):
        ctx.set_switching_times(c["sw"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


def reference_of(c, dirs=None, blocks=None, rows=None):
    Z = c["Z"] if rows is None else c["Z"][rows]
    r = sr.sensitivity_batch(c["model"], [float(p) for p in c["params"]], c["sw"], c["prob"], Z, c["N"], c["dirs"] if dirs is None else dirs,
                             blocks=blocks)
    return r["dz"], r["info"], r["g"]


def reference(name):
    if name not in _REF:
        _REF[name] = reference_of(sc.CASES[name]())
    return _REF[name]


# ---- the forms on guarded buffers: each returns the three WHOLE buffers (dZ, info, G) as integer views ---------------------------------

def split(dirs):
    return np.array([d[0] for d in dirs], dtype=np.int32), np.array([d[1] for d in dirs], dtype=np.int32)


def run_host(ctx, Z, dirs, g=True, blocks=None):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B, n, K = len(Z), ctx.n, len(dirs)
    kind, index = split(dirs)
    out = (sentinel(B * K * n), sentinel_i(B), sentinel(B * K * n))
    tail = (K, kind.ctypes.data_as(IP), index.ctypes.data_as(IP), out[0].ctypes.data_as(DP), out[1].ctypes.data_as(IP),
            out[2].ctypes.data_as(DP) if g else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_sensitivity_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in blocks)
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None        # noqa: E731
        ctx._chk(ctx.L.socp_sensitivity_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt),
                                                     ptr(xx), *tail))
    return views(out)


def run_dev(ctx, Z, dirs, g=True):
    import torch
    B, n, K = len(Z), ctx.n, len(dirs)
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (sentinel(B * K * n), sentinel_i(B), sentinel(B * K * n))]
    bytes_ = ctx.sensitivity_work_bytes(B, K)
    assert bytes_ >= 8 * (B * n * n + B * K * n)
    work = torch.empty(bytes_ // 8 + GUARD, dtype=torch.float64, device="cuda")
    work[bytes_ // 8:] = 12345.0
    torch.cuda.synchronize()
    ctx.sensitivity_batch_dev(B, dZ.data_ptr(), dirs, work.data_ptr(), bytes_, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr() if g else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((work[bytes_ // 8:] == 12345.0).all()), "the workspace is not overrun"
    return views(tuple(t.cpu().numpy() for t in dev))


def check_whole(got, want, what):
    for name, g, w in zip(("dZ", "info", "G"), got, want):
        fill = np.uint64(SENT) if g.dtype == np.uint64 else SENT_I
        if w is None:
            assert np.all(g == fill), "%s: %s was written although its pointer was NULL" % (what, name)
            continue
        w = np.ascontiguousarray(w).ravel()
        w = w.view(np.uint64) if w.dtype == np.float64 else w.astype(np.int32)
        assert np.all(g[w.size:] == fill), "%s: guard words behind %s were written" % (what, name)
        gg, ww = canon(g[:w.size]), canon(w)
        bad = np.argwhere(gg != ww).ravel()
        assert len(bad) == 0, (what, name, "%d differ; first flat indices:" % len(bad), bad[:5].tolist(),
                               gg[bad[:5]].view(np.float64) if gg.dtype == np.uint64 else gg[bad[:5]],
                               ww[bad[:5]].view(np.float64) if ww.dtype == np.uint64 else ww[bad[:5]])


def expected_counters(c, dirs, B):
    """(trajectories, launches) of one call: B M (S + 1) plus B M per integrating direction; 3 launches plus one per integrating kind."""
    prob = c["prob"]
    M, S = prob.M, 2 * prob.dim
    npar = sum(1 for k, _ in dirs if k == DIR_PARAM)
    ntime = sum(1 for k, i in dirs if k == DIR_TIME and prob.mode_t[i] == 0)
    return B * M * (S + 1) + B * M * (npar + ntime), 3 + (npar > 0) + (ntime > 0)


# ---- 1. every case, every form, both flavours, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.CASES))
def test_equals_the_restatement(name):
    c = sc.CASES[name]()
    want = reference(name)
    dirs, Z = c["dirs"], c["Z"]
    B, K, n = len(Z), len(dirs), c["prob"].n
    assert {k for k, _ in dirs} == {DIR_PARAM, DIR_TIME, DIR_XNODE}
    ctx = context(c)
    assert ctx.has_sensitivity()
    t0, l0 = ctx.counters()
    check_whole(run_host(ctx, Z, dirs), want, name + ", host form")
    t1, l1 = ctx.counters()
    assert (t1 - t0, l1 - l0) == expected_counters(c, dirs, B), "the counters advance as the header says"
    check_whole(run_dev(ctx, Z, dirs), want, name + ", _dev form")
    assert tuple(np.subtract(ctx.counters(), (t1, l1))) == expected_counters(c, dirs, B)
    check_whole(run_dev(ctx, Z, dirs, g=False), (want[0], want[1], None), name + ", NULL Gp")
    check_whole(run_host(ctx, Z, dirs, g=False), (want[0], want[1], None), name + ", host form, NULL Gp")
    G = np.ascontiguousarray(want[2]).view(np.uint64).reshape(B, K, n)
    for k in c["unread"]:
        assert not G[:, k].any(), "G of a TIME direction on a FREE / CONTINUOUS node and of an unread XNODE entry is all +0.0"
    assert np.all(want[1] == 0) and np.isfinite(want[0]).all()
    ctx.close()
    fast = context(c, "fast")
    assert fast.has_sensitivity()
    check_whole(run_dev(fast, Z, dirs), want, name + ", throughput flavour, _dev form")
    check_whole(run_host(fast, Z, dirs), want, name + ", throughput flavour, host form")
    fast.close()


def test_one_direction_and_sixteen():
    """Goddard M = 1 (n = 14): K = 1, and K = 16 mixing all three kinds (the case's own table); one row alone."""
    c = sc.goddard_single()
    assert len(c["dirs"]) == 16
    ctx = context(c)
    full = reference("goddard_single")
    for k in (2, 8, 13):
        one = [c["dirs"][k]]
        want = (full[0][:, k:k + 1], full[1], full[2][:, k:k + 1])
        check_whole(run_dev(ctx, c["Z"], one), want, "K = 1, direction %d" % k)
        assert ctx.counters() is not None
    t0 = ctx.counters()
    check_whole(run_host(ctx, c["Z"][:1], [c["dirs"][13]]), (full[0][:1, 13:14], full[1][:1], full[2][:1, 13:14]), "B = 1, an XNODE direction alone")
    assert tuple(np.subtract(ctx.counters(), t0)) == (15, 3), "no integrating direction: the exact Jacobian, the finish, the elimination"
    ctx.close()


# ---- 2. the J the call uses --------------------------------------------------------------------------------------------------------

def test_the_jacobian_is_socp_exact_jacobian_batch_dev():
    """dZ of the call against socp_linsolve_batch_dev of a reference-order context on socp_exact_jacobian_batch_dev's matrices and -G:
    equal bit for bit, so the J the call eliminates is that call's."""
    import torch
    c = sc.goddard_m3()
    ctx = context(c)
    Z, dirs = c["Z"], c["dirs"]
    B, K, n = len(Z), len(dirs), ctx.n
    got = run_dev(ctx, Z, dirs)
    dZ = torch.from_numpy(np.array(Z)).cuda()
    J = torch.empty(B * n * n, dtype=torch.float64, device="cuda")
    Y = torch.from_numpy(-got[2][:B * K * n].view(np.float64)).cuda()
    info = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.exact_jacobian_batch_dev(B, dZ.data_ptr(), J.data_ptr(), None)
    ctx.linsolve_batch_dev(B, n, K, J.data_ptr(), Y.data_ptr(), info.data_ptr())
    ctx.synchronize()
    assert np.array_equal(canon(Y.cpu().numpy().view(np.uint64)), canon(got[0][:B * K * n])) and np.array_equal(info.cpu().numpy(), got[1][:B])
    ctx.close()


# ---- 3. per-row blocks: B = 1, 63, 64, 65 and 70 rows -----------------------------------------------------------------------------

def mixed_rows():
    """70 Goddard M = 1 rows drawn from five distinct (row, block) pairs -- a row's result depends on the row and its blocks alone, so
    the restatement computes each once -- plus one row whose t_f equals its t_0 (three exactly zero Jacobian columns: singular)."""
    c = sc.goddard_single()
    prob, B = c["prob"], 70
    pick = np.random.default_rng(70).integers(0, 5, B)
    Z = np.array(c["Z"])[pick]
    params = np.tile(np.concatenate([c["params"], [0.0, 0.0]]), (B, 1))
    params[:, 2] = np.array([250.0, 280.0, 310.0, 330.0, 350.0])[pick]      # KD
    params[:, 6] = np.array([0.5, 0.8, 1.0, 1.2, 1.5])[pick]                # mu2 > 0 in every row
    time = np.tile(prob.time, (B, 1))
    time[:, 1] *= np.array([1.0, 0.9, 1.1, 1.0, 0.95])[pick]
    xnode = np.tile(prob.xnode.ravel(), (B, 1))
    xnode[:, 14] = np.array([1.01, 1.011, 1.009, 1.012, 1.01])[pick]         # the final altitude
    time[40, 1] = time[40, 0]
    dirs = [(DIR_PARAM, 2), (DIR_PARAM, 6), (DIR_TIME, 1), (DIR_XNODE, 14)]
    return c, Z, (params, time, xnode), dirs


def test_rows_with_their_own_blocks_and_a_singular_row():
    from oracle.oracle import Problem
    c, Z, blocks, dirs = mixed_rows()
    B, K, n = len(Z), len(dirs), 14
    ctx = context(c)
    plain = run_host(ctx, Z[:3], dirs)
    want = reference_of(dict(c, Z=Z), dirs=dirs, blocks=blocks)
    assert want[1][40] != 0 and np.isnan(want[0][40]).all(), "the singular row: info != 0 and NaN rows"
    assert np.all(np.delete(want[1], 40) == 0) and np.isfinite(np.delete(want[0], 40, axis=0)).all(), "and only it"
    for rows in (1, 63, 64, 65, 70):
        sub = tuple(a[:rows] for a in blocks)
        got = run_host(ctx, Z[:rows], dirs, blocks=sub)
        check_whole(got, tuple(w[:rows] for w in want), "_blocks form, B = %d" % rows)
    again = run_host(ctx, Z[:3], dirs)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again)), "the context's own blocks are back"
    fast = context(c, "fast")
    check_whole(run_host(fast, Z, dirs, blocks=blocks), want, "_blocks form, throughput flavour, B = 70")
    fast.close()
    only_time = run_host(ctx, Z[:3], dirs, blocks=(None, blocks[1][:3], None))
    check_whole(only_time, reference_of(dict(c, Z=Z[:3]), dirs=dirs, blocks=(None, blocks[1][:3], None)), "_blocks form, the time block alone")
    for b in (0, 39, 40, 41, 69):                                         # a row equals the row run alone under its own setting
        one = dict(c, params=blocks[0][b, :8], prob=Problem(7, c["prob"].mode_t, c["prob"].mode_x, blocks[1][b], blocks[2][b].reshape(2, 14)))
        cb = context(one)
        row = run_host(cb, Z[b:b + 1], dirs)
        cb.close()
        check_whole(row, tuple(w[b:b + 1] for w in want), "row %d alone" % b)
    ctx.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------

def raw(ctx, B, Z, dirs, out, form="host", K=None, work=None, work_bytes=None):
    kind, index = split(dirs) if dirs is not None else (None, None)
    K = len(dirs) if K is None else K
    ip = lambda a: a.ctypes.data_as(IP) if a is not None else None               # noqa: E731
    if form == "host":
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None          # noqa: E731
        return ctx.L.socp_sensitivity_batch(ctx.h, B, ptr(Z), K, ip(kind), ip(index), ptr(out[0]), ip(out[1]), ptr(out[2]))
    adr = lambda a: a.ctypes.data if a is not None else None                     # noqa: E731
    return ctx.L.socp_sensitivity_batch_dev(ctx.h, B, adr(Z), K, ip(kind), ip(index), work, work_bytes or 0, adr(out[0]), adr(out[1]), adr(out[2]))


def test_refusals_write_nothing_and_carry_a_message():
    import torch
    from socp_amd import capi
    from oracle.oracle import FREE
    c = sc.goddard_m3()
    ctx = context(c)
    Z, dirs = np.ascontiguousarray(c["Z"]), c["dirs"]
    B, n, K = len(Z), ctx.n, len(dirs)
    out = (sentinel(B * K * n), sentinel_i(B), sentinel(B * K * n))
    fresh_out = lambda o: all(np.all(v == (np.uint64(SENT) if v.dtype == np.uint64 else SENT_I)) for v in views(o))      # noqa: E731
    L, h = ctx.L, ctx.h
    err = lambda: L.socp_last_error(h).decode()                                  # noqa: E731
    bytes_ = ctx.sensitivity_work_bytes(B, K)
    work = torch.zeros(bytes_ // 8, dtype=torch.float64, device="cuda")
    t0 = ctx.counters()
    assert raw(ctx, -1, Z, dirs, out) == capi.ERR_ARG and "B >= 0" in err()
    for k in (0, 17):
        assert raw(ctx, B, Z, dirs, out, K=k) == capi.ERR_ARG and "1 <= K <= 16" in err()
        assert ctx.sensitivity_work_bytes(B, k) == 0
    assert raw(ctx, B, Z, None, out, K=2) == capi.ERR_ARG
    for bad in ((DIR_PARAM, 8), (DIR_PARAM, 9)):
        assert raw(ctx, B, Z, [dirs[0], bad], out) == capi.ERR_ARG and "switching time" in err(), "a PARAM index >= nparams"
    for bad in ((DIR_PARAM, 10), (DIR_PARAM, -1), (3, 0), (DIR_TIME, 4), (DIR_XNODE, 7), (DIR_XNODE, 56)):
        assert raw(ctx, B, Z, [bad], out) == capi.ERR_ARG, bad
    for form in ("host", "dev"):
        assert raw(ctx, B, None, dirs, out, form, work=work.data_ptr(), work_bytes=bytes_) == capi.ERR_ARG
        assert raw(ctx, B, Z, dirs, (None, out[1], out[2]), form, work=work.data_ptr(), work_bytes=bytes_) == capi.ERR_ARG
        assert raw(ctx, 0, None, dirs, (None, None, None), form) == capi.OK
    dZ = torch.from_numpy(np.array(Z)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in out]
    torch.cuda.synchronize()
    args = (h, B, dZ.data_ptr(), K, *(a.ctypes.data_as(IP) for a in split(dirs)))
    tail = (dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr())
    assert L.socp_sensitivity_batch_dev(*args, work.data_ptr(), bytes_ - 8, *tail) == capi.ERR_ARG and "workspace" in err(), "short work_bytes"
    assert L.socp_sensitivity_batch_dev(*args, None, bytes_, *tail) == capi.ERR_ARG
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    kind, index = split(dirs)
    for pstride in (8, 9, 11):
        assert L.socp_sensitivity_batch_blocks(h, B, Z.ctypes.data_as(DP), params.ctypes.data_as(DP), pstride, None, None, K, kind.ctypes.data_as(IP),
                                               index.ctypes.data_as(IP), out[0].ctypes.data_as(DP), out[1].ctypes.data_as(IP), None) == capi.ERR_ARG
    assert "nparams + 2" in err()
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    for form in ("host", "dev"):
        assert raw(ctx, B, Z, dirs, out, form, work=work.data_ptr(), work_bytes=bytes_) == capi.ERR_UNSUPPORTED and "DOPRI5" in err()
    ctx.set_integrator(capi.INT_RK4)
    prob = c["prob"]
    mode_x = prob.mode_x.copy()
    mode_x[1, 2] = FREE
    assert ctx.problem_set(prob.mode_t, mode_x, prob.time, prob.xnode) == prob.n
    assert raw(ctx, B, Z, dirs, out) == capi.ERR_UNSUPPORTED and "FREE state component" in err()
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    torch.cuda.synchronize()
    assert ctx.counters() == t0 and fresh_out(out) and fresh_out(tuple(t.cpu().numpy() for t in dev)), "nothing was launched, counted or written"
    assert not bool(work.any()), "nor was the workspace touched"
    fresh = capi.Context(capi.MODEL_GODDARD)
    assert fresh.has_sensitivity() and fresh.sensitivity_work_bytes(B, K) == 0
    assert raw(fresh, B, Z, dirs, out) == capi.ERR_ARG and "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    fresh.close()

    # models without the entry: the interceptor, vtolUAV, and a plugin whose traits are not generic in the parameter view
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    from test_gpu_cost_batch import build_vtol
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    Xs, Xf = scenario_state(gamma=1.49)
    iprob, iz = multi_shooting_problem(Oracle(MODEL_INTERCEPTOR), 4, X0=Xs, Xf=Xf)
    ci = capi.Context(capi.MODEL_INTERCEPTOR)
    assert ci.problem_set(iprob.mode_t, iprob.mode_x, iprob.time, iprob.xnode) == iprob.n
    assert not ci.has_sensitivity() and ci.L.socp_ctx_has_sensitivity(ci.h) == 0
    io = (sentinel(iprob.n), sentinel_i(1), sentinel(iprob.n))
    c0 = ci.counters()
    assert raw(ci, 1, np.ascontiguousarray(iz), [(DIR_PARAM, 0)], io) == capi.ERR_UNSUPPORTED
    assert "no sensitivity entry" in ci.L.socp_last_error(ci.h).decode() and ci.counters() == c0 and fresh_out(io)
    with pytest.raises(capi.SocpError):
        ci.sensitivity_batch(iz[None, :], [(DIR_PARAM, 0)])
    ci.close()
    cv, _, Zv, _ = build_vtol("exact")
    assert not cv.has_sensitivity()
    vo = (sentinel(len(Zv) * cv.n), sentinel_i(len(Zv)), sentinel(len(Zv) * cv.n))
    c0 = cv.counters()
    assert raw(cv, len(Zv), np.ascontiguousarray(Zv), [(DIR_PARAM, 0)], vo) == capi.ERR_UNSUPPORTED and fresh_out(vo) and cv.counters() == c0
    assert "no sensitivity entry" in cv.L.socp_last_error(cv.h).decode()
    cv.close()
    old = dict(sc.osc1d_plugin(), model="osc1d_exact_jacobian")
    co = context(old)
    assert co.has_exact_jacobian() and not co.has_sensitivity()
    oo = (sentinel(5 * 6), sentinel_i(5), sentinel(5 * 6))
    c0 = co.counters()
    assert raw(co, 5, np.ascontiguousarray(old["Z"]), [(DIR_PARAM, 0)], oo) == capi.ERR_UNSUPPORTED and fresh_out(oo) and co.counters() == c0
    assert "rebuild" in co.L.socp_last_error(co.h).decode()
    co.close()
    for model in (capi.MODEL_GODDARD, capi.MODEL_DOUBLE_INTEGRATOR, capi.MODEL_COVID19):
        for variant in (capi.VARIANT_LANE_EXACT, capi.VARIANT_LANE_FAST):
            cm = capi.Context(model)
            cm.set_variant(variant)
            assert cm.has_sensitivity()
            cm.close()

    # a valid call afterwards: the bits of the restatement
    check_whole(run_host(ctx, Z, dirs), reference("goddard_m3"), "after the refused calls")
    ctx.close()


# ---- 5. the sweep tool -------------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_sensitivity_file_and_record(tmp_path):
    out = str(tmp_path / "sens")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--sens-out", out, "--sens-param", "C"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["sensitivity"]
    assert {"rows", "refused", "dz_norm_median"} <= set(entry) and entry["parameter"] == "C"
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and sorted(npz.files) == ["dz", "g", "index", "info", "theta", "z"]
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0
    assert npz["dz"].shape == (k, 14) and npz["g"].shape == (k, 14) and npz["z"].shape == (k, 14) and npz["info"].shape == (k,) and npz["theta"].shape == (k,)
    assert entry["refused"] == int(np.sum(npz["info"] != 0)) and np.all(npz["theta"] == 3.5)
    assert entry["dz_norm_median"] > 0 and np.isfinite(npz["dz"][npz["info"] == 0]).all()
    print("sweep --sens-out, 64 starts: %s" % {q: entry[q] for q in ("rows", "refused", "dz_norm_median")})
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--sens-out", out], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode != 0 and "--sens-out" in bad.stderr
