"""GPU: the batched Jacobi-field test (socp_jacobi_batch[_dev] / _blocks, capi.Context.jacobi_batch) against
tests/jacobi_reference.py -- the definition restated in numpy on the CPU oracle's RK4 step (the example plugins: on their restated
right-hand sides).  Outputs live in sentinel-filled buffers followed by 64 guard words and are compared WHOLE on integer views
(the conventions of test_gpu_events_batch.py), so a store past a slab, past min(count, cap) or through a NULL Jend shows.
Reference-order flavour: every output bit-equal to the restatement; the one exception is the payload of a NaN that arithmetic
produced from a NaN input (the x86 and the gfx950 units pick different ones), so NaNs other than the sentinel are compared as NaN.
The inputs are tests/jacobi_cases.py.  The figures the tests print are kept in profiles/jacobi_gpu_tests.txt."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import jacobi_cases as jc
import jacobi_reference as jr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x7FF8DEADBEEF0001                       # a NaN no kernel produces
SENT_I = 0x5EADBEE1
QNAN = np.uint64(0x7FF8000000000000)
GUARD = 64
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
STRIDE, SKIP, CAP = 7, 2, 16
NAMES = ("tq", "det", "count", "nchange", "tconj", "Jend")


def sentinel(size):
    return np.full(size + GUARD, np.uint64(SENT), dtype=np.uint64).view(np.float64)


def sentinel_i(size):
    return np.full(size + GUARD, SENT_I, dtype=np.int32)


def plugin_path(name):
    path = os.path.join(ROOT, "socp_amd", "_build", "plugins", "lib%s_plugin.so" % name)
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def context(c, variant="exact"):
    """A context set to a case: model, parameters, step number, problem."""
    from socp_amd import capi
    if c["model"] in ("lqr1d", "osc1d"):
        capi.plugin_load(plugin_path(c["model"]))
        ctx = capi.Context({"lqr1d": 1001, "osc1d": 1002}[c["model"]], nparams=1)
    else:
        ctx = capi.Context({"goddard": capi.MODEL_GODDARD, "dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[c["model"]])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(c["params"])
    ctx.set_step_number(c["N"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


# ---- the three forms on guarded buffers: each returns the six WHOLE buffers as integer views ---------------------------------

def buffers(B, M, cap, d):
    return (sentinel(B * M * cap), sentinel(B * M * cap), sentinel_i(B * M), sentinel_i(B * M), sentinel(B * M), sentinel(B * M * d * d))


def views(bufs):
    return tuple(a.view(np.uint64) if a.dtype == np.float64 else a for a in bufs)


def run_host(ctx, Z, stride=STRIDE, skip=SKIP, cap=CAP, jend=True, blocks=None, epsfcn=0.0):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B = len(Z)
    out = buffers(B, ctx.M, cap, ctx.dim)
    tail = (epsfcn, stride, skip, cap, out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP), out[2].ctypes.data_as(IP), out[3].ctypes.data_as(IP),
            out[4].ctypes.data_as(DP), out[5].ctypes.data_as(DP) if jend else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_jacobi_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in blocks)
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None        # noqa: E731
        ctx._chk(ctx.L.socp_jacobi_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx), *tail))
    return views(out)


def run_dev(ctx, Z, stride=STRIDE, skip=SKIP, cap=CAP, jend=True, epsfcn=0.0):
    import torch
    B = len(Z)
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in buffers(B, ctx.M, cap, ctx.dim)]
    torch.cuda.synchronize()
    ctx.jacobi_batch_dev(B, dZ.data_ptr(), epsfcn, stride, skip, cap, *(t.data_ptr() for t in dev[:5]), dev[5].data_ptr() if jend else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    return views(tuple(t.cpu().numpy() for t in dev))


def expected(c, slabs, cap=CAP, jend=True):
    return jr.pack(slabs, len(slabs), c["prob"].M, c["prob"].dim, cap, SENT, SENT_I, jend=jend)


def canon(a):
    """NaNs other than the sentinel -> one quiet NaN."""
    if a.dtype != np.uint64:
        return a
    a = a.copy()
    a[np.isnan(a.view(np.float64)) & (a != np.uint64(SENT))] = QNAN
    return a


def check_whole(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        fill = np.uint64(SENT) if g.dtype == np.uint64 else SENT_I
        if w is None:
            assert np.all(g == fill), "%s: %s was written although its pointer was NULL" % (what, name)
            continue
        w = np.ascontiguousarray(w).ravel()
        assert np.all(g[w.size:] == fill), "%s: guard words behind %s were written" % (what, name)
        gg, ww = canon(g[:w.size]), canon(w)
        bad = np.argwhere(gg != ww).ravel()
        shown = (gg[bad[:5]].view(np.float64), ww[bad[:5]].view(np.float64)) if gg.dtype == np.uint64 else (gg[bad[:5]], ww[bad[:5]])
        assert len(bad) == 0, (what, name, "%d differ; first flat indices:" % len(bad), bad[:5].tolist(), *shown)


def coverage(slabs):
    flat = [s for row in slabs for s in row]
    return sum(sum(s["swaps"]) for s in flat), sum(1 for s in flat if s["nchange"] >= 1), sum(1 for s in flat if s["nchange"] == 0)


# ---- 1. reference-order flavour, bit for bit, six models ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard_single", "goddard_m3_free_tf", "dint", "covid", "lqr1d", "osc1d"])
def test_exact_flavour_equals_the_restatement(name):
    c = jc.case(name)
    D, M, B = c["prob"].dim, c["prob"].M, len(c["Z"])
    gpw = 64 // (D + 1)
    assert B * M > gpw and (B * M) % gpw != 0, "more than one wavefront, the last one partly filled"
    ctx = context(c)
    assert ctx.has_jacobi()
    for skip in (SKIP, 0):
        slabs = jc.reference(name, skip=skip)
        swaps, with_change, without = coverage(slabs)
        print("%s skip %d: %d slabs, %d row swaps, %d slabs with a change, %d without" % (name, skip, B * M, swaps, with_change, without))
        assert all(s["count"] == 9 for row in slabs for s in row), "60 steps at stride 7: eight samples on the stride and the last"
        if D >= 2:
            assert swaps >= 1, "the batch has a sample with a row swap"
        if name in ("goddard_single", "goddard_m3_free_tf", "covid"):
            assert with_change >= 1 and without >= 1, "slabs with and without a sign change"
        if name == "osc1d":
            assert without == 0, "the certain sign change"
        want = expected(c, slabs)
        check_whole(run_host(ctx, c["Z"], skip=skip), want, "%s skip %d, host form" % (name, skip))
        check_whole(run_dev(ctx, c["Z"], skip=skip), want, "%s skip %d, _dev form" % (name, skip))
    check_whole(run_dev(ctx, c["Z"], jend=False), expected(c, jc.reference(name), jend=False), name + ", NULL Jend")
    ctx.close()


def test_python_form_returns_device_tensors():
    import torch
    c = jc.case("covid")
    ctx = context(c)
    r = ctx.jacobi_batch(c["Z"], stride=STRIDE, skip=SKIP, cap=4, jend=True)        # cap 4 < 9: the call is repeated with cap 9
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in r.values()) and r["det"].shape == (7, 4, 9)
    want = expected(c, jc.reference("covid"), cap=9)
    for key, w in zip(("tq", "det", "count", "nchange", "tconj", "jend"), want):
        g = r[key].cpu().numpy()
        assert np.array_equal(canon(g.view(np.uint64)) if g.dtype == np.float64 else g, canon(w)), key
    ctx.close()


# ---- 2. overflow ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard_m3_free_tf", "osc1d"])
def test_cap_below_count_counts_all_stores_cap_and_detects_on_all(name):
    c = jc.case(name)
    ctx = context(c)
    slabs = jc.reference(name)
    want = expected(c, slabs, cap=2)
    assert want[2].min() == 9 and want[3].max() >= 1, "nine samples, two stored; with skip = 2 every change lies beyond the stored ones"
    check_whole(run_host(ctx, c["Z"], cap=2), want, name + " cap = 2, host form")
    check_whole(run_dev(ctx, c["Z"], cap=2), want, name + " cap = 2, _dev form")
    ctx.close()


# ---- 3. per-row blocks ---------------------------------------------------------------------------------------------------------

def test_blocks_form_equals_row_by_row_calls():
    from oracle.oracle import Problem
    c = jc.case("goddard_single")
    B, prob = len(c["Z"]), c["prob"]
    params = np.tile(np.concatenate([c["params"], [0.0, 0.0]]), (B, 1))
    params[:, 2] = np.linspace(250.0, 330.0, B)                           # KD
    time = np.tile(prob.time, (B, 1))
    time[:, 1] = np.linspace(0.05, 0.25, B)                               # the final time
    ctx = context(c)
    plain = run_host(ctx, c["Z"])
    got = run_host(ctx, c["Z"], blocks=(params, time, None))
    want = expected(c, jc.reference_of(c, blocks=(params, time, None)))
    check_whole(got, want, "_blocks form against the restatement")
    assert not np.array_equal(got[1], plain[1])
    again = run_host(ctx, c["Z"])
    assert all(np.array_equal(a, b) for a, b in zip(plain, again)), "the context's own blocks are back"
    # row by row: a context set to row b's KD and final time, one row
    for b in (0, 4, B - 1):
        one = dict(c, params=params[b, :8], prob=Problem(7, prob.mode_t, prob.mode_x, time[b], prob.xnode))
        cb = context(one)
        row = run_host(cb, c["Z"][b:b + 1])
        cb.close()
        for name, g, r, per in zip(NAMES, got, row, (CAP, CAP, 1, 1, 1, 49)):
            assert np.array_equal(canon(g[b * per:(b + 1) * per]), canon(r[:per])), (b, name)
    # the Python form with blocks
    r = ctx.jacobi_batch(c["Z"], stride=STRIDE, skip=SKIP, cap=CAP, jend=True, blocks=(params, time, None))
    filled = canon(want[1]).ravel()
    filled[filled == np.uint64(SENT)] = QNAN                                 # the Python form hands NaN-filled buffers in
    assert np.array_equal(canon(r["det"].cpu().numpy().view(np.uint64)).ravel(), filled)
    again = run_host(ctx, c["Z"])
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    ctx.close()


# ---- 4. a zero-length segment and a NaN costate ------------------------------------------------------------------------------------

def test_zero_length_segment_and_nan_costate():
    c = jc.case("goddard_degenerate")
    ctx = context(c)
    slabs = jc.reference("goddard_degenerate")
    for b in range(3):
        s = slabs[b][1]
        assert s["count"] == 0 and s["nchange"] == 0 and math.isnan(s["tconj"]) and np.all(s["jend"] == 0.0) and not np.any(np.signbit(s["jend"]))
    assert all(math.isnan(d) for d in slabs[1][0]["det"]) and slabs[1][0]["nchange"] == 0 and slabs[1][0]["count"] == 9
    want = expected(c, slabs)
    got = run_host(ctx, c["Z"])
    check_whole(got, want, "degenerate, host form")
    check_whole(run_dev(ctx, c["Z"]), want, "degenerate, _dev form")
    # the neighbours in the same wavefront: what they give when the NaN row is a clean one
    Z = np.array(c["Z"])
    Z[1] = Z[0]
    clean = run_host(ctx, Z)
    for name, g, k, per in zip(NAMES, got, clean, (3 * CAP, 3 * CAP, 3, 3, 3, 3 * 49)):
        for b in (0, 2):
            assert np.array_equal(g[b * per:(b + 1) * per], k[b * per:(b + 1) * per]), (name, b)
    ctx.close()


# ---- 5. throughput flavour -------------------------------------------------------------------------------------------------------

def test_fast_flavour_closed_forms():
    from test_jacobi_cpu import OSC, LQR, osc_bound, lqr_bound
    c = jc.osc1d(N=OSC["N"], w=OSC["w"], Z=OSC["X0"], T=OSC["T"])
    ctx = context(c, "fast")
    got = run_dev(ctx, c["Z"], stride=1, skip=0, cap=4)
    tconj = float(got[4][:1].view(np.float64)[0])
    print("osc1d fast: tconj - pi/2 = %.3e (bound %.3e)" % (tconj - math.pi / 2, osc_bound(math.pi / 2)))
    assert got[2][0] == OSC["N"] and got[3][0] == 2 and abs(tconj - math.pi / 2) <= osc_bound(math.pi / 2)
    ctx.close()
    c0 = jc.osc1d(N=OSC["N"], w=0.0, Z=OSC["X0"], T=OSC["T"])
    ctx = context(c0, "fast")
    got = run_dev(ctx, c0["Z"], stride=1, skip=0, cap=4)
    assert got[3][0] == 0 and math.isnan(float(got[4][:1].view(np.float64)[0]))
    ctx.close()
    c = jc.lqr1d(N=LQR["N"], Z=LQR["X0"], T=LQR["T"])
    ctx = context(c, "fast")
    got = run_dev(ctx, c["Z"], stride=1, skip=LQR["skip"], cap=LQR["N"])
    tq, det = got[0][:LQR["N"]].view(np.float64), got[1][:LQR["N"]].view(np.float64)
    assert got[2][0] == LQR["N"] and got[3][0] == 0
    worst = 0.0
    for j in range(LQR["skip"], LQR["N"]):
        want = LQR["g"] ** 2 * tq[j] ** 4 / 12.0
        assert abs(det[j] - want) <= lqr_bound(tq[j], j + 1) < want, j
        worst = max(worst, abs(det[j] - want) / lqr_bound(tq[j], j + 1))
    print("lqr1d fast: largest |det - g^2 t^4 / 12| / bound = %.3e" % worst)
    ctx.close()


def test_fast_flavour_goddard_within_the_step_size_uncertainty():
    """count and tq equal the reference order's; |det_fast - det_ref| <= 10 x |det_ref(epsfcn = 0) - det_ref(epsfcn = 4 DBL_EPSILON)|,
    both as the largest over a slab relative to the slab's largest |det|.  Measured largest ratio of the two sides: see
    profiles/jacobi_gpu_tests.txt."""
    name = "goddard_single"
    c = jc.case(name)
    ref0, ref4 = jc.reference(name), jc.reference(name, epsfcn=4.0 * jr.DBL_EPSILON)
    ctx = context(c, "fast")
    got = run_dev(ctx, c["Z"])
    ctx.close()
    B = len(c["Z"])
    want = expected(c, ref0)
    assert np.array_equal(got[2][:B], want[2].ravel()) and np.array_equal(got[0][:B * CAP], want[0].ravel()), "count and tq are the reference order's"
    assert all(np.all(g[n:] == (np.uint64(SENT) if g.dtype == np.uint64 else SENT_I)) for g, n in zip(got, (B * CAP, B * CAP, B, B, B, B * 49)))
    det = got[1][:B * CAP].view(np.float64).reshape(B, CAP)
    worst = 0.0
    for b in range(B):
        d0, d4 = np.array(ref0[b][0]["det"]), np.array(ref4[b][0]["det"])
        scale = np.max(np.abs(d0))
        moved = np.max(np.abs(d4 - d0)) / scale
        dev = np.max(np.abs(det[b, :9] - d0)) / scale
        print("goddard fast row %d: deviation %.3e, the restatement's own movement %.3e, ratio %.3e" % (b, dev, moved, dev / moved))
        worst = max(worst, dev / moved)
    print("goddard fast: largest ratio %.3e (bound 10)" % worst)
    assert worst <= 10.0


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------

def raw(ctx, B, Z, stride, skip, cap, out, form="host", epsfcn=0.0):
    fn = ctx.L.socp_jacobi_batch if form == "host" else ctx.L.socp_jacobi_batch_dev
    ptr = (lambda a, T: a.ctypes.data_as(T) if a is not None else None) if form == "host" else (lambda a, T: a.ctypes.data if a is not None else None)
    return fn(ctx.h, B, ptr(Z, DP), epsfcn, stride, skip, cap, ptr(out[0], DP), ptr(out[1], DP), ptr(out[2], IP), ptr(out[3], IP), ptr(out[4], DP),
              ptr(out[5], DP))


def test_errors_leave_the_context_unchanged_and_counters():
    from socp_amd import capi
    name = "goddard_m3_free_tf"
    c = jc.case(name)
    ctx = context(c)
    Z = np.ascontiguousarray(c["Z"])
    B, M, D = len(Z), ctx.M, ctx.dim
    out = buffers(B, M, CAP, D)
    fresh_out = lambda: all(np.all(v == (np.uint64(SENT) if v.dtype == np.uint64 else SENT_I)) for v in views(out))      # noqa: E731
    L, h = ctx.L, ctx.h
    t0, l0 = ctx.counters()
    tl0 = ctx.timeline(Z[0]).copy()
    for stride, skip, cap, what in ((0, 2, 4, "stride = 0"), (7, -1, 4, "skip = -1"), (7, 2, 0, "cap = 0")):
        for form in ("host", "dev"):
            assert raw(ctx, B, Z, stride, skip, cap, out, form) == capi.ERR_ARG, what
            assert what.split()[0] in L.socp_last_error(h).decode()
    assert raw(ctx, -1, Z, 7, 2, 4, out) == capi.ERR_ARG
    assert raw(ctx, B, None, 7, 2, 4, out) == capi.ERR_ARG
    for k in range(5):
        holed = tuple(None if j == k else a for j, a in enumerate(out))
        assert raw(ctx, B, Z, 7, 2, 4, holed) == capi.ERR_ARG and raw(ctx, B, Z, 7, 2, 4, holed, "dev") == capi.ERR_ARG, NAMES[k]
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for pstride in (8, 9, 11):
        assert L.socp_jacobi_batch_blocks(h, B, Z.ctypes.data_as(DP), params.ctypes.data_as(DP), pstride, None, None, 0.0, 7, 2, 4,
                                          out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP), out[2].ctypes.data_as(IP), out[3].ctypes.data_as(IP),
                                          out[4].ctypes.data_as(DP), None) == capi.ERR_ARG, pstride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    # B = 0: SOCP_OK and no launch
    assert raw(ctx, 0, None, 7, 2, 4, (None,) * 6) == capi.OK and raw(ctx, 0, None, 7, 2, 4, (None,) * 6, "dev") == capi.OK
    # the adaptive integrator
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    for form in ("host", "dev"):
        assert raw(ctx, B, Z, 7, 2, 4, out, form) == capi.ERR_UNSUPPORTED and "DOPRI5" in L.socp_last_error(h).decode()
    ctx.set_integrator(capi.INT_RK4)
    assert ctx.counters() == (t0, l0), "nothing was launched or counted"
    assert fresh_out(), "nothing was written"
    assert np.array_equal(ctx.timeline(Z[0]), tl0)

    fresh = capi.Context(capi.MODEL_GODDARD)
    assert fresh.has_jacobi()
    assert raw(fresh, B, Z, 7, 2, 4, out) == capi.ERR_ARG and "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    fresh.close()

    # models without the entry: the interceptor (its own ComputeTraj) and vtolUAV (not offered)
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    from test_gpu_cost_batch import build_vtol
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    Xs, Xf = scenario_state(gamma=1.49)
    iprob, iz = multi_shooting_problem(Oracle(MODEL_INTERCEPTOR), 4, X0=Xs, Xf=Xf)
    for variant in (capi.VARIANT_LANE_EXACT, capi.VARIANT_LANE_FAST):
        ci = capi.Context(capi.MODEL_INTERCEPTOR)
        ci.set_variant(variant)
        assert ci.problem_set(iprob.mode_t, iprob.mode_x, iprob.time, iprob.xnode) == iprob.n
        assert not ci.has_jacobi() and ci.L.socp_ctx_has_jacobi(ci.h) == 0
        c0 = ci.counters()
        io = buffers(1, 4, 4, 6)
        assert raw(ci, 1, np.ascontiguousarray(iz), 7, 2, 4, io) == capi.ERR_UNSUPPORTED
        assert "no jacobi entry" in ci.L.socp_last_error(ci.h).decode() and ci.counters() == c0
        with pytest.raises(capi.SocpError):
            ci.jacobi_batch(iz[None, :])
        ci.close()
        cv, _, Zv, _ = build_vtol("fast" if variant == capi.VARIANT_LANE_FAST else "exact")
        assert not cv.has_jacobi()
        c0 = cv.counters()
        vo = buffers(len(Zv), cv.M, 4, 6)
        assert raw(cv, len(Zv), np.ascontiguousarray(Zv), 7, 2, 4, vo) == capi.ERR_UNSUPPORTED
        assert "no jacobi entry" in cv.L.socp_last_error(cv.h).decode() and cv.counters() == c0
        cv.close()

    # a valid call afterwards reproduces test 1's bits; the counters advance by B M (d + 1) trajectories and ONE launch
    want = expected(c, jc.reference(name))
    check_whole(run_host(ctx, Z), want, "after the refused calls")
    t1, l1 = ctx.counters()
    assert t1 - t0 == B * M * (D + 1) and l1 - l0 == 1
    check_whole(run_dev(ctx, Z, jend=False), want[:5] + (None,), "_dev form afterwards")
    t2, l2 = ctx.counters()
    assert t2 - t1 == B * M * (D + 1) and l2 - l1 == 1
    ctx.close()


# ---- 7. the sweep tool -----------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_jacobi_file_and_record(tmp_path):
    out = str(tmp_path / "jac")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "100", "--jacobi-out", out, "--jacobi-stride", "10",
                          "--jacobi-skip", "2"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["jacobi"]
    assert {"rows", "with_change", "tconj_min", "tconj_median"} <= set(entry)
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and sorted(npz.files) == sorted(["index", "tq", "det", "count", "nchange", "tconj"])
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0
    assert npz["det"].shape[:2] == (k, 1) and np.all(npz["count"] == 10) and npz["tconj"].shape == (k, 1)
    changed = npz["nchange"].sum(axis=1) > 0
    assert entry["with_change"] == int(changed.sum())
    if changed.any():
        assert entry["tconj_min"] == float(np.nanmin(npz["tconj"][changed])) and entry["tconj_min"] <= entry["tconj_median"]
    else:
        assert entry["tconj_min"] is None and entry["tconj_median"] is None
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--jacobi-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--jacobi-out" in bad.stderr
