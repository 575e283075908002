"""GPU: the batched exact fields (socp_fields_batch[_dev] / _blocks, capi.Context.fields_batch) against tests/fields_reference.py --
the definition restated in Python on dual numbers.  Outputs live in sentinel-filled buffers followed by 64 guard words and are
compared WHOLE on integer views (the conventions of test_gpu_jacobi_batch.py), so a store past a slab, past min(count, cap) or
through a NULL Phi shows.  Every output is bit-equal to the restatement, in BOTH flavours (the kernels are one object without
contraction); the one exception is the payload of a NaN that arithmetic produced from a NaN input, so NaNs other than the sentinel
are compared as NaN.  N = 50 steps at stride 7: seven samples on the stride and the k == K one.  A reference is computed once
(all s columns; the costate columns are its last d, the other skip is DETECTION alone) and shared read-only.
The figures the tests print are kept in profiles/fields_gpu_tests.txt."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import fields_reference as fr
import jacobi_cases as jc
from test_gpu_jacobi_batch import SENT, SENT_I, QNAN, GUARD, DP, IP, sentinel, sentinel_i, views, canon, plugin_path   # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE, SKIP, CAP, N = 7, 2, 16, 50
NAMES = ("tq", "det", "count", "nchange", "tconj", "Phi")
PLUGIN_IDS = {"lqr1d": 1001, "osc1d": 1002, "osc1d_fields": 1004}


def context(c, variant="exact"):
    from socp_amd import capi
    if c["model"] in PLUGIN_IDS:
        capi.plugin_load(plugin_path(c["model"]))
        ctx = capi.Context(PLUGIN_IDS[c["model"]], nparams=1)
    else:
        ctx = capi.Context({"goddard": capi.MODEL_GODDARD, "dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[c["model"]])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(c["params"])
    ctx.set_step_number(c["N"])
    if c.get("sw") is not None:
        ctx.set_switching_times(c["sw"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def goddard_single():
    """Single shooting, smooth law, 9 rows (cols = ALL: 4 groups per wave, three waves, the last with one group), row 4 with a NaN."""
    c = dict(jc.goddard_single(), N=N)
    c["o"] = jc.goddard_oracle(N)
    Z = np.array(c["Z"])
    Z[4, 9] = np.nan
    return dict(c, Z=Z)


def goddard_general():
    """mu2 = 0: full thrust up to sw0 = 0.05, the closed-form singular control up to sw1 = 0.15, then off; 3 rows."""
    c = dict(jc.goddard_single(), N=N, sw=(0.05, 0.15))
    o = jc.goddard_oracle(N)
    o.set_param("mu2", 0.0)
    o.set_switching([0.05, 0.15])
    assert o.params()[7] < 0
    return dict(c, o=o, params=o.params()[:8], Z=np.array(c["Z"][:3]))


def goddard_m3():
    """M = 3 with FIXED interior times and a FREE final time, 5 rows."""
    from oracle.oracle import Problem, FIXED, FREE
    c = dict(jc.goddard_m3(B=5, seed=9), N=N)
    p = c["prob"]
    return dict(c, o=jc.goddard_oracle(N), prob=Problem(7, [FIXED, FIXED, FIXED, FREE], p.mode_x, p.time, p.xnode))


def dint_m2():
    """M = 2, fixed times; the costates of node 1 saturate the control in segment 1, segment 0 stays unsaturated; 3 rows."""
    from oracle.oracle import Oracle, Problem, MODEL_DINT, FIXED
    o = Oracle(MODEL_DINT, step_nbr=N)
    X = np.zeros((3, 12))
    n0 = np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.1, 0.02, -0.01, 0.015, 0.4, -0.3, 0.2])
    n1 = np.array([0.5, -0.3, 0.2, 0.1, 0.1, -0.2, 0.02, -0.01, 0.015, 2.0, -1.5, 1.0])
    Z = np.tile(np.concatenate([n0, n1]), (3, 1)) * (1.0 + 0.05 * np.random.default_rng(3).uniform(-1.0, 1.0, size=(3, 24)))
    prob = Problem(6, [FIXED, FIXED, FIXED], np.zeros((3, 6), dtype=np.int32), np.array([0.0, 1.5, 3.0]), X)
    return dict(model="dint", o=o, prob=prob, N=N, Z=Z, params=o.params()[:3])


def covid_m2():
    """M = 2, fixed times; node 0 with the control on its upper bound, node 1 with I >= Imax (the penalty); 3 rows."""
    from oracle.oracle import Oracle, Problem, MODEL_COVID, FIXED
    o = Oracle(MODEL_COVID, step_nbr=N)
    n0 = np.array([0.9, 0.01, 0.05, 0.04, -1500.0, 300.0, 0.5, 0.1])     # u = (pE - pS) S I / Tinf / N R0 = 32.4 >= umax = 20
    n1 = np.array([0.6, 0.05, 0.2, 0.15, -0.5, 0.8, 0.3, 0.1])           # I = 0.2 >= Imax = 0.1
    Z = np.tile(np.concatenate([n0, n1]), (3, 1)) * (1.0 + 0.02 * np.random.default_rng(4).uniform(-1.0, 1.0, size=(3, 16)))
    prob = Problem(4, [FIXED, FIXED, FIXED], np.zeros((3, 4), dtype=np.int32), np.array([0.0, 5.0, 10.0]), np.zeros((3, 8)))
    return dict(model="covid", o=o, prob=prob, N=N, Z=Z, params=o.params()[:8])


def osc1d_fields():
    """tests/plugin/osc1d_fields_plugin.hip over [0, 4], w = 4: conjugate times k pi / 2, the certain sign change; 5 rows."""
    return dict(jc.osc1d(N=N, Z=np.random.default_rng(4).uniform(0.2, 1.0, size=(5, 2))), model="osc1d_fields")


CASES = {"goddard_single": goddard_single, "goddard_general": goddard_general, "goddard_m3": goddard_m3, "dint_m2": dint_m2,
         "covid_m2": covid_m2, "osc1d_fields": osc1d_fields}
_CASE, _REF = {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = CASES[name]()
        _CASE[name]["Z"].setflags(write=False)
    return _CASE[name]


def reference_of(c, blocks=None, rows=None):
    """slabs[b][i] with cols = ALL, skip = 0 for the rows of a case (blocks = (params, time, xnode), any of them None)."""
    from oracle.oracle import Problem
    prob, D = c["prob"], c["prob"].dim
    pp, tt, xx = blocks if blocks is not None else (None, None, None)
    model = "osc1d" if c["model"] == "osc1d_fields" else c["model"]
    sw = c.get("sw") or (0.0, 0.0)
    out = []
    for b in (range(len(c["Z"])) if rows is None else rows):
        z = c["Z"][b]
        pb = Problem(D, prob.mode_t, prob.mode_x, prob.time if tt is None else tt[b], prob.xnode if xx is None else xx[b])
        P = [float(v) for v in (c["params"] if pp is None else pp[b][:len(c["params"])])]
        tl = jc.timeline(c, pb, z)
        out.append([fr.fields_segment(model, P, sw, D, float(tl[i]), float(tl[i + 1]), z[2 * D * i:2 * D * (i + 1)], c["N"], cols=fr.ALL,
                                      stride=STRIDE, skip=0) for i in range(prob.M)])
    return out


def reference(name):
    if name not in _REF:
        _REF[name] = reference_of(case(name))
    return _REF[name]


def shaped(slabs, cols, skip):
    D = len(slabs[0][0]["phi"]) // 2
    return [[fr.with_skip(s if cols == fr.ALL else fr.costate_columns(s, D), skip) for s in row] for row in slabs]


def expected(c, slabs, cols, skip=SKIP, cap=CAP, phi=True):
    return fr.pack(shaped(slabs, cols, skip), len(slabs), c["prob"].M, c["prob"].dim, cap, SENT, SENT_I, cols=cols, phi=phi)


# ---- the three forms on guarded buffers: each returns the six WHOLE buffers as integer views ---------------------------------

def buffers(B, M, cap, d, cols):
    return (sentinel(B * M * cap), sentinel(B * M * cap), sentinel_i(B * M), sentinel_i(B * M), sentinel(B * M),
            sentinel(B * M * 2 * d * (2 * d if cols else d)))


def run_host(ctx, Z, cols, stride=STRIDE, skip=SKIP, cap=CAP, phi=True, blocks=None):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B = len(Z)
    out = buffers(B, ctx.M, cap, ctx.dim, cols)
    tail = (cols, stride, skip, cap, out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP), out[2].ctypes.data_as(IP), out[3].ctypes.data_as(IP),
            out[4].ctypes.data_as(DP), out[5].ctypes.data_as(DP) if phi else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_fields_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in blocks)
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None        # noqa: E731
        ctx._chk(ctx.L.socp_fields_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx), *tail))
    return views(out)


def run_dev(ctx, Z, cols, stride=STRIDE, skip=SKIP, cap=CAP, phi=True):
    import torch
    B = len(Z)
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in buffers(B, ctx.M, cap, ctx.dim, cols)]
    torch.cuda.synchronize()
    ctx.fields_batch_dev(B, dZ.data_ptr(), cols, stride, skip, cap, *(t.data_ptr() for t in dev[:5]), dev[5].data_ptr() if phi else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    return views(tuple(t.cpu().numpy() for t in dev))


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


# ---- 1. Goddard, single shooting, smooth law: every form and option, bit for bit ---------------------------------------------

@pytest.mark.parametrize("cols", [fr.COSTATE, fr.ALL])
def test_goddard_single_equals_the_restatement(cols):
    c = case("goddard_single")
    slabs = reference("goddard_single")
    assert all(s["count"] == 8 for row in slabs for s in row), "50 steps at stride 7: seven samples on the stride and the k == K one"
    assert all(math.isnan(d) for d in slabs[4][0]["det"]) and slabs[4][0]["nchange"] == 0, "the NaN row"
    ctx = context(c)
    assert ctx.has_fields()
    t0, l0 = ctx.counters()
    for skip in (SKIP, 0):
        want = expected(c, slabs, cols, skip=skip)
        check_whole(run_host(ctx, c["Z"], cols, skip=skip), want, "cols %d skip %d, host form" % (cols, skip))
        check_whole(run_dev(ctx, c["Z"], cols, skip=skip), want, "cols %d skip %d, _dev form" % (cols, skip))
    t1, l1 = ctx.counters()
    B, Ccols = len(c["Z"]), (14 if cols else 7)
    assert t1 - t0 == 4 * B * 1 * Ccols and l1 - l0 == 4, "B M C trajectories and one launch per call"
    check_whole(run_dev(ctx, c["Z"], cols, phi=False), expected(c, slabs, cols, phi=False), "NULL Phi")
    want2 = expected(c, slabs, cols, cap=2)
    assert want2[2].min() == 8, "eight samples, two stored"
    check_whole(run_host(ctx, c["Z"], cols, cap=2), want2, "cap = 2, host form")
    check_whole(run_dev(ctx, c["Z"], cols, cap=2), want2, "cap = 2, _dev form")
    print("goddard_single cols %d: det of the last sample, row 0: %.11e; slabs with a change (skip %d): %d of %d"
          % (cols, slabs[0][0]["det"][-1], SKIP, int((want2[3] > 0).sum()), B))
    ctx.close()


def test_python_form_repeats_with_the_largest_count():
    import torch
    c = case("goddard_single")
    ctx = context(c)
    r = ctx.fields_batch(c["Z"], cols=fr.ALL, stride=STRIDE, skip=SKIP, cap=4, phi=True)        # cap 4 < 8: repeated with cap 8
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in r.values()) and r["det"].shape == (9, 1, 8) and r["phi"].shape == (9, 1, 14, 14)
    want = expected(c, reference("goddard_single"), fr.ALL, cap=8)
    for key, w in zip(("tq", "det", "count", "nchange", "tconj", "phi"), want):
        g = r[key].cpu().numpy()
        assert np.array_equal(canon(g.view(np.uint64)) if g.dtype == np.float64 else g, canon(w)), key
    assert np.array_equal(canon(r["jend"].contiguous().cpu().numpy().view(np.uint64)), canon(want[5][:, :, :7, 7:])), "jend: x-rows of the costate columns"
    rc = ctx.fields_batch(c["Z"], cols=fr.COSTATE, stride=STRIDE, skip=SKIP, phi=True)
    assert np.array_equal(canon(rc["jend"].contiguous().cpu().numpy().view(np.uint64)), canon(want[5][:, :, :7, 7:]))
    ctx.close()


# ---- 2. the general law -------------------------------------------------------------------------------------------------------

def test_goddard_general_law_with_the_singular_arc():
    c = case("goddard_general")
    slabs = reference("goddard_general")
    ctx = context(c)
    for cols in (fr.COSTATE, fr.ALL):
        want = expected(c, slabs, cols)
        check_whole(run_host(ctx, c["Z"], cols), want, "general law cols %d, host form" % cols)
        check_whole(run_dev(ctx, c["Z"], cols), want, "general law cols %d, _dev form" % cols)
    # the smooth law on the same rows gives other fields: the launch took the general-law kernel
    smooth = reference_of(dict(case("goddard_single"), Z=c["Z"]), rows=[0])
    assert not np.array_equal(smooth[0][0]["phi"], slabs[0][0]["phi"])
    ctx.close()


# ---- 3. M = 3 with a free final time, per-row blocks --------------------------------------------------------------------------

def test_goddard_m3_free_tf_and_per_row_blocks():
    from oracle.oracle import Problem
    c = case("goddard_m3")
    B, prob = len(c["Z"]), c["prob"]
    ctx = context(c)
    plain_want = expected(c, reference("goddard_m3"), fr.ALL)
    plain = run_host(ctx, c["Z"], fr.ALL)
    check_whole(plain, plain_want, "M = 3, free tf")
    params = np.tile(np.concatenate([c["params"], [0.0, 0.0]]), (B, 1))
    params[:, 2] = np.linspace(250.0, 330.0, B)                           # KD
    params[:, 6] = np.linspace(0.5, 1.5, B)                               # mu2 > 0 in every row
    time = np.tile(prob.time, (B, 1))
    time[:, 1] = np.linspace(0.02, 0.04, B)
    time[:, 2] = np.linspace(0.05, 0.07, B)
    time[3, 2] = time[3, 1]                                               # row 3: segment 1 has no length
    slabs = reference_of(c, blocks=(params, time, None))
    z3 = slabs[3][1]
    assert z3["count"] == 0 and z3["nchange"] == 0 and math.isnan(z3["tconj"]) and np.array_equal(z3["phi"], np.eye(14))
    for cols in (fr.ALL, fr.COSTATE):
        got = run_host(ctx, c["Z"], cols, blocks=(params, time, None))
        check_whole(got, expected(c, slabs, cols), "_blocks form, cols %d" % cols)
    assert not np.array_equal(got[1], run_host(ctx, c["Z"], fr.COSTATE)[1])
    again = run_host(ctx, c["Z"], fr.ALL)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again)), "the context's own blocks are back"
    # each row equals the row run alone on a context set to its parameters and times
    got = run_host(ctx, c["Z"], fr.ALL, blocks=(params, time, None))
    for b in (0, 3, B - 1):
        one = dict(c, params=params[b, :8], prob=Problem(7, prob.mode_t, prob.mode_x, time[b], prob.xnode))
        cb = context(one)
        row = run_host(cb, c["Z"][b:b + 1], fr.ALL)
        cb.close()
        for name, g, r, per in zip(NAMES, got, row, (3 * CAP, 3 * CAP, 3, 3, 3, 3 * 196)):
            assert np.array_equal(canon(g[b * per:(b + 1) * per]), canon(r[:per])), (b, name)
    ctx.close()


# ---- 4. the other models ------------------------------------------------------------------------------------------------------

def start_margins(c, b, i):
    """The decisions of the right-hand side at the start of segment i of row b."""
    D = c["prob"].dim
    K = fr.PlainKit()
    fr.rhs_on(fr.RHS[c["model"]], K, [float(p) for p in c["params"]], [0.0, 0.0], 0.0, [float(x) for x in c["Z"][b][2 * D * i:2 * D * (i + 1)]])
    return K.margins


@pytest.mark.parametrize("name", ["dint_m2", "covid_m2", "osc1d_fields"])
def test_other_models_equal_the_restatement(name):
    c = case(name)
    slabs = reference(name)
    if name == "dint_m2":
        assert start_margins(c, 0, 0)["|u|-umax"] < 0 < start_margins(c, 0, 1)["|u|-umax"], "segment 1 saturates, segment 0 does not"
    if name == "covid_m2":
        assert start_margins(c, 0, 0)["u-umax"] >= 0 and start_margins(c, 0, 1)["I-Imax"] >= 0, "a clamp and the penalty are active"
    if name == "osc1d_fields":
        assert all(s["nchange"] >= 1 for row in slabs for s in row), "the certain sign change"
        first = slabs[0][0]["tconj"]
        print("osc1d_fields: first conjugate time %.6f (pi / 2 = %.6f, samples %.2f apart)" % (first, math.pi / 2, 7 * 4.0 / N))
        assert abs(first - math.pi / 2) <= 7 * 4.0 / N
    ctx = context(c)
    assert ctx.has_fields()
    for cols in (fr.COSTATE, fr.ALL):
        for skip in (0, SKIP):
            want = expected(c, slabs, cols, skip=skip)
            check_whole(run_host(ctx, c["Z"], cols, skip=skip), want, "%s cols %d skip %d, host form" % (name, cols, skip))
            check_whole(run_dev(ctx, c["Z"], cols, skip=skip), want, "%s cols %d skip %d, _dev form" % (name, cols, skip))
    ctx.close()


# ---- 5. invariants ---------------------------------------------------------------------------------------------------------------

def test_rebatching_leaves_every_row_its_values():
    """The value trajectory and the fields of a row do not depend on its neighbours in the wavefront, nor on cols or Phi."""
    c = case("goddard_single")
    ctx = context(c)
    whole = run_dev(ctx, c["Z"], fr.ALL)
    order = [8, 2, 6, 0]
    part = run_dev(ctx, c["Z"][order], fr.COSTATE, phi=False)
    for k, b in enumerate(order):
        for j, per in ((0, CAP), (1, CAP), (2, 1), (3, 1), (4, 1)):
            assert np.array_equal(canon(whole[j][b * per:(b + 1) * per]), canon(part[j][k * per:(k + 1) * per])), (b, NAMES[j])
    ctx.close()


@pytest.mark.parametrize("name", ["goddard_single", "goddard_general", "covid_m2"])
def test_throughput_flavour_returns_the_same_bits(name):
    c = case(name)
    ctx = context(c, "fast")
    assert ctx.has_fields()
    for cols in (fr.COSTATE, fr.ALL):
        check_whole(run_dev(ctx, c["Z"], cols), expected(c, reference(name), cols), "%s, throughput flavour, cols %d" % (name, cols))
    ctx.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

def raw(ctx, B, Z, cols, stride, skip, cap, out, form="host"):
    fn = ctx.L.socp_fields_batch if form == "host" else ctx.L.socp_fields_batch_dev
    ptr = (lambda a, T: a.ctypes.data_as(T) if a is not None else None) if form == "host" else (lambda a, T: a.ctypes.data if a is not None else None)
    return fn(ctx.h, B, ptr(Z, DP), cols, stride, skip, cap, ptr(out[0], DP), ptr(out[1], DP), ptr(out[2], IP), ptr(out[3], IP), ptr(out[4], DP),
              ptr(out[5], DP))


def test_refusals_write_nothing_and_leave_the_context_unchanged():
    from socp_amd import capi
    c = case("goddard_m3")
    ctx = context(c)
    Z = np.ascontiguousarray(c["Z"])
    B, M, D = len(Z), ctx.M, ctx.dim
    out = buffers(B, M, CAP, D, fr.ALL)
    fresh_out = lambda o: all(np.all(v == (np.uint64(SENT) if v.dtype == np.uint64 else SENT_I)) for v in views(o))      # noqa: E731
    L, h = ctx.L, ctx.h
    t0, l0 = ctx.counters()
    tl0 = ctx.timeline(Z[0]).copy()
    for cols, stride, skip, cap, what in ((2, 7, 2, 4, "cols"), (-1, 7, 2, 4, "cols"), (1, 0, 2, 4, "stride"), (1, 7, -1, 4, "skip"), (1, 7, 2, 0, "cap")):
        for form in ("host", "dev"):
            assert raw(ctx, B, Z, cols, stride, skip, cap, out, form) == capi.ERR_ARG, what
            assert what in L.socp_last_error(h).decode()
    assert raw(ctx, -1, Z, 1, 7, 2, 4, out) == capi.ERR_ARG
    assert raw(ctx, B, None, 1, 7, 2, 4, out) == capi.ERR_ARG
    for k in range(5):
        holed = tuple(None if j == k else a for j, a in enumerate(out))
        assert raw(ctx, B, Z, 1, 7, 2, 4, holed) == capi.ERR_ARG and raw(ctx, B, Z, 1, 7, 2, 4, holed, "dev") == capi.ERR_ARG, NAMES[k]
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for pstride in (8, 9, 11):
        assert L.socp_fields_batch_blocks(h, B, Z.ctypes.data_as(DP), params.ctypes.data_as(DP), pstride, None, None, 1, 7, 2, 4,
                                          out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP), out[2].ctypes.data_as(IP), out[3].ctypes.data_as(IP),
                                          out[4].ctypes.data_as(DP), None) == capi.ERR_ARG, pstride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    assert raw(ctx, 0, None, 1, 7, 2, 4, (None,) * 6) == capi.OK and raw(ctx, 0, None, 1, 7, 2, 4, (None,) * 6, "dev") == capi.OK
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    for form in ("host", "dev"):
        assert raw(ctx, B, Z, 1, 7, 2, 4, out, form) == capi.ERR_UNSUPPORTED and "DOPRI5" in L.socp_last_error(h).decode()
    ctx.set_integrator(capi.INT_RK4)
    assert ctx.counters() == (t0, l0), "nothing was launched or counted"
    assert fresh_out(out), "nothing was written"
    assert np.array_equal(ctx.timeline(Z[0]), tl0)
    assert L.socp_ctx_has_variational(h) == 0, "Goddard keeps no variational equations"

    fresh = capi.Context(capi.MODEL_GODDARD)
    assert fresh.has_fields()
    assert raw(fresh, B, Z, 1, 7, 2, 4, out) == capi.ERR_ARG and "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    fresh.close()

    # models without the entry: the interceptor (its own ComputeTraj), vtolUAV and lqr1d (no rhs_t trait)
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    from test_gpu_cost_batch import build_vtol
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    Xs, Xf = scenario_state(gamma=1.49)
    iprob, iz = multi_shooting_problem(Oracle(MODEL_INTERCEPTOR), 4, X0=Xs, Xf=Xf)
    for variant in (capi.VARIANT_LANE_EXACT, capi.VARIANT_LANE_FAST):
        ci = capi.Context(capi.MODEL_INTERCEPTOR)
        ci.set_variant(variant)
        assert ci.problem_set(iprob.mode_t, iprob.mode_x, iprob.time, iprob.xnode) == iprob.n
        assert not ci.has_fields() and ci.L.socp_ctx_has_fields(ci.h) == 0
        c0 = ci.counters()
        io = buffers(1, 4, 4, 6, fr.ALL)
        assert raw(ci, 1, np.ascontiguousarray(iz), 1, 7, 2, 4, io) == capi.ERR_UNSUPPORTED
        assert "no fields entry" in ci.L.socp_last_error(ci.h).decode() and ci.counters() == c0 and fresh_out(io)
        with pytest.raises(capi.SocpError):
            ci.fields_batch(iz[None, :])
        ci.close()
        cv, _, Zv, _ = build_vtol("fast" if variant == capi.VARIANT_LANE_FAST else "exact")
        assert not cv.has_fields()
        c0 = cv.counters()
        vo = buffers(len(Zv), cv.M, 4, 6, fr.ALL)
        assert raw(cv, len(Zv), np.ascontiguousarray(Zv), 0, 7, 2, 4, vo) == capi.ERR_UNSUPPORTED
        assert "no fields entry" in cv.L.socp_last_error(cv.h).decode() and cv.counters() == c0 and fresh_out(vo)
        cv.close()
    lq = jc.case("lqr1d")
    cl = context(dict(lq))
    assert not cl.has_fields() and cl.has_jacobi()
    lo = buffers(len(lq["Z"]), cl.M, 4, 2, fr.ALL)
    assert raw(cl, len(lq["Z"]), np.ascontiguousarray(lq["Z"]), 0, 7, 2, 4, lo) == capi.ERR_UNSUPPORTED and fresh_out(lo)
    assert "no fields entry" in cl.L.socp_last_error(cl.h).decode()
    cl.close()
    for model in (capi.MODEL_GODDARD, capi.MODEL_DOUBLE_INTEGRATOR, capi.MODEL_COVID19):
        cm = capi.Context(model)
        assert cm.has_fields()
        cm.close()

    # a valid call afterwards: the bits of the restatement; the counters advance by B M C trajectories and ONE launch
    check_whole(run_host(ctx, Z, fr.ALL), expected(c, reference("goddard_m3"), fr.ALL), "after the refused calls")
    t1, l1 = ctx.counters()
    assert t1 - t0 == B * M * 2 * D and l1 - l0 == 1
    run_dev(ctx, Z, fr.COSTATE, phi=False)
    t2, l2 = ctx.counters()
    assert t2 - t1 == B * M * D and l2 - l1 == 1
    ctx.close()


# ---- 7. the sweep tool -----------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_fields_file_and_record(tmp_path):
    out = str(tmp_path / "fld")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--fields-out", out, "--fields-stride", "10",
                          "--fields-skip", "1", "--fields-phi"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["fields"]
    assert {"rows", "with_change", "tconj_min", "tconj_median"} <= set(entry)
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and sorted(npz.files) == sorted(["index", "tq", "det", "count", "nchange", "tconj", "phi"])
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0
    assert npz["det"].shape[:2] == (k, 1) and np.all(npz["count"] == 5) and npz["tconj"].shape == (k, 1) and npz["phi"].shape == (k, 1, 14, 14)
    changed = npz["nchange"].sum(axis=1) > 0
    assert entry["with_change"] == int(changed.sum())
    if changed.any():
        assert entry["tconj_min"] == float(np.nanmin(npz["tconj"][changed])) and entry["tconj_min"] <= entry["tconj_median"]
    else:
        assert entry["tconj_min"] is None and entry["tconj_median"] is None
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--fields-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--fields-out" in bad.stderr
