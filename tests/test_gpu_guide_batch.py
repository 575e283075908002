"""GPU: the closed-loop flight under the sampled neighbouring-extremal law (socp_guide_batch[_dev] / _blocks,
capi.Context.guide_batch) against tests/guide_reference.py -- the definition restated in Python.  The tables the call reads are the
restatements' own (tests/gain_reference.py, tests/gain_free_reference.py: the gain calls' outputs bit for bit, as their own GPU tests
show), packed into sentinel-filled buffers.  Outputs live in sentinel-filled buffers followed by 64 guard words and are compared WHOLE
on integer views (the conventions of test_gpu_gain_batch.py), so a store past a slab, past count or through a NULL pointer shows.  In
REFERENCE ORDER every output is bit-equal to the restatement, in the host, _dev and _blocks forms; the throughput flavour flies its own
arithmetic and is compared with the reference order's under a stated allowance.  The Goddard cases fly NG = 20 steps: stride 3 gives
seven samples (six blocks of 3 steps and one of 2), stride 1 twenty, stride 16 two -- a full block of 16 steps, a second sample at
step 16 (where a free final time is re-timed with k = 16) and a clamped block of 4.  The other models fly the N = 10 of the gain tests.  A case's result depends on its row, the row's blocks and its deviation alone: a reference
is computed once per distinct case and shared read-only.  The figures the tests print are kept in profiles/guide_gpu_tests.txt."""
import numpy as np
import pytest

import gain_free_reference as gf
import gain_reference as gr
import guide_reference as gd
import hamiltonian_exact_reference as hx
import jacobi_cases as jc
from test_gpu_jacobi_batch import SENT, SENT_I, DP, IP, sentinel, sentinel_i, views, canon
from test_gpu_gain_batch import context, cap_of, untouched, goddard, goddard_m3, dint_fixed, covid_m2, osc1d_plugin, dint_hx_plugin
from test_gpu_gain_batch import reference_rows as fixed_rows
from test_gpu_gain_free_batch import freed, goddard_free
from test_gpu_gain_free_batch import reference_rows as free_rows

pytestmark = pytest.mark.gpu
N = 10
NG = 20                                          # the Goddard cases' step number
_CASES = {}


def goddard_case(law, free=False):
    """test_gpu_gain_batch.goddard / test_gpu_gain_free_batch.goddard_free flown at NG steps."""
    return dict(goddard_free(law) if free else goddard(law), N=NG)


def is_free(c):
    from oracle.oracle import FREE
    return int(c["prob"].mode_t[c["prob"].M]) == FREE


def deviations(c, B, K, sigma=1e-6, seed=3):
    """dX0[B][K][d] = sigma max(1, |x0_c|) N(0, 1): one seeded table, so that case (b, k) is the same case whatever B and K are."""
    d = c["prob"].dim
    table = np.random.default_rng(seed).standard_normal((16, 16, d))
    Z = np.asarray(c["Z"], dtype=np.float64)
    rows = np.arange(B) % len(Z)
    return np.ascontiguousarray(sigma * np.maximum(1.0, np.abs(Z[rows, None, :d])) * table[np.arange(B)[:, None] % 16, np.arange(K)[None, :] % 16])


def gain_rows(c, Z, stride, blocks=None):
    return (free_rows if is_free(c) else fixed_rows)(c, Z, stride, blocks=blocks)


def table_arrays(c, rows, cap):
    """(Xq, Kg, info, count) as the gain call leaves them in sentinel-filled buffers."""
    B, M, D = len(rows), c["prob"].M, c["prob"].dim
    if is_free(c):
        _, Kg, info, count, Xq, _, _, _ = gf.pack(rows, B, M, D, cap, SENT, SENT_I)
    else:
        _, Kg, info, count, Xq, _, _ = gr.pack(rows, B, M, D, cap, SENT, SENT_I)
    return (np.ascontiguousarray(Xq).view(np.float64).ravel(), np.ascontiguousarray(Kg).view(np.float64).ravel(),
            np.ascontiguousarray(info).ravel(), np.ascontiguousarray(count).ravel())


def reference_cases(c, Z, rows, stride, cap, dX0, every, blocks=None):
    """cases[b][k] of guide_reference.guide_case; blocks = (params, time, xnode), any of them None."""
    from oracle.oracle import Problem
    prob = c["prob"]
    model = {"osc1d_exact_jacobian": "osc1d"}.get(c["model"], c["model"])
    pp, tt, xx = blocks if blocks is not None else (None, None, None)
    nP = len(c["params"])
    free = is_free(c)
    out = []
    for b, z in enumerate(np.asarray(Z, dtype=np.float64)):
        P = [float(v) for v in (c["params"] if pp is None else pp[b][:nP])]
        sw = tuple(c.get("sw") or (0.0, 0.0)) if pp is None else tuple(float(v) for v in pp[b][nP:nP + 2])
        tl = np.array(prob.time if tt is None else tt[b], dtype=np.float64)
        xn = np.array(prob.xnode if xx is None else xx[b], dtype=np.float64).reshape(prob.M + 1, 2 * prob.dim)
        pb = Problem(prob.dim, prob.mode_t, prob.mode_x, tl, xn)
        tab = gd.tables_of(rows[b], free)
        row = []
        for k in range(dX0.shape[1]):
            key = (model, c.get("N", N), stride, cap, every, tuple(P), sw, tl.tobytes(), xn.tobytes(), z.tobytes(), np.asarray(prob.mode_x).tobytes(),
                   tuple(int(m) for m in prob.mode_t), dX0[b, k].tobytes())
            if key not in _CASES:
                _CASES[key] = gd.guide_case(model, P, sw, pb, z, c.get("N", N), stride, tab, dX0[b, k], every, cap=cap)
            row.append(_CASES[key])
        out.append(row)
    return out


def expected(c, cases, cap, tf=True, dxmax=True, xs=True):
    return gd.pack(cases, len(cases), len(cases[0]), c["prob"].M, c["prob"].dim, cap, is_free(c), SENT, SENT_I, tf=tf, dxmax=dxmax, xs=xs)


# ---- the three forms on guarded buffers: each returns the seven WHOLE buffers as integer views, in the order of gd.NAMES ---------

def buffers(B, K, M, cap, d, free):
    n = B * K
    return (sentinel(n * 2 * d), sentinel(n * (d + 1 if free else d)), sentinel_i(n), sentinel_i(n), sentinel(n), sentinel(n), sentinel(n * M * cap * 2 * d))


def run_host(ctx, c, Z, stride, cap, tabs, dX0, every, tf=True, dxmax=True, xs=True, blocks=None):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B, K = dX0.shape[0], dX0.shape[1]
    out = buffers(B, K, ctx.M, cap, ctx.dim, is_free(c))
    Xq, Kg, info, count = tabs
    opt = lambda k, on: out[k].ctypes.data_as(DP) if on else None              # noqa: E731
    tail = (stride, cap, Xq.ctypes.data_as(DP), Kg.ctypes.data_as(DP), info.ctypes.data_as(IP), count.ctypes.data_as(IP), K,
            np.ascontiguousarray(dX0).ctypes.data_as(DP), every, out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP), out[2].ctypes.data_as(IP),
            out[3].ctypes.data_as(IP), opt(4, tf), opt(5, dxmax), opt(6, xs))
    if blocks is None:
        ctx._chk(ctx.L.socp_guide_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in blocks)
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None        # noqa: E731
        ctx._chk(ctx.L.socp_guide_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx), *tail))
    return views(out)


def run_dev(ctx, c, Z, stride, cap, tabs, dX0, every, tf=True, dxmax=True, xs=True):
    import torch
    B, K = dX0.shape[0], dX0.shape[1]
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dT = [torch.from_numpy(np.array(a)).cuda() for a in tabs]
    dD = torch.from_numpy(np.array(dX0, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in buffers(B, K, ctx.M, cap, ctx.dim, is_free(c))]
    torch.cuda.synchronize()
    opt = lambda k, on: dev[k].data_ptr() if on else None                      # noqa: E731
    ctx.guide_batch_dev(B, dZ.data_ptr(), stride, cap, dT[0].data_ptr(), dT[1].data_ptr(), dT[2].data_ptr(), dT[3].data_ptr(), K, dD.data_ptr(),
                        every, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), opt(4, tf), opt(5, dxmax), opt(6, xs))
    ctx.synchronize()
    torch.cuda.synchronize()
    for t, a in zip(dT, tabs):                                                  # the tables are inputs
        assert np.array_equal(t.cpu().numpy().view(np.uint8), np.asarray(a).view(np.uint8)), "a table was written"
    return views(tuple(t.cpu().numpy() for t in dev))


def check_whole(got, want, what):
    for name, g, w in zip(gd.NAMES, got, want):
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


def both_forms(ctx, c, Z, stride, cap, rows, dX0, every, what, blocks=None):
    """The host (or _blocks) form and, without blocks, the _dev form against the restatement; returns the cases."""
    cases = reference_cases(c, Z, rows, stride, cap, dX0, every, blocks=blocks)
    want = expected(c, cases, cap)
    tabs = table_arrays(c, rows, cap)
    check_whole(run_host(ctx, c, Z, stride, cap, tabs, dX0, every, blocks=blocks), want, what + (", _blocks form" if blocks else ", host form"))
    if blocks is None:
        check_whole(run_dev(ctx, c, Z, stride, cap, tabs, dX0, every), want, what + ", _dev form")
    return cases


def miss_norm(cases):
    return np.array([[max(abs(v) for v in k["miss"]) for k in row] for row in cases])


# ---- 1. Goddard, single shooting, the three laws, fixed and free final time: strides, lane counts, forms, `every` ------------------

@pytest.mark.parametrize("free", [False, True], ids=["fixed_tf", "free_tf"])
@pytest.mark.parametrize("law", ["mu2=1", "mu2=0.2", "mu2=0"])
def test_goddard_equals_the_restatement(law, free):
    c = goddard_case(law, free)
    ctx = context(c, "exact")
    assert ctx.has_guide()
    Z10 = np.array(c["Z"])[np.arange(10) % 9]
    rows3 = gain_rows(c, Z10, 3)
    cap3 = cap_of(3, NG)
    assert all(r[0]["count"] == cap3 == 7 for r in rows3)
    for B, K in ((1, 1), (9, 7), (8, 8), (5, 13), (10, 13)):          # 1, 63, 64, 65 and 130 lanes
        t0, l0 = ctx.counters()
        cases = both_forms(ctx, c, Z10[:B], 3, cap3, rows3[:B], deviations(c, B, K), 1, "%s B %d K %d" % (law, B, K))
        t1, l1 = ctx.counters()
        assert (t1 - t0, l1 - l0) == (2 * B * K, 2), "B K M trajectories and one launch per call"
    closed = miss_norm(cases)
    for every in (0, 3, 10 ** 6):
        other = both_forms(ctx, c, Z10[:2], 3, cap3, rows3[:2], deviations(c, 2, 3), every, "%s every %d" % (law, every))
        due = {0: 0, 3: 3, 10 ** 6: 1}[every]                         # seven samples: 0, 3 and 6 are due with every = 3
        assert all(k["nupd"] + k["nskip"] == due for row in other for k in row)
        if every == 0:
            opened = miss_norm(other)
    for stride in (1, 16):
        cap = cap_of(stride, NG)
        rows = gain_rows(c, Z10[:3], stride)
        for every in (1, 2):
            far = both_forms(ctx, c, Z10[:3], stride, cap, rows, deviations(c, 3, 5), every, "%s stride %d every %d" % (law, stride, every))
        if stride == 16:
            assert cap == 2 and any(k["samples"] == 2 and k["nupd"] >= 1 for row in far for k in row), "a full block, a second sample at step 16, a clamped block of 4"
    # a larger cap: the slots at or beyond count keep what the buffer held
    both_forms(ctx, c, Z10[:2], 3, cap3 + 2, rows3[:2], deviations(c, 2, 3), 1, "%s cap + 2" % law)
    print("goddard %s %s: dX0 = 1e-6 max(1, |x|) N(0, 1): median ||miss||inf closed %.3e (every = 1, 130 cases), open %.3e (6 cases); nupd %s nskip %s"
          % (law, "free t_f" if free else "fixed t_f", np.median(closed), np.median(opened), cases[0][0]["nupd"], cases[0][0]["nskip"]))
    ctx.close()


# ---- 2. M = 3 across the segment boundaries, per-row blocks -------------------------------------------------------------------------

@pytest.mark.parametrize("free", [False, True], ids=["fixed_tf", "free_tf"])
def test_goddard_m3_per_row_blocks(free):
    c = dict(jc.goddard_m3(free_tf=True, B=5, seed=11) if free else goddard_m3(), N=NG)
    prob, B = c["prob"], len(c["Z"])
    pp = np.tile(np.concatenate([c["params"], [0.0227, 0.08]]), (B, 1))
    pp[:, 4] = 1.0 - 0.1 * np.arange(B)
    tt = np.tile(prob.time, (B, 1))
    tt[:, 0] = 0.001 * np.arange(B)
    xx = np.tile(np.asarray(prob.xnode).ravel(), (B, 1))
    xx[:, 3 * 14] += 0.001 * np.arange(B)
    stride, cap, K = 3, cap_of(3, NG), 3
    dX0 = deviations(c, B, K)
    ctx = context(c, "exact")
    rows = gain_rows(c, c["Z"], stride)
    shared = both_forms(ctx, c, c["Z"], stride, cap, rows, dX0, 1, "M = 3 shared blocks")
    own_rows = gain_rows(c, c["Z"], stride, blocks=(pp, tt, xx))
    own = both_forms(ctx, c, c["Z"], stride, cap, own_rows, dX0, 1, "M = 3 per-row blocks", blocks=(pp, tt, xx))
    both_forms(ctx, c, c["Z"], stride, cap, rows, dX0, 1, "the context's own blocks are back")
    for b in (0, B - 1):                                              # the row run alone, on the device
        both_forms(ctx, c, c["Z"][b:b + 1], stride, cap, own_rows[b:b + 1], dX0[b:b + 1], 1, "row %d alone" % b,
                   blocks=(pp[b:b + 1], tt[b:b + 1], xx[b:b + 1]))
    assert not np.array_equal(own[1][0]["xf"], shared[1][0]["xf"]), "the blocks move the flight"
    assert all(len(k["xs"]) == 3 and k["samples"] == 21 for row in shared for k in row), "three segments of seven samples in flight order"
    print("goddard M = 3 %s: nupd %s nskip %s, ||miss||inf of row 0 %s" % ("free t_f" if free else "fixed t_f", shared[0][0]["nupd"], shared[0][0]["nskip"],
                                                                          miss_norm(shared)[0]))
    ctx.close()


# ---- 3. the other models -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("free", [False, True], ids=["fixed_tf", "free_tf"])
def test_double_integrator_with_saturated_rows(free):
    c = dint_fixed(10)
    if free:
        c = freed(c, 3.0 * (1.0 + 0.03 * np.arange(10)))
    ctx = context(c, "exact")
    both_forms(ctx, c, c["Z"], 3, 4, gain_rows(c, c["Z"], 3), deviations(c, 10, 4), 1, "dint %s" % ("free t_f" if free else "fixed t_f"))
    ctx.close()


def test_covid19_m2_fixed_fixed_free():
    from oracle.oracle import FIXED, FREE
    c = freed(covid_m2(), [10.0, 9.5, 10.5], mode_t=[FIXED, FIXED, FREE])
    ctx = context(c, "exact")
    for stride in (3, 16):
        both_forms(ctx, c, c["Z"], stride, cap_of(stride), gain_rows(c, c["Z"], stride), deviations(c, 3, 3, sigma=1e-4), 1, "covid stride %d" % stride)
    ctx.close()


@pytest.mark.parametrize("name", ["osc1d_plugin", "dint_hx_plugin"])
def test_plugins_have_the_entry_with_no_source_change(name):
    c = {"osc1d_plugin": osc1d_plugin, "dint_hx_plugin": dint_hx_plugin}[name]()
    with hx.entries():                                                # lends the references the H-only models' texts
        ctx = context(c, "exact")
        assert ctx.has_guide()
        both_forms(ctx, c, c["Z"], 3, 4, gain_rows(c, c["Z"], 3), deviations(c, len(c["Z"]), 3), 1, name)
        ctx.close()


def test_models_without_the_entry():
    from socp_amd import capi
    from test_gpu_cost_batch import build_vtol
    ci = capi.Context(capi.MODEL_INTERCEPTOR)
    assert not ci.has_guide()
    ci.close()
    cv = build_vtol("exact")[0]
    assert not cv.has_guide()
    cv.close()
    lq = jc.case("lqr1d")
    cl = context(dict(lq, N=N))
    assert not cl.has_guide()
    cl.close()
    for model in ("goddard", "dint", "covid"):
        for variant in ("exact", "fast"):
            ctx = context(dict(model=model), variant)
            assert ctx.has_guide(), (model, variant)
            ctx.close()


# ---- 4. edge rows ----------------------------------------------------------------------------------------------------------------------

def test_zero_length_segment_and_nan_row():
    c = goddard_case("mu2=1")
    Z = np.array(c["Z"][:5])
    Z[3, 9] = np.nan                                                  # a NaN costate beside healthy rows
    tt = np.tile(c["prob"].time, (5, 1))
    tt[1, 1] = tt[1, 0]                                               # row 1: a segment without a step
    stride, cap, K = 3, cap_of(3, NG), 3
    dX0 = deviations(c, 5, K)
    rows = gain_rows(c, Z, stride, blocks=(None, tt, None))
    ctx = context(c, "exact")
    cases = both_forms(ctx, c, Z, stride, cap, rows, dX0, 1, "edge rows", blocks=(None, tt, None))
    assert all(k["samples"] == 1 and np.array_equal(k["xf"][:7], Z[1, :7] + d) for k, d in zip(cases[1], dX0[1])), "no step: the start state stays"
    assert all(np.all(np.isnan(k["xf"])) for k in cases[3]), "the cases of the NaN row are NaN"
    for b in (2, 4):                                                  # the neighbours equal their own run alone
        both_forms(ctx, c, Z[b:b + 1], stride, cap, rows[b:b + 1], dX0[b:b + 1], 1, "row %d alone" % b, blocks=(None, tt[b:b + 1], None))
    ctx.close()


def test_a_case_of_a_row_equals_the_same_case_with_one_case_per_row():
    c = goddard_case("mu2=1", free=True)
    stride, cap, B, K = 3, cap_of(3, NG), 3, 5
    rows = gain_rows(c, c["Z"][:B], stride)
    tabs = table_arrays(c, rows, cap)
    dX0 = deviations(c, B, K)
    ctx = context(c, "exact")
    whole = run_dev(ctx, c, c["Z"][:B], stride, cap, tabs, dX0, 1)
    s, d = 14, 7
    for k in (0, 4):
        one = run_dev(ctx, c, c["Z"][:B], stride, cap, tabs, np.ascontiguousarray(dX0[:, k:k + 1]), 1)
        for name, g, w, width in zip(gd.NAMES, one, whole, (s, d + 1, 1, 1, 1, 1, cap * s)):
            assert np.array_equal(canon(g[:B * width]), canon(w[:B * K * width].reshape(B, K, width)[:, k].ravel())), (name, k)
    ctx.close()


# ---- 5. NULL outputs -------------------------------------------------------------------------------------------------------------------

def test_each_optional_output_null_in_turn():
    c = goddard_case("mu2=1")
    stride, cap = 3, cap_of(3, NG)
    rows = gain_rows(c, c["Z"][:3], stride)
    tabs = table_arrays(c, rows, cap)
    dX0 = deviations(c, 3, 5)
    cases = reference_cases(c, c["Z"][:3], rows, stride, cap, dX0, 1)
    ctx = context(c, "exact")
    for tf, dxmax, xs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        want = expected(c, cases, cap, tf=tf, dxmax=dxmax, xs=xs)
        what = "tf %s dxmax %s Xs %s" % (tf, dxmax, xs)
        check_whole(run_dev(ctx, c, c["Z"][:3], stride, cap, tabs, dX0, 1, tf=tf, dxmax=dxmax, xs=xs), want, what + ", _dev form")
        check_whole(run_host(ctx, c, c["Z"][:3], stride, cap, tabs, dX0, 1, tf=tf, dxmax=dxmax, xs=xs), want, what + ", host form")
    ctx.close()


# ---- 6. cross-checks on the device -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_zero_deviation_is_the_nominal_flight_and_the_python_form(variant):
    """M = 1, dX0 = 0.  Reference order, every = 1: the samples are the table's Xq and miss is socp_residual_batch's final rows, bit for
    bit.  Throughput flavour: the tables hold the REFERENCE-order nominal states (the gain calls are one object for both flavours), so a
    throughput flight sees the flavours' own deviation as dx and corrects it; flown OPEN loop (every = 0) its miss is the throughput
    residual's final rows up to the contraction the compiler chose in another translation unit -- a perturbation of the size of the
    flavours' own difference: asked to stay within 8 x max |F_exact - F_fast| on the same rows (the house margin), on the polished
    nominal root, where that difference is at rounding level."""
    import torch
    cases = (goddard_case("mu2=1"), goddard_case("mu2=0.2", free=True)) if variant == "exact" else (nominal_goddard(False), nominal_goddard(True))
    for c in cases:
        ctx = context(c, variant)
        B, d = len(c["Z"]), 7
        every = 1 if variant == "exact" else 0
        stride = 3 if variant == "exact" else 7
        Q = cap_of(stride, c["N"])
        r = ctx.guide_batch(c["Z"], np.zeros((B, 2, d)), stride=stride, every=every, xs=True)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for k, v in r.items() if k != "tables")
        free = is_free(c)
        assert r["xf"].shape == (B, 2, 14) and r["miss"].shape == (B, 2, 8 if free else 7) and r["xs"].shape == (B, 2, 1, Q, 14)
        F = ctx.residual_batch(c["Z"])
        want = np.hstack([F[:, d:2 * d], F[:, 14:15]]) if free else F[:, d:2 * d]
        miss = r["miss"].cpu().numpy()
        if variant == "exact":
            assert np.array_equal(miss[:, 0].view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), "miss is the residual's final rows"
        else:
            other = context(c, "exact")
            room = 8.0 * float(np.abs(other.residual_batch(c["Z"]) - F).max())
            other.close()
            worst = float(np.abs(miss[:, 0] - want).max())
            print("throughput flavour, open loop, dX0 = 0 (%s): miss off its own residual's final rows by %.3e, allowance %.3e" % ("free t_f" if free else "fixed t_f", worst, room))
            assert 0 < room < 1e-6 and worst <= room, "the allowance is at rounding level: the check says something"
        assert np.array_equal(miss[:, 0].view(np.uint64), miss[:, 1].view(np.uint64))
        xs, xq = r["xs"].cpu().numpy(), r["tables"]["xq"].cpu().numpy()
        if variant == "exact":
            assert np.array_equal(xs[:, 0].view(np.uint64), xq.view(np.uint64)), "Xs is the table's Xq"
        assert np.all(r["dxmax"].cpu().numpy() == 0.0)
        info = r["tables"]["info"].cpu().numpy()
        if variant == "exact":
            assert np.array_equal(r["nupd"].cpu().numpy()[:, 0], (info[:, 0] == 0).sum(axis=1)) and np.all((r["nupd"] + r["nskip"]).cpu().numpy() == Q)
        else:
            assert np.all((r["nupd"] + r["nskip"]).cpu().numpy() == 0)
        tf = r["tf"].cpu().numpy()
        if variant == "exact":
            assert np.array_equal(tf[:, 0], np.asarray(c["Z"])[:, -1] if free else np.full(B, c["prob"].time[1]))
        ctx.close()


# ---- 7. the throughput flavour -----------------------------------------------------------------------------------------------------------

def nominal_goddard(free):
    """The polished nominal Goddard root of the CPU gain tests (mu2 = 1, M = 1, N = 50), four rows of it: a flight that stays in the
    regime the law is meant for, unlike the unconverged rows of the bit-equality cases."""
    import test_gain_cpu as tg
    import test_gain_free_cpu as tgf
    c = tgf.case("goddard") if free else tg.case("goddard")
    return dict(model="goddard", params=np.array(c["P"]), prob=c["prob"], N=c["N"] if free else tg.N, Z=np.tile(np.asarray(c["z"], dtype=np.float64), (4, 1)))


@pytest.mark.parametrize("free", [False, True], ids=["fixed_tf", "free_tf"])
def test_throughput_flavour_against_the_reference_order(free):
    """nupd and nskip equal the reference order's.  Xf, miss and tf are compared with the reference order's under the allowance
    8 x (1 + the largest ||Kg||inf over the applied samples) x e_old, e_old the deviation between the two flavours' own
    socp_trace_batch rows on the same nominal rows: a flight's state error enters the reset costate multiplied by the gain, and
    nothing else accumulates; 8 is the house margin over a first-order estimate."""
    c = nominal_goddard(free)
    B, K, d = len(c["Z"]), 7, 7
    dX0 = deviations(c, B, K, sigma=1e-6)
    out, trace = {}, {}
    for variant in ("exact", "fast"):
        ctx = context(c, variant)
        r = ctx.guide_batch(c["Z"], dX0, stride=7, every=1)
        out[variant] = {k: v.cpu().numpy() for k, v in r.items() if k != "tables"}
        tables = {k: v.cpu().numpy() for k, v in r["tables"].items()}
        rows, count = ctx.trace_batch(c["Z"], stride=1)
        trace[variant] = rows[:, :, :c["N"] + 1, 1:15]
        ctx.close()
    assert np.array_equal(out["exact"]["nupd"], out["fast"]["nupd"]) and np.array_equal(out["exact"]["nskip"], out["fast"]["nskip"])
    e_old = float(np.abs(trace["exact"] - trace["fast"]).max())
    kg = tables["ke" if free else "kp"]
    applied = tables["info"] == 0
    knorm = float(np.abs(kg[applied]).sum(axis=-2).max())          # the induced inf-norm: rows r summed over the columns c (kg[..., c, r])
    room = 8.0 * (1.0 + knorm) * e_old
    worst = max(float(np.abs(out["exact"][k] - out["fast"][k]).max()) for k in ("xf", "miss", "tf"))
    print("throughput flavour %s: e_old = %.3e, max ||Kg||inf over the applied samples = %.3e, allowance %.3e, measured %.3e (ratio %.2e)"
          % ("free t_f" if free else "fixed t_f", e_old, knorm, room, worst, worst / room))
    closed = float(np.abs(out["exact"]["miss"]).max())
    print("    the law on the nominal flight, dX0 = 1e-6 max(1, |x|) N(0, 1): ||miss||inf closed loop %.3e (reference order), nupd %d nskip %d"
          % (closed, out["exact"]["nupd"][0, 0], out["exact"]["nskip"][0, 0]))
    assert e_old > 0 and worst <= room


# ---- 8. refusals: the message, the sentinels, the counters ---------------------------------------------------------------------------------

def refused(ctx, c, code, text, Z, stride, cap, K=2, every=1, null=None, form="dev", blocks=None, null_z=False):
    import torch
    from socp_amd import capi
    before = ctx.counters()
    B, M, d = len(Z), max(getattr(ctx, "M", None) or 1, 1), ctx.dim
    cc = max(cap, 1)
    tabs = (np.zeros(B * M * cc * 2 * d), np.zeros(B * M * cc * (d + 1) * d), np.zeros(B * M * cc, dtype=np.int32), np.ones(B * M, dtype=np.int32))
    dX0 = np.zeros((B, max(K, 1), d))
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dT = [torch.from_numpy(a).cuda() for a in tabs] + [torch.from_numpy(dX0).cuda()]
    dev = [torch.from_numpy(a).cuda() for a in buffers(B, max(K, 1), M, cc, d, True)]
    p = [t.data_ptr() for t in dT] + [t.data_ptr() for t in dev]
    if null is not None:
        p[null] = None
    torch.cuda.synchronize()
    with pytest.raises(capi.SocpError) as e:
        if form == "dev":
            ctx.guide_batch_dev(B, None if null_z else dZ.data_ptr(), stride, cap, p[0], p[1], p[2], p[3], K, p[4], every, *p[5:])
        else:
            run_host(ctx, dict(c, prob=c["prob"]), Z, stride, cap, tabs, dX0, every, blocks=blocks)
    torch.cuda.synchronize()
    assert e.value.code == code and text in str(e.value), (code, text, str(e.value))
    assert ctx.counters() == before, "an error leaves the counters unchanged"
    assert untouched(views(tuple(t.cpu().numpy() for t in dev))), "an error writes nothing"


def test_refusals():
    from socp_amd import capi
    from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
    c = goddard("mu2=1")
    Z = c["Z"][:2]
    ARG, UNS = capi.ERR_ARG, capi.ERR_UNSUPPORTED
    bare = context(dict(c, prob=None))
    refused(bare, c, ARG, "no problem set", Z, 3, 4)
    bare.close()
    ctx = context(c)
    refused(ctx, c, ARG, "K >= 1 and every >= 0", Z, 3, 4, K=0)
    refused(ctx, c, ARG, "K >= 1 and every >= 0", Z, 3, 4, every=-1)
    refused(ctx, c, ARG, "stride >= 1", Z, 0, 4)
    refused(ctx, c, ARG, "cap >= ceil(step_nbr / stride)", Z, 3, 3)
    for k in range(9):                                                # Xq, Kg, info, count, dX0, Xf, miss, nupd, nskip
        refused(ctx, c, ARG, "null argument", Z, 3, 4, null=k)
    refused(ctx, c, ARG, "null argument", Z, 3, 4, null_z=True)
    before = ctx.counters()
    nothing = (None,) * 4
    assert ctx.L.socp_guide_batch_dev(ctx.h, -1, None, 3, 4, *nothing, 1, None, 1, *(None,) * 7) == ARG and "B >= 0" in ctx.L.socp_last_error(ctx.h).decode()
    assert ctx.L.socp_guide_batch_dev(ctx.h, 0, None, 3, 4, *nothing, 1, None, 1, *(None,) * 7) == 0, "B == 0: SOCP_OK without a launch"
    assert ctx.L.socp_guide_batch(ctx.h, 0, None, 3, 4, *nothing, 1, None, 1, *(None,) * 7) == 0
    assert ctx.counters() == before
    pp = np.tile(np.concatenate([c["params"], [0.0, 0.0, 0.0]]), (2, 1))
    refused(ctx, c, ARG, "the parameter stride", Z, 3, 4, form="host", blocks=(pp, None, None))
    ctx.set_integrator(capi.INT_DOPRI5)
    refused(ctx, c, UNS, "SOCP_INT_DOPRI5", Z, 3, 4)
    ctx.set_integrator(capi.INT_RK4)
    both_forms(ctx, c, Z, 3, 4, gain_rows(c, Z, 3), deviations(c, 2, 3), 1, "the context still works")
    ctx.close()
    # a free interior time; an interior node with a FIXED and with a FREE component, under both final-time structures
    m3 = goddard_m3(2)
    q = m3["prob"]
    inner = context(dict(m3, prob=Problem(7, [FIXED, FREE, CONTINUOUS, FIXED], q.mode_x, q.time, q.xnode)))
    refused(inner, m3, UNS, "a free time (node 1)", np.hstack([m3["Z"], [[0.03], [0.03]]]), 3, 4)
    inner.close()
    inner = context(dict(m3, prob=Problem(7, [FIXED, FREE, CONTINUOUS, FREE], q.mode_x, q.time, q.xnode)))
    refused(inner, m3, UNS, "a free time before the final node (node 1)", np.hstack([m3["Z"], [[0.03, 0.26], [0.03, 0.26]]]), 3, 4)
    inner.close()
    for mode, comp in ((FIXED, 2), (FREE, 5)):
        mx = np.array(q.mode_x)
        mx[1, comp] = mode
        node = context(dict(m3, prob=Problem(7, q.mode_t, mx, q.time, q.xnode)))
        refused(node, m3, UNS, "a FIXED or FREE state component on an interior node (node 1, component %d)" % comp, m3["Z"], 3, 4)
        node.close()
        node = context(dict(m3, prob=Problem(7, [FIXED, CONTINUOUS, CONTINUOUS, FREE], mx, q.time, q.xnode)))
        refused(node, m3, UNS, "a FIXED or FREE state component on an interior node (node 1, component %d)" % comp,
                np.hstack([m3["Z"], [[0.26], [0.26]]]), 3, 4)
        node.close()
    # ("too many states for the batched linear solve" cannot be reached: a model has 2 d <= 64, and 3 d + 2 doubles always fit the LDS)
    # a model without the entries
    lq = jc.case("lqr1d")
    cl = context(dict(lq, N=N))
    refused(cl, lq, UNS, "launch table has no gain", lq["Z"], 3, 4)
    cl.close()


# ---- 9. the sweep tool -------------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_guide_file_and_record(tmp_path):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "guide")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--gain-stride", "1", "--guide-out", out, "--guide-cases", "4",
                          "--guide-sigma", "1e-4", "--guide-every", "2", "--guide-seed", "5"], cwd=root, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["guide"]
    assert {"rows", "cases", "miss_median", "miss_p95", "miss_open_median", "miss_open_p95", "skipped_samples"} <= set(entry)
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and sorted(npz.files) == sorted(["index", "dx0", "miss", "miss_open", "nupd", "nskip", "tf"])
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0 and entry["cases"] == 4
    assert npz["dx0"].shape == (k, 4, 7) and npz["miss"].shape == (k, 4, 7) and npz["miss_open"].shape == (k, 4, 7) and npz["tf"].shape == (k, 4)
    assert np.all(npz["nupd"] + npz["nskip"] == 25), "50 steps: 50 samples, every second one due"
    assert entry["skipped_samples"] == int(npz["nskip"].sum())
    assert entry["miss_median"] < entry["miss_open_median"], "the law brings the dispersed cases closer to the target"
    again = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--gain-stride", "1", "--guide-out", out + "2", "--guide-cases", "4",
                            "--guide-sigma", "1e-4", "--guide-every", "2", "--guide-seed", "5"], cwd=root, capture_output=True, text=True, timeout=300)
    assert again.returncode == 0 and np.array_equal(np.load(out + "2.rank0.npz")["dx0"], npz["dx0"]), "the seed fixes the deviations"
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--guide-out", out], cwd=root,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--guide-out" in bad.stderr
