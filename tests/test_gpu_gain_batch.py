"""GPU: the batched neighbouring-extremal gains (socp_gain_batch[_dev] / _blocks, capi.Context.gain_batch) against
tests/gain_reference.py -- the definition restated in Python: blocks on dual numbers, the backward product sweep, the elimination of
tests/tangent_reference.py.  Outputs live in sentinel-filled buffers followed by 64 guard words and are compared WHOLE on integer
views (the conventions of test_gpu_fields_batch.py), so a store past a slab, past count or through a NULL pointer shows.  Every
output is bit-equal to the restatement, in BOTH flavours (the kernels are one object without contraction, the elimination runs in
reference order); the one exception is the payload of a NaN that arithmetic produced from a NaN input, so NaNs other than the
sentinel are compared as NaN.  N = 10 steps: stride 3 gives blocks of 3, 3, 3, 1 steps, stride 1 ten blocks, stride 16 one.  A row's
result depends on the row and its blocks alone: a reference is computed once per distinct row and shared read-only.
The figures the tests print are kept in profiles/gain_gpu_tests.txt."""
import numpy as np
import pytest

import fields_reference as fr
import gain_reference as gr
import hamiltonian_exact_reference as hx
import jacobi_cases as jc
from test_gpu_jacobi_batch import SENT, SENT_I, DP, IP, sentinel, sentinel_i, views, canon, plugin_path

pytestmark = pytest.mark.gpu
N = 10
PLUGIN_IDS = {"lqr1d": 1001, "osc1d_exact_jacobian": 1005, "dint_hx": 1011}
IN_TREE = ("goddard", "dint", "covid")
VARIANTS = ("exact", "fast")
_ROWS = {}


def context(c, variant="exact"):
    from socp_amd import capi
    if c["model"] in PLUGIN_IDS:
        capi.plugin_load(plugin_path(c["model"]))
        ctx = capi.Context(PLUGIN_IDS[c["model"]], nparams=len(c["params"]))
    else:
        ctx = capi.Context({"goddard": capi.MODEL_GODDARD, "dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19,
                            "interceptor": capi.MODEL_INTERCEPTOR}[c["model"]])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    if c.get("params") is not None:
        ctx.set_params(np.asarray(c["params"], dtype=np.float64))
    ctx.set_step_number(c.get("N", N))
    if c.get("sw") is not None:
        ctx.set_switching_times(c["sw"])
    prob = c.get("prob")
    if prob is not None:
        assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


def cap_of(stride, steps=N):
    return max(1, -(-steps // stride))


# ---- the restatement, one row at a time ----------------------------------------------------------------------------------------

def reference_rows(c, Z, stride, cap=None, blocks=None):
    """rows[b][i] of gain_reference.gain_row; blocks = (params, time, xnode), any of them None.  Every time is FIXED."""
    prob = c["prob"]
    D, M = prob.dim, prob.M
    model = {"osc1d_exact_jacobian": "osc1d"}.get(c["model"], c["model"])
    pp, tt, _ = blocks if blocks is not None else (None, None, None)
    nP = len(c["params"])
    out = []
    for b, z in enumerate(np.asarray(Z, dtype=np.float64)):
        P = [float(v) for v in (c["params"] if pp is None else pp[b][:nP])]
        sw = tuple(c.get("sw") or (0.0, 0.0)) if pp is None else tuple(float(v) for v in pp[b][nP:nP + 2])
        tl = [float(t) for t in (prob.time if tt is None else tt[b])]
        key = (model, c.get("N", N), stride, cap, tuple(P), sw, tuple(tl), z.tobytes(), np.asarray(prob.mode_x).tobytes())
        if key not in _ROWS:
            _ROWS[key] = gr.gain_row(model, P, sw, D, tl, prob.mode_x[M], z, c.get("N", N), stride, cap=cap)
        out.append(_ROWS[key])
    return out


def expected(c, rows, cap, xq=True, wq=True, psi=True):
    return gr.pack(rows, len(rows), c["prob"].M, c["prob"].dim, cap, SENT, SENT_I, xq=xq, wq=wq, psi=psi)


# ---- the three forms on guarded buffers: each returns the seven WHOLE buffers as integer views, in the order of gr.NAMES ---------

def buffers(B, M, cap, d):
    slots = B * M * cap
    return (sentinel(slots), sentinel(slots * d * d), sentinel_i(slots), sentinel_i(B * M), sentinel(slots * 2 * d), sentinel(slots * 2 * d * d),
            sentinel(slots * 4 * d * d))


def run_host(ctx, Z, stride, cap, xq=True, wq=True, psi=True, blocks=None):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B = len(Z)
    out = buffers(B, ctx.M, cap, ctx.dim)
    tail = (stride, cap, out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP), out[2].ctypes.data_as(IP), out[3].ctypes.data_as(IP),
            out[4].ctypes.data_as(DP) if xq else None, out[5].ctypes.data_as(DP) if wq else None, out[6].ctypes.data_as(DP) if psi else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_gain_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in blocks)
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None        # noqa: E731
        ctx._chk(ctx.L.socp_gain_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx), *tail))
    return views(out)


def run_dev(ctx, Z, stride, cap, xq=True, wq=True, psi=True):
    import torch
    B = len(Z)
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in buffers(B, ctx.M, cap, ctx.dim)]
    torch.cuda.synchronize()
    ctx.gain_batch_dev(B, dZ.data_ptr(), stride, cap, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                       dev[4].data_ptr() if xq else None, dev[5].data_ptr() if wq else None, dev[6].data_ptr() if psi else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    return views(tuple(t.cpu().numpy() for t in dev))


def check_whole(got, want, what):
    for name, g, w in zip(gr.NAMES, got, want):
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


def untouched(got):
    return all(np.all(g == (np.uint64(SENT) if g.dtype == np.uint64 else SENT_I)) for g in got)


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def goddard(law):
    """Single shooting with a fixed final time, 9 rows: the smooth law at mu2 = 1 and 0.2, and mu2 = 0 with full thrust up to
    sw0 = 0.05 -- inside the first block of stride 3 (steps of 0.0264) -- and the singular arc up to sw1 = 0.15."""
    c = dict(jc.goddard_single(), N=N)
    o = jc.goddard_oracle(N)
    if law == "mu2=0":
        o.set_param("mu2", 0.0)
        o.set_switching([0.05, 0.15])
        c["sw"] = (0.05, 0.15)
    elif law == "mu2=0.2":
        o.set_param("mu2", 0.2)
    return dict(c, o=o, params=o.params()[:8], Z=np.array(c["Z"]))


def goddard_m3(B=5):
    """M = 3, every interior node CONTINUOUS, every time FIXED: the sweep crosses two segment boundaries."""
    c = jc.goddard_m3(free_tf=False, B=B, seed=11)
    return dict(c, N=N)


def dint_fixed(B=17):
    """The double integrator over [0, 3], final position fixed and final velocity free; the later rows saturate the control."""
    from oracle.oracle import Oracle, Problem, MODEL_DINT, FIXED, FREE
    o = Oracle(MODEL_DINT, step_nbr=N)
    n0 = np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.1, 0.02, -0.01, 0.015, 0.4, -0.3, 0.2])
    Z = np.tile(n0, (B, 1)) * (1.0 + 0.05 * np.random.default_rng(13).uniform(-1.0, 1.0, size=(B, 12)))
    Z[B // 2:, 9:] *= 6.0
    mode_x = np.zeros((2, 6), dtype=np.int32)
    mode_x[1, 3:] = FREE
    xn = np.zeros((2, 12))
    xn[1, :3] = (0.5, -0.3, 0.2)
    return dict(model="dint", o=o, prob=Problem(6, [FIXED, FIXED], mode_x, np.array([0.0, 3.0]), xn), N=N, Z=Z, params=o.params()[:3])


def covid_m2():
    """covid19, M = 2 with a CONTINUOUS interior node: node 0 with the control on its upper bound, node 1 inside the penalty; 3 rows."""
    from oracle.oracle import Oracle, Problem, MODEL_COVID, FIXED, CONTINUOUS
    o = Oracle(MODEL_COVID, step_nbr=N)
    n0 = np.array([0.9, 0.01, 0.05, 0.04, -1500.0, 300.0, 0.5, 0.1])
    n1 = np.array([0.6, 0.05, 0.2, 0.15, -0.5, 0.8, 0.3, 0.1])
    Z = np.tile(np.concatenate([n0, n1]), (3, 1)) * (1.0 + 0.02 * np.random.default_rng(4).uniform(-1.0, 1.0, size=(3, 16)))
    mode_x = np.zeros((3, 4), dtype=np.int32)
    mode_x[1] = CONTINUOUS
    prob = Problem(4, [FIXED, FIXED, FIXED], mode_x, np.array([0.0, 5.0, 10.0]), np.zeros((3, 8)))
    return dict(model="covid", o=o, prob=prob, N=N, Z=Z, params=o.params()[:8])


def osc1d_plugin():
    """tests/plugin/osc1d_exact_jacobian_plugin.hip as it stands, M = 2 with a CONTINUOUS interior node, fixed times; 5 rows."""
    from oracle.oracle import Problem, FIXED, CONTINUOUS
    Z = np.random.default_rng(5).uniform(0.2, 1.0, size=(5, 4))
    mode_x = np.zeros((3, 1), dtype=np.int32)
    mode_x[1] = CONTINUOUS
    return dict(model="osc1d_exact_jacobian", prob=Problem(1, [FIXED, FIXED, FIXED], mode_x, np.array([0.0, 1.0, 2.0]), np.zeros((3, 2))),
                N=N, Z=Z, params=np.array([4.0]))


def dint_hx_plugin():
    """tests/plugin/dint_hx_plugin.hip: the double integrator from its Hamiltonian alone; the rows of dint_fixed."""
    c = dint_fixed(5)
    return dict(c, model="dint_hx", o=None)


# ---- 1. Goddard, single shooting, the three laws: every stride, B and form, both flavours -------------------------------------------

@pytest.mark.parametrize("law", ["mu2=1", "mu2=0.2", "mu2=0"])
def test_goddard_single_equals_the_restatement(law):
    c = goddard(law)
    ctx = {v: context(c, v) for v in VARIANTS}
    assert ctx["exact"].has_gain() and ctx["fast"].has_gain()
    for stride in (3, 1, 16):
        cap = cap_of(stride)
        rows = reference_rows(c, c["Z"], stride)
        assert all(r[0]["count"] == cap for r in rows), "ten steps: %d blocks" % cap
        assert all(r[0]["info"][0] == 0 for r in rows), "a costate correction at t0 reaches the target"
        for B in (1, 4, 5, 9):                    # fourteen lanes per group: four groups per wave, so 5 and 9 cross a wave
            want = expected(c, rows[:B], cap)
            t0, l0 = ctx["exact"].counters()
            check_whole(run_dev(ctx["exact"], c["Z"][:B], stride, cap), want, "%s stride %d B %d, _dev form" % (law, stride, B))
            t1, l1 = ctx["exact"].counters()
            assert (t1 - t0, l1 - l0) == (B * 1 * 14, 3), "B M S trajectories and three launches"
            check_whole(run_host(ctx["exact"], c["Z"][:B], stride, cap), want, "%s stride %d B %d, host form" % (law, stride, B))
        check_whole(run_dev(ctx["fast"], c["Z"], stride, cap), want, "%s stride %d, _dev form, throughput flavour" % (law, stride))
        check_whole(run_host(ctx["fast"], c["Z"], stride, cap), want, "%s stride %d, host form, throughput flavour" % (law, stride))
        # a larger cap: the slots at or beyond count keep what the buffers held
        check_whole(run_dev(ctx["exact"], c["Z"], stride, cap + 2), expected(c, rows, cap + 2), "%s stride %d cap + 2" % (law, stride))
    k0 = np.array(reference_rows(c, c["Z"][:1], 3)[0][0]["kp"][0]).T
    rows3 = reference_rows(c, c["Z"][:1], 3)[0][0]["info"]
    print("goddard %s: |K(t0)|max = %.6e, K[0][0] = %.17g, info by sample at stride 3: %s" % (law, np.abs(k0).max(), k0[0, 0], rows3))
    if law == "mu2=0":
        smooth = reference_rows(dict(goddard("mu2=1"), Z=c["Z"]), c["Z"][:1], 3)
        assert not np.array_equal(smooth[0][0]["psi"][0], reference_rows(c, c["Z"][:1], 3)[0][0]["psi"][0]), "the general-law kernel ran"
    for x in ctx.values():
        x.close()


def test_python_form():
    import torch
    c = goddard("mu2=1")
    ctx = context(c)
    r = ctx.gain_batch(c["Z"], stride=3, wq=True, psi=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in r.values()) and r["kp"].shape == (9, 1, 4, 7, 7) and r["psi"].shape == (9, 1, 4, 14, 14)
    want = expected(c, reference_rows(c, c["Z"], 3), 4)
    for key, w in zip(("tq", "kp", "info", "count", "xq", "wq", "psi"), want):
        g = r[key].cpu().numpy()
        assert np.array_equal(canon(g.view(np.uint64)) if g.dtype == np.float64 else g, canon(w.reshape(g.shape))), key
    ctx.close()


# ---- 2. M = 3 across segment boundaries, per-row blocks: each row equals the row run alone -----------------------------------------

def test_goddard_m3_per_row_blocks():
    c = goddard_m3()
    prob, B = c["prob"], len(c["Z"])
    rng = np.random.default_rng(21)
    pp = np.tile(np.concatenate([c["params"], [0.0227, 0.08]]), (B, 1))
    pp[:, 4] = 1.0 - 0.1 * np.arange(B)                              # mu2 of each row: the smooth law throughout, no promise given
    tt = np.tile(prob.time, (B, 1)) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(B, 1)))
    xx = np.tile(np.asarray(prob.xnode).ravel(), (B, 1))
    xx[:, 3 * 14] += 0.001 * np.arange(B)
    stride, cap = 3, 4
    for variant in VARIANTS:
        ctx = context(c, variant)
        rows = reference_rows(c, c["Z"], stride)
        check_whole(run_host(ctx, c["Z"], stride, cap), expected(c, rows, cap), "M = 3 shared blocks, host form, %s" % variant)
        check_whole(run_dev(ctx, c["Z"], stride, cap), expected(c, rows, cap), "M = 3 shared blocks, _dev form, %s" % variant)
        own = reference_rows(c, c["Z"], stride, blocks=(pp, tt, xx))
        got = run_host(ctx, c["Z"], stride, cap, blocks=(pp, tt, xx))
        check_whole(got, expected(c, own, cap), "M = 3 per-row blocks, %s" % variant)
        check_whole(run_host(ctx, c["Z"], stride, cap), expected(c, rows, cap), "the context's own blocks are back, %s" % variant)
        for b in (0, B - 1):                                          # the row run alone, on the device
            alone = run_host(ctx, c["Z"][b:b + 1], stride, cap, blocks=(pp[b:b + 1], tt[b:b + 1], xx[b:b + 1]))
            check_whole(alone, expected(c, own[b:b + 1], cap), "row %d alone, %s" % (b, variant))
        ctx.close()
    assert not np.array_equal(own[1][0]["kp"][0], rows[1][0]["kp"][0]), "the blocks move the gains"
    w_end = rows[0][2]["wq"][3]
    w_first = rows[0][0]["wq"][0]
    print("goddard M = 3: |W| at the last sample %.3e, at the first %.3e (the sweep crossed two nodes)" % (np.abs(w_end).max(), np.abs(w_first).max()))


# ---- 3. the other models -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [15, 16, 17])
def test_double_integrator_sixteen_groups_per_wave(B):
    c = dint_fixed(17)
    stride, cap = 3, 4
    rows = reference_rows(c, c["Z"][:B], stride)
    for variant in VARIANTS:
        ctx = context(c, variant)
        check_whole(run_dev(ctx, c["Z"][:B], stride, cap), expected(c, rows, cap), "dint B %d, _dev form, %s" % (B, variant))
        check_whole(run_host(ctx, c["Z"][:B], stride, cap), expected(c, rows, cap), "dint B %d, host form, %s" % (B, variant))
        ctx.close()


def test_covid19():
    c = covid_m2()
    for stride in (3, 16):
        cap = cap_of(stride)
        rows = reference_rows(c, c["Z"], stride)
        for variant in VARIANTS:
            ctx = context(c, variant)
            check_whole(run_dev(ctx, c["Z"], stride, cap), expected(c, rows, cap), "covid stride %d, _dev form, %s" % (stride, variant))
            check_whole(run_host(ctx, c["Z"], stride, cap), expected(c, rows, cap), "covid stride %d, host form, %s" % (stride, variant))
            ctx.close()


@pytest.mark.parametrize("name", ["osc1d_plugin", "dint_hx_plugin"])
def test_plugins_have_the_entry_with_no_source_change(name):
    c = {"osc1d_plugin": osc1d_plugin, "dint_hx_plugin": dint_hx_plugin}[name]()
    stride, cap = 3, 4
    with hx.entries():                                                # lends fields_reference the H-only models' right-hand sides
        rows = reference_rows(c, c["Z"], stride)
    for variant in VARIANTS:
        ctx = context(c, variant)
        assert ctx.has_gain()
        check_whole(run_dev(ctx, c["Z"], stride, cap), expected(c, rows, cap), "%s, _dev form, %s" % (name, variant))
        check_whole(run_host(ctx, c["Z"], stride, cap), expected(c, rows, cap), "%s, host form, %s" % (name, variant))
        ctx.close()


# ---- 4. edge rows --------------------------------------------------------------------------------------------------------------------

def test_zero_length_segment_and_nan_row():
    c = goddard("mu2=1")
    Z = np.array(c["Z"][:5])
    Z[3, 9] = np.nan                                                  # a NaN costate beside healthy rows
    tt = np.tile(c["prob"].time, (5, 1))
    tt[1, 1] = tt[1, 0]                                               # row 1: a segment without a step
    stride, cap = 3, 4
    rows = reference_rows(c, Z, stride, blocks=(None, tt, None))
    s = rows[1][0]
    assert s["count"] == 1 and np.array_equal(s["psi"][0], np.eye(14)), "no step: Q = 1 and Psi_0 = I"
    assert np.array_equal(s["wq"][0], gr.selector(c["prob"].mode_x[1], 7)), "W = E"
    assert s["info"][0] == 1 and np.all(np.isnan(s["kp"][0])), "the fixed final states leave A_p without a pivot in column 0"
    assert all(i != 0 for i in rows[3][0]["info"]) and all(i == 0 for i in rows[2][0]["info"])
    for variant in VARIANTS:
        ctx = context(c, variant)
        check_whole(run_host(ctx, Z, stride, cap, blocks=(None, tt, None)), expected(c, rows, cap), "edge rows, %s" % variant)
        ctx.close()
    print("edge rows: info of the zero-length row %s, of the NaN row %s" % (rows[1][0]["info"], rows[3][0]["info"]))


# ---- 5. NULL outputs -------------------------------------------------------------------------------------------------------------------

def test_each_optional_output_null_in_turn():
    c = goddard("mu2=1")
    stride, cap = 3, 4
    rows = reference_rows(c, c["Z"], stride)
    ctx = context(c)
    for xq, wq, psi in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        want = expected(c, rows, cap, xq=xq, wq=wq, psi=psi)
        what = "Xq %s Wq %s Psi %s" % (xq, wq, psi)
        check_whole(run_dev(ctx, c["Z"], stride, cap, xq=xq, wq=wq, psi=psi), want, what + ", _dev form")
        check_whole(run_host(ctx, c["Z"], stride, cap, xq=xq, wq=wq, psi=psi), want, what + ", host form")
    ctx.close()


# ---- 6. cross-checks on the device -----------------------------------------------------------------------------------------------------

def test_one_block_per_segment_is_phi_and_samples_are_trace_rows():
    import torch
    c = goddard_m3()
    B, M = len(c["Z"]), 3
    for variant in VARIANTS:
        ctx = context(c, variant)
        one = ctx.gain_batch(c["Z"], stride=16, psi=True)
        f = ctx.fields_batch(c["Z"], cols=fr.ALL, stride=16, cap=4, phi=True)
        assert one["psi"].shape == (B, M, 1, 14, 14) and torch.equal(one["psi"][:, :, 0].view(torch.int64), f["phi"].view(torch.int64)), variant
        ctx.close()
    ctx = context(c, "exact")
    for stride in (3, 1):
        g = ctx.gain_batch(c["Z"], stride=stride)
        rows, count = ctx.trace_batch(c["Z"], stride=stride)
        Q = cap_of(stride)
        assert np.all(g["count"].cpu().numpy() == Q) and np.all(count >= Q)
        assert np.array_equal(g["tq"].cpu().numpy().view(np.uint64), np.ascontiguousarray(rows[:, :, :Q, 0]).view(np.uint64)), "tq, stride %d" % stride
        assert np.array_equal(g["xq"].cpu().numpy().view(np.uint64), np.ascontiguousarray(rows[:, :, :Q, 1:15]).view(np.uint64)), "Xq, stride %d" % stride
    ctx.close()


# ---- 7. refusals: the message, the sentinels, the counters -----------------------------------------------------------------------------

def refused(ctx, code, text, Z, stride, cap, form="dev", blocks=None, null=None):
    """The call fails with `code` and a message holding `text`; the counters stay and, in the _dev form, so does every sentinel."""
    import torch
    from socp_amd import capi
    before = ctx.counters()
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in buffers(len(Z), 3, max(cap, 1), ctx.dim)]
    p = [t.data_ptr() for t in dev]
    if null is not None:
        p[null] = None
    torch.cuda.synchronize()
    with pytest.raises(capi.SocpError) as e:
        if form == "dev":
            ctx.gain_batch_dev(len(Z), dZ.data_ptr(), stride, cap, *p)
        else:
            run_host(ctx, Z, stride, cap, blocks=blocks)
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
    refused(bare, ARG, "no problem set", Z, 3, 4)
    bare.close()
    ctx = context(c)
    refused(ctx, ARG, "stride >= 1", Z, 0, 4)
    refused(ctx, ARG, "cap >= ceil(step_nbr / stride)", Z, 3, 3)
    for k in (0, 1, 2, 3):
        refused(ctx, ARG, "null argument", Z, 3, 4, null=k)
    before = ctx.counters()
    assert ctx.L.socp_gain_batch_dev(ctx.h, -1, None, 3, 4, None, None, None, None, None, None, None) == ARG and "B >= 0" in ctx.L.socp_last_error(ctx.h).decode()
    assert ctx.L.socp_gain_batch_dev(ctx.h, 0, None, 3, 4, None, None, None, None, None, None, None) == 0, "B == 0: SOCP_OK without a launch"
    assert ctx.L.socp_gain_batch(ctx.h, 0, None, 3, 4, None, None, None, None, None, None, None) == 0
    assert ctx.counters() == before
    pp = np.tile(np.concatenate([c["params"], [0.0, 0.0, 0.0]]), (2, 1))
    refused(ctx, ARG, "the parameter stride", Z, 3, 4, form="host", blocks=(pp, None, None))
    ctx.set_integrator(capi.INT_DOPRI5)
    refused(ctx, UNS, "SOCP_INT_DOPRI5", Z, 3, 4)
    ctx.set_integrator(capi.INT_RK4)
    check_whole(run_dev(ctx, Z, 3, 4), expected(c, reference_rows(c, Z, 3), 4), "the context still works")
    ctx.close()
    # a free final time; a free interior time; an interior node with a FIXED and with a FREE component
    p = c["prob"]
    free_tf = context(dict(c, prob=Problem(7, [FIXED, FREE], p.mode_x, p.time, p.xnode)))
    refused(free_tf, UNS, "a free time (node 1)", np.hstack([Z, [[0.26], [0.26]]]), 3, 4)
    free_tf.close()
    m3 = goddard_m3(2)
    q = m3["prob"]
    inner = context(dict(m3, prob=Problem(7, [FIXED, FREE, CONTINUOUS, FIXED], q.mode_x, q.time, q.xnode)))
    refused(inner, UNS, "a free time (node 1)", np.hstack([m3["Z"], [[0.03], [0.03]]]), 3, 4)
    inner.close()
    for mode, comp in ((FIXED, 2), (FREE, 5)):
        mx = np.array(q.mode_x)
        mx[1, comp] = mode
        node = context(dict(m3, prob=Problem(7, q.mode_t, mx, q.time, q.xnode)))
        refused(node, UNS, "a FIXED or FREE state component on an interior node (node 1, component %d)" % comp, m3["Z"], 3, 4)
        node.close()
    # models without the entry: the interceptor (its own ComputeTraj), vtolUAV and lqr1d (no rhs_t trait)
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    from test_gpu_cost_batch import build_vtol
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    Xs, Xf = scenario_state(gamma=1.49)
    iprob, iz = multi_shooting_problem(Oracle(MODEL_INTERCEPTOR), 4, X0=Xs, Xf=Xf)
    ci = capi.Context(capi.MODEL_INTERCEPTOR)
    assert ci.problem_set(iprob.mode_t, iprob.mode_x, iprob.time, iprob.xnode) == iprob.n
    assert not ci.has_gain()
    refused(ci, UNS, "no gain entry", np.ascontiguousarray(iz)[None, :], 3, 400)
    ci.close()
    cv, _, Zv, _ = build_vtol("exact")
    assert not cv.has_gain()
    refused(cv, UNS, "no gain entry", Zv, 3, 400)
    cv.close()
    lq = jc.case("lqr1d")
    cl = context(dict(lq, N=N))
    assert not cl.has_gain()
    refused(cl, UNS, "no gain entry", lq["Z"], 3, 4)
    cl.close()


# ---- 8. the sweep tool -------------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_gain_file_and_record(tmp_path):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "gain")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--gain-out", out, "--gain-stride", "10"],
                         cwd=root, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["gain"]
    assert {"rows", "singular_samples", "kp_norm_median"} <= set(entry)
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and sorted(npz.files) == sorted(["index", "tq", "xq", "kp", "info", "count"])
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0
    assert npz["kp"].shape == (k, 1, 5, 7, 7) and npz["xq"].shape == (k, 1, 5, 14) and np.all(npz["count"] == 5)
    assert entry["singular_samples"] == int((npz["info"] > 0).sum()) and np.all(npz["info"][:, 0, 0] == 0)
    assert entry["kp_norm_median"] > 0
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--gain-out", out], cwd=root,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--gain-out" in bad.stderr
