"""GPU: the batched neighbouring-extremal gains with a FREE final time (socp_gain_free_batch[_dev] / _blocks,
capi.Context.gain_free_batch) against tests/gain_free_reference.py -- the definition restated in Python: blocks on dual numbers with a
dual step and a length column, the bordered backward sweep, the elimination of tests/tangent_reference.py.  Outputs live in
sentinel-filled buffers followed by 64 guard words and are compared WHOLE on integer views (the conventions of
test_gpu_gain_batch.py), so a store past a slab, past count or through a NULL pointer shows.  Every output is bit-equal to the
restatement, in BOTH flavours; NaNs other than the sentinel are compared as NaN.  N = 10 steps: stride 3 gives blocks of 3, 3, 3, 1
steps, stride 1 ten blocks, stride 16 one.  A row's result depends on the row and its blocks alone: a reference is computed once per
distinct row and shared read-only.  The figures the tests print are kept in profiles/gain_free_gpu_tests.txt."""
import numpy as np
import pytest

import gain_free_reference as gf
import gain_reference as gr
import hamiltonian_exact_reference as hx
import jacobi_cases as jc
from test_gpu_jacobi_batch import SENT, SENT_I, DP, IP, sentinel, sentinel_i, views, canon
from test_gpu_gain_batch import context, cap_of, untouched, goddard, dint_fixed, covid_m2, osc1d_plugin, dint_hx_plugin

pytestmark = pytest.mark.gpu
N = 10
VARIANTS = ("exact", "fast")
_ROWS = {}


def freed(c, tfs, mode_t=None):
    """The case with node M's time FREE (or the time modes given): every row gets its own t_f as its last unknown."""
    from oracle.oracle import Problem, FREE
    p = c["prob"]
    mt = list(p.mode_t[:-1]) + [FREE] if mode_t is None else list(mode_t)
    Z = np.asarray(c["Z"], dtype=np.float64)
    tfs = np.resize(np.asarray(tfs, dtype=np.float64), len(Z))
    return dict(c, prob=Problem(p.dim, mt, p.mode_x, p.time, p.xnode), Z=np.hstack([Z, tfs[:, None]]))


def goddard_free(law):
    """test_gpu_gain_batch.goddard(law) with the final time released: nine rows, t_f within 4 % of the nominal 0.264."""
    c = goddard(law)
    return freed(c, float(c["prob"].time[1]) * (1.0 + 0.01 * np.arange(-4, 5)))


# ---- the restatement, one row at a time ----------------------------------------------------------------------------------------

def reference_rows(c, Z, stride, cap=None, blocks=None):
    """rows[b][i] of gain_free_reference.gain_free_row; blocks = (params, time, xnode), any of them None."""
    from oracle.oracle import Problem
    prob = c["prob"]
    model = {"osc1d_exact_jacobian": "osc1d"}.get(c["model"], c["model"])
    pp, tt, xx = blocks if blocks is not None else (None, None, None)
    nP = len(c["params"])
    out = []
    for b, z in enumerate(np.asarray(Z, dtype=np.float64)):
        P = [float(v) for v in (c["params"] if pp is None else pp[b][:nP])]
        sw = tuple(c.get("sw") or (0.0, 0.0)) if pp is None else tuple(float(v) for v in pp[b][nP:nP + 2])
        tl = np.array(prob.time if tt is None else tt[b], dtype=np.float64)
        xn = np.array(prob.xnode if xx is None else xx[b], dtype=np.float64).reshape(prob.M + 1, 2 * prob.dim)
        key = (model, c.get("N", N), stride, cap, tuple(P), sw, tl.tobytes(), xn.tobytes(), z.tobytes(), np.asarray(prob.mode_x).tobytes(),
               tuple(int(m) for m in prob.mode_t))
        if key not in _ROWS:
            _ROWS[key] = gf.gain_free_row(model, P, sw, Problem(prob.dim, prob.mode_t, prob.mode_x, tl, xn), z, c.get("N", N), stride, cap=cap)
        out.append(_ROWS[key])
    return out


def expected(c, rows, cap, xq=True, wq=True, psi=True, length=True):
    return gf.pack(rows, len(rows), c["prob"].M, c["prob"].dim, cap, SENT, SENT_I, xq=xq, wq=wq, psi=psi, length=length)


# ---- the three forms on guarded buffers: each returns the eight WHOLE buffers as integer views, in the order of gf.NAMES ---------

def buffers(B, M, cap, d):
    slots, s = B * M * cap, 2 * d
    return (sentinel(slots), sentinel(slots * (d + 1) * d), sentinel_i(slots), sentinel_i(B * M), sentinel(slots * s), sentinel(slots * (d + 1) * (s + 1)),
            sentinel(slots * s * s), sentinel(slots * s))


def run_host(ctx, Z, stride, cap, xq=True, wq=True, psi=True, length=True, blocks=None):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B = len(Z)
    out = buffers(B, ctx.M, cap, ctx.dim)
    opt = lambda k, on: out[k].ctypes.data_as(DP) if on else None              # noqa: E731
    tail = (stride, cap, out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP), out[2].ctypes.data_as(IP), out[3].ctypes.data_as(IP),
            opt(4, xq), opt(5, wq), opt(6, psi), opt(7, length))
    if blocks is None:
        ctx._chk(ctx.L.socp_gain_free_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in blocks)
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None        # noqa: E731
        ctx._chk(ctx.L.socp_gain_free_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx),
                                                   *tail))
    return views(out)


def run_dev(ctx, Z, stride, cap, xq=True, wq=True, psi=True, length=True):
    import torch
    B = len(Z)
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in buffers(B, ctx.M, cap, ctx.dim)]
    torch.cuda.synchronize()
    opt = lambda k, on: dev[k].data_ptr() if on else None                      # noqa: E731
    ctx.gain_free_batch_dev(B, dZ.data_ptr(), stride, cap, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                            opt(4, xq), opt(5, wq), opt(6, psi), opt(7, length))
    ctx.synchronize()
    torch.cuda.synchronize()
    return views(tuple(t.cpu().numpy() for t in dev))


def check_whole(got, want, what):
    for name, g, w in zip(gf.NAMES, got, want):
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


def both_forms(c, Z, stride, cap, rows, what, variants=VARIANTS):
    want = expected(c, rows, cap)
    for variant in variants:
        ctx = context(c, variant)
        assert ctx.has_gain_free()
        check_whole(run_dev(ctx, Z, stride, cap), want, "%s, _dev form, %s" % (what, variant))
        check_whole(run_host(ctx, Z, stride, cap), want, "%s, host form, %s" % (what, variant))
        ctx.close()


# ---- 1. Goddard, single shooting with a free final time, the three laws: every stride, B and form, both flavours --------------------

@pytest.mark.parametrize("law", ["mu2=1", "mu2=0.2", "mu2=0"])
def test_goddard_free_tf_equals_the_restatement(law):
    c = goddard_free(law)
    ctx = {v: context(c, v) for v in VARIANTS}
    assert ctx["exact"].has_gain_free() and ctx["fast"].has_gain_free()
    for stride in (3, 1, 16):
        cap = cap_of(stride)
        rows = reference_rows(c, c["Z"], stride)
        assert all(r[0]["count"] == cap for r in rows), "ten steps: %d blocks" % cap
        assert all(r[0]["info"][0] == 0 for r in rows), "a costate and final-time correction at t0 reaches the target"
        for B in (4, 5, 8, 9):    # fifteen lanes per block group: four per wave (4, 5); eight lanes per sweep group: eight per wave (8, 9)
            want = expected(c, rows[:B], cap)
            t0, l0 = ctx["exact"].counters()
            check_whole(run_dev(ctx["exact"], c["Z"][:B], stride, cap), want, "%s stride %d B %d, _dev form" % (law, stride, B))
            t1, l1 = ctx["exact"].counters()
            assert (t1 - t0, l1 - l0) == (B * 1 * 15, 3), "B M (S + 1) trajectories and three launches"
            check_whole(run_host(ctx["exact"], c["Z"][:B], stride, cap), want, "%s stride %d B %d, host form" % (law, stride, B))
        check_whole(run_dev(ctx["fast"], c["Z"], stride, cap), want, "%s stride %d, _dev form, throughput flavour" % (law, stride))
        check_whole(run_host(ctx["fast"], c["Z"], stride, cap), want, "%s stride %d, host form, throughput flavour" % (law, stride))
        # a larger cap: the slots at or beyond count keep what the buffers held
        check_whole(run_dev(ctx["exact"], c["Z"], stride, cap + 2), expected(c, rows, cap + 2), "%s stride %d cap + 2" % (law, stride))
    r0 = reference_rows(c, c["Z"][:1], 3)[0][0]
    ke = np.array(r0["ke"][0])
    print("goddard free t_f %s: |K_p(t0)|max = %.6e, |k_t(t0)|max = %.6e, k_t[0] = %.17g, info by sample at stride 3: %s"
          % (law, np.abs(ke[:, :7]).max(), np.abs(ke[:, 7]).max(), ke[0, 7], r0["info"]))
    if law == "mu2=0":
        smooth = reference_rows(dict(goddard_free("mu2=1"), Z=c["Z"]), c["Z"][:1], 3)
        assert not np.array_equal(smooth[0][0]["psi"][0], r0["psi"][0]), "the general-law kernel ran"
    for x in ctx.values():
        x.close()


def test_python_form():
    import torch
    c = goddard_free("mu2=1")
    ctx = context(c)
    r = ctx.gain_free_batch(c["Z"], stride=3, wq=True, psi=True, length=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in r.values())
    assert r["kp"].shape == (9, 1, 4, 7, 7) and r["kt"].shape == (9, 1, 4, 7) and r["wq"].shape == (9, 1, 4, 8, 15) and r["len"].shape == (9, 1, 4, 14)
    want = expected(c, reference_rows(c, c["Z"], 3), 4)
    for key, w in zip(("tq", "ke", "info", "count", "xq", "wq", "psi", "len"), want):
        g = r[key].cpu().numpy()
        assert np.array_equal(canon(g.view(np.uint64)) if g.dtype == np.float64 else g, canon(w.reshape(g.shape))), key
    ke = r["ke"].cpu().numpy()
    assert np.array_equal(r["kp"].cpu().numpy().view(np.uint64), np.ascontiguousarray(ke[..., :7]).view(np.uint64)), "kp: gain_batch's layout"
    assert np.array_equal(r["kt"].cpu().numpy().view(np.uint64), np.ascontiguousarray(ke[..., 7]).view(np.uint64))
    ctx.close()


# ---- 2. M = 3 across segment boundaries (weights 1/3), per-row blocks: each row equals the row run alone ---------------------------

def test_goddard_m3_free_tf_per_row_blocks():
    c = dict(jc.goddard_m3(free_tf=True, B=5, seed=11), N=N)
    prob, B = c["prob"], len(c["Z"])
    pp = np.tile(np.concatenate([c["params"], [0.0227, 0.08]]), (B, 1))
    pp[:, 4] = 1.0 - 0.1 * np.arange(B)                              # u_max of each row; no smooth-law promise given: the general-law kernel
    tt = np.tile(prob.time, (B, 1))
    tt[:, 0] = 0.001 * np.arange(B)                                  # each row's own t0; node M's entry is not read (FREE)
    xx = np.tile(np.asarray(prob.xnode).ravel(), (B, 1))
    xx[:, 3 * 14] += 0.001 * np.arange(B)
    stride, cap = 3, 4
    rows = reference_rows(c, c["Z"], stride)
    own = reference_rows(c, c["Z"], stride, blocks=(pp, tt, xx))
    both_forms(c, c["Z"], stride, cap, rows, "M = 3 shared blocks")
    for variant in VARIANTS:
        ctx = context(c, variant)
        got = run_host(ctx, c["Z"], stride, cap, blocks=(pp, tt, xx))
        check_whole(got, expected(c, own, cap), "M = 3 per-row blocks, %s" % variant)
        check_whole(run_host(ctx, c["Z"], stride, cap), expected(c, rows, cap), "the context's own blocks are back, %s" % variant)
        for b in (0, B - 1):                                          # the row run alone, on the device
            alone = run_host(ctx, c["Z"][b:b + 1], stride, cap, blocks=(pp[b:b + 1], tt[b:b + 1], xx[b:b + 1]))
            check_whole(alone, expected(c, own[b:b + 1], cap), "row %d alone, %s" % (b, variant))
        ctx.close()
    assert not np.array_equal(own[1][0]["ke"][0], rows[1][0]["ke"][0]), "the blocks move the gains"
    third = gf.gain_free_row("goddard", [float(v) for v in c["params"]], (0.0, 0.0), prob, c["Z"][0], N, stride, mutate=("w_one",))
    assert not np.array_equal(third[0]["wq"][0], rows[0][0]["wq"][0]), "the weights 1/3 are in the border"
    print("goddard M = 3 free t_f: wtau at the last sample %s, at the first %s; info %s"
          % (rows[0][2]["wq"][3][:, -1], rows[0][0]["wq"][0][:, -1], [list(s["info"]) for s in rows[0]]))


def test_m2_with_a_fixed_interior_time_skips_the_first_segment():
    """Times [FIXED, FIXED, FREE]: segment 0's length does not depend on t_f, w_0 = 0 and the border is not touched there -- a NaN in
    l of segment 0 could not reach wtau.  covid19 keeps t_f fixed upstream: a made-up free-t_f problem."""
    from oracle.oracle import FIXED, FREE
    c = freed(covid_m2(), [10.0, 9.5, 10.5], mode_t=[FIXED, FIXED, FREE])
    for stride in (3, 16):
        cap = cap_of(stride)
        rows = reference_rows(c, c["Z"], stride)
        last = rows[0][1]["wq"][0][:, -1]
        assert np.array_equal(rows[0][0]["wq"][0][:, -1], last) and np.any(last != 0), "wtau stays through segment 0"
        both_forms(c, c["Z"], stride, cap, rows, "covid M = 2 [FIXED, FIXED, FREE] stride %d" % stride)


# ---- 3. the other models -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [9, 10])
def test_double_integrator_nine_sweep_groups_per_wave(B):
    """Seven lanes per sweep group, nine groups per wave (one idle lane); thirteen lanes per block group.  The later rows saturate."""
    c = freed(dint_fixed(10), 3.0 * (1.0 + 0.03 * np.arange(10)))
    stride, cap = 3, 4
    rows = reference_rows(c, c["Z"][:B], stride)
    both_forms(c, c["Z"][:B], stride, cap, rows, "dint free t_f B %d" % B)
    if B == 10:
        print("dint free t_f: info by row %s" % [r[0]["info"] for r in rows])


@pytest.mark.parametrize("name", ["osc1d_plugin", "dint_hx_plugin"])
def test_plugins_have_the_entry_with_no_source_change(name):
    if name == "osc1d_plugin":
        c = freed(osc1d_plugin(), 2.0 + 0.1 * np.arange(5))          # M = 2: [FIXED, FIXED, FREE]
    else:
        c = freed(dint_hx_plugin(), 3.0 + 0.1 * np.arange(5))
    stride, cap = 3, 4
    with hx.entries():                                                # lends the references the H-only models' texts
        rows = reference_rows(c, c["Z"], stride)
    both_forms(c, c["Z"], stride, cap, rows, name)


def test_a_plugin_with_rhs_t_only_has_gain_but_not_gain_free():
    from socp_amd import capi
    from test_gpu_jacobi_batch import plugin_path
    capi.plugin_load(plugin_path("osc1d_fields"))
    ctx = capi.Context(1004, nparams=1)
    assert ctx.has_gain() and not ctx.has_gain_free()
    ctx.close()


# ---- 4. edge rows --------------------------------------------------------------------------------------------------------------------

def test_zero_length_row_and_nan_row():
    c = goddard_free("mu2=1")
    Z = np.array(c["Z"][:5])
    Z[3, 9] = np.nan                                                  # a NaN costate beside healthy rows
    Z[1, 14] = float(c["prob"].time[0])                               # row 1: t_f = t0, a segment without a step
    stride, cap = 3, 4
    rows = reference_rows(c, Z, stride)
    s = rows[1][0]
    assert s["count"] == 1 and np.array_equal(s["psi"][0], np.eye(14)) and np.all(s["len"][0] == 0), "no step: Q = 1, Psi_0 = I, l_0 = 0"
    assert np.array_equal(s["wq"][0][:7, :14], gr.selector(c["prob"].mode_x[1], 7)) and np.all(s["wq"][0][:, 14] == 0), "W = E, wtau = 0"
    assert s["info"][0] != 0 and np.all(np.isnan(s["ke"][0])), "singular"
    assert all(i != 0 for i in rows[3][0]["info"]) and all(i == 0 for i in rows[2][0]["info"][:1])
    both_forms(c, Z, stride, cap, rows, "edge rows")
    print("edge rows: info of the zero-length row %s, of the NaN row %s" % (rows[1][0]["info"], rows[3][0]["info"]))


# ---- 5. NULL outputs and cap -----------------------------------------------------------------------------------------------------------

def test_each_optional_output_null_in_turn():
    c = goddard_free("mu2=1")
    stride, cap = 3, 4
    rows = reference_rows(c, c["Z"], stride)
    ctx = context(c)
    for k in range(5):
        on = [k != j for j in range(4)] if k < 4 else [False] * 4
        want = expected(c, rows, cap, *on)
        what = "Xq %s Wq %s Psi %s Len %s" % tuple(on)
        check_whole(run_dev(ctx, c["Z"], stride, cap, *on), want, what + ", _dev form")
        check_whole(run_host(ctx, c["Z"], stride, cap, *on), want, what + ", host form")
    ctx.close()


def test_cap_overflow_leaves_the_chain_incomplete():
    """A row whose loop counts a block beyond cap cannot be made from outside (cap < ceil(step_nbr / stride) is refused and the loop
    takes step_nbr steps), so the rule is checked where it lives: the restatement with cap one short starts W from NaN, and the call
    refuses that cap."""
    from socp_amd import capi
    c = goddard_free("mu2=1")
    short = reference_rows(c, c["Z"][:1], 3, cap=3)[0][0]
    assert short["count"] == 4 and all(i != 0 for i in short["info"][:3]) and np.all(np.isnan(short["wq"][2][:, 7:14]))
    ctx = context(c)
    refused(ctx, capi.ERR_ARG, "cap >= ceil(step_nbr / stride)", c["Z"][:2], 3, 3)
    ctx.close()


# ---- 6. cross-checks on the device -----------------------------------------------------------------------------------------------------

def test_blocks_are_gain_batch_blocks_of_the_fixed_time_twin_as_numbers():
    """Psi, tq, Xq against socp_gain_batch on the twin problem with t_f FIXED at the row's value (per-row time blocks): equal AS NUMBERS
    -- the dual step with a zero derivative part adds products with zero, which may turn a -0.0 into +0.0."""
    c = goddard_free("mu2=1")
    B = len(c["Z"])
    twin = goddard("mu2=1")
    tt = np.tile(twin["prob"].time, (B, 1))
    tt[:, 1] = c["Z"][:, 14]
    for stride in (3, 16):
        ctx = context(c)
        g = ctx.gain_free_batch(c["Z"], stride=stride, psi=True)
        ctx.close()
        ctw = context(twin)
        f = ctw.gain_batch(c["Z"][:, :14], stride=stride, psi=True, blocks=(None, tt, None))
        ctw.close()
        for key in ("tq", "xq", "psi", "count"):
            assert np.array_equal(g[key].cpu().numpy(), f[key].cpu().numpy()), (key, stride)


def test_one_block_per_segment_is_the_exact_jacobian():
    """M = 1, stride >= the step count: the final rows of socp_exact_jacobian_batch are rows of Psi_0 (state block) and of l_0 (t_f
    column) bit for bit."""
    c = goddard_free("mu2=1")
    B, D, S, n = len(c["Z"]), 7, 14, 15
    for variant in VARIANTS:
        ctx = context(c, variant)
        g = ctx.gain_free_batch(c["Z"], stride=16, psi=True, length=True)
        J = ctx.exact_jacobian_batch(c["Z"]).cpu().numpy().reshape(B, n, n).transpose(0, 2, 1)                  # [b][row][col]
        psi, ln = g["psi"].cpu().numpy()[:, 0, 0], g["len"].cpu().numpy()[:, 0, 0]
        pick = [D + j if int(c["prob"].mode_x[1][j]) == 1 else j for j in range(D)]
        bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)                              # noqa: E731
        assert np.array_equal(bits(psi[:, pick, :]), bits(J[:, D:2 * D, :S])), variant
        assert np.array_equal(bits(ln[:, pick]), bits(J[:, D:2 * D, n - 1])), variant
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
            ctx.gain_free_batch_dev(len(Z), dZ.data_ptr(), stride, cap, *p)
        else:
            run_host(ctx, Z, stride, cap, blocks=blocks)
    torch.cuda.synchronize()
    assert e.value.code == code and text in str(e.value), (code, text, str(e.value))
    assert ctx.counters() == before, "an error leaves the counters unchanged"
    assert untouched(views(tuple(t.cpu().numpy() for t in dev))), "an error writes nothing"


def test_refusals():
    from socp_amd import capi
    from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
    c = goddard_free("mu2=1")
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
    nulls = (None,) * 8
    assert ctx.L.socp_gain_free_batch_dev(ctx.h, -1, None, 3, 4, *nulls) == ARG and "B >= 0" in ctx.L.socp_last_error(ctx.h).decode()
    assert ctx.L.socp_gain_free_batch_dev(ctx.h, 0, None, 3, 4, *nulls) == 0, "B == 0: SOCP_OK without a launch"
    assert ctx.L.socp_gain_free_batch(ctx.h, 0, None, 3, 4, *nulls) == 0
    assert ctx.counters() == before
    pp = np.tile(np.concatenate([c["params"], [0.0, 0.0, 0.0]]), (2, 1))
    refused(ctx, ARG, "the parameter stride", Z, 3, 4, form="host", blocks=(pp, None, None))
    ctx.set_integrator(capi.INT_DOPRI5)
    refused(ctx, UNS, "SOCP_INT_DOPRI5", Z, 3, 4)
    ctx.set_integrator(capi.INT_RK4)
    check_whole(run_dev(ctx, Z, 3, 4), expected(c, reference_rows(c, Z, 3), 4), "the context still works")
    ctx.close()
    # a fixed final time; a free time before the final node; an interior node with a FIXED and with a FREE component
    fixed = goddard("mu2=1")
    ctf = context(fixed)
    refused(ctf, UNS, "use socp_gain_batch", fixed["Z"][:2], 3, 4)
    ctf.close()
    m3 = dict(jc.goddard_m3(free_tf=True, B=2, seed=11), N=N)
    q = m3["prob"]
    inner = context(dict(m3, prob=Problem(7, [FIXED, FREE, CONTINUOUS, FREE], q.mode_x, q.time, q.xnode)))
    refused(inner, UNS, "a free time before the final node (node 1)", np.hstack([m3["Z"][:, :42], [[0.03, 0.09], [0.03, 0.09]]]), 3, 4)
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
    assert not ci.has_gain_free()
    refused(ci, UNS, "no gain_free entry", np.ascontiguousarray(iz)[None, :], 3, 400)
    ci.close()
    cv, _, Zv, _ = build_vtol("exact")
    assert not cv.has_gain_free()
    refused(cv, UNS, "no gain_free entry", Zv, 3, 400)
    cv.close()
    lq = jc.case("lqr1d")
    cl = context(dict(lq, N=N))
    assert not cl.has_gain_free()
    refused(cl, UNS, "no gain_free entry", lq["Z"], 3, 4)
    cl.close()


# ---- 8. the sweep tool -------------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_kt_for_multiple_shooting(tmp_path):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "gain")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--segments", "2", "--gain-out", out,
                          "--gain-stride", "10"], cwd=root, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["gain"]
    assert entry["with_free_tf"] is True and {"rows", "singular_samples", "kp_norm_median"} <= set(entry)
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and sorted(npz.files) == sorted(["index", "tq", "xq", "kp", "kt", "info", "count"])
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0
    assert npz["kp"].shape == (k, 2, 5, 7, 7) and npz["kt"].shape == (k, 2, 5, 7) and npz["xq"].shape == (k, 2, 5, 14) and np.all(npz["count"] == 5)
    assert entry["singular_samples"] == int((npz["info"] > 0).sum()) and np.all(npz["info"][:, 0, 0] == 0)
    assert entry["kp_norm_median"] > 0 and np.all(np.isfinite(npz["kt"][:, 0, 0]))
