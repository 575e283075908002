"""GPU: socp_newton_batch[_dev] / _blocks (capi.Context.newton_batch) against tests/newton_reference.py -- the rounds of
include/socp_hip.h ("Polishing a table of roots") restated in numpy on the CPU oracle and on exact_jacobian_reference.  Outputs
live in sentinel-filled buffers followed by 64 guard words and are compared WHOLE on integer views (the conventions of
test_gpu_branch_batch.py); the workspace is followed by a guard too.  Reference-order flavour: every output buffer bit-equal to the
restatement (a NaN equals any NaN).  Throughput flavour: the statuses where the reference-order margins are clear, and the CPU
oracle's residual at the polished rows.  N = 50 steps.  A reference is computed once and shared read-only
(profiles/newton_gpu_tests.txt keeps the figures).  Without the feature every test fails at the missing symbol."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import newton_cases as nc
import newton_reference as nr
from test_gpu_branch_batch import SENT, SENT_I, GUARD, DP, IP, sentinel, sentinel_i, up, plugin_path, same_doubles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = nc.N
PLUGIN_IDS = {"osc1d": 1002, "osc1d_exact_jacobian": 1005}
DOUBLES, INTS = ("z", "f", "rnorm", "dnorm", "rhist"), ("iters", "nhalf", "status")
ORDER = ("z", "f", "rnorm", "dnorm", "iters", "nhalf", "status", "rhist")      # the C argument order
OPTIONAL = ("f", "rhist")


def sizes(B, n, rounds):
    return dict(z=B * n, f=B * n, rnorm=B, dnorm=B, iters=B, nhalf=B, status=B, rhist=B * (rounds + 1))


def fresh(B, n, rounds):
    sz = sizes(B, n, rounds)
    return {k: (sentinel(sz[k]) if k in DOUBLES else sentinel_i(sz[k])) for k in ORDER}


def both(**kw):
    """(the restatement's options, the device's) from one set of keywords."""
    from socp_amd import capi
    return nr.options(**kw), capi.newton_options(**kw)


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


class DevBlocks:
    """Per-row blocks (params, time, xnode; any of them None) uploaded and in force inside the with-block."""

    def __init__(self, ctx, blocks):
        self.ctx, self.blocks = ctx, blocks

    def __enter__(self):
        if self.blocks is not None:
            self.keep = [up(np.ascontiguousarray(a)) if a is not None else None for a in self.blocks]
            ptr = [t.data_ptr() if t is not None else None for t in self.keep]
            stride = self.blocks[0].shape[1] if self.blocks[0] is not None else 0
            self.ctx._chk(self.ctx.L.socp_problem_set_blocks_dev(self.ctx.h, ptr[0], stride, ptr[1], ptr[2]))
        return self

    def __exit__(self, *exc):
        if self.blocks is not None:
            self.ctx.L.socp_problem_set_blocks_dev(self.ctx.h, None, 0, None, None)


def views(bufs):
    return {k: (np.asarray(v).view(np.uint64) if k in DOUBLES else np.asarray(v)) for k, v in bufs.items()}


def run_dev(ctx, Z, opts, blocks=None, null=()):
    """The _dev form on guarded device buffers: the WHOLE buffers back as integer views."""
    import torch
    Z = np.ascontiguousarray(Z)
    B, n = len(Z), ctx.n
    dev = {k: up(v) for k, v in fresh(B, n, opts.rounds).items()}
    dZ = up(Z)
    wb = ctx.newton_work_bytes(B, opts)
    assert wb > 0 and wb % 8 == 0
    work = up(sentinel(wb // 8))
    with DevBlocks(ctx, blocks):
        torch.cuda.synchronize()
        ctx.newton_batch_dev(B, dZ.data_ptr(), opts, work.data_ptr(), wb, *(dev[k].data_ptr() if k not in null else None for k in ORDER))
        ctx.synchronize()
        torch.cuda.synchronize()
    assert np.all(work.cpu().numpy().view(np.uint64)[wb // 8:] == np.uint64(SENT)), "guard words behind the workspace were written"
    return views({k: v.cpu().numpy() for k, v in dev.items()})


def run_host(ctx, Z, opts, blocks=None, blocks_form=False, null=()):
    Z = np.ascontiguousarray(Z)
    B, n = len(Z), ctx.n
    out = fresh(B, n, opts.rounds)
    tail = (C.byref(opts),) + tuple(out[k].ctypes.data_as(DP if k in DOUBLES else IP) if k not in null else None for k in ORDER)
    if blocks_form:
        pp, tt, xx = (np.ascontiguousarray(a) if a is not None else None for a in blocks)
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None        # noqa: E731
        ctx._chk(ctx.L.socp_newton_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx), *tail))
    else:
        with DevBlocks(ctx, blocks):
            ctx._chk(ctx.L.socp_newton_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    return views(out)


def check_whole(got, ref, what, null=()):
    for name in ORDER:
        g, fill = got[name], (np.uint64(SENT) if name in DOUBLES else SENT_I)
        if name in null:
            assert np.all(g == fill), "%s: %s was written although its pointer was NULL" % (what, name)
            continue
        w = np.ascontiguousarray(ref[name]).ravel()
        assert g.size == w.size + GUARD, (what, name, g.size, w.size)
        assert np.all(g[w.size:] == fill), "%s: guard words behind %s were written" % (what, name)
        ok = same_doubles(g[:w.size], w) if name in DOUBLES else g[:w.size] == w
        bad = np.argwhere(~ok).ravel()
        assert len(bad) == 0, (what, name, "%d differ, first flat indices:" % len(bad), bad[:5].tolist(),
                               g[:w.size][bad[:5]].view(np.float64 if name in DOUBLES else np.int32), w[bad[:5]])


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ORDER)


def reference(c, Z, ropts, blocks=None, own=None):
    pp, tt, xx = blocks if blocks is not None else (None, None, None)
    model = "osc1d" if c["model"] == "osc1d_exact_jacobian" else c["model"]
    return nr.newton_reference(model, c.get("o"), c["prob"], c["nparams"], c["N"], Z, ropts, params=pp, time=tt, xnode=xx, own=own)


def live_per_round(ref, rounds):
    return [int(np.sum(ref["rounds_used"] > r)) for r in range(rounds)]


def host_counts(ctx, ref, B, opts, jac_traj, jac_launches=1):
    """(trajectories, launches) the host forms add: the start, then per round the compaction and -- on the live slots -- the rest."""
    traj, launches = B * ctx.M, 2
    for live in live_per_round(ref, opts.rounds):
        launches += 3
        if live == 0:
            break
        traj += live * (jac_traj + opts.trials * ctx.M)
        launches += 5 + jac_launches
    return traj, launches


# ---- 1. the mixed batch: all six statuses, the three forms, the optional outputs, the counters ---------------------------------------

def test_mixed_batch_in_all_forms_bit_for_bit():
    """Goddard M = 1 (n = 14: four eliminations per workgroup), B = 70 (two wavefronts of rows in the compaction's first workgroup),
    every row with its own node times; rows leave in rounds 0, 1, 2 and 3, so every round compacts another list."""
    m = nc.mixed()
    ref, Z, blocks = m["ref"], m["Z"], (None, m["time"], None)
    assert set(ref["status"].tolist()) == set(range(6))
    print("mixed: rows per status %s, live rows per round %s" % (np.bincount(ref["status"], minlength=6).tolist(), live_per_round(ref, 3)))
    ropts, dopts = both(**nc.MIXED)
    ctx = context(m)
    assert ctx.n == 14
    B, M, S = len(Z), ctx.M, ctx.s
    t0, l0 = ctx.counters()
    dev = run_dev(ctx, Z, dopts, blocks=blocks)
    t1, l1 = ctx.counters()
    check_whole(dev, ref, "mixed, _dev form")
    assert l1 - l0 == 2 + 9 * 3 and t1 - t0 == B * M + 3 * (B * M * (S + 1) + B * 4 * M), "the _dev form runs every round on all B slots"
    host = run_host(ctx, Z, dopts, blocks=blocks)
    t2, l2 = ctx.counters()
    check_whole(host, ref, "mixed, host form")
    assert (t2 - t1, l2 - l1) == host_counts(ctx, ref, B, dopts, M * (S + 1)), "the host form runs every round on the live slots only"
    check_whole(run_host(ctx, Z, dopts, blocks=blocks, blocks_form=True), ref, "mixed, _blocks form")
    assert same_bits(dev, host)
    check_whole(run_dev(ctx, Z, dopts, blocks=blocks, null=OPTIONAL), ref, "mixed, NULL Fout and rhist", null=OPTIONAL)
    check_whole(run_host(ctx, Z, dopts, blocks=blocks, null=OPTIONAL), ref, "mixed host, NULL Fout and rhist", null=OPTIONAL)
    # the shared node times are back: the last row is no longer flat
    shared = run_host(ctx, Z[69:], dopts)
    assert shared["status"][0] == nr.CONVERGED
    # the Python form
    r = ctx.newton_batch(Z, dopts, time=m["time"])
    for k in ORDER:
        want = np.ascontiguousarray(ref[k]).ravel()
        got = np.ascontiguousarray(r[k]).ravel()
        assert np.all(same_doubles(got.view(np.uint64), want)) if k in DOUBLES else np.array_equal(got, want), k
    ctx.close()


# ---- 2. the other models and structures ---------------------------------------------------------------------------------------------------

def goddard_m3(law):
    """M = 3 with a free t_f (n = 43: one elimination per workgroup), 2 rows whose costates are 1 % off: far from a root, so the
    halving works; law "general": mu2 = 0 with both switching times inside a segment."""
    def build():
        import jacobi_cases as jc
        c = dict(jc.goddard_m3(B=2, seed=9), N=N, nparams=8)
        o = jc.goddard_oracle(N)
        P = np.array(c["params"], dtype=np.float64)
        sw = None
        if law == "general":
            P[6], sw = 0.0, (0.02, 0.05)
            o.set_switching(sw)
        o.set_params(P)
        c.update(o=o, params=P, sw=sw)
        c["ref"] = reference(c, c["Z"], nr.options(jac=2, ftol=1e-9, trials=6, rounds=2))
        return c
    return nc.cached(("gpu-newton-m3", law), build)


@pytest.mark.parametrize("law", ["smooth", "general"])
def test_goddard_three_segments_free_tf(law):
    c = goddard_m3(law)
    ref = c["ref"]
    print("goddard M = 3, %s law: status %s iters %s nhalf %s rnorm %s" % (law, ref["status"], ref["iters"], ref["nhalf"], ref["rnorm"]))
    ctx = context(c)
    assert ctx.n == 43
    dopts = both(jac=2, ftol=1e-9, trials=6, rounds=2)[1]
    check_whole(run_dev(ctx, c["Z"], dopts), ref, "goddard M = 3 %s, _dev form" % law)
    check_whole(run_host(ctx, c["Z"], dopts), ref, "goddard M = 3 %s, host form" % law)
    ctx.close()


def dint_rows():
    c = nc.dint()
    Z = np.stack([c["root"]] + [nc.perturbed(c["root"], 1e-3, s) for s in (1, 2, 3)] + [nc.perturbed(c["root"], 3e-2, 4)])
    return c, Z


DINT = dict(ftol=1e-12, trials=4, rounds=6)


def dint_ref(jac):
    return nc.cached(("gpu-newton-dint", jac), lambda: reference(*dint_rows(), nr.options(**dict(DINT, jac=jac))))


@pytest.mark.parametrize("jac", [0, 1, 2])
def test_dint_with_the_three_jacobians(jac):
    """n = 13; the variational Jacobian takes three launches."""
    c, Z = dint_rows()
    ref = dint_ref(jac)
    print("dint jac %d: status %s iters %s nhalf %s rnorm %s" % (jac, ref["status"], ref["iters"], ref["nhalf"], ref["rnorm"]))
    assert ref["status"][0] == nr.CONVERGED and ref["iters"][0] == 0 and np.all(ref["status"][1:4] == nr.CONVERGED)
    ctx = context(c)
    assert ctx.n == 13
    dopts = both(**dict(DINT, jac=jac))[1]
    t0, l0 = ctx.counters()
    check_whole(run_host(ctx, Z, dopts), ref, "dint jac %d, host form" % jac)
    t1, l1 = ctx.counters()
    z, F = np.ascontiguousarray(Z[0]), ctx.residual(Z[0])
    ta, _ = ctx.counters()
    ctx.fd_jacobian(z, F, dedup=True)
    T_dedup = ctx.counters()[0] - ta
    jac_traj, jac_launches = {0: (T_dedup, 1), 1: (ctx.M, 3), 2: (ctx.M * (ctx.s + 1), 1)}[jac]
    assert (t1 - t0, l1 - l0) == host_counts(ctx, ref, len(Z), dopts, jac_traj, jac_launches)
    check_whole(run_dev(ctx, Z, dopts), ref, "dint jac %d, _dev form" % jac)
    ctx.close()


def covid_case():
    def build():
        from oracle.oracle import Oracle, MODEL_COVID
        from test_gpu_exact_jacobian import covid_m2
        c = dict(covid_m2(), N=N, nparams=8)
        c["o"] = Oracle(MODEL_COVID, step_nbr=N)
        c["ref"] = reference(c, c["Z"], nr.options(jac=2, ftol=1e-9, trials=6, rounds=2))
        return c
    return nc.cached("gpu-newton-covid", build)


def test_covid():
    c = covid_case()
    ref = c["ref"]
    print("covid19: status %s iters %s nhalf %s rnorm %s" % (ref["status"], ref["iters"], ref["nhalf"], ref["rnorm"]))
    ctx = context(c)
    dopts = both(jac=2, ftol=1e-9, trials=6, rounds=2)[1]
    check_whole(run_dev(ctx, c["Z"], dopts), ref, "covid19, _dev form")
    check_whole(run_host(ctx, c["Z"], dopts), ref, "covid19, host form")
    ctx.close()


def osc1d_case(model):
    """The structure of test_gpu_exact_jacobian.osc1d_plugin (M = 2, a FREE interior time and a FREE t_f, n = 6); no oracle: the
    residual is the value part of exact_jacobian_reference, the forward differences are newton_reference.fd_jacobian's."""
    def build():
        from test_gpu_exact_jacobian import osc1d_plugin
        c = dict(osc1d_plugin(), model=model, N=N, nparams=1, o=None)
        opts = nr.options(jac=2 if model == "osc1d_exact_jacobian" else 0, ftol=1e-12, trials=4, rounds=4)
        c["ref"] = reference(c, c["Z"], opts, own=np.array([4.0, 0.0, 0.0]))
        c["opts"] = opts
        return c
    return nc.cached(("gpu-newton-osc1d", model), build)


@pytest.mark.parametrize("model", ["osc1d_exact_jacobian", "osc1d"])
def test_plugins(model):
    """A plugin with the traits takes jac = 2; one without them takes jac = 0 and is refused jac = 2."""
    from socp_amd import capi
    c = osc1d_case(model)
    ref = c["ref"]
    print("%s: status %s iters %s nhalf %s rnorm %s" % (model, ref["status"], ref["iters"], ref["nhalf"], ref["rnorm"]))
    ctx = context(c)
    dopts = capi.newton_options(**c["opts"])
    check_whole(run_dev(ctx, c["Z"], dopts), ref, model + ", _dev form")
    check_whole(run_host(ctx, c["Z"], dopts), ref, model + ", host form")
    if model == "osc1d":
        assert not ctx.has_exact_jacobian()
        before = ctx.counters()
        out = fresh(len(c["Z"]), ctx.n, 4)
        Z = np.ascontiguousarray(c["Z"])
        o2 = capi.newton_options(**dict(c["opts"], jac=2))
        rc = ctx.L.socp_newton_batch(ctx.h, len(Z), Z.ctypes.data_as(DP), C.byref(o2), *(out[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER))
        assert rc == capi.ERR_UNSUPPORTED and "no exact_jacobian entry" in ctx.L.socp_last_error(ctx.h).decode() and ctx.counters() == before
        assert all(np.all(v == (np.uint64(SENT) if k in DOUBLES else SENT_I)) for k, v in views(out).items())
    ctx.close()


# ---- 3. batch sizes, isolation, per-row blocks, rounds beyond the last live row -----------------------------------------------------------

@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_batch_sizes_each_row_as_if_alone(B):
    """The restatement computes every row alone, so bit equality at every B is "each row equals the row run alone"."""
    c, rows = dint_rows()
    Z = rows[(np.arange(B) * 3 + 1) % len(rows)]
    ropts, dopts = both(**dict(DINT, jac=0))
    ref = reference(c, Z, ropts)
    ctx = context(c)
    got = run_dev(ctx, Z, dopts)
    check_whole(got, ref, "B = %d, _dev form" % B)
    assert same_bits(got, run_host(ctx, Z, dopts)), "host form"
    if B == 65:
        # one unfinished row among rows that finish at the start: the list holds that row alone from round 0 on
        for at in (0, 17, 64):
            Zq = np.tile(rows[0], (B, 1))
            Zq[at] = rows[4]
            one = run_dev(ctx, Zq, dopts)
            check_whole(one, reference(c, Zq, ropts), "the only unfinished row is row %d" % at)
            alone = run_dev(ctx, rows[4:5], dopts)
            n, R1 = ctx.n, dopts.rounds + 1
            assert np.array_equal(one["z"][at * n:(at + 1) * n], alone["z"][:n]) and np.array_equal(one["rhist"][at * R1:(at + 1) * R1], alone["rhist"][:R1])
            assert one["status"][at] == alone["status"][0] and one["iters"][at] == alone["iters"][0] >= 2
    ctx.close()


def kd_blocks():
    """Goddard M = 1 with 70 distinct KD, jac = 0: every row polishes the root of its own parameter block."""
    def build():
        c = nc.goddard(1.0)
        B = 70
        pp = np.tile(np.concatenate([c["params"], [0.0, 0.0]]), (B, 1))
        pp[:, 2] = 310.0 * (1.0 + 1e-10 * np.arange(B))
        Z = np.tile(c["root"], (B, 1))
        opts = nr.options(jac=0, ftol=1e-11, trials=4, rounds=6)
        ref = reference(c, Z, opts, blocks=(pp, None, None))
        return dict(c, Z=Z, pp=pp, ref=ref, opts=opts)
    return nc.cached("gpu-newton-kd", build)


def test_seventy_rows_with_their_own_kd():
    from socp_amd import capi
    c = kd_blocks()
    ref, Z, blocks = c["ref"], c["Z"], (c["pp"], None, None)
    print("70 KD: rows per status %s, iters %s, rnorm max %.2e, start rnorm max %.2e" % (np.bincount(ref["status"], minlength=6).tolist(),
                                                                                     np.bincount(ref["iters"]).tolist(), ref["rnorm"].max(), ref["rhist"][:, 0].max()))
    assert ref["status"][0] == nr.CONVERGED and ref["iters"][0] == 0 and np.sum(ref["iters"] > 0) >= 60 and len(np.unique(ref["z"][:, 7])) >= 60
    dopts = capi.newton_options(**c["opts"])
    ctx = context(c)
    got = run_host(ctx, Z, dopts, blocks=blocks, blocks_form=True)
    check_whole(got, ref, "70 KD, _blocks form")
    assert same_bits(got, run_dev(ctx, Z, dopts, blocks=blocks)), "_dev form"
    n = ctx.n
    for b in (0, 37, 69):
        alone = run_dev(ctx, Z[b:b + 1], dopts, blocks=(c["pp"][b:b + 1], None, None))
        assert np.array_equal(alone["z"][:n], got["z"][b * n:(b + 1) * n]) and alone["status"][0] == got["status"][b], b
    ctx.close()


def test_rounds_beyond_the_last_live_row_leave_the_outputs_alone():
    c, Z = dint_rows()
    Z = Z[:4]
    ropts, dopts = both(**dict(DINT, jac=0, rounds=12))
    ref = reference(c, Z, ropts)
    used = int(ref["rounds_used"].max())
    assert np.all(ref["status"] == nr.CONVERGED) and used <= 5
    ctx = context(c)
    t0, l0 = ctx.counters()
    dev = run_dev(ctx, Z, dopts)                                   # twelve rounds, at least seven of them with a live count of 0
    t1, l1 = ctx.counters()
    check_whole(dev, ref, "_dev form, 12 rounds")
    assert l1 - l0 == 2 + 9 * 12
    host = run_host(ctx, Z, dopts)
    t2, l2 = ctx.counters()
    assert same_bits(dev, host) and l2 - l1 == 2 + 9 * used + 3, "the host form stops at the first live count of 0"
    ctx.close()


# ---- 4. throughput flavour ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard", "dint"])
def test_fast_flavour_reaches_the_same_roots(name):
    """Rows whose reference-order run converges with a clear margin (final rn <= ftol / 4) reach CONVERGED in the throughput flavour
    too, and for CONVERGED rows the CPU oracle's ||F(Zout)||inf <= ftol + 10 x the deviation of this context's residual launch from
    the oracle on the same rows (measured here; the margin socp_branch_batch's test uses)."""
    if name == "goddard":
        c = nc.goddard(1.0)
        Z = np.stack([c["root"]] + [nc.perturbed(c["root"], 1e-7, s) for s in (1, 2, 3)])
        kw = dict(jac=2, ftol=1e-10, trials=4, rounds=8)
    else:
        c, Z = dint_rows()
        kw = dict(DINT, jac=2, ftol=1e-11)
    ropts, dopts = both(**kw)
    ref = reference(c, Z, ropts)
    clear = (ref["status"] == nr.CONVERGED) & (ref["rnorm"] <= kw["ftol"] / 4)
    assert clear.sum() >= 3
    fast = context(c, "fast")
    r = fast.newton_batch(Z, dopts)
    assert np.all(r["status"][clear] == nr.CONVERGED), (r["status"], ref["status"])
    done = r["status"] == nr.CONVERGED
    Fdev = fast.residual_batch(np.ascontiguousarray(r["z"][done]))
    Forc = np.array([c["o"].residual(c["prob"], np.ascontiguousarray(z)) for z in r["z"][done]])
    deviation = float(np.max(np.abs(Fdev - Forc)))
    worst = float(np.max(np.abs(Forc)))
    print("fast %s: statuses %s (reference order %s); oracle ||F(Zout)||inf max %.3e; bound ftol %.0e + 10 x %.3e (deviation of the residual launch)"
          % (name, r["status"].tolist(), ref["status"].tolist(), worst, kw["ftol"], deviation))
    assert np.array_equal(np.max(np.abs(Fdev), axis=1), r["rnorm"][done]), "rnorm is this context's own residual"
    assert worst <= kw["ftol"] + 10.0 * deviation
    fast.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_context_unchanged():
    from socp_amd import capi
    c, Z = dint_rows()
    Z = np.ascontiguousarray(Z)
    ctx = context(c)
    B, n = len(Z), ctx.n
    L, h = ctx.L, ctx.h
    good = dict(DINT, jac=0)
    out = fresh(B, n, good["rounds"])
    ptrs = {k: out[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER}
    zp = Z.ctypes.data_as(DP)

    def call(B_=B, Z_=zp, opts=None, null=None, **kw):
        o = capi.newton_options(**dict(good, **kw)) if opts is None else opts
        return L.socp_newton_batch(h, B_, Z_, C.byref(o) if o is not False else None, *(None if k == null else ptrs[k] for k in ORDER))
    before = ctx.counters()
    assert call(B_=-1) == capi.ERR_ARG and call(opts=False) == capi.ERR_ARG
    for kw in (dict(jac=3), dict(jac=-1), dict(trials=0), dict(trials=9), dict(rounds=0), dict(ftol=0.0), dict(ftol=-1.0), dict(ftol=np.nan),
               dict(xtol=-1e-9), dict(xtol=np.nan)):
        assert call(**kw) == capi.ERR_ARG, kw
    assert call(Z_=None) == capi.ERR_ARG
    for k in ORDER:
        assert call(null=k) == (capi.OK if k in OPTIONAL else capi.ERR_ARG), k
    after_ok = ctx.counters()
    assert after_ok != before                                      # the two calls with an optional NULL ran
    for k, v in views(out).items():
        assert not np.all(v[:v.size - GUARD] == (np.uint64(SENT) if k in DOUBLES else SENT_I)), k
    out = fresh(B, n, good["rounds"])
    ptrs = {k: out[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER}
    before = ctx.counters()
    # _dev: NULL pointers, a workspace one byte short
    go = capi.newton_options(**good)
    wb = ctx.newton_work_bytes(B, go)
    assert wb > 0 and ctx.newton_work_bytes(-1, go) == 0 and ctx.newton_work_bytes(B, capi.newton_options(**dict(good, trials=9))) == 0
    assert ctx.newton_work_bytes(B, capi.newton_options(**dict(good, trials=8))) > wb
    fake = C.c_void_p(256)              # never dereferenced: every call below is refused before anything is enqueued

    def dev(Z_=fake, work=fake, bytes_=wb, null=None):
        return L.socp_newton_batch_dev(h, B, Z_, C.byref(go), work, bytes_, *(None if k == null else fake for k in ORDER))
    assert dev(Z_=None) == capi.ERR_ARG and dev(work=None) == capi.ERR_ARG
    for k in ORDER:
        if k not in OPTIONAL:
            assert dev(null=k) == capi.ERR_ARG, k
    assert dev(bytes_=wb - 1) == capi.ERR_ARG and "socp_newton_work_bytes" in L.socp_last_error(h).decode()
    # _blocks: the stride
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for stride in (3, 4, 6):
        assert L.socp_newton_batch_blocks(h, B, zp, params.ctypes.data_as(DP), stride, None, None, C.byref(go), *(ptrs[k] for k in ORDER)) == capi.ERR_ARG, stride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    assert ctx.counters() == before, "the refused calls launched and counted nothing"
    # B == 0: SOCP_OK without a launch, in all forms
    nul = (None,) * 8
    assert L.socp_newton_batch(h, 0, None, C.byref(go), *nul) == capi.OK
    assert L.socp_newton_batch_dev(h, 0, None, C.byref(go), None, 0, *nul) == capi.OK
    assert L.socp_newton_batch_blocks(h, 0, None, None, 0, None, None, C.byref(go), *nul) == capi.OK
    assert ctx.counters() == before
    # the adaptive integrator: jac = 2 is refused
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    assert call(jac=2) == capi.ERR_UNSUPPORTED and "fixed-step" in L.socp_last_error(h).decode() and ctx.counters() == before
    ctx.set_integrator(capi.INT_RK4)
    # no problem set; a model without variational equations; a FREE interior state component
    fresh_ctx = capi.Context(capi.MODEL_GODDARD)
    assert L.socp_newton_batch(fresh_ctx.h, B, zp, C.byref(go), *(ptrs[k] for k in ORDER)) == capi.ERR_ARG
    assert "no problem set" in L.socp_last_error(fresh_ctx.h).decode() and fresh_ctx.newton_work_bytes(1, go) == 0
    fresh_ctx.close()
    g = nc.goddard(1.0)
    gctx = context(g)
    gout = fresh(1, 14, good["rounds"])
    gp = [gout[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER]
    gz = np.ascontiguousarray(g["root"][None, :])
    assert L.socp_newton_batch(gctx.h, 1, gz.ctypes.data_as(DP), C.byref(capi.newton_options(**dict(good, jac=1))), *gp) == capi.ERR_UNSUPPORTED
    assert "variational" in L.socp_last_error(gctx.h).decode() and gctx.counters() == (0, 0)
    from oracle.oracle import FREE
    mode_x = np.array(g["prob"].mode_x)
    mode_x = np.vstack([mode_x[:1], mode_x[:1], mode_x[1:]])
    mode_x[1, 2] = FREE
    X = np.vstack([g["prob"].xnode[:1], np.zeros((1, 14)), g["prob"].xnode[1:]])
    assert gctx.problem_set([0, 0, 0], mode_x, np.array([0.0, 0.1, 0.2640825]), X) == 28
    gout2 = fresh(1, 28, good["rounds"])
    gz2 = np.zeros((1, 28))
    rc = L.socp_newton_batch(gctx.h, 1, gz2.ctypes.data_as(DP), C.byref(capi.newton_options(**dict(good, jac=2))),
                             *(gout2[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER))
    assert rc == capi.ERR_UNSUPPORTED and "FREE state component" in L.socp_last_error(gctx.h).decode() and gctx.counters() == (0, 0)
    gctx.close()
    # n beyond the elimination's bound: 2 n + 1 + 16 doubles must fit 64 KiB, so n <= 4087 (host tables only: nothing is integrated)
    from socp_amd import sweep
    big = capi.Context(capi.MODEL_GODDARD)
    big.set_params(sweep.GODDARD_PARAMS)
    assert sweep.goddard_multiple_shooting_problem(big, 292) == 4089
    bo = capi.newton_options(**dict(good, jac=2))
    assert big.L.socp_newton_batch_dev(big.h, 1, fake, C.byref(bo), fake, 0, *(fake for _ in ORDER)) == capi.ERR_UNSUPPORTED
    assert "too many unknowns" in big.L.socp_last_error(big.h).decode() and big.counters() == (0, 0)
    big.close()
    for k, v in list(views(out).items()) + list(views(gout).items()) + list(views(gout2).items()):
        assert np.all(v == (np.uint64(SENT) if k in DOUBLES else SENT_I)), "a refused call wrote into " + k
    # a valid call afterwards gives the reference's bits
    check_whole(run_host(ctx, Z, go), dint_ref(0), "after the refused calls")
    ctx.close()


# ---- 6. the sweep tool --------------------------------------------------------------------------------------------------------------------

def test_sweep_tool_polishes_its_converged_chains(tmp_path):
    out = str(tmp_path / "newton")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "8", "--rk4-steps", "10", "--newton-out", out, "--newton-rounds", "6"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["newton"]
    assert sorted(entry) == sorted(["rows", "jac", "running", "converged", "small_step", "stalled", "singular", "bad_start", "rnorm_median", "rnorm_max",
                                    "iters_median"])
    npz = np.load(out + ".rank0.npz")
    assert sorted(npz.files) == sorted(["index", "z", "rnorm", "dnorm", "iters", "nhalf", "status"])
    k = entry["rows"]
    assert k == rec["converged"] > 0 and npz["z"].shape == (k, 14) and npz["status"].shape == (k,) and entry["jac"] == 2
    for value, key in enumerate(["running", "converged", "small_step", "stalled", "singular", "bad_start"]):
        assert entry[key] == int(np.sum(npz["status"] == value)), key
    assert entry["rnorm_median"] == float(np.median(npz["rnorm"])) and entry["rnorm_max"] == float(np.max(npz["rnorm"]))
    print("sweep --newton-out: %s" % json.dumps(entry))
    assert entry["bad_start"] == 0 and sum(entry[key] for key in ("running", "converged", "small_step", "stalled", "singular")) == k
    assert np.all(np.isfinite(npz["rnorm"])) and np.all(np.isfinite(npz["z"]))
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--newton-out", out], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 2 and "--newton-out" in bad.stderr
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--newton-out", out, "--newton-trials", "9"], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 2 and "--newton-trials" in bad.stderr
