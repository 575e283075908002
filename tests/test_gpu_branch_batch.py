"""GPU: socp_branch_batch[_dev] / _blocks (capi.Context.branch_batch) against tests/branch_reference.py -- the rounds of
include/socp_hip.h ("Past a fold") restated in numpy on the CPU oracle.  Outputs live in sentinel-filled buffers followed by 64 guard
words and are compared WHOLE on integer views (the conventions of test_gpu_tangent_batch.py); the workspace is followed by a guard too.
Reference-order flavour: every output buffer bit-equal to the restatement (a NaN equals any NaN).  Throughput flavour: the statuses,
the structure of the path and the residuals of its points on the same context; the deviation of zgoal is measured against the
reference-order run (profiles/branch_gpu_tests.txt keeps the figures)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import branch_reference as br
import tangent_reference as tr
from tangent_reference import DIR_PARAM, DIR_XNODE
from test_branch_cpu import FOLD, GODDARD, KD, check_fold

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x7FF8DEADBEEF0001                       # a NaN no kernel produces
SENT_I = 0x5EADBEE1
GUARD = 64
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
MODEL = {"goddard": 1, "dint": 2}
DOUBLES, INTS = ("y", "ttheta", "rnorm", "hlast", "zgoal"), ("count", "nfold", "ifold", "status", "nreject")
ORDER = ("y", "ttheta", "rnorm", "count", "nfold", "ifold", "status", "nreject", "hlast", "zgoal")      # the C argument order


def sizes(B, n, cap):
    return dict(y=B * cap * (n + 1), ttheta=B * cap, rnorm=B * cap, hlast=B, zgoal=B * n, count=B, nfold=B, ifold=B, status=B, nreject=B)


def sentinel(size):
    return np.full(size + GUARD, np.uint64(SENT), dtype=np.uint64).view(np.float64)


def sentinel_i(size):
    return np.full(size + GUARD, SENT_I, dtype=np.int32)


def fresh(B, n, cap):
    sz = sizes(B, n, cap)
    return {k: (sentinel(sz[k]) if k in DOUBLES else sentinel_i(sz[k])) for k in ORDER}


def up(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def both(**kw):
    """(the restatement's options, the device's) from one set of keywords."""
    from socp_amd import capi
    return br.options(**kw), capi.branch_options(**kw)


def context(c, variant="exact"):
    from socp_amd import capi
    if c["model"] == "fold1d":
        capi.plugin_load(plugin_path("fold1d"))
        ctx = capi.Context(1003, nparams=1)
    else:
        ctx = capi.Context(MODEL[c["model"]])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(c["params"])
    ctx.set_step_number(c["N"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


def plugin_path(name):
    path = os.path.join(ROOT, "socp_amd", "_build", "plugins", "lib%s_plugin.so" % name)
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


class DevBlocks:
    """Per-row blocks uploaded and in force (socp_problem_set_blocks_dev) inside the with-block."""

    def __init__(self, ctx, blocks):
        self.ctx, self.blocks = ctx, blocks

    def __enter__(self):
        if self.blocks is not None:
            self.keep = [up(a) for a in self.blocks]
            self.ctx._chk(self.ctx.L.socp_problem_set_blocks_dev(self.ctx.h, self.keep[0].data_ptr(), self.blocks[0].shape[1], self.keep[1].data_ptr(),
                                                                 self.keep[2].data_ptr()))
        return self

    def __exit__(self, *exc):
        if self.blocks is not None:
            self.ctx.L.socp_problem_set_blocks_dev(self.ctx.h, None, 0, None, None)


def views(bufs):
    return {k: (np.asarray(v).view(np.uint64) if k in DOUBLES else np.asarray(v)) for k, v in bufs.items()}


def run_dev(ctx, Z, d, opts, blocks=None, zgoal=True):
    """The _dev form on guarded device buffers: the WHOLE buffers back as integer views."""
    import torch
    Z = np.ascontiguousarray(Z)
    B, n, cap = len(Z), ctx.n, opts.cap
    dev = {k: up(v) for k, v in fresh(B, n, cap).items()}
    dZ = up(Z)
    wb = ctx.branch_work_bytes(B)
    assert wb > 0 and wb % 8 == 0
    work = up(sentinel(wb // 8))
    with DevBlocks(ctx, blocks):
        torch.cuda.synchronize()
        ctx.branch_batch_dev(B, dZ.data_ptr(), d, opts, work.data_ptr(), wb, *(dev[k].data_ptr() if (k != "zgoal" or zgoal) else None for k in ORDER))
        ctx.synchronize()
        torch.cuda.synchronize()
    assert np.all(work.cpu().numpy().view(np.uint64)[wb // 8:] == np.uint64(SENT)), "guard words behind the workspace were written"
    return views({k: v.cpu().numpy() for k, v in dev.items()})


def run_host(ctx, Z, d, opts, blocks=None, blocks_form=False):
    Z = np.ascontiguousarray(Z)
    B, n = len(Z), ctx.n
    out = fresh(B, n, opts.cap)
    tail = (int(d[0]), int(d[1]), C.byref(opts)) + tuple(out[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER)
    if blocks_form:
        pp, tt, xx = (np.ascontiguousarray(a) for a in blocks)
        ctx._chk(ctx.L.socp_branch_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), pp.ctypes.data_as(DP), pp.shape[1], tt.ctypes.data_as(DP),
                                                xx.ctypes.data_as(DP), *tail))
    else:
        ctx._chk(ctx.L.socp_branch_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    return views(out)


def same_doubles(got, want):
    """Bit equality, a NaN equal to any NaN."""
    g, w = got.view(np.float64), np.ascontiguousarray(want, dtype=np.float64).ravel()
    return (got == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))


def check_whole(got, ref, what, zgoal=True):
    for name in ORDER:
        g, fill = got[name], (np.uint64(SENT) if name in DOUBLES else SENT_I)
        if name == "zgoal" and not zgoal:
            assert np.all(g == fill), "%s: zgoal was written although its pointer was NULL" % what
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


def arrays(got, B, n, cap):
    """The buffers of run_dev / run_host without their guards, shaped as Context.branch_batch returns them."""
    sz = sizes(B, n, cap)
    out = {k: (got[k][:sz[k]].view(np.float64) if k in DOUBLES else got[k][:sz[k]]) for k in ORDER}
    out["y"], out["ttheta"], out["rnorm"], out["zgoal"] = out["y"].reshape(B, cap, n + 1), out["ttheta"].reshape(B, cap), out["rnorm"].reshape(B, cap), out["zgoal"].reshape(B, n)
    return out


# ---- the cases and their references, computed once ---------------------------------------------------------------------------------

SETTINGS = {"reached": {}, "rejects": dict(h0=6.4, hmax=6.4, max_corr=3), "full": dict(h0=0.4, hmax=0.4, max_corr=1, cap=40),
            "too_small": dict(h0=8.0, hmax=8.0, hmin=3.0, max_corr=2), "running": dict(rounds=5)}


def goddard_rows():
    """The polished row, a 1e-3-perturbed copy that starts off the branch, a NaN row."""
    g = tr.goddard_case()
    Z = np.repeat(g["Z"], 3, axis=0)
    Z[1] = Z[1] * (1.0 + 1e-3 * np.random.default_rng(11).uniform(-1.0, 1.0, Z.shape[1]))
    Z[2, 40] = np.nan
    return g, Z


def goddard_ref(setting):
    def build():
        g, Z = goddard_rows()
        return br.branch_reference(g["o"], g["prob"], 8, Z, KD, dict(GODDARD, **SETTINGS[setting]))
    return tr.cached(("gpu-branch", setting), build)


def dint_rows():
    c = tr.dint_case()
    Z = np.vstack([c["Z"], c["Z"][0] * (1.0 + 1e-4), c["Z"][0]])
    return c, Z


DINT = {"xnode": ((DIR_XNODE, 12), dict(dir=1, goal=14.0, h0=1.0, hmax=4.0, ftol=1e-9, cap=12, rounds=60)),
        "param": ((DIR_PARAM, 2), dict(dir=1, h0=0.05, hmax=0.2, ftol=1e-9, cap=6, rounds=40))}


def dint_ref(name, jac):
    def build():
        c, Z = dint_rows()
        d, o = DINT[name]
        return br.branch_reference(c["o"], c["prob"], 3, Z, d, dict(o, jac=jac))
    return tr.cached(("gpu-branch-dint", name, jac), build)


SINGLE = dict(wtheta=310.0, dir=-1, goal=300.0, h0=0.05, hmax=0.2, ftol=1e-10, cap=12, rounds=60)


def single_case():
    """Goddard single shooting (n = 14) at 60 steps -- where plain Newton from the nominal costates finds the root -- and two copies
    moved by 1e-6 and 1e-3: the first starts off the branch (||F|| = 1.5e-2) and is pulled onto it, the second is answered by single
    shooting with a residual of 1e29 and ends in STEP_TOO_SMALL."""
    def build():
        import jacobi_cases as jc
        o = jc.goddard_oracle(jc.N_STEPS)
        prob, _ = jc.goddard_single_problem()
        z = tr.polished(o, prob, jc.goddard_costate_batch(1, 0.0)[0])
        Z = np.stack([z, z * (1.0 + 1e-6), z * (1.0 + 1e-3)])
        c = dict(model="goddard", o=o, prob=prob, N=jc.N_STEPS, Z=Z, params=o.params()[:8])
        c["ref"] = br.branch_reference(o, prob, 8, Z, KD, SINGLE)
        return c
    return tr.cached("gpu-branch-single", build)


def dint_blocks(B):
    """B double-integrator rows whose final position -- the theta the call starts from -- differs from row to row."""
    c = tr.dint_case()
    o, prob = c["o"], c["prob"]
    pp = np.tile(np.concatenate([o.params()[:3], [o.m.sw[0], o.m.sw[1]]]), (B, 1))
    tt = np.tile(prob.time, (B, 1))
    xx = np.tile(prob.xnode.ravel(), (B, 1))
    xx[:, 12] = 10.0 + 0.05 * np.arange(B)
    Z = np.tile(c["Z"][0], (B, 1))
    return c, Z, (pp, tt, xx)


BLOCKS70 = dict(dir=-1, goal=6.0, h0=1.0, hmax=4.0, ftol=1e-9, cap=8, rounds=40)


def blocks70_ref():
    def build():
        c, Z, blocks = dint_blocks(70)
        return br.branch_reference(c["o"], c["prob"], 3, Z, (DIR_XNODE, 12), BLOCKS70, params=blocks[0], time=blocks[1], xnode=blocks[2])
    return tr.cached("gpu-branch-70", build)


# ---- 1. reference-order flavour, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("setting", list(SETTINGS))
def test_goddard_reference_order_bit_for_bit(setting):
    """n = 85, B = 3: two wavefronts per bordered matrix in LDS; every status of the polished row, BAD_START of the NaN row."""
    g, Z = goddard_rows()
    ref = goddard_ref(setting)
    want = {"reached": br.REACHED, "rejects": br.REACHED, "full": br.FULL, "too_small": br.STEP_TOO_SMALL, "running": br.RUNNING}[setting]
    print("goddard %s: status %s count %s nreject %s rounds %s" % (setting, ref["status"], ref["count"], ref["nreject"], ref["rounds_used"]))
    assert ref["status"][0] == want and ref["status"][2] == br.BAD_START
    if setting in ("rejects", "full", "too_small"):
        assert ref["nreject"][0] >= 1
    ropts, dopts = both(**dict(GODDARD, **SETTINGS[setting]))
    ctx = context(g)
    check_whole(run_dev(ctx, Z, KD, dopts), ref, "goddard %s, _dev form" % setting)
    if setting == "reached":
        check_whole(run_dev(ctx, Z, KD, dopts, zgoal=False), ref, "goddard, NULL zgoal", zgoal=False)
    ctx.close()


@pytest.mark.parametrize("jac", [0, 1])
@pytest.mark.parametrize("name", ["xnode", "param"])
def test_dint_reference_order_bit_for_bit(name, jac):
    """n = 13, so n + 1 = 14: four bordered matrices per workgroup; B = 5; both Jacobians; a boundary value and a parameter."""
    c, Z = dint_rows()
    ref = dint_ref(name, jac)
    print("dint %s jac %d: status %s count %s nreject %s" % (name, jac, ref["status"], ref["count"], ref["nreject"]))
    if name == "xnode":
        assert np.all(ref["status"] == br.REACHED)
    assert np.all(ref["count"] >= 2)
    d, o = DINT[name]
    ropts, dopts = both(**dict(o, jac=jac))
    ctx = context(c)
    assert ctx.n == 13
    check_whole(run_dev(ctx, Z, d, dopts), ref, "dint %s jac %d, _dev form" % (name, jac))
    ctx.close()


def test_goddard_single_shooting_reference_order_bit_for_bit():
    """n = 14, so n + 1 = 15: the largest size on the elimination's four-per-workgroup path but one."""
    c = single_case()
    ref = c["ref"]
    print("goddard single shooting: status %s count %s nreject %s" % (ref["status"], ref["count"], ref["nreject"]))
    assert ref["status"].tolist() == [br.REACHED, br.REACHED, br.STEP_TOO_SMALL] and ref["nfold"][0] == 0 and ref["count"][0] >= 3
    ctx = context(c)
    assert ctx.n == 14
    check_whole(run_dev(ctx, c["Z"], KD, both(**SINGLE)[1]), ref, "goddard single shooting, _dev form")
    ctx.close()


def test_seventy_rows_with_their_own_blocks_equal_the_rows_run_alone():
    """More than one wavefront of rows in the update kernel, every row with its own starting theta; rows finish in different rounds."""
    c, Z, blocks = dint_blocks(70)
    ref = blocks70_ref()
    # the far rows start too far off their branch for the distance guard: both ends occur, in rounds of their own
    assert set(ref["status"].tolist()) == {br.REACHED, br.STEP_TOO_SMALL} and len(set(ref["rounds_used"].tolist())) >= 4
    ropts, dopts = both(**BLOCKS70)
    ctx = context(c)
    got = run_dev(ctx, Z, (DIR_XNODE, 12), dopts, blocks=blocks)
    check_whole(got, ref, "70 rows with blocks")
    full = arrays(got, 70, 13, dopts.cap)
    for b in (0, 37, 69):
        alone = arrays(run_dev(ctx, Z[b:b + 1], (DIR_XNODE, 12), dopts, blocks=tuple(a[b:b + 1] for a in blocks)), 1, 13, dopts.cap)
        for k in ORDER:
            assert np.array_equal(np.asarray(alone[k][0]).view(np.uint64 if k in DOUBLES else np.int32),
                                  np.asarray(full[k][b]).view(np.uint64 if k in DOUBLES else np.int32)), (b, k)
    ctx.close()


# ---- 2. the forms ---------------------------------------------------------------------------------------------------------------------

def test_forms_give_the_same_bits_and_the_early_stop_changes_nothing():
    c, Z, blocks = dint_blocks(9)
    ropts, dopts = both(**dict(BLOCKS70, rounds=200))
    ctx = context(c)
    d = (DIR_XNODE, 12)
    t0, l0 = ctx.counters()
    want = run_dev(ctx, Z, d, dopts, blocks=blocks)              # all 200 rounds
    t1, l1 = ctx.counters()
    z, F = np.ascontiguousarray(Z[0]), ctx.residual(Z[0])
    ta, _ = ctx.counters()
    ctx.fd_jacobian(z, F, dedup=True)
    T_dedup = ctx.counters()[0] - ta
    assert l1 - l0 == 6 * 200 and t1 - t0 == 200 * (2 * 9 * ctx.M + 9 * T_dedup), "per round: six launches, 2 B M trajectories and the Jacobian's"
    used = int(blocks70_ref()["rounds_used"][:9].max())
    assert used < 64
    t0, l0 = ctx.counters()
    got = run_host(ctx, Z, d, dopts, blocks=blocks, blocks_form=True)
    t1, l1 = ctx.counters()
    assert same_bits(got, want), "_blocks form, stopped early"
    assert (l1 - l0) % (6 * 8) == 0 and 6 * used <= l1 - l0 < 6 * (used + 8), "the host form stops at the first multiple of 8 rounds with no row left"
    # the context's own blocks are back: the plain host form is the shared-table call and equals the _dev form without blocks
    shared = run_host(ctx, Z, d, dopts)
    assert not same_bits(shared, want) and same_bits(shared, run_dev(ctx, Z, d, dopts))
    # variational: eight launches per round
    vo, vd = both(**dict(BLOCKS70, rounds=3, jac=1))
    t0, l0 = ctx.counters()
    run_dev(ctx, Z, d, vd)
    t1, l1 = ctx.counters()
    assert l1 - l0 == 8 * 3 and t1 - t0 == 3 * (2 * 9 * ctx.M + 9 * ctx.M)
    # the Python form
    r = ctx.branch_batch(Z, d, dopts, params=blocks[0], time=blocks[1], xnode=blocks[2])
    w = arrays(want, 9, 13, dopts.cap)
    for k in ORDER:
        assert np.array_equal(np.asarray(r[k]).view(np.uint64 if k in DOUBLES else np.int32), np.asarray(w[k]).view(np.uint64 if k in DOUBLES else np.int32)), k
    ctx.close()


# ---- 3. the certain fold, through the device ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_fold1d_plugin_is_followed_through_its_fold(variant):
    from oracle.oracle import Problem, FIXED
    X = np.zeros((2, 2))
    X[1, 0] = 1.0
    c = dict(model="fold1d", prob=Problem(1, [FIXED, FIXED], np.zeros((2, 1), dtype=np.int32), np.array([0.0, 1.0]), X), N=10, params=np.array([0.0]))
    ctx = context(c, variant)
    assert ctx.n == 2
    ropts, dopts = both(**dict(FOLD, cap=40, rounds=200))
    # two equal rows: each is followed as if alone
    Z = np.array([[0.0, 1.0], [0.0, 1.0]])
    got = arrays(run_dev(ctx, Z, (DIR_PARAM, 0), dopts), 2, 2, 40)
    for b in range(2):
        check_fold({k: got[k][b] for k in ORDER}, ropts, "fold1d %s row %d" % (variant, b))
    assert np.array_equal(got["y"][0].view(np.uint64), got["y"][1].view(np.uint64))
    # natural-parameter continuation asks for a root at a > 1 next, where there is none: the residual there cannot vanish
    worst = np.min(np.abs(ctx.residual_batch_blocks(np.array([[0.0, p] for p in np.linspace(-1, 1, 41)]), params=np.tile([1.05, 0.0, 0.0], (41, 1)))[:, 1]))
    assert worst >= 0.05 - 1e-12
    ctx.close()


# ---- 4. throughput flavour ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard", "dint"])
def test_fast_flavour_follows_the_same_branch(name):
    """Same statuses, no fold, theta monotone, rnorm equal to the residual of the same context at the reported points, zgoal within
    10 x (largest deviation of the throughput residual from the oracle at those points) x ||J^-1|| of the reference-order zgoal.
    "Every reported rnorm <= ftol" is asserted for every ACCEPTED point, that is from point 1 on: by the definition point 0 is
    recorded without an acceptance test, and rows 1, 2 and 3 of the double-integrator batch start off the branch (||F||inf = 4.1e-2,
    4.3e-2 and 1.5e-3 there).  Point 0 must meet ftol wherever the reference-order run's point 0 does, and its rnorm is compared bit for bit with
    residual_batch_blocks like all the others.
    The continuation layer runs in reference order in both flavours, so only the model's launches make the two runs differ.
    Measured on one MI355X: goddard 2.937e-10 against a margin of 10 x 2.363e-13 x 5.290e+02 = 1.250e-09; dint 0.0 against a margin
    of 0.0 (the double integrator's throughput residual equals the oracle's bit for bit, and so do its paths)."""
    if name == "goddard":
        c = tr.goddard_case()
        Z, d, o, ref, nparams, slot = c["Z"], KD, dict(GODDARD), goddard_ref("reached"), 8, ("params", 2)
    else:
        c, Z = dint_rows()
        d, o = DINT["xnode"]
        ref, nparams, slot = dint_ref("xnode", 0), 3, ("xnode", 12)
    B, n = len(Z), c["prob"].n
    ropts, dopts = both(**o)
    fast = context(c, "fast")
    got = arrays(run_dev(fast, Z, d, dopts), B, n, dopts.cap)
    assert np.array_equal(got["status"], ref["status"][:B]) and np.all(got["status"] == br.REACHED) and np.all(got["nfold"] == 0)
    oracle, prob = c["o"], c["prob"]
    worst_dev, worst_res = 0.0, 0.0
    for b in range(B):
        cnt = int(got["count"][b])
        pts = got["y"][b, :cnt]
        assert np.all(np.diff(pts[:, n]) * o["dir"] > 0), "theta is monotone"
        pp = np.tile(np.concatenate([c["params"][:nparams], [oracle.m.sw[0], oracle.m.sw[1]]]), (cnt, 1))
        xx = np.tile(prob.xnode.ravel(), (cnt, 1))
        (pp if slot[0] == "params" else xx)[:, slot[1]] = pts[:, n]
        # the call's launches take Goddard's smooth-law kernel (mu2 > 0 in every moved block): the same promise for these blocks
        fast._chk(fast.L.socp_problem_blocks_all_smooth(fast.h, 1 if name == "goddard" else 0))
        F = fast.residual_batch_blocks(np.ascontiguousarray(pts[:, :n]), params=pp, time=np.tile(prob.time, (cnt, 1)), xnode=xx)
        fast._chk(fast.L.socp_problem_blocks_all_smooth(fast.h, 0))
        print("fast %s row %d: largest |rnorm - ||F||inf of residual_batch_blocks| = %.3e; rnorm of point 0 %.3e (no acceptance test), largest of the accepted points %.3e (ftol %.0e)"
              % (name, b, float(np.max(np.abs(np.max(np.abs(F), axis=1) - got["rnorm"][b, :cnt]))), got["rnorm"][b, 0], float(got["rnorm"][b, 1:cnt].max()), o["ftol"]))
        # point 0 is recorded without an acceptance test: a row that starts off the branch reports its start's residual there
        assert np.array_equal(np.max(np.abs(F), axis=1), got["rnorm"][b, :cnt]) and np.all(got["rnorm"][b, 1:cnt] <= o["ftol"])
        assert got["rnorm"][b, 0] <= o["ftol"] or ref["rnorm"][b, 0] > o["ftol"]
        # the throughput residual against the oracle's at the same points
        own = oracle.params().copy()
        try:
            for i in range(cnt):
                blk, pb = pp[i], prob
                if slot[0] == "xnode":
                    from oracle.oracle import Problem
                    pb = Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time, xx[i].reshape(prob.M + 1, 2 * prob.dim))
                worst_res = max(worst_res, float(np.max(np.abs(tr._residual(oracle, nparams, blk, pb, np.ascontiguousarray(pts[i, :n])) - F[i]))))
        finally:
            oracle.set_params(own)
        worst_dev = max(worst_dev, float(np.max(np.abs(got["zgoal"][b] - ref["zgoal"][b]))))
    # ||J^-1|| at the goal point of row 0, on the oracle
    from oracle.oracle import Problem
    blk = np.concatenate([c["params"][:nparams], [oracle.m.sw[0], oracle.m.sw[1]]])
    xg = prob.xnode.ravel().copy()
    (blk if slot[0] == "params" else xg)[slot[1]] = o["goal"]
    pg = Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time, xg.reshape(prob.M + 1, 2 * prob.dim))
    own = oracle.params().copy()
    try:
        zg = np.ascontiguousarray(ref["zgoal"][0])
        Fg = tr._residual(oracle, nparams, blk, pg, zg)
        inv = float(np.linalg.norm(np.linalg.inv(oracle.fdjac(pg, zg, Fg, 1e-15)), 2))
    finally:
        oracle.set_params(own)
    margin = 10.0 * worst_res * inv
    print("fast %s: max |zgoal_fast - zgoal_exact| = %.3e; margin 10 x %.3e (residual deviation from the oracle) x %.3e (||J^-1||) = %.3e"
          % (name, worst_dev, worst_res, inv, margin))
    assert worst_dev <= margin
    fast.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_context_unchanged():
    from socp_amd import capi
    c, Z = dint_rows()
    ctx = context(c)
    B, n, M, S, dim = len(Z), ctx.n, ctx.M, ctx.s, ctx.dim
    L, h = ctx.L, ctx.h
    good = dict(DINT["xnode"][1])
    out = fresh(B, n, good["cap"])
    ptrs = {k: out[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER}
    zp = Z.ctypes.data_as(DP)

    def call(B_=B, Z_=zp, d=(DIR_XNODE, 12), opts=None, null=None, **kw):
        o = capi.branch_options(**dict(good, **kw)) if opts is None else opts
        args = [None if k == null else ptrs[k] for k in ORDER]
        return L.socp_branch_batch(h, B_, Z_, d[0], d[1], C.byref(o) if o is not False else None, *args)
    before = ctx.counters()
    assert call(B_=-1) == capi.ERR_ARG and call(opts=False) == capi.ERR_ARG
    for d in ((3, 0), (-1, 0), (0, 5), (0, -1), (1, M + 1), (1, -1), (2, (M + 1) * S), (2, dim), (2, S + dim), (2, -1)):
        assert call(d=d) == capi.ERR_ARG, d
    bad = [dict(jac=2), dict(jac=-1), dict(wtheta=0.0), dict(wtheta=-1.0), dict(wtheta=np.inf), dict(wtheta=np.nan), dict(dir=0), dict(dir=2),
           dict(hmin=0.0), dict(hmin=2.0), dict(h0=8.0), dict(hmax=np.nan), dict(grow=0.5), dict(grow=np.nan), dict(max_corr=0), dict(kfast=-1),
           dict(ftol=0.0), dict(ftol=np.nan), dict(cap=1), dict(rounds=0)]
    for kw in bad:
        assert call(**kw) == capi.ERR_ARG, kw
    assert call(Z_=None) == capi.ERR_ARG
    for k in ORDER[:-1]:
        assert call(null=k) == capi.ERR_ARG, k
    # _dev: NULL pointers, a workspace one byte short
    wb = ctx.branch_work_bytes(B)
    assert wb > 0 and ctx.branch_work_bytes(-1) == 0
    fake = C.c_void_p(256)              # never dereferenced: every call below is refused before anything is enqueued
    go = capi.branch_options(**good)

    def dev(Z_=fake, work=fake, bytes_=wb, null=None):
        return L.socp_branch_batch_dev(h, B, Z_, DIR_XNODE, 12, C.byref(go), work, bytes_, *(None if k == null else fake for k in ORDER))
    assert dev(Z_=None) == capi.ERR_ARG and dev(work=None) == capi.ERR_ARG
    for k in ORDER[:-1]:
        assert dev(null=k) == capi.ERR_ARG, k
    assert dev(bytes_=wb - 1) == capi.ERR_ARG and "socp_branch_work_bytes" in L.socp_last_error(h).decode()
    # _blocks: the stride
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for stride in (3, 4, 6):
        assert L.socp_branch_batch_blocks(h, B, zp, params.ctypes.data_as(DP), stride, None, None, DIR_XNODE, 12, C.byref(go),
                                          *(ptrs[k] for k in ORDER)) == capi.ERR_ARG, stride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    assert ctx.counters() == before, "the refused calls launched and counted nothing"
    # B == 0: SOCP_OK without a launch, in all forms
    nul = (None,) * 10
    assert L.socp_branch_batch(h, 0, None, DIR_XNODE, 12, C.byref(go), *nul) == capi.OK
    assert L.socp_branch_batch_dev(h, 0, None, DIR_XNODE, 12, C.byref(go), None, 0, *nul) == capi.OK
    assert L.socp_branch_batch_blocks(h, 0, None, None, 0, None, None, DIR_XNODE, 12, C.byref(go), *nul) == capi.OK
    assert ctx.counters() == before
    # no problem set; a model without variational equations
    fresh_ctx = capi.Context(capi.MODEL_GODDARD)
    assert L.socp_branch_batch(fresh_ctx.h, B, zp, DIR_PARAM, 2, C.byref(go), *(ptrs[k] for k in ORDER)) == capi.ERR_ARG
    assert "no problem set" in L.socp_last_error(fresh_ctx.h).decode() and fresh_ctx.branch_work_bytes(1) == 0
    fresh_ctx.close()
    g = tr.goddard_case()
    gctx = context(g)
    gout = fresh(1, 85, good["cap"])
    gz = np.ascontiguousarray(g["Z"])
    assert L.socp_branch_batch(gctx.h, 1, gz.ctypes.data_as(DP), DIR_PARAM, 2, C.byref(capi.branch_options(**dict(good, jac=1))),
                               *(gout[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER)) == capi.ERR_UNSUPPORTED
    assert "variational" in L.socp_last_error(gctx.h).decode() and gctx.counters() == (0, 0)
    gctx.close()
    # n + 1 beyond the elimination's bound: 2 (n + 1) + 1 + 16 doubles must fit 64 KiB, so n + 1 <= 4087.  Goddard with 292 segments
    # has n = 14 * 292 + 1 = 4089 (host tables only: nothing is integrated); 291 segments, n + 1 = 4076, still passes that check
    from socp_amd import sweep
    big = capi.Context(capi.MODEL_GODDARD)
    big.set_params(sweep.GODDARD_PARAMS)
    assert sweep.goddard_multiple_shooting_problem(big, 292) == 4089
    bout = fresh(1, 4089, 2)
    bptr = [bout[k].ctypes.data_as(DP if k in DOUBLES else IP) for k in ORDER]
    bz = np.zeros((1, 4089))
    bo = capi.branch_options(**dict(good, cap=2))
    bblock = np.concatenate([big.get_params(), [0.0, 0.0]])[None, :]
    bwork = big.branch_work_bytes(1)
    counted = big.counters()
    for form, rc in (("host", big.L.socp_branch_batch(big.h, 1, bz.ctypes.data_as(DP), DIR_PARAM, 2, C.byref(bo), *bptr)),
                     ("_dev", big.L.socp_branch_batch_dev(big.h, 1, fake, DIR_PARAM, 2, C.byref(bo), fake, bwork, *(fake for _ in ORDER))),
                     ("_blocks", big.L.socp_branch_batch_blocks(big.h, 1, bz.ctypes.data_as(DP), bblock.ctypes.data_as(DP), 10, None, None, DIR_PARAM, 2,
                                                                C.byref(bo), *bptr))):
        assert rc == capi.ERR_UNSUPPORTED, form
        assert "too many unknowns" in big.L.socp_last_error(big.h).decode() and "64 KiB" in big.L.socp_last_error(big.h).decode(), form
    # the refusal comes before the option and pointer checks' later neighbours: a bad workspace on the SAME problem is still UNSUPPORTED
    assert big.L.socp_branch_batch_dev(big.h, 1, fake, DIR_PARAM, 2, C.byref(bo), fake, 0, *(fake for _ in ORDER)) == capi.ERR_UNSUPPORTED
    assert big.counters() == counted, "the refused calls launched and counted nothing"
    assert sweep.goddard_multiple_shooting_problem(big, 291) == 4075
    assert big.L.socp_branch_batch_dev(big.h, 1, fake, DIR_PARAM, 2, C.byref(bo), fake, 0, *(fake for _ in ORDER)) == capi.ERR_ARG
    assert "socp_branch_work_bytes" in big.L.socp_last_error(big.h).decode(), "n + 1 = 4076 passes the bound and is refused for its workspace only"
    assert big.counters() == counted
    big.close()
    for k, v in list(views(out).items()) + list(views(gout).items()) + list(views(bout).items()):
        assert np.all(v == (np.uint64(SENT) if k in DOUBLES else SENT_I)), "a refused call wrote into " + k
    # a valid call afterwards gives the reference's bits
    check_whole(run_host(ctx, Z, DINT["xnode"][0], go), dint_ref("xnode", 0), "after the refused calls")
    ctx.close()


# ---- 6. the sweep tool --------------------------------------------------------------------------------------------------------------------

def test_sweep_tool_follows_the_branch_of_its_converged_chains(tmp_path):
    out = str(tmp_path / "branch")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "8", "--rk4-steps", "10", "--branch-out", out, "--branch-param", "KD",
                          "--branch-goal", "300", "--branch-wtheta", "310", "--branch-points", "16", "--branch-rounds", "80"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["branch"]
    assert sorted(entry) == sorted(["rows", "reached", "with_fold", "step_too_small", "singular", "points_median"])
    npz = np.load(out + ".rank0.npz")
    assert sorted(npz.files) == sorted(["index", "y", "ttheta", "rnorm", "count", "nfold", "ifold", "status", "zgoal"])
    k = entry["rows"]
    assert k == rec["converged"] > 0 and npz["y"].shape == (k, 16, 15) and npz["zgoal"].shape == (k, 14) and npz["status"].shape == (k,)
    assert entry["reached"] == int(np.sum(npz["status"] == br.REACHED)) and entry["with_fold"] == int(np.sum(npz["nfold"] > 0))
    assert entry["step_too_small"] == int(np.sum(npz["status"] == br.STEP_TOO_SMALL)) and entry["singular"] == int(np.sum(npz["status"] == br.SINGULAR))
    assert entry["points_median"] == float(np.median(npz["count"])) and entry["reached"] >= 1
    reached = npz["status"] == br.REACHED
    assert np.all(np.isfinite(npz["zgoal"][reached])) and np.all(npz["y"][:, 0, 14] == 310.0)
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--branch-out", out, "--branch-goal", "0"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--branch-out" in bad.stderr
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--branch-out", out, "--branch-param", "nosuch", "--branch-goal", "0"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--branch-param" in bad.stderr
