"""GPU: what the six _blocks entry points (residual, trace, cost, move, events, regrid) have in common -- the per-row blocks are
in force for the call only.  One parametrised case per entry point on the Goddard C1 problem of tests/test_gpu_cost_batch.py
(B = 3, 4 steps, per-row blocks for params, time and xnode; row 1 with its own KD), while blocks of the context's OWN
(socp_problem_set_blocks_dev, KD = 250 for every row) are in force.  The probe is a socp_residual_batch_dev into a device buffer
with a 64-word sentinel band on each side: its whole buffer must hold the same bits before and after a _blocks call, successful
or refused.  Outputs of the _blocks calls live in sentinel-filled host buffers followed by 64 guard words and are compared whole.

What "no blocks" means (recorded from the code, and asserted here): a _blocks call with params = time = xnode = NULL puts NO blocks
in force for its duration -- every NULL block means "the context's shared value", as include/socp_hip.h says -- so while blocks of
the context's own are set it gives the bits of the non-_blocks form WITHOUT them, not with them."""
import ctypes as C

import numpy as np
import pytest

from conftest import goddard_c1_problem
from test_gpu_cost_batch import build_goddard_c1

pytestmark = pytest.mark.gpu
SENT = np.uint64(0x7FF8DEADBEEF0001)            # a NaN no kernel produces
SENT_I = np.int32(0x5EADBEE1)                   # no event id, no count
GUARD = 64
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
B, STRIDE, CAP, E, REFINE, M2 = 3, 2, 8, 1, 2, 2


def f64(size):
    return np.full(size + GUARD, SENT, dtype=np.uint64).view(np.float64)


def i32(size):
    return np.full(size + GUARD, SENT_I, dtype=np.int32)


def ptr(a):
    return None if a is None else a.ctypes.data_as(IP if a.dtype == np.int32 else DP)


def same(xs, ys):
    return len(xs) == len(ys) and all(x.tobytes() == y.tobytes() for x, y in zip(xs, ys))


class Setup:
    def __init__(self):
        import torch
        from socp_amd import capi
        self.torch = torch
        self.ctx, o, _, Z, _ = build_goddard_c1(B=B, N=4)
        ctx = self.ctx
        prob, _ = goddard_c1_problem(o)
        self.M, self.n, self.s, self.W = ctx.M, ctx.n, ctx.s, ctx.trace_width()
        self.Z = np.ascontiguousarray(Z)
        base = np.concatenate([ctx.get_params(), [0.0227, 0.08]])
        self.P = np.tile(base, (B, 1))
        self.P[1, 2] = 200.0                                    # row 1's KD differs from the context's 310
        self.T = np.tile(prob.time, (B, 1))
        self.T[1, 0], self.T[2, 0] = 0.001, -0.002              # the FIXED initial time is the one the timeline reads
        self.X = np.tile(prob.xnode.ravel(), (B, 1))
        self.X[:, 6 * 14] = [1.01, 1.012, 1.008]
        own = np.tile(base, (B, 1))
        own[:, 2] = 250.0
        self.own = torch.from_numpy(own).cuda()                 # the context's own blocks: KD = 250 for every row
        self.dev = [torch.from_numpy(a).cuda() for a in (self.P, self.T, self.X)]
        self.dZ = torch.from_numpy(self.Z).cuda()
        tl = np.stack([ctx.timeline(z) for z in self.Z])
        self.tq = np.ascontiguousarray(0.5 * (tl[:, :-1] + tl[:, 1:]))          # K = M queries per row: the segment midpoints
        self.chan = np.zeros(E, dtype=np.int32)
        self.levels = np.zeros((B, E))
        self.mode_t2 = np.array([capi.FIXED, capi.CONTINUOUS, capi.FREE], dtype=np.int32)
        self.T2 = np.ascontiguousarray(np.stack([np.linspace(t[0], t[-1], M2 + 1) for t in tl]))
        self.n2 = ctx.regrid_num_param(self.mode_t2)
        assert ctx.event_channels() == 1 and self.n2 == self.s * M2 + 1
        torch.cuda.synchronize()

    # the context's own blocks
    def set_own(self, on):
        L, h = self.ctx.L, self.ctx.h
        self.ctx._chk(L.socp_problem_set_blocks_dev(h, self.own.data_ptr(), self.P.shape[1], None, None) if on else
                      L.socp_problem_set_blocks_dev(h, None, 0, None, None))
        self.torch.cuda.synchronize()

    def probe(self):
        """socp_residual_batch_dev with whatever the context holds: the WHOLE guarded device buffer."""
        torch = self.torch
        t = torch.from_numpy(np.full(B * self.n + 2 * GUARD, SENT, dtype=np.uint64).view(np.float64)).cuda()
        torch.cuda.synchronize()                                # the context has its own stream: the fill is complete first
        self.ctx.residual_batch_dev(B, self.dZ.data_ptr(), t.data_ptr() + 8 * GUARD)
        self.ctx.synchronize()
        a = t.cpu().numpy().view(np.uint64)
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT) and not np.any(a[GUARD:-GUARD] == SENT)
        return a

    # output buffers of an entry point, sentinel-filled
    def outs(self, name):
        M, s, n = self.M, self.s, self.n
        return {"residual": lambda: [f64(B * n)],
                "trace": lambda: [f64(B * M * CAP * self.W), i32(B * M)],
                "cost": lambda: [f64(B * M), f64(B), f64(B * M * s)],
                "move": lambda: [f64(B * M * s), f64(B * M)],
                "events": lambda: [f64(B * M * CAP), i32(B * M * CAP), i32(B * M), f64(B * M * CAP * s)],
                "regrid": lambda: [f64(B * self.n2), f64(B * (M2 + 1) * s)]}[name]()

    def tail(self, name, o):
        """The arguments of an entry point behind (ctx, B, Z[, blocks])."""
        o = [ptr(a) for a in o]
        return {"residual": lambda: o,
                "trace": lambda: [STRIDE, CAP] + o,
                "cost": lambda: o,
                "move": lambda: [self.M, ptr(self.tq)] + o,
                "events": lambda: [E, ptr(self.chan), ptr(self.levels), REFINE, CAP] + o,
                "regrid": lambda: [M2, ptr(self.mode_t2), ptr(self.T2)] + o}[name]()

    def blocks_call(self, name, o, blocks=True, pstride=None, rows=B):
        """The raw _blocks call; returns its status."""
        blk = [ptr(self.P), self.P.shape[1] if pstride is None else pstride, ptr(self.T), ptr(self.X)] if blocks else [None, 0, None, None]
        fn = getattr(self.ctx.L, "socp_%s_batch_blocks" % name)
        return fn(self.ctx.h, rows, ptr(self.Z), *blk, *self.tail(name, o))

    def plain_call(self, name, o):
        """The non-_blocks form with whatever the context holds (regrid has the _dev form only: through device copies of o)."""
        L, h = self.ctx.L, self.ctx.h
        if name != "regrid":
            return getattr(L, "socp_%s_batch" % name)(h, B, ptr(self.Z), *self.tail(name, o))
        torch = self.torch
        d = [torch.from_numpy(a).cuda() for a in o]
        dT2 = torch.from_numpy(self.T2).cuda()
        torch.cuda.synchronize()
        rc = L.socp_regrid_batch_dev(h, B, self.dZ.data_ptr(), M2, ptr(self.mode_t2), dT2.data_ptr(), d[0].data_ptr(), d[1].data_ptr())
        self.ctx.synchronize()
        for a, t in zip(o, d):
            a[:] = t.cpu().numpy()
        return rc


@pytest.fixture(scope="module")
def S():
    s = Setup()
    yield s
    s.ctx.close()


FORMS = ["residual", "trace", "cost", "move", "events", "regrid"]


@pytest.mark.parametrize("name", FORMS)
def test_blocks_form_puts_its_blocks_in_force_for_the_call_only(S, name):
    from socp_amd import capi
    ctx = S.ctx
    fresh = S.outs(name)
    S.set_own(False)
    shared = S.probe()
    want_plain = S.outs(name)                               # the non-_blocks form with no blocks in force
    assert S.plain_call(name, want_plain) == capi.OK
    ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, S.dev[0].data_ptr(), S.P.shape[1], S.dev[1].data_ptr(), S.dev[2].data_ptr()))
    want_blocks = S.outs(name)                              # ... and with the per-row blocks put in force on the device
    assert S.plain_call(name, want_blocks) == capi.OK
    if name != "events" or want_plain[2][:B * S.M].sum() > 0:          # (a batch without a single event has nothing to differ in)
        assert not same(want_blocks[:1], want_plain[:1]), "the per-row blocks are read"
    S.set_own(True)
    try:
        before = S.probe()
        assert not np.array_equal(before, shared), "the context's own blocks are read"
        # (a) a successful call: its blocks are the ones read, the context's own are back afterwards
        got = S.outs(name)
        assert S.blocks_call(name, got) == capi.OK, ctx.L.socp_last_error(ctx.h)
        assert same(got, want_blocks), "_blocks against set_blocks_dev + the non-_blocks form"
        assert np.array_equal(S.probe(), before), "(a) the context's own blocks after a successful call"
        # (b) a refused call: status, message, counters, outputs, and the context's own blocks
        count0 = ctx.counters()
        got = S.outs(name)
        assert S.blocks_call(name, got, pstride=S.P.shape[1] - 1) == capi.ERR_ARG
        msg = ctx.L.socp_last_error(ctx.h).decode()
        assert "nparams + 2" in msg and msg.startswith(name + "_batch_blocks: "), msg
        assert ctx.counters() == count0 and same(got, fresh), "(b) a refused call counts and writes nothing"
        assert np.array_equal(S.probe(), before), "(b) the context's own blocks after a refused call"
        # (c) NULL blocks: the non-_blocks form with no blocks in force, although the context's own are set
        got = S.outs(name)
        assert S.blocks_call(name, got, blocks=False) == capi.OK
        assert same(got, want_plain), "(c) NULL blocks"
        assert np.array_equal(S.probe(), before), "(c) the context's own blocks after a call with NULL blocks"
        # (d) an empty batch: SOCP_OK, nothing counted, nothing written
        count0 = ctx.counters()
        got = S.outs(name)
        assert S.blocks_call(name, got, rows=0) == capi.OK and S.blocks_call(name, got, blocks=False, rows=0) == capi.OK
        assert ctx.counters() == count0 and same(got, fresh), "(d) B = 0"
        assert np.array_equal(S.probe(), before), "(d) the context's own blocks after an empty batch"
    finally:
        S.set_own(False)
    # (c) without blocks of the context's own: the same bits again
    got = S.outs(name)
    assert S.blocks_call(name, got, blocks=False) == capi.OK and same(got, want_plain)
    assert np.array_equal(S.probe(), shared)
