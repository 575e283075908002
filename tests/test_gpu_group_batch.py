"""GPU: socp_group_batch[_dev] (capi.Context.group_batch, group_batch_dev) against tests/group_reference.py -- the sequential
definition of include/socp_hip.h restated in numpy, the only reference.  The conventions of test_gpu_tangent_batch.py: every output
lives in a sentinel-filled buffer followed by 64 guard words and is compared WHOLE, on integer views, with array_equal (a radius is a
maximum of exactly rounded differences, so it is compared bit for bit too).  The call has no caller-owned workspace to put a guard
behind: its scratch (max_groups + 1 words) is the context's own.  Columns n .. ld-1 of every table hold NaN: they never reach a
verdict."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import group_reference as gr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x7FF8DEADBEEF0001                       # a NaN no kernel produces
SENT_I = 0x5EADBEE1
GUARD = 64
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
NAMES = ("label", "leader", "count", "radius", "summary")
_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def sentinel(size):
    return np.full(size + GUARD, np.uint64(SENT), dtype=np.uint64).view(np.float64)


def sentinel_i(size):
    return np.full(size + GUARD, SENT_I, dtype=np.int32)


def outputs(B, max_groups):
    """Sentinel-filled label, leader, count, radius, summary, each with its guard (sized for the valid call: max_groups >= 1)."""
    mg = max(max_groups, 1)
    return [sentinel_i(max(B, 0)), sentinel_i(mg), sentinel_i(mg), sentinel(mg), sentinel_i(4)]


def views(bufs):
    return [np.ascontiguousarray(b).view(np.uint64) if b.dtype == np.float64 else np.ascontiguousarray(b) for b in bufs]


def expected(ref):
    """The reference's arrays as the whole buffers should look: the values, then the untouched guard."""
    out = []
    for name in NAMES:
        a = np.ascontiguousarray(ref[name])
        if a.dtype == np.float64:
            out.append(np.concatenate([a.view(np.uint64), np.full(GUARD, np.uint64(SENT), dtype=np.uint64)]))
        else:
            out.append(np.concatenate([a.astype(np.int32), np.full(GUARD, SENT_I, dtype=np.int32)]))
    return out


def up(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def context(variant="exact"):
    from socp_amd import capi
    ctx = capi.Context(capi.MODEL_DOUBLE_INTEGRATOR)            # any model: the grouping needs no problem
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    return ctx


@pytest.fixture(scope="module")
def ctx():
    c = context()
    yield c
    c.close()


def run_dev(ctx, V, n, mask=None, atol=0.0, rtol=1e-6, max_groups=8):
    """The _dev form on guarded device buffers: the WHOLE buffers back."""
    import torch
    V = np.ascontiguousarray(V, dtype=np.float64)
    B, ld = V.shape
    dV = up(np.concatenate([V.ravel(), sentinel(0)]))
    dM = up(np.ascontiguousarray(mask, dtype=np.int32)) if mask is not None and B > 0 else None
    bufs = [up(b) for b in outputs(B, max_groups)]
    torch.cuda.synchronize()
    ctx.group_batch_dev(B, n, ld, dV.data_ptr(), dM.data_ptr() if dM is not None else None, atol, rtol, max_groups, *[b.data_ptr() for b in bufs])
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(dV.cpu().numpy().view(np.uint64), np.concatenate([V.ravel(), sentinel(0)]).view(np.uint64)), "the table was written"
    return views([b.cpu().numpy() for b in bufs])


def run_host(ctx, V, n, mask=None, atol=0.0, rtol=1e-6, max_groups=8):
    V = np.ascontiguousarray(V, dtype=np.float64)
    B, ld = V.shape
    m = np.ascontiguousarray(mask, dtype=np.int32) if mask is not None else None
    bufs = outputs(B, max_groups)
    ctx._chk(ctx.L.socp_group_batch(ctx.h, B, n, ld, V.ctypes.data_as(DP), m.ctypes.data_as(IP) if m is not None else None, atol, rtol, max_groups,
                                    bufs[0].ctypes.data_as(IP), bufs[1].ctypes.data_as(IP), bufs[2].ctypes.data_as(IP), bufs[3].ctypes.data_as(DP),
                                    bufs[4].ctypes.data_as(IP)))
    return views(bufs)


def check_whole(got, ref, what):
    for name, g, w in zip(NAMES, got, expected(ref)):
        assert g.shape == w.shape, (what, name)
        bad = np.argwhere(g != w).ravel()
        assert len(bad) == 0, (what, name, "%d differ, first flat indices:" % len(bad), bad[:6].tolist(), g[bad[:6]], w[bad[:6]])
    assert np.array_equal(got[0], expected(ref)[0])


def check(ctx, V, n, what, **kw):
    kw.setdefault("max_groups", 8)
    ref = gr.group_reference(V, n=n, **kw)
    check_whole(run_dev(ctx, V, n, **kw), ref, what)
    return ref


# ---- tables -----------------------------------------------------------------------------------------------------------------------

def roots_of(G, n):
    """G rows, pairwise far apart in every entry, both signs, magnitudes from 1 to G + 1."""
    i = np.arange(n)
    return (1.0 + np.arange(G)[:, None]) * (1.0 + 0.01 * i[None, :]) * np.where(i % 2 == 0, 1.0, -1.0)[None, :]


def table(pick, n, ld, seed=0, noise=1e-9):
    """Row b = root pick[b] with relative noise, trailing columns NaN."""
    pick = np.asarray(pick)
    rng = np.random.default_rng(seed)
    V = np.full((len(pick), ld), np.nan)
    V[:, :n] = roots_of(int(pick.max()) + 1 if len(pick) else 1, n)[pick] * (1.0 + noise * rng.uniform(-1.0, 1.0, (len(pick), n)))
    return V


# ---- 1. shapes --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("n", [1, 14, 85, 253])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 4097])
def test_shapes_whole_outputs_equal_the_restatement(ctx, B, n, pad):
    """Five roots in random order, some rows NaN / +-Inf in one entry, some masked (a masked row may hold anything); max_groups = 8."""
    def build():
        rng = np.random.default_rng(1000 * B + 10 * n + pad)
        V = table(rng.integers(0, 5, B), n, n + pad, seed=B + n)
        mask = np.ones(B, dtype=np.int32)
        if B >= 63:
            for k, bad in enumerate((np.nan, np.inf, -np.inf)):
                rows = rng.choice(B, max(1, B // 50), replace=False)
                V[rows, rng.integers(0, n, len(rows))] = bad
            mask[rng.choice(B, B // 10, replace=False)] = 0
        return V, mask, gr.group_reference(V, n=n, mask=mask, rtol=1e-6, max_groups=8)
    V, mask, ref = cached(("shape", B, n, pad), build)
    assert ref["summary"][0] == min(5, B) or B < 63 and ref["summary"][0] >= 1
    if B >= 63:
        assert ref["summary"][2] > 0 and ref["summary"][3] == B // 10 and ref["summary"][1] == 0
    check_whole(run_dev(ctx, V, n, mask=mask, rtol=1e-6, max_groups=8), ref, "B %d n %d ld %d" % (B, n, n + pad))


def test_a_leader_row_longer_than_the_lds_panel(ctx):
    """n = 2100 > the 2048 leader columns a workgroup keeps in LDS: the columns behind them come from memory; the deciding entries
    sit there."""
    n, B = 2100, 65
    V = np.tile(roots_of(1, n), (B, 1))
    V[:, 2099], V[:, 2050] = 1.0, -1.0
    V[1::3, 2099] = 1.0 + 2.0 ** -10                       # near at rtol = 2^-10, exactly on the bound
    V[2::3, 2050] = np.nextafter(-1.0 - 2.0 ** -10, -2.0)  # one ulp outside it
    V[7, 2070] = np.inf
    ref = check(ctx, V, n, "n = 2100", rtol=2.0 ** -10, max_groups=4)
    assert ref["summary"].tolist() == [2, 0, 1, 0] and ref["label"][:4].tolist() == [0, 0, 1, 0]


# ---- 2. group counts ----------------------------------------------------------------------------------------------------------------

def test_group_counts_rounds_and_launches(ctx):
    B, n, ld = 4097, 14, 16
    rng = np.random.default_rng(3)
    # G = 1: one round, although 1024 are allowed: begin (2 launches), one round, end
    l0 = ctx.counters()[1]
    ref = check(ctx, table(np.zeros(B, dtype=int), n, ld), n, "G = 1", max_groups=1024)
    assert ref["summary"].tolist() == [1, 0, 0, 0] and ref["count"][0] == B and ctx.counters() == (0, l0 + 4)
    # G = 3: leaders at row 0 and at the LAST row, which is alone in its group
    pick = rng.integers(0, 2, B)
    pick[0], pick[1], pick[-1] = 0, 1, 2
    ref = check(ctx, table(pick, n, ld), n, "G = 3", max_groups=8)
    assert ref["leader"][:3].tolist() == [0, 1, B - 1] and ref["count"][2] == 1 and ref["summary"][0] == 3
    # G = 2: rounds come singly, then in twos: round 2 is enqueued after the rows ran out, and returns at once
    l0 = ctx.counters()[1]
    ref = check(ctx, table(rng.integers(0, 2, B), n, ld), n, "G = 2", max_groups=8)
    assert ref["summary"][0] == 2 and ctx.counters()[1] == l0 + 2 + 3 + 1
    # G = 70 with max_groups = 128: more rounds than any chunk
    pick70 = rng.integers(0, 70, B)
    ref = check(ctx, table(pick70, n, ld), n, "G = 70", max_groups=128)
    assert ref["summary"].tolist() == [70, 0, 0, 0] and ref["count"].sum() == B
    # max_groups reached exactly: 70 of 70
    ref = check(ctx, table(pick70, n, ld), n, "G = max_groups = 70", max_groups=70)
    assert ref["summary"].tolist() == [70, 0, 0, 0]
    # overflow by many rows; max_groups = 1
    ref = check(ctx, table(pick70, n, ld), n, "70 roots, 16 groups", max_groups=16)
    assert ref["summary"][0] == 16 and ref["summary"][1] > B // 2
    ref = check(ctx, table(pick70, n, ld), n, "70 roots, 1 group", max_groups=1)
    assert ref["summary"][0] == 1 and ref["summary"][1] == B - ref["count"][0] > B // 2 and ref["leader"].tolist() == [0]
    # every row its own group: max_groups rounds, the rest overflow
    ref = check(ctx, table(np.arange(300), 1, 3), 1, "all distinct", max_groups=40)
    assert ref["summary"].tolist() == [40, 260, 0, 0] and ref["leader"].tolist() == list(range(40))


# ---- 3. the boundary ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,c", [(3, 1), (85, 70)])
def test_the_bound_is_inclusive_and_exact(ctx, n, c):
    """Exact numbers: l = 1, atol = 0, rtol = 2^-10: v = 1 + 2^-10 is near (difference and bound are both exactly 2^-10), the next
    double is not; the same with l = -1; a zero leader entry with atol = 0 takes +-0.0 only.  Column c decides (n = 85: a column the
    wave's second load instruction of a row brings)."""
    e = 2.0 ** -10

    def rows(lead, values):
        V = np.full((1 + len(values), n + 2), np.nan)
        V[:, :n] = lead
        V[1:, c] = values
        return V
    for sign in (1.0, -1.0):
        v_in = sign * (1.0 + e)
        v_out = np.nextafter(v_in, sign * 2.0)
        assert abs(v_in - sign) == e and abs(v_out - sign) > e
        ref = check(ctx, rows(sign, [v_in, v_out, sign * (1.0 - e), np.nextafter(sign * (1.0 - e), 0.0)]), n, "l = %g" % sign, atol=0.0, rtol=e)
        assert ref["label"].tolist() == [0, 0, 1, 0, 2] and ref["radius"][0] == e
    lead = np.ones(n)
    lead[c] = 0.0
    ref = check(ctx, rows(lead, [0.0, -0.0, 5e-324, -5e-324, 0.0]), n, "l = 0", atol=0.0, rtol=e)
    assert ref["label"].tolist() == [0, 0, 0, 1, 2, 0] and ref["radius"][:3].tolist() == [0.0, 0.0, 0.0]
    # and the absolute term alone: atol = 1, rtol = 0 on the chain 0, 0.75, 1.5 -- near is not transitive
    chain = rows(np.zeros(n), [0.75, 1.5])
    ref = check(ctx, chain, n, "chain", atol=1.0, rtol=0.0)
    assert ref["label"].tolist() == [0, 0, 1]


# ---- 4. exclusions, order, flavours, forms ------------------------------------------------------------------------------------------

def mixed_table(B=300, n=14, ld=16):
    def build():
        rng = np.random.default_rng(11)
        V = table(rng.integers(0, 4, B), n, ld, seed=5)
        V[0, 3], V[1, 0], V[2, n - 1] = np.nan, np.inf, -np.inf            # the first rows: they must not lead
        V[150, 5], V[151, 6], V[B - 1, 0] = np.inf, np.nan, -np.inf
        return V
    return cached(("mixed", B, n, ld), build)


def test_rows_that_are_not_finite_never_lead_and_never_join(ctx):
    V = mixed_table()
    ref = check(ctx, V, 14, "not finite", rtol=1e-6)
    assert ref["label"][[0, 1, 2, 150, 151, 299]].tolist() == [gr.NOTFINITE] * 6 and ref["leader"][0] == 3 and ref["summary"].tolist() == [4, 0, 6, 0]
    # an infinite bound does not let an infinite entry in: rtol |l| overflows for l = 1.7e308, rtol = 1e10 (and so does v - l of row 2, which IS near)
    W = np.full((4, 3), np.nan)
    W[:, :2] = [[1.7e308, 1.0], [np.inf, 1.0], [-1.7e308, 1.0], [1.7e308, np.nan]]
    ref = check(ctx, W, 2, "infinite bound", atol=0.0, rtol=1e10)
    assert ref["label"].tolist() == [0, gr.NOTFINITE, 0, gr.NOTFINITE] and ref["radius"][0] == np.inf


def test_masks(ctx):
    V = mixed_table()
    B = len(V)
    mask = np.ones(B, dtype=np.int32)
    mask[[0, 3, B - 1]] = 0                                 # the first row, the first finite row and the last row
    ref = check(ctx, V, 14, "mask at both ends", mask=mask, rtol=1e-6)
    assert ref["label"][[0, 3, B - 1]].tolist() == [gr.MASKED] * 3 and ref["leader"][0] == 4 and ref["summary"].tolist() == [4, 0, 4, 3]
    ref = check(ctx, V, 14, "mask of zeros", mask=np.zeros(B, dtype=np.int32), rtol=1e-6)
    assert ref["summary"].tolist() == [0, 0, 0, B] and np.all(ref["leader"] == -1)
    # any non-zero word is "in"
    ref2 = gr.group_reference(V, n=14, mask=mask, rtol=1e-6, max_groups=8)
    check_whole(run_dev(ctx, V, 14, mask=mask * np.int32(-7), rtol=1e-6), ref2, "mask words")


def test_a_row_permutation_changes_the_labels_as_the_restatement_says(ctx):
    V = mixed_table()
    perm = np.random.default_rng(2).permutation(len(V))
    a = check(ctx, V, 14, "identity", rtol=1e-6)
    b = check(ctx, V[perm], 14, "permuted", rtol=1e-6)
    assert not np.array_equal(a["leader"], b["leader"]) and sorted(a["count"].tolist()) == sorted(b["count"].tolist())
    # on the non-transitive chain the order decides the grouping itself
    chain = np.array([[0.0], [0.75], [1.5]])
    assert check(ctx, chain, 1, "chain", atol=1.0, rtol=0.0)["label"].tolist() == [0, 0, 1]
    assert check(ctx, chain[[1, 0, 2]], 1, "chain, middle first", atol=1.0, rtol=0.0)["label"].tolist() == [0, 0, 0]


def test_both_flavours_the_host_form_and_the_python_form_give_the_same_bits(ctx):
    V = mixed_table()
    B = len(V)
    mask = np.ones(B, dtype=np.int32)
    mask[10:20] = 0
    kw = dict(mask=mask, atol=1e-12, rtol=1e-6, max_groups=3)             # 4 roots, 3 groups: overflow too
    want = run_dev(ctx, V, 14, **kw)
    check_whole(want, gr.group_reference(V, n=14, **kw), "reference order")
    fast = context("fast")
    for got, what in ((run_dev(fast, V, 14, **kw), "throughput flavour"), (run_host(ctx, V, 14, **kw), "host form"), (run_host(fast, V, 14, **kw), "host form, throughput flavour")):
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), what
    fast.close()
    r = ctx.group_batch(V, n=14, **kw)
    G = int(want[4][0])
    assert G == 3 and np.array_equal(r["label"], want[0][:B]) and np.array_equal(r["summary"], want[4][:4]) and r["summary"][1] > 0
    assert np.array_equal(r["leader"], want[1][:G]) and np.array_equal(r["count"], want[2][:G]) and np.array_equal(r["radius"].view(np.uint64), want[3][:G])
    # n defaults to the whole row
    r = ctx.group_batch(V[:, :14], rtol=1e-6)
    assert np.array_equal(r["label"], gr.group_reference(V[:, :14], rtol=1e-6)["label"])


def test_an_empty_table(ctx):
    ref = gr.group_reference(np.zeros((0, 5)), n=3, max_groups=6)
    l0 = ctx.counters()[1]
    check_whole(run_dev(ctx, np.zeros((0, 5)), 3, max_groups=6), ref, "B = 0, _dev")
    assert ctx.counters()[1] == l0 + 1
    check_whole(run_host(ctx, np.zeros((0, 5)), 3, max_groups=6), ref, "B = 0, host")
    # B == 0 needs neither a table nor labels
    bufs = outputs(0, 6)
    assert ctx.L.socp_group_batch(ctx.h, 0, 3, 5, None, None, 0.0, 1e-6, 6, None, bufs[1].ctypes.data_as(IP), bufs[2].ctypes.data_as(IP),
                                  bufs[3].ctypes.data_as(DP), bufs[4].ctypes.data_as(IP)) == 0
    check_whole(views(bufs), ref, "B = 0, NULL table and labels")
    r = ctx.group_batch(np.zeros((0, 5)), n=3)
    assert r["summary"].tolist() == [0, 0, 0, 0] and len(r["label"]) == len(r["leader"]) == len(r["count"]) == len(r["radius"]) == 0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_say_why_and_write_nothing(ctx):
    from socp_amd import capi
    V = np.ascontiguousarray(mixed_table()[:20])
    B, ld, n = 20, 16, 14
    L, h = ctx.L, ctx.h
    fresh = views(outputs(B, 8))
    before = ctx.counters()

    def host(B_=B, n_=n, ld_=ld, V_=V.ctypes.data_as(DP), atol=0.0, rtol=1e-6, mg=8, null=None):
        bufs = outputs(B, 8)
        ptrs = [b.ctypes.data_as(DP if b.dtype == np.float64 else IP) for b in bufs]
        if null is not None:
            ptrs[null] = None
        rc = L.socp_group_batch(h, B_, n_, ld_, V_, None, atol, rtol, mg, *ptrs)
        assert all(np.array_equal(g, w) for g, w in zip(views(bufs), fresh)), "a refused call wrote into an output"
        return rc, L.socp_last_error(h).decode()
    sizes = "B >= 0, n >= 1, ld >= n and max_groups >= 1"
    for kw in (dict(B_=-1), dict(n_=0), dict(n_=-3), dict(ld_=13), dict(mg=0), dict(mg=-2)):
        rc, msg = host(**kw)
        assert rc == capi.ERR_ARG and sizes in msg, (kw, msg)
    for kw in (dict(atol=-1e-300), dict(rtol=-1.0), dict(atol=np.nan), dict(rtol=np.nan), dict(atol=np.inf), dict(rtol=np.inf)):
        rc, msg = host(**kw)
        assert rc == capi.ERR_ARG and "finite and not negative" in msg, (kw, msg)
    for k in range(5):
        rc, msg = host(null=k)
        assert rc == capi.ERR_ARG and "null output pointer" in msg, (NAMES[k], msg)
    rc, msg = host(V_=None)
    assert rc == capi.ERR_ARG and "null table" in msg
    # the _dev form: the same checks, before anything is enqueued (the pointers are never dereferenced)
    fake = C.c_void_p(256)
    dev = lambda B_=B, n_=n, ld_=ld, V_=fake, atol=0.0, rtol=1e-6, mg=8, outs=(fake,) * 5: L.socp_group_batch_dev(h, B_, n_, ld_, V_, None, atol, rtol, mg, *outs)  # noqa: E731
    for kw in (dict(B_=-1), dict(n_=0), dict(ld_=13), dict(mg=0), dict(atol=-1.0), dict(rtol=np.nan), dict(V_=None)):
        assert dev(**kw) == capi.ERR_ARG, kw
    for k in range(5):
        assert dev(outs=tuple(None if j == k else fake for j in range(5))) == capi.ERR_ARG and "null output pointer" in L.socp_last_error(h).decode()
    with pytest.raises(capi.SocpError, match="max_groups >= 1"):
        ctx.group_batch(V, n=14, max_groups=0)
    with pytest.raises(capi.SocpError, match="not negative"):
        ctx.group_batch(V, n=14, rtol=-1e-6)
    assert ctx.counters() == before, "the refused calls launched nothing"
    # a valid call afterwards gives the reference's bits
    check(ctx, V, n, "after the refused calls", rtol=1e-6)


# ---- 6. the sweep tool --------------------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_roots_of_its_sweep(tmp_path):
    out = str(tmp_path / "roots")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "100", "--roots-out", out],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["roots"]
    assert sorted(entry) == sorted(["groups", "overflow", "largest_count", "radius_max", "best_cost", "best_root", "rtol", "atol", "wall_s", "file"])
    assert entry["file"] == out + ".npz" and entry["rtol"] == 1e-6 and entry["atol"] == 0.0 and "solution_spread_rel" in rec
    npz = np.load(entry["file"])
    assert sorted(npz.files) == ["cost", "count", "label", "leader", "radius", "z"]
    label, leader, count, z, cost = npz["label"], npz["leader"], npz["count"], npz["z"], npz["cost"]
    G = entry["groups"]
    assert G >= 1 and label.shape == (64,) and leader.shape == count.shape == npz["radius"].shape == cost.shape == (G,) and z.shape == (G, 14)
    assert np.array_equal(np.bincount(label[label >= 0], minlength=G), count)
    assert np.array_equal(label[leader], np.arange(G)) and np.all(np.diff(leader) > 0)
    assert count.sum() + entry["overflow"] == rec["converged"] > 0
    assert np.sum(label == -3) == 64 - rec["converged"] and np.sum(label == -1) == entry["overflow"]
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(cost))
    assert entry["largest_count"] == count.max() and entry["radius_max"] == npz["radius"].max()
    assert entry["best_root"] == int(np.argmin(cost)) and entry["best_cost"] == float(cost.min())
