"""CPU: the instrument that pins the throughput flavour (tests/fast_reference.py, tests/golden/fast_pin.npz) is itself checked
before any kernel is judged by it.

  * the reference-order oracle, in its double arithmetic, stays within B_ref of the stored value on every decidable row: the error
    model covers a correct implementation;
  * the fast structure emulated in numpy.float64 stays within B_fast;
  * three deliberately wrong emulations (1/sqrt truncated to 40 bits, exp scaled by 1 + 1e-13, one gravity-gradient sign flipped)
    each VIOLATE B_fast: the bound is tight enough to be worth having;
  * with mpmath present, sixteen rows evaluated afresh equal the stored fixture bit for bit."""
import os
import sys

import numpy as np
import pytest

import fast_reference as fr
from oracle.oracle import Oracle, MODEL_GODDARD, MODEL_COVID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "fast_pin.npz"))
GROUPS = [str(g) for g in FIX["group_names"]]
MODELS = {"goddard": ("g_", MODEL_GODDARD), "covid": ("c_", MODEL_COVID)}


def rows_of(model, group=None):
    p = MODELS[model][0]
    idx = np.arange(len(FIX[p + "X"]))
    if group is not None:
        idx = idx[FIX[p + "group"] == GROUPS.index(group)]
    return idx


def row(model, i):
    p = MODELS[model][0]
    return FIX[p + "blocks"][FIX[p + "block"][i]], FIX[p + "sw"][i], FIX[p + "t"][i], FIX[p + "X"][i]


def ratios(got, val, B):
    """|got - val| / B per component, 0 where both vanish (a bound of zero demands equality)."""
    err = np.abs(got - val)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, err / B)


def report(title, model, idx, r):
    p = MODELS[model][0]
    for g in sorted(set(FIX[p + "group"][idx])):
        sel = FIX[p + "group"][idx] == g
        print("%s %-14s max err/B per component: %s" % (title, GROUPS[g], " ".join("%.3f" % v for v in r[sel].max(axis=0))))


def test_fixture_shape():
    total = len(FIX["g_X"]) + len(FIX["c_X"])
    und = len(FIX["g_und"]) + len(FIX["c_und"])
    assert 0 < und <= 0.02 * total
    assert np.array_equal(np.flatnonzero(~FIX["g_dec"]), FIX["g_und"]) and np.array_equal(np.flatnonzero(~FIX["c_dec"]), FIX["c_und"])
    assert set(GROUPS[g] for g in FIX["g_group"]) | set(GROUPS[g] for g in FIX["c_group"]) == set(GROUPS)
    assert np.all(np.isfinite(FIX["g_val"])) and np.all(np.isfinite(FIX["c_val"]))
    # every arc of the bang / singular / off law, both singular forms, both sides of every clamp
    g0 = FIX["g_blocks"][FIX["g_block"], 6] == 0
    t, sw = FIX["g_t"][g0], FIX["g_sw"][g0]
    assert np.any(t <= sw[:, 0]) and np.any((t > sw[:, 0]) & (t <= sw[:, 1])) and np.any(t > sw[:, 1])
    assert {-1.0, 0.6} <= set(FIX["g_blocks"][:, 7])
    cu = FIX["c_u"][:, 0]
    assert np.any(cu == -10) and np.any(cu == 20) and np.any((cu > -10) & (cu < 20))
    cI = FIX["c_X"][:, 2] - FIX["c_blocks"][FIX["c_block"], 4]
    assert np.any(cI > 0) and np.any(cI < 0) and np.any(cI == 0)
    sub = rows_of("goddard", "air_subnormal")
    r = np.linalg.norm(FIX["g_X"][sub, 0:3], axis=1)
    assert np.sum(np.exp(-500.0 * (r - 1)) < 2.0 ** -1022) >= 14


@pytest.mark.parametrize("model", ["goddard", "covid"])
def test_oracle_within_b_ref(built, model, capsys):
    p, mid = MODELS[model]
    o = Oracle(mid)
    idx = rows_of(model)[FIX[p + "dec"]]
    got = np.empty((len(idx), FIX[p + "val"].shape[1]))
    gu = np.empty((len(idx), FIX[p + "u"].shape[1]))
    gh = np.empty(len(idx))
    for k, i in enumerate(idx):
        P, sw, t, X = row(model, i)
        o.set_params(P)
        o.set_switching(sw)
        with np.errstate(all="ignore"):
            got[k] = o.rhs(t, X)
            gu[k] = o.control(t, X)
            gh[k] = o.hamiltonian(t, X)[0]
    r = ratios(got, FIX[p + "val"][idx], FIX[p + "Bref"][idx])
    ru = ratios(gu, FIX[p + "u"][idx], FIX[p + "Bu"][idx])
    with capsys.disabled():
        print()
        report("oracle/B_ref", model, idx, r)
        report("control/B_u ", model, idx, ru)
    assert np.all(np.isfinite(got))
    assert np.all(r <= 1.0), np.argwhere(r > 1.0)[:5]
    assert np.all(ru <= 1.0), np.argwhere(ru > 1.0)[:5]
    if model == "goddard":
        rh = ratios(gh, FIX["g_H"][idx], FIX["g_BH"][idx])
        assert np.all(rh <= 1.0), np.argwhere(rh > 1.0)[:5]


def emulate(model, idx, **mutation):
    return np.array([fr.emulate_fast(model, *row(model, i), **mutation) for i in idx])


@pytest.mark.parametrize("model", ["goddard", "covid"])
def test_float64_emulation_within_b_fast(model, capsys):
    p = MODELS[model][0]
    idx = rows_of(model)[FIX[p + "dec"]]
    r = ratios(emulate(model, idx), FIX[p + "val"][idx], FIX[p + "Bfast"][idx])
    with capsys.disabled():
        print()
        report("float64/B_fast", model, idx, r)
    assert np.all(r <= 1.0), np.argwhere(r > 1.0)[:5]


def _truncated_rsqrt(x):
    y = np.float64(1.0) / np.sqrt(x)
    m, e = np.frexp(y)
    return np.ldexp(np.floor(m * 2.0 ** 40) / 2.0 ** 40, e)


@pytest.mark.parametrize("group,mutation,components", [
    ("iso_rsqrt", dict(rsqrt=_truncated_rsqrt), [3, 4, 5]),                                  # a lost correction step of 1/sqrt
    ("iso_exp", dict(exp=lambda x: np.exp(x) * np.float64(1 + 1e-13)), [3, 4, 5, 10, 11, 12]),   # an exp coefficient slightly off
    ("nominal", dict(flip_gravity_gradient=True), [7]),                                      # a wrong sign in the factored block
])
def test_mutations_violate_b_fast(group, mutation, components):
    """The instrument notices each of the defects it was built for, in the group built for it."""
    idx = rows_of("goddard", group)
    idx = idx[FIX["g_dec"][idx]]
    good = ratios(emulate("goddard", idx), FIX["g_val"][idx], FIX["g_Bfast"][idx])
    bad = ratios(emulate("goddard", idx, **mutation), FIX["g_val"][idx], FIX["g_Bfast"][idx])
    assert np.all(good <= 1.0)
    assert np.any(bad[:, components] > 1.0), bad[:, components].max(axis=0)


@pytest.mark.skipif(not fr.HAVE_MPMATH, reason="the generator's arithmetic (mpmath) is not installed")
def test_sixteen_rows_regenerate_bit_for_bit():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_fast_golden as gen
    n = gen.REGEN_ROWS
    for model, k in (("goddard", n - 4), ("covid", 4)):
        total = len(FIX[MODELS[model][0] + "X"])
        idx = np.unique(np.linspace(0, total - 1, k).astype(int))
        for stored, fresh in gen.regenerate(FIX, idx, model):
            assert np.array_equal(np.asarray(stored).view(np.uint8), np.asarray(fresh, dtype=np.asarray(stored).dtype).view(np.uint8))
