"""CPU: the definition of socp_newton_batch (include/socp_hip.h) as tests/newton_reference.py restates it -- no library call.  What
the GPU tests compare the device with is checked here on its own: perturbed starts converge, every status is reached by
construction, and three wrong restatements are caught.  The histories the tests print are kept in profiles/newton_cpu_tests.txt."""
import numpy as np
import pytest

import newton_cases as nc
import newton_reference as nr

# perturbation and ftol per case: rounding level of the case's residual (the polished root's rn: 5.4e-14, 2.3e-12, 1.4e-14) times
# at least 40, and a start close enough for single shooting (1e-6 relative already gives ||F||inf = 7e-3 .. 1e-2 on Goddard)
CASES = {"goddard_mu2_1": (lambda: nc.goddard(1.0), 1e-7, 1e-11, 8), "goddard_mu2_0.2": (lambda: nc.goddard(0.2), 1e-7, 1e-10, 8),
         "dint": (nc.dint, 1e-3, 1e-12, 8)}
RECORD = ((1e-7, 1), (1e-7, 2), (1e-8, 1))               # (relative perturbation, seed) of the recorded histories
BAR = 1e-11                                               # "steps to bring rn below" of the record


def run(c, z, mutate=(), **opts):
    r = nr.newton_reference(c["model"], c["o"], c["prob"], c["nparams"], c["N"], np.atleast_2d(z), opts, mutate=mutate)
    return {k: v[0] for k, v in r.items()}


def steps_to(rhist, bar):
    below = np.nonzero(rhist <= bar)[0]
    return int(below[0]) if len(below) else None


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("jac", [0, 2])
def test_perturbed_starts_converge(name, jac):
    build, rel, ftol, rounds = CASES[name]
    c = build()
    assert c["floor"] * 40 <= ftol, "ftol stands clear of the rounding level the polished root shows"
    q = run(c, nc.perturbed(c["root"], rel, 1), jac=jac, ftol=ftol, rounds=rounds, trials=4)
    print("%s jac %d: %s after %d steps (nhalf %d), rhist %s, dnorm %.2e" % (name, jac, nr.STATUS_NAMES[q["status"]], q["iters"], q["nhalf"],
                                                                             ["%.1e" % v for v in q["rhist"][:q["iters"] + 1]], q["dnorm"]))
    assert q["status"] == nr.CONVERGED and 1 <= q["iters"] <= rounds and q["rnorm"] <= ftol
    assert q["rnorm"] == np.max(np.abs(q["f"])) == q["rhist"][q["iters"]] and np.all(np.isnan(q["rhist"][q["iters"] + 1:]))
    assert np.max(np.abs(q["z"] - c["root"])) <= 1e-6 * np.max(np.abs(c["root"])), "the same root"


def test_forward_difference_against_exact_record():
    """The rounds and the final rn the forward difference needs against the exact matrix, to rounding level (ftol = 1e-300).
    The record (profiles/newton_cpu_tests.txt): with mu2 = 1 the two matrices need the same number of steps to bring rn below 1e-11
    (2/2, 3/3, 2/1) -- no ordering is asserted there.  With mu2 = 0.2 the forward-difference iteration is linear (rn falls by about 25
    per step) and the exact one quadratic: 4/2, 5/3 and 4/2 steps.  Asserted: at mu2 = 0.2 the exact matrix needs strictly fewer steps
    in every recorded case -- the record's margin is 2 steps in each."""
    for mu2 in (1.0, 0.2):
        c = nc.goddard(mu2)
        for rel, seed in RECORD:
            k = {}
            for jac in (0, 2):
                q = run(c, nc.perturbed(c["root"], rel, seed), jac=jac, ftol=1e-300, rounds=30, trials=8)
                k[jac] = steps_to(q["rhist"], BAR)
                print("mu2 %g rel %g seed %d jac %d: %s, %d steps, rn %.2e, below %.0e after %s, rhist %s"
                      % (mu2, rel, seed, jac, nr.STATUS_NAMES[q["status"]], q["iters"], q["rnorm"], BAR, k[jac], ["%.1e" % v for v in q["rhist"][:q["iters"] + 1]]))
                assert q["status"] == nr.STALLED and q["rnorm"] <= 1e-11
            if mu2 == 0.2:
                assert k[2] < k[0], (rel, seed, k)


def test_every_status_is_reached_by_construction():
    c = nc.goddard(1.0)
    start = nc.perturbed(c["root"], 1e-7, 2)
    q = run(c, start, ftol=1e-11, rounds=1)
    assert q["status"] == nr.RUNNING and q["iters"] == 1 and q["rnorm"] > 1e-11
    q = run(c, start, ftol=1e-300, rounds=30, trials=8)
    assert q["status"] == nr.STALLED and q["rnorm"] <= 1e-12, "as good as this arithmetic gets"
    bad = start.copy()
    bad[9] = np.nan
    q = run(c, bad)
    assert q["status"] == nr.BAD_START and q["iters"] == 0 and np.isnan(q["rnorm"]) and np.isnan(q["dnorm"]) and np.array_equal(q["z"], bad, equal_nan=True)
    q = run(c, c["root"], ftol=1e-11)
    assert q["status"] == nr.CONVERGED and q["iters"] == 0 and q["rounds_used"] == 0 and np.isnan(q["dnorm"]) and np.all(np.isnan(q["rhist"][1:]))
    q = run(c, start, ftol=1e-300, xtol=1e-3)
    assert q["status"] == nr.SMALL_STEP and q["iters"] == 1 and q["dnorm"] <= 1e-3 * np.max(np.abs(q["z"]))
    # tests/plugin/fold1d_plugin.hip restated (RK4 is exact on its constant right-hand side): F = [x0 ; x0 + p0^2 + a - 1], at its fold
    a = 0.5
    fold = lambda z: np.array([z[0], z[0] + z[1] * z[1] + a - 1.0])                     # noqa: E731
    fold_j = lambda z, F0: np.array([[1.0, 0.0], [1.0, 2.0 * z[1]]])                    # noqa: E731
    q = nr.polish(fold, fold_j, [0.0, 0.0], dict(rounds=5))
    assert q["status"] == nr.SINGULAR and q["iters"] == 0 and np.isnan(q["dnorm"]) and q["rnorm"] == 0.5 and np.array_equal(q["z"], [0.0, 0.0])
    q = nr.polish(fold, fold_j, [0.0, 0.5], dict(rounds=20, ftol=1e-15))
    assert q["status"] == nr.CONVERGED and abs(q["z"][1] - np.sqrt(0.5)) <= 1e-15
    # a crafted zero column on the Goddard row
    rs, js = nr.row_callables("goddard", c["o"], c["prob"], 8, c["N"], np.concatenate([c["params"], [0.0, 0.0]]), c["prob"], 0, 1e-15)

    def zero_column(z, F0):
        J = js(z, F0)
        J[:, 5] = 0.0
        return J
    q = nr.polish(rs, zero_column, start, dict(rounds=5))
    assert q["status"] == nr.SINGULAR and np.array_equal(q["z"], start)


def test_the_mixed_batch_holds_all_six_statuses():
    m = nc.mixed()
    ref, first = m["ref"], {name: m["names"].index(name) for name in set(m["names"])}
    for name, b in sorted(first.items(), key=lambda kv: kv[1]):
        print("mixed %-5s (row %2d): %-10s iters %d nhalf %d rn %.2e dnorm %.2e" % (name, b, nr.STATUS_NAMES[ref["status"][b]], ref["iters"][b],
                                                                                  ref["nhalf"][b], ref["rnorm"][b], ref["dnorm"][b]))
    want = dict(root=nr.CONVERGED, near=nr.SMALL_STEP, near2=nr.CONVERGED, mid=nr.RUNNING, mid2=nr.RUNNING, far=nr.STALLED, nan=nr.BAD_START,
                flat=nr.SINGULAR)
    assert {k: int(ref["status"][b]) for k, b in first.items()} == want
    assert ref["iters"][first["root"]] == 0 and len(set(ref["rounds_used"].tolist())) >= 4, "rows finish in rounds of their own"


def test_wrong_restatements_are_caught():
    # F = atan z from 1.2: the full step lands at -0.94 with |F| = 0.86 rn -- below rn, above c_0 rn = 0.75 rn -- and the half step passes
    f = lambda z: np.arctan(z)                                                          # noqa: E731
    j = lambda z, F0: np.array([[1.0 / (1.0 + z[0] * z[0])]])                           # noqa: E731
    opts = dict(rounds=8, ftol=1e-15, trials=4)
    good = nr.polish(f, j, [1.2], opts)
    assert good["status"] == nr.CONVERGED and good["nhalf"] == 1 and abs(good["z"][0]) <= 1e-15
    no_ck = nr.polish(f, j, [1.2], opts, mutate=("no_ck",))
    assert no_ck["nhalf"] == 0 and no_ck["rhist"][1] != good["rhist"][1], "the bar without c_k takes the full step"
    desc = nr.polish(f, j, [1.2], opts, mutate=("descending",))
    assert desc["nhalf"] > good["nhalf"] and desc["rhist"][1] != good["rhist"][1], "descending trials take the shortest step first"
    c = nc.goddard(1.0)
    start = nc.perturbed(c["root"], 1e-7, 2)
    want = run(c, start, ftol=1e-11, rounds=8)
    for mutation in nr.MUTATIONS:
        got = run(c, start, mutate=(mutation,), ftol=1e-11, rounds=8)
        same = all(np.array_equal(got[k], want[k], equal_nan=True) for k in ("z", "f", "rnorm", "dnorm", "iters", "nhalf", "status", "rhist"))
        print("goddard, mutation %s: %s after %d steps, rhist %s" % (mutation, nr.STATUS_NAMES[got["status"]], got["iters"],
                                                                     ["%.1e" % v for v in got["rhist"][:got["iters"] + 1]]))
        assert not same or mutation == "no_ck", mutation                               # no_ck shows on marginal steps only: the atan row above
    stale = run(c, start, mutate=("stale_f0",), ftol=1e-11, rounds=8)
    assert stale["status"] != nr.CONVERGED or stale["iters"] > want["iters"], "a stale F0 repeats the first step"
