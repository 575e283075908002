"""GPU: bench.py prints exactly one JSON line with the fields the driver reads, and the numbers hang together."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(out):
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_line_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--starts", "4096",
                          "--cpu-seconds", "2", "--sweep-starts", "2048", "--sweep-c5-starts", "512"], capture_output=True, text=True, timeout=900)
    d = _line(out)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "exact", "parity", "single_problem",
                "north_star_128", "sweep"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["dtype"] == "f64"
    assert d["vs_baseline"] is None and d["higher_is_better"] is True and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    per_step = d["config"]["trajectories_per_step_per_gpu"]
    assert abs(d["value"] - per_step / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source"):
        assert key in r, key
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] <= 1.0
    # the algorithmic flops of a launch follow from the line itself, whatever --rk4-steps is
    assert r["flop_per_trajectory"] == r["flop_per_rk4_step"] * d["config"]["rk4_steps"]
    assert abs(r["achieved"] - r["flop_per_trajectory"] * per_step / (r["kernel_ms"] * 1e-3) / 1e12) <= 1e-9 * r["achieved"]
    # the traffic figure is the PMC counters of THIS run (two child runs under rocprofv3 --pmc); the recorded figure
    # stays beside it.  One launch moves at least z in and the rows out, and not much more.
    assert "traffic_recorded" in r and "traffic_live_measurement" in r
    if r["traffic_measured_in_this_run"]:
        assert "MEASURED IN THIS RUN" in r["traffic_source"] and r["traffic_live_measurement"] == "ok"
        alg = 4096 * (14 * 8 + 15 * 14 * 8)
        assert 0.9 * alg <= r["traffic"] <= 3.0 * alg, (r["traffic"], alg)
    else:
        # (a box on which the profiler cannot collect counters: the line must say why and fall back to the recorded figure -- the
        # bench itself never depends on the profiler; tests/test_bench_live_traffic.py covers the failure paths on the CPU)
        import warnings
        warnings.warn("bench.py could not measure the traffic in its run: " + str(r["traffic_live_measurement"]))
        assert "rocprofv3" in r["traffic_live_measurement"] and r["traffic"] == r["traffic_recorded"]["bytes"]
    assert r["kernel_ms"] <= d["ms_per_step"] * 1.05                 # the kernel is (nearly all of) the step
    assert r["hbm"]["bound"] == "hbm" and r["hbm"]["peak"] == 8000.0
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    # the bit-identical flavour beside the headline one, and the in-run parity of both against the oracle
    assert d["config"]["variant"] == "fast" and d["exact"]["value"] > 0 and 0 < d["exact"]["roofline_frac"] < d["roofline"]["frac"]
    p = d["parity"]
    assert p["pass"] is True and p["rows_checked"] >= 15
    assert p["fast"]["max_rel_err"] <= 1e-8
    assert p["exact"]["max_rel_err"] <= 1e-10
    assert set(d["single_problem"]) >= {"fast", "exact", "trajectories"}
    ns = d["north_star_128"]
    assert ns["unknowns"] == 128 and ns["fast"]["full"]["trajectories_integrated"] == 128 * 9
    assert ns["fast"]["dedup"]["trajectories_integrated"] < ns["fast"]["full"]["trajectories_integrated"]
    assert ns["fast"]["full"]["finite"] and ns["exact"]["full"]["finite"]
    if "b0" in c:
        assert c["b0"]["info"] == 1 and c["b0"]["value"] > 0
    # the strong-scaling leg: a fixed total of starts, solved
    sw = d["sweep"]
    assert sw["scaling"] == "strong" and sw["total_starts"] == 2048 and sw["n_gpus"] == 1 and sw["converged"] >= 2030
    assert abs(sw["solves_per_s"] - 2048 / sw["wall_s"]) <= 1e-6 * sw["solves_per_s"] and sw["trajectories"] > 2048 * 15
    big = d["sweep_large"]
    assert big["total_starts"] == 8 * 2048 and big["scaling"] == "strong" and big["converged"] >= 8 * 2030
    # the leg whose per-rank share at N = 8 equals the large leg's total, and the expectation for 2 / 4 / 8 GPUs read off this run's
    # one-GPU curve (VERDICT r3 #1a): the eighth-size sweep is measured so that the smallest leg has a point to be read from
    xl = d["sweep_xl"]
    assert xl["total_starts"] == 64 * 2048 and xl["converged"] >= 64 * 2030
    curve = d["sweep_curve_one_gpu"]["curve"]
    assert [c[0] for c in curve] == [256, 2048, 8 * 2048, 64 * 2048]
    for leg in (sw, big, xl):
        pr = leg["predicted"]
        assert set(pr) == {"2", "4", "8"} and pr["2"]["wall_s"] >= pr["4"]["wall_s"] >= pr["8"]["wall_s"] > 0
        assert pr["8"]["speedup"] <= 8.0 + 1e-9 and leg["prediction_source"] == "this run"
    assert abs(xl["predicted"]["8"]["wall_s"] - big["wall_s"]) <= 1e-9 * big["wall_s"]          # a rank's block of 8 IS the large leg
    # BASELINE config 5 as a strong-scaling leg of its own family (parity unpinned, and labelled so), with its own one-GPU curve
    c5 = d["sweep_config5"]
    assert c5["total_starts"] == 512 and c5["scaling"] == "strong" and c5["converged"] >= 500 and "UNPINNED" in c5["workload"]
    assert [q[0] for q in d["sweep_curve_one_gpu"]["curve_config5"]] == [64, 512] and d["sweep_config5_eighth"]["total_starts"] == 64
    assert set(c5["predicted"]) == {"2", "4", "8"} and abs(c5["predicted"]["8"]["wall_s"] - d["sweep_config5_eighth"]["wall_s"]) <= 1e-12
    g = c["gpu_ratios"]
    # the CPU figures are medians of >= 5 samples with the spread in the record, and the 128-unknown leg carries the
    # ratio that does not swing with the host's other tenants beside the all-core one
    assert c["value"] == c["median"] and c["worst"] <= c["median"] <= c["best"] and len(c["samples"]) >= 5 and c["spread"] >= 0
    assert c["p1"]["value"] == c["p1"]["median"] and len(c["p1"]["samples"]) >= 5 and c["p1"]["spread"] >= 0
    for tag in ("fast", "exact"):
        assert abs(ns[tag]["x_over_16xP1"] - ns[tag]["reference_trajectories_per_s"] / (16 * c["p1"]["value"])) <= 1e-9 * ns[tag]["x_over_16xP1"]
        assert abs(ns[tag]["x_over_cpu_baseline"] - ns[tag]["reference_trajectories_per_s"] / c["value"]) <= 1e-9 * ns[tag]["x_over_cpu_baseline"]
    assert abs(g["headline_over_16xP1"] - d["value"] / (16 * c["p1"]["value"])) <= 1e-9 * g["headline_over_16xP1"]
    assert "reference_trajectories_per_s" in ns["fast"] and "trajectories_per_s" not in ns["fast"]
    assert ns["fast"]["integrated_trajectories_per_s"] <= ns["fast"]["reference_trajectories_per_s"]
    # the sweeps' second kernel with a roofline of its own: the matrix-core Jacobian refresh
    ff = d["solver_kernels"]["factor_fast"]
    assert ff["kernel_ms"] > 0 and 0 < ff["roofline"]["frac"] < 1 and ff["roofline"]["bound"] == "mfma_fp64"
    assert abs(ff["roofline"]["frac"] - ff["roofline"]["achieved"] / ff["roofline"]["peak"]) < 1e-12
    assert ff["roofline"]["traffic"] is None or ff["roofline"]["traffic_over_algorithmic"] > 1.0
    # ... its traffic from this run's counters too (the qrfac and the qform launch summed), the recorded figure beside it
    assert "traffic_recorded" in ff["roofline"] and "traffic_live_measurement" in ff["roofline"]
    if ff["roofline"]["traffic_measured_in_this_run"]:
        assert 2.0 < ff["roofline"]["traffic_over_algorithmic"] < 8.0
    assert ff["roofline"]["traffic_measured_in_this_run"] in (True, False) and (r["traffic_measured_in_this_run"] or not ff["roofline"]["traffic_measured_in_this_run"])
    # CPU baseline as SURVEY 8d asks: one thread and all cores, pinned; the host is named
    assert c["p1"]["cores"] == 1 and c["p1"]["value"] > 0 and c["cores"] >= c["p1"]["cores"] and c["pinned"] in (True, False)
    assert isinstance(c["cpu_model"], str) and c["cpu_model"]


def test_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) times the headline steps and nothing else; --dump-outputs writes what the last timed step left in HBM
    -- the FD rows and the Jacobians formed from them -- and two runs with the same arguments write the same arrays."""
    import numpy as np
    from socp_amd.sweep import goddard_starts
    lines, dirs = [], []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--starts", "1024",
                              "--rk4-steps", "1000", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        lines.append(_line(out))
        dirs.append(d)
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert abs(d["value"] - 1024 * 15 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for key in ("exact", "parity", "single_problem", "north_star_128", "cpu_baseline", "solver_kernels", "sweep", "sweep_config5"):
        assert key not in d, key
    assert d["roofline"]["traffic_measured_in_this_run"] is False and d["roofline"]["kernel_ms"] <= d["ms_per_step"] * 1.05
    rows, jac = (np.load(dirs[0] / n) for n in ("residual_rows.npy", "jacobians.npy"))
    assert rows.dtype == np.float64 and rows.shape == (1024, 15, 14) and jac.dtype == np.float64 and jac.shape == (1024, 14, 14)
    assert not (dirs[0] / "sample_starts.npy").exists()
    assert int(np.isfinite(jac).all(axis=(1, 2)).sum()) == d["finite_jacobians"][0] == 1024
    # jac[p][j] = (row j + 1 - row 0) / h_j, h_j = sqrt(epsfcn) |z_j| with bench's epsfcn = 1e-15 (socp_fd_diff_dev), z the run's
    # rank-0 starts (none of them has a zero component)
    h = np.sqrt(1e-15) * np.abs(goddard_starts(1024, 1e-3, 20250905))
    assert np.allclose(jac, (rows[:, 1:, :] - rows[:, :1, :]) / h[:, :, None], rtol=1e-13, atol=0.0)
    for n in ("residual_rows.npy", "jacobians.npy"):
        assert np.array_equal(np.load(dirs[0] / n), np.load(dirs[1] / n)), n


def test_gpus_2_really_runs_two_ranks():
    """`python bench.py --gpus 2` (no launcher): the parent starts two ranks; here both share device 0 and the collectives
    run over gloo (a one-GPU box), the code path is otherwise the N > 1 path of the driver."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo", "--share-device0",
                          "--steps", "2", "--warmup", "1", "--starts", "1024", "--rk4-steps", "1000", "--sweep-starts", "301", "--sweep-c5-starts", "65"],
                         capture_output=True, text=True, timeout=900)
    d = _line(out)
    # the sweep leg at N = 2: a FIXED total (odd: blocks of 151 + 150), every start reported once
    assert d["sweep"]["n_gpus"] == 2 and d["sweep"]["total_starts"] == 301 and d["sweep"]["starts_per_gpu"] == 151
    assert d["sweep"]["converged"] + d["sweep"]["stopped_by_round_limit"] >= 295
    assert d["n_gpus"] == 2 and d["ranks_reported"] == 2 and len(d["finite_jacobians"]) == 2
    assert d["finite_jacobians"] == [1024, 1024]
    assert d["config"]["trajectories_per_step_per_gpu"] == 1024 * 15
    assert abs(d["value"] - 2 * 1024 * 15 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert "cpu_baseline" not in d and "exact" not in d               # N = 1 extras only
    # 1000-step trajectories: a tenth of the flops per trajectory, so the fraction stays below 1 whatever the step count
    assert d["roofline"]["flop_per_trajectory"] == 1170.0 * 1000 and 0 < d["roofline"]["frac"] <= 1.0
    assert d["sweep_xl"]["total_starts"] == 64 * 301 and "sweep_eighth" not in d
    c5 = d["sweep_config5"]
    assert c5["n_gpus"] == 2 and c5["total_starts"] == 65 and c5["starts_per_gpu"] == 33 and c5["converged"] >= 60
    assert "sweep_config5_eighth" not in d


def test_rccl_code_path_with_one_rank():
    """The N > 1 path talks to RCCL (torch.distributed backend "nccl"): process-group creation with a device id, barrier,
    all_reduce(MAX) of the timing and all_gather of the result records on DEVICE tensors.  A one-GPU box cannot host two RCCL
    ranks, so this runs that exact code with a world of one (--force-dist); the two-rank plumbing is the gloo test above."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--force-dist", "--lean", "--steps", "2", "--warmup", "1",
                          "--starts", "1024", "--rk4-steps", "1000", "--cpu-seconds", "0", "--sweep-starts", "200", "--sweep-c5-starts", "48"],
                         capture_output=True, text=True, timeout=900)
    d = _line(out)
    # the sweep leg's barrier / all_reduce(MAX, SUM) / gather over RCCL too (a world of one)
    assert d["sweep"]["total_starts"] == 200 and d["sweep"]["n_gpus"] == 1 and d["sweep"]["converged"] >= 195
    assert d["sweep_config5"]["total_starts"] == 48 and d["sweep_config5"]["converged"] >= 44
    assert d["n_gpus"] == 1 and d["ranks_reported"] == 1 and d["finite_jacobians"] == [1024]
    assert abs(d["value"] - 1024 * 15 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]


def test_four_rank_rehearsal_of_the_driver_job():
    """keep the 8-GPU path one command from a measurement.  The driver's job is `bench.py --gpus 8`, one rank per GPU;
    no 8-GPU node can be asked for here, and a one-GPU box admits at most SIX processes on its card (gpurun's process guard: this
    test runner is one of them), so the rehearsal on the card is four ranks sharing device 0, collectives over gloo -- the N > 1
    code path of the driver otherwise (self-launch, rendezvous, barrier + max over ranks, one gather of the records, the
    strong-scaling legs sharded in contiguous blocks of an ODD total).  Every rank reports, every strong-scaling leg states what
    the recorded one-GPU curve expects of it (`expected`) and how the measurement compares (`measured_over_expected`).  (EIGHT
    ranks of the same plumbing run on the CPU: tests/test_sweep_gloo.py; eight emulated ranks through the C++ entry points:
    test_gpu_multistart.py.)"""
    W = 4
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(W), "--backend", "gloo", "--share-device0",
                          "--steps", "1", "--warmup", "1", "--starts", "256", "--rk4-steps", "1000", "--sweep-starts", "301", "--sweep-c5-starts", "67"],
                         capture_output=True, text=True, timeout=1200)
    d = _line(out)
    assert d["n_gpus"] == W and d["ranks_reported"] == W and d["finite_jacobians"] == [256] * W
    assert abs(d["value"] - W * 256 * 15 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    legs = [d[k] for k in ("sweep", "sweep_large", "sweep_xl", "sweep_config5")]
    for leg in legs:
        assert leg["scaling"] == "strong" and leg["n_gpus"] == W
        assert leg["starts_per_gpu"] == -(-leg["total_starts"] // W)                 # the largest block of the contiguous split
        assert leg["converged"] + leg.get("stopped_by_round_limit", 0) >= 0.95 * leg["total_starts"]
    assert d["sweep"]["total_starts"] == 301 and d["sweep_config5"]["total_starts"] == 67
    # the expectation: present whenever a recorded curve applies (the Goddard legs' curve is recorded for 10^4 steps: a 1000-step
    # rehearsal has none and says so; config 5 has no step count and always has one)
    c5 = d["sweep_config5"]
    assert set(c5["expected"]) >= {"wall_s", "one_gpu_wall_s", "speedup", "measured_over_expected"} and c5["expected"]["measured_over_expected"] > 0
    assert "RECORDED" in c5["prediction_source"]
    for leg in legs[:3]:
        assert ("expected" in leg and leg["expected"]["measured_over_expected"] > 0) or "prediction_source" not in leg
