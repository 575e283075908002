"""Multi-start sweep (BASELINE config 4): P independent initial-costate starts of one shooting problem,
sharded over the ranks of a torch.distributed job -- one process per GPU -- solved locally in lock-step
(socp_multistart_solve) with NO data-path collective, then ONE small all_gather of the per-start
records {z*[n], |F|, info, nfev} (RCCL over xGMI when the backend is nccl; n = 14 -> 136 B per start).

    python -m torch.distributed.run --nproc-per-node N -m socp_amd.sweep --starts 4096 --rk4-steps 10000

Rank r owns the contiguous block of starts [r*P/W, (r+1)*P/W): the gathered table is in start order.
"""
import argparse
import json
import os
import time

import numpy as np

X0_STATE = np.array([0.999949994, 1e-4, 0.01, 1e-10, 1e-10, 1e-10, 1.0])          # testGoddard.cpp:53-59
PSTAR = np.array([-8.121947733, 7.775439382e-3, 0.7775438809, -0.4779369965, 5.715013318e-4,
                  5.715009222e-2, 9.958404873e-2])
TF = 0.2640825
GODDARD_PARAMS = [3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 1.0, -1.0]


def mt19937_64(seed, count):
    """`count` raw outputs of std::mt19937_64(seed) (the generator SURVEY 8d prescribes for the synthetic
    starts), as uint64."""
    NN, MM = 312, 156
    M64 = (1 << 64) - 1
    mt = [0] * NN
    mt[0] = seed & M64
    for i in range(1, NN):
        mt[i] = (6364136223846793005 * (mt[i - 1] ^ (mt[i - 1] >> 62)) + i) & M64
    out = np.empty(count, dtype=np.uint64)
    idx, k = NN, 0
    while k < count:
        if idx >= NN:
            for i in range(NN):
                x = (mt[i] & 0xFFFFFFFF80000000) | (mt[(i + 1) % NN] & 0x7FFFFFFF)
                mt[i] = mt[(i + MM) % NN] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
            idx = 0
        x = mt[idx]
        idx += 1
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000
        x ^= (x << 37) & 0xFFF7EEE000000000
        x ^= x >> 43
        out[k] = x & M64
        k += 1
    return out


def goddard_starts(P, eps, seed=20250905):
    """p = p*(1 + eps*xi), xi = (x >> 11) * 2^-53 * 2 - 1 from raw std::mt19937_64(seed) draws (SURVEY 8d
    "Synthetic inputs"); the SAME table on every rank, sliced by shard()."""
    raw = mt19937_64(seed, 7 * P)
    xi = ((raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 * 2.0 - 1.0).reshape(P, 7)
    Z = np.empty((P, 14))
    Z[:, :7] = X0_STATE
    Z[:, 7:] = PSTAR * (1.0 + eps * xi)
    return Z


def shard(P, rank, world):
    """Contiguous block of rank `rank`: sizes differ by at most one."""
    base, rem = divmod(P, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def goddard_single_shooting_problem(ctx, tf=TF):
    """BASELINE config 2/4 problem: n = 14, fixed tf, final velocity and mass free."""
    from . import capi
    mode_x = np.zeros((2, 7), dtype=np.int32)
    mode_x[1, 3:7] = capi.FREE
    X = np.zeros((2, 14))
    X[0, :7] = X0_STATE
    X[1, 0] = 1.01
    return ctx.problem_set([capi.FIXED, capi.FIXED], mode_x, np.array([0.0, tf]), X)


def goddard_multiple_shooting_problem(ctx, M, tf=TF):
    """The testGoddard layout (testGoddard.cpp:24-82) with M segments: initial state fixed, interior nodes
    CONTINUOUS, final altitude pinned at 1.01, final velocity and mass free, final time FREE: n = 14 M + 1."""
    from . import capi
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FREE]
    mode_x = np.zeros((M + 1, 7), dtype=np.int32)
    mode_x[1:M] = capi.CONTINUOUS
    mode_x[M, 3:7] = capi.FREE
    X = np.zeros((M + 1, 14))
    X[0, :7] = X0_STATE
    X[M, 0] = 1.01
    return ctx.problem_set(mode_t, mode_x, np.linspace(0.0, tf, M + 1), X)


def goddard_multiple_shooting_starts(ctx, Z14, M, tf=TF):
    """Unknown vectors [node states | tf] of the M-segment problem: node 0 = the start's perturbed initial state,
    nodes 1..M-1 = the converged trajectory re-gridded to M uniform segments (the set-up of the survey's
    convergence-basin probe), integrated on the device."""
    P = Z14.shape[0]
    Z = np.empty((P, 14 * M + 1))
    Z[:, :14] = Z14
    Z[:, -1] = tf
    if M > 1:
        star = np.concatenate([X0_STATE, PSTAR])[None, :]
        tk = np.linspace(0.0, tf, M + 1)[1:M]
        nodes = ctx.integrate_batch(np.zeros(M - 1), tk, np.repeat(star, M - 1, axis=0))
        Z[:, 14:14 * M] = nodes.reshape(1, 14 * (M - 1))
    return Z


def goddard_north_star_128_problem(ctx, M=9):
    """north_star's "128-unknown" Goddard layout: M = 9 segments, FREE final time plus ONE FREE interior time (node
    M // 2) -> n = 14 * 9 + 2 = 128.  Node states along the p* trajectory, integrated on the device.  The interior free time adds
    the row H(X-) = 0 (goddard.cpp:343-370, shooting.cpp:961-973) and spaces the CONTINUOUS nodes on either side of it uniformly
    (shooting.cpp:1592-1609); under the smooth law (mu2 > 0) that row is redundant with the free-tf row, so this layout is for
    Jacobian batches at a fixed z, not for solves.  Returns (n, z, mode_t, mode_x, time, X)."""
    from . import capi
    d, s = 7, 14
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FREE]
    mode_t[M // 2] = capi.FREE
    mode_x = np.full((M + 1, d), capi.CONTINUOUS, dtype=np.int32)
    mode_x[0] = capi.FIXED
    mode_x[M] = capi.FIXED
    mode_x[M, 3:7] = capi.FREE
    tn = np.linspace(0.0, TF, M + 1)
    X = np.zeros((M + 1, s))
    X[0] = np.concatenate([X0_STATE, PSTAR])
    X[M, 0] = 1.01
    X[1:M] = ctx.integrate_batch(np.zeros(M - 1), tn[1:M], np.repeat(X[0][None, :], M - 1, axis=0))
    n = ctx.problem_set(mode_t, mode_x, tn, X)
    z = np.concatenate([X[:M].ravel(), [tn[j] for j in range(M + 1) if mode_t[j] == capi.FREE]])
    return n, z, mode_t, mode_x, tn, X


def torch_at_least(major, minor):
    """The running torch build is at least major.minor (local version tags such as +rocm7.0 ignored; unparsable: False)."""
    import re
    import torch
    m = re.match(r"(\d+)\.(\d+)", getattr(torch, "__version__", ""))
    return bool(m) and (int(m.group(1)), int(m.group(2))) >= (major, minor)


def single_tensor_gather(dist, device_type="cpu"):
    """Whether the gather runs as all_gather_into_tensor.  Decided from facts every rank shares -- the torch build, the process group's
    backend, where the collective's buffers live -- so the answer is the same on every rank:
    nccl (= RCCL) implements it; gloo does from torch 2.1 on and for CPU tensors only (older builds HAVE the function but
    ProcessGroupGloo raises "no support for _allgather_base"), anything else takes the list form.
    SOCP_SWEEP_GATHER=list forces the list form, SOCP_SWEEP_GATHER=tensor the single-tensor one."""
    forced = os.environ.get("SOCP_SWEEP_GATHER")
    if forced == "list":
        return False
    if not hasattr(dist, "all_gather_into_tensor"):
        return False
    if forced == "tensor":
        return True
    backend = dist.get_backend()
    if backend == "nccl":
        return True
    return backend == "gloo" and device_type == "cpu" and torch_at_least(2, 1)


def run_sweep(Z0, solve_local, dist=None, device=None):
    """Shard the rows of Z0 over the ranks, solve, gather.  `solve_local(Zblock)` returns a dict with
    z [k][n], info [k], nfev [k], fnorm [k].  Returns (table [P][n+3] in start order, local dict)."""
    import torch
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    P, n = Z0.shape
    lo, hi = shard(P, rank, world)
    local = solve_local(Z0[lo:hi])
    rec = np.concatenate([local["z"], local["fnorm"][:, None], local["info"][:, None].astype(float),
                          local["nfev"][:, None].astype(float)], axis=1)
    if world == 1:
        return rec, local
    # equal-size records for all_gather: pad the short shards by one row
    kmax = max(shard(P, r, world)[1] - shard(P, r, world)[0] for r in range(world))
    buf = torch.zeros((kmax, n + 3), dtype=torch.float64, device=device or "cpu")
    buf[:hi - lo] = torch.from_numpy(rec).to(buf.device)
    # ONE collective into ONE tensor and one copy back (a list of per-rank tensors costs a device-to-host copy and a concatenation
    # per rank: 0.2 s of a 3 s sweep at 4 M starts on 8 ranks)
    # The FORM of the collective is chosen before anything is communicated, from facts every rank shares (the torch build and the
    # process group's backend) -- never by catching an error of the collective itself: an error raised on one rank only (a timeout, an
    # out-of-memory condition) would send that rank into a different collective than its peers, and the job would hang.
    # Communication errors propagate.
    full = torch.empty((world * kmax, n + 3), dtype=torch.float64, device=buf.device)
    if single_tensor_gather(dist, buf.device.type):
        try:
            dist.all_gather_into_tensor(full, buf)
        except RuntimeError as exc:
            # NOT a fallback (see above: a rank must never change the collective's form on its own) -- only the way out named
            raise RuntimeError("%s  [socp_amd.sweep: the single-tensor gather failed on backend %s; SOCP_SWEEP_GATHER=list on every "
                               "rank selects the list form]" % (exc, dist.get_backend())) from exc
    else:
        parts = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(parts, buf)
        full = torch.cat(parts)
    host = full.cpu().numpy()
    if P == world * kmax:
        return host, local                                            # equal blocks: the gathered tensor IS the table
    table = np.concatenate([host[r * kmax:r * kmax + shard(P, r, world)[1] - shard(P, r, world)[0]] for r in range(world)])
    return table, local


def interceptor_config5_problem(ctx, M=21):
    """BASELINE config 5 class: the interceptor's scenario 1 (tests/testInterceptor.cpp) as an M-segment multiple-shooting problem,
    final time and final velocity free: n = 12 M + 1 (253 at M = 21).  Node states along the CONVERGED trajectory of the test program
    (tests/golden/interceptor_flow.json), integrated on the device with the reference's fixed-step scheme.  Returns the unknown vector."""
    from . import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gold = json.load(open(os.path.join(root, "tests", "golden", "interceptor_flow.json")))["scenario1_xtol1e-12"][-1]["z"]
    RE = 6378145.0
    X0, tf = np.array(gold[:12]), gold[12]
    Xf = np.zeros(12)
    Xf[:6] = [12000, 1000, 0.0, np.pi / 8, 5475000 / RE, 42000 / RE]
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FREE]
    mode_x = np.zeros((M + 1, 6), dtype=np.int32)
    mode_x[1:M] = capi.CONTINUOUS
    mode_x[M, 1] = capi.FREE
    time = np.array([tf * i / M for i in range(M + 1)])
    X = np.zeros((M + 1, 12))
    X[0], X[M] = X0, Xf
    ctx.set_integrator(capi.INT_RK4)
    X[1:M] = ctx.integrate_batch(np.zeros(M - 1), time[1:M], np.repeat(X0[None, :], M - 1, axis=0))
    n = ctx.problem_set(mode_t, mode_x, time, X)
    return n, np.concatenate([X[:M].ravel(), [tf]])


def interceptor_config5_sweep(P, variant="fast", eps=1e-3, ode_tol=1e-8, fixed_step=False, device=0, xtol=1e-8):
    """The config-5 solve sweep: a context with the n = 253 problem set and the adaptive integrator chosen, P starts around the
    converged trajectory (node-0 costates perturbed by eps xi, SURVEY 8d's generator) and the keyword arguments of chains_solve.
    Returns (ctx, Z0, kw)."""
    from . import capi
    ctx = capi.Context(capi.MODEL_INTERCEPTOR, device=device)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    n, z = interceptor_config5_problem(ctx)
    if not fixed_step:
        ctx.set_integrator(capi.INT_DOPRI5, ode_tol)
    raw = mt19937_64(20250905, 6 * P)
    xi = ((raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 * 2.0 - 1.0).reshape(P, 6)
    Z0 = np.tile(z, (P, 1))
    Z0[:, 6:12] *= 1.0 + eps * xi
    return ctx, Z0, dict(kind=capi.CHAIN_PLAIN, xtol=xtol)


def goddard_kd_chains(ctx, P, eps=0.05, kd_goal=310.0, kd_spread=0.0):
    """testGoddard's state before its KD continuation as P chains: M = 6, free tf, KD = 0, the converged no-drag unknowns
    (tests/golden/goddard_flow.json) with node-0 costates perturbed by eps xi; chain p's goal = kd_goal (1 + kd_spread xi_p).
    Sets the problem on ctx.  Returns (Z0, params, goals, index of KD in the parameter block)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gold = json.load(open(os.path.join(root, "tests", "golden", "goddard_flow.json")))
    z_nd = np.array([g for g in gold["goddard_single_stage"] if g["stage"] == 2 and g["xtol"] == 1e-6][0]["init_z"])
    goddard_multiple_shooting_problem(ctx, 6, tf=z_nd[-1])
    xi = (goddard_starts(P, eps)[:, 7:] / PSTAR - 1.0) / eps              # the sweep's own uniform(-1, 1) draws
    Z0 = np.tile(z_nd, (P, 1))
    Z0[:, 7:14] *= 1.0 + eps * xi
    params = np.tile(np.array(GODDARD_PARAMS), (P, 1))
    params[:, 2] = 0.0
    goals = kd_goal * (1.0 + kd_spread * xi[:, 0])
    return Z0, params, goals, 2


SOLVERS = {"auto": 0, "host": 1, "device": 2, "device_fast": 3}         # socp_chain_options.solver (include/socp_solver.h)
SOLVER_HELP = ("socp_chain_options.solver (include/socp_solver.h has the rule): where the chains' hybrd state machines run.  auto: on the "
               "device where the host side is the bottleneck (P n^2 >= 1.6e6 -- 4e5 for n <= 32 -- and 20 P >= n: 2048 starts of n = 14, 222 of "
               "n = 85, 25 of n = 253) and the state fits HBM, with the matrix-core factorisation on a throughput-flavour context (39 <= n <= 256); "
               "device: the bit-equal device solvers; device_fast: the matrix-core factorisation asked for explicitly")


def warm_up(ctx, args, solve_first):
    """What a process pays ONCE, kept out of the timed solve like the context and the problem set-up: the context's second stream
    (~6 ms), the copy engines' start-up at the first pinned copy above 16 KB (~8 ms; both: socp_ctx_warm_up) and the first
    launch of every kernel the engine uses (code-object load, ~9 ms) -- the last through a solve of the first --warmup starts
    (0: no warm-up at all; the timed call then includes all three).  Returns the trajectory counter to subtract."""
    if args.warmup > 0:
        ctx.warm_up()
        solve_first(min(args.warmup, args.starts))
    return ctx.counters()[0]


def converged_rows(local, lo, rank, params, out):
    """What the *_local functions below start from: the positions of this rank's CONVERGED chains in its block, their unknown vectors,
    their parameter blocks (None when the chains have none), their index in the sweep's start table, and the file OUT.rank<r>.npz."""
    conv = np.where(np.asarray(local["info"]) == 1)[0]
    return conv, np.asarray(local["z"])[conv], None if params is None else np.asarray(params)[conv], lo + conv, "%s.rank%d.npz" % (out, rank)


def trace_local(ctx, args, local, lo, rank, params=None):
    """--trace-stride / --trace-out: the sampled trajectories (socp_trace_batch) of this rank's CONVERGED chains, each with its own
    parameter block when the chains have one, written to PATH.rank<r>.npz: rows [k][M][cap][W] (t, X, u, H, aux0, aux1),
    count [k][M], index [k] = position of the chain in the sweep's start table.  Runs after the timed solve; trajectories stay on
    the rank that solved them (a 4096-start sweep at stride 100 is 70 MB).  Returns the record entry of this rank."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.trace_out)
    t0 = time.perf_counter()
    rows, count = ctx.trace_batch(z, stride=args.trace_stride, params=own)
    wall = time.perf_counter() - t0
    np.savez(path, rows=rows, count=count, index=index)
    return {"stride": args.trace_stride, "chains": int(len(conv)), "rows_per_segment_max": int(count.max()) if len(conv) else 0,
            "wall_s": wall, "file": path}


def cost_local(ctx, args, local, lo, rank, params=None):
    """--cost-out: the integrated running cost (socp_cost_batch) of this rank's CONVERGED chains, each with its own parameter block
    when the chains have one, written to PATH.rank<r>.npz: cost [k][M] per segment, total [k], index [k] = position of the chain
    in the sweep's start table, z [k][n] = the unknown vectors costed.  Runs after the timed solve.  Returns the record entry of
    this rank: what ranks the extremals the sweep found."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.cost_out)
    t0 = time.perf_counter()
    r = ctx.cost_batch(z, params=own)
    wall = time.perf_counter() - t0
    total = r["total"]
    np.savez(path, cost=r["cost"], total=total, index=index, z=z)
    some = len(conv) > 0
    return {"chains": int(len(conv)), "min": float(total.min()) if some else None, "median": float(np.median(total)) if some else None,
            "max": float(total.max()) if some else None, "best_index": int(index[int(np.argmin(total))]) if some else None,
            "wall_s": wall, "file": path}


def events_local(ctx, args, local, lo, rank, params=None):
    """--events-out: the control-structure events (socp_events_batch) of this rank's CONVERGED chains, each with its own parameter
    block when the chains have one: the crossings of Goddard's switching function Switch = mu1 - b p_mass - C / m |p_v| through
    -2 mu2 u_max (watch 1: saturation) and through 0 (watch 2: thrust on / off), the levels from each chain's own parameters, every
    crossing refined by --events-refine false-position steps.  Written to PATH.rank<r>.npz: t [k][M][cap] and id [k][M][cap]
    (+e rising / -e falling through the level of watch e), count [k][M], index [k] = position of the chain in the sweep's start
    table.  Runs after the timed solve.  Returns the record entry of this rank, with the number of chains per event signature
    (the ids of a chain in time order): a measuring instrument for structure, not a structure guess for a next stage."""
    from . import capi
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.events_out)
    held = np.tile(np.asarray(ctx.get_params()), (len(conv), 1)) if own is None else own
    levels = np.stack([-2.0 * held[:, 6] * held[:, 4], np.zeros(len(conv))], axis=1)
    t0 = time.perf_counter()
    t, ident, count = ctx.events_batch(z, [0, 0], levels, refine=args.events_refine, params=own)
    wall = time.perf_counter() - t0
    np.savez(path, index=index, t=t, id=ident, count=count)
    signatures = {}
    for _times, ids in capi.merge_events(t, ident, count):
        key = ",".join("%+d" % i for i in ids)
        signatures[key] = signatures.get(key, 0) + 1
    return {"chains": int(len(conv)), "refine": args.events_refine, "events_per_segment_max": int(count.max()) if len(conv) else 0,
            "signatures": signatures, "wall_s": wall, "file": path}


def jacobi_local(ctx, args, local, lo, rank, params=None):
    """--jacobi-out: the conjugate-time test (socp_jacobi_batch) of this rank's CONVERGED chains, each with its own parameter block
    when the chains have one: det of J(t) = dx(t)/dp(t0) sampled every --jacobi-stride steps of every segment, its sign changes
    from sample --jacobi-skip on.  Written to PATH.rank<r>.npz: index [k] = position of the chain in the sweep's start table,
    tq [k][M][cap], det [k][M][cap], count [k][M], nchange [k][M], tconj [k][M] (NaN: none).  Runs after the timed solve.  Returns
    the record entry of this rank: how many rows show a change and where the first ones lie -- a measuring instrument (the
    classical statement is for single shooting, --segments 1), not a verdict."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.jacobi_out)
    t0 = time.perf_counter()
    r = ctx.jacobi_batch(z, stride=args.jacobi_stride, skip=args.jacobi_skip, blocks=None if own is None else (own, None, None))
    r = {k: v.cpu().numpy() for k, v in r.items()}
    wall = time.perf_counter() - t0
    np.savez(path, index=index, tq=r["tq"], det=r["det"], count=r["count"], nchange=r["nchange"], tconj=r["tconj"])
    changed = r["nchange"].sum(axis=1) > 0 if len(conv) else np.zeros(0, dtype=bool)
    first = np.array([np.nanmin(row) for row in r["tconj"][changed]]) if changed.any() else np.zeros(0)
    return {"rows": int(len(conv)), "with_change": int(changed.sum()), "tconj_min": float(first.min()) if len(first) else None,
            "tconj_median": float(np.median(first)) if len(first) else None, "stride": args.jacobi_stride, "skip": args.jacobi_skip,
            "wall_s": wall, "file": path}


def exactjac_local(ctx, args, local, lo, rank, params=None):
    """--exactjac-out: the exact shooting Jacobian (socp_exact_jacobian_batch) of this rank's CONVERGED chains, each with its own
    parameter block when the chains have one, beside the forward difference the solver read: socp_fd_jacobian_multi_dev, epsfcn
    1e-15, at (z, F(z)) with F from socp_residual_batch_dev of the context's OWN flavour -- not the F the exact call returns, which is
    the reference-order residual whatever the flavour; differencing a throughput-flavour F(z + h) against it would divide the
    flavours' difference by h.  Written to PATH.rank<r>.npz: index [k], fd_dev [k] = max|J_fd - J| / max|J| per row, and sigma [k][n] = the singular
    values of the exact matrices (socp_svd_batch_dev, 60 sweeps) where n <= 142, else an empty array.  Runs after the timed solve.
    Returns the record entry of this rank; a measuring instrument, not a verdict."""
    import torch
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.exactjac_out)
    k, n = len(conv), ctx.n
    t0 = time.perf_counter()
    fd_dev, sigma = np.zeros(k), np.zeros((k, 0))
    if k:
        dev = torch.device("cuda")
        Zd = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64)).to(dev)
        held = None if own is None else torch.from_numpy(np.ascontiguousarray(own, dtype=np.float64)).to(dev)
        J = ctx.exact_jacobian_batch(Zd, blocks=None if held is None else (held, None, None))
        Jfd = torch.empty_like(J)
        Ffd = torch.empty((k, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        if held is not None:
            ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, held.data_ptr(), held.shape[1], None, None))
        try:
            ctx.residual_batch_dev(k, Zd.data_ptr(), Ffd.data_ptr())
            ctx.fd_jacobian_multi_dev(k, Zd.data_ptr(), Ffd.data_ptr(), 1e-15, Jfd.data_ptr())
            ctx.synchronize()
        finally:
            if held is not None:
                ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None)
        fd_dev = ((Jfd - J).abs().amax(dim=(1, 2)) / J.abs().amax(dim=(1, 2))).cpu().numpy()
        if n <= 142:
            sig = torch.empty((k, n), dtype=torch.float64, device=dev)
            sweeps = torch.zeros(k, dtype=torch.int32, device=dev)
            info = torch.zeros(k, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.svd_batch_dev(k, n, J.data_ptr(), 60, sig.data_ptr(), None, sweeps.data_ptr(), info.data_ptr())
            ctx.synchronize()
            sigma = sig.cpu().numpy()
    wall = time.perf_counter() - t0
    np.savez(path, index=index, fd_dev=fd_dev, sigma=sigma)
    some = k > 0
    return {"rows": int(k), "fd_dev_median": float(np.median(fd_dev)) if some else None, "fd_dev_max": float(fd_dev.max()) if some else None,
            "sigma_min_min": float(sigma[:, -1].min()) if some and sigma.shape[1] else None, "wall_s": wall, "file": path}


def guide_local(ctx, args, local, lo, rank, params=None):
    """--guide-out: this rank's CONVERGED chains flown in closed loop under the sampled neighbouring-extremal law (socp_guide_batch),
    --guide-cases dispersed cases per chain: dX0 = --guide-sigma max(1, |x0_c|) N(0, 1) from a numpy generator seeded with --guide-seed
    (+ rank), once with a correction at every --guide-every-th sample of the gains at stride --gain-stride and once open loop.  Written to
    PATH.rank<r>.npz: index [k], dx0 [k][K][d], miss and miss_open [k][K][d (+ 1 with a free final time: the H row)], nupd, nskip [k][K],
    tf [k][K].  Runs after the timed solve.  With --segments > 1 the final time is FREE and the flight is re-timed.  Returns the record
    entry of this rank: the median and the 95th percentile of ||miss||inf over all cases, closed loop and open."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.guide_out)
    K, d = args.guide_cases, ctx.dim
    rng = np.random.default_rng(args.guide_seed + rank)
    dx0 = args.guide_sigma * np.maximum(1.0, np.abs(np.asarray(z)[:, None, :d])) * rng.standard_normal((len(conv), K, d))
    blocks = None if own is None else (own, None, None)
    t0 = time.perf_counter()
    closed = ctx.guide_batch(z, dx0, stride=args.gain_stride, every=args.guide_every, blocks=blocks)
    opened = ctx.guide_batch(z, dx0, stride=args.gain_stride, every=0, tables=closed["tables"], blocks=blocks)
    wall = time.perf_counter() - t0
    host = lambda t: np.ascontiguousarray(t.cpu().numpy())                                          # noqa: E731
    miss, miss_open, nupd, nskip, tf = host(closed["miss"]), host(opened["miss"]), host(closed["nupd"]), host(closed["nskip"]), host(closed["tf"])
    np.savez(path, index=index, dx0=dx0, miss=miss, miss_open=miss_open, nupd=nupd, nskip=nskip, tf=tf)
    norm = lambda m: np.abs(m).reshape(-1, m.shape[-1]).max(axis=1) if m.size else np.zeros(0)      # noqa: E731
    pct = lambda v, p: float(np.nanpercentile(v, p)) if len(v) and not np.all(np.isnan(v)) else None    # noqa: E731
    a, b = norm(miss), norm(miss_open)
    return {"rows": int(len(conv)), "cases": K, "miss_median": pct(a, 50), "miss_p95": pct(a, 95), "miss_open_median": pct(b, 50),
            "miss_open_p95": pct(b, 95), "skipped_samples": int(nskip.sum()), "every": args.guide_every, "stride": args.gain_stride,
            "sigma": args.guide_sigma, "wall_s": wall, "file": path}


def gain_local(ctx, args, local, lo, rank, params=None):
    """--gain-out: the neighbouring-extremal feedback gains (socp_gain_batch) of this rank's CONVERGED chains, each with its own
    parameter block when the chains have one: at the start of every --gain-stride-th step of every segment, the d x d matrix dp/dx with
    which a costate correction keeps the final boundary rows satisfied to first order -- exact for the discrete flow.  Written to
    PATH.rank<r>.npz: index [k], tq [k][M][cap], xq [k][M][cap][s], kp [k][M][cap][d][d] (column-major: kp[..., c, r] = dp_r/dx_c), info
    [k][M][cap] (the elimination's code; -1: no sample), count [k][M].  Runs after the timed solve.  With --segments > 1 the final time is
    FREE: the gains come from socp_gain_free_batch, the file also holds kt [k][M][cap][d] (dt_f/dx_c, the time-to-go feedback) and the
    record entry says with_free_tf.  Needs CONTINUOUS interior nodes (the calls refuse the rest).  Returns the record entry of this rank."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.gain_out)
    free_tf = args.segments > 1                  # the multiple-shooting layout frees the final time: the bordered sweep (socp_gain_free_batch)
    t0 = time.perf_counter()
    call = ctx.gain_free_batch if free_tf else ctx.gain_batch
    r = call(z, stride=args.gain_stride, blocks=None if own is None else (own, None, None))
    r = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in r.items()}
    wall = time.perf_counter() - t0
    if free_tf:
        np.savez(path, index=index, tq=r["tq"], xq=r["xq"], kp=r["kp"], kt=r["kt"], info=r["info"], count=r["count"])
    else:
        np.savez(path, index=index, tq=r["tq"], xq=r["xq"], kp=r["kp"], info=r["info"], count=r["count"])
    solved = r["info"] == 0
    norms = np.abs(r["kp"][solved]).reshape(-1, r["kp"].shape[-1] ** 2).max(axis=1) if solved.any() else np.zeros(0)
    out = {"rows": int(len(conv)), "singular_samples": int((r["info"] > 0).sum()), "kp_norm_median": float(np.median(norms)) if len(norms) else None,
           "stride": args.gain_stride, "wall_s": wall, "file": path}
    if free_tf:
        out["with_free_tf"] = True
    return out


def fields_local(ctx, args, local, lo, rank, params=None):
    """--fields-out: the conjugate-time test with EXACT Jacobi fields (socp_fields_batch) of this rank's CONVERGED chains, each with
    its own parameter block when the chains have one: det of J(t) = dx(t)/dp(t0), carried through the residual's RK4 steps on dual
    numbers, sampled every --fields-stride steps of every segment, its sign changes from sample --fields-skip on.  Written to
    PATH.rank<r>.npz: index [k], tq [k][M][cap], det [k][M][cap], count [k][M], nchange [k][M], tconj [k][M] (NaN: none) and, with
    --fields-phi, phi [k][M][s][s] = the transition matrix dX(t_{i+1})/dX(t_i) of every segment.  Runs after the timed solve.
    Returns the record entry of this rank; a measuring instrument like --jacobi-out, not a verdict."""
    from . import capi
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.fields_out)
    t0 = time.perf_counter()
    r = ctx.fields_batch(z, cols=capi.FIELDS_ALL if args.fields_phi else capi.FIELDS_COSTATE, stride=args.fields_stride, skip=args.fields_skip,
                         phi=args.fields_phi, blocks=None if own is None else (own, None, None))
    r = {k: v.cpu().numpy() for k, v in r.items()}
    wall = time.perf_counter() - t0
    arrays = dict(index=index, tq=r["tq"], det=r["det"], count=r["count"], nchange=r["nchange"], tconj=r["tconj"])
    if args.fields_phi:
        arrays["phi"] = r["phi"]
    np.savez(path, **arrays)
    changed = r["nchange"].sum(axis=1) > 0 if len(conv) else np.zeros(0, dtype=bool)
    first = np.array([np.nanmin(row) for row in r["tconj"][changed]]) if changed.any() else np.zeros(0)
    return {"rows": int(len(conv)), "with_change": int(changed.sum()), "tconj_min": float(first.min()) if len(first) else None,
            "tconj_median": float(np.median(first)) if len(first) else None, "stride": args.fields_stride, "skip": args.fields_skip,
            "phi": bool(args.fields_phi), "wall_s": wall, "file": path}


def extrema_local(ctx, args, local, lo, rank, params=None):
    """--extrema-out: the per-segment extrema (socp_extrema_batch) of this rank's CONVERGED chains, each with its own parameter block
    when the chains have one: over every row of every segment (the rows of a trace with stride 1, none of them stored) the smallest
    and the largest value of each state, and by --extrema-what of the controls, the Hamiltonian and the switching function, with the
    times of their first attainment.  Written to PATH.rank<r>.npz: index [k] = position of the chain in the sweep's start table,
    vmin / vmax / tmin / tmax [k][M][C], count [k][M], nbad [k][M].  Runs after the timed solve.  Returns the record entry of this
    rank: the spread of the Hamiltonian along a row, max_i(Hmax) - min_i(Hmin) -- the integration-quality figure of an autonomous
    problem (NaN figures when H is not selected) -- and the number of rows with a value that is not finite."""
    from . import capi
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.extrema_out)
    t0 = time.perf_counter()
    r = ctx.extrema_batch(z, what=args.extrema_what, blocks=None if own is None else (own, None, None))
    wall = time.perf_counter() - t0
    np.savez(path, index=index, vmin=r["vmin"], vmax=r["vmax"], tmin=r["tmin"], tmax=r["tmax"], count=r["count"], nbad=r["nbad"])
    h = r["channels"].index("H")
    some = len(conv) > 0 and bool(args.extrema_what & capi.EXTREMA_HAMILTONIAN)
    spread = r["vmax"][:, :, h].max(axis=1) - r["vmin"][:, :, h].min(axis=1) if some else np.zeros(0)
    return {"rows": int(len(conv)), "h_spread_max": float(spread.max()) if some else None,
            "h_spread_median": float(np.median(spread)) if some else None, "nbad_rows": int(np.sum(r["nbad"].sum(axis=1) > 0)),
            "what": args.extrema_what, "wall_s": wall, "file": path}


def observe_local(ctx, args, local, lo, rank, params=None):
    """--observe-out: the model-defined observables (socp_observe_batch) of this rank's CONVERGED chains, each with its own parameter
    block when the chains have one: over every row of every segment (the rows of a trace with stride 1, none of them stored) the
    smallest and the largest value of each observable, the times of their first attainment and the trapezoid integral.  Written to
    PATH.rank<r>.npz: index [k] = position of the chain in the sweep's start table, names [NO], ymin / ymax / tmin / tmax / integral
    [k][M][NO], count [k][M], nbad [k][M].  Runs after the timed solve.  Returns the record entry of this rank: per name the smallest
    minimum, the largest maximum and the median over the chains of the integral summed over the segments (in numpy, in segment
    order), and the number of chains with a value that is not finite."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.observe_out)
    t0 = time.perf_counter()
    r = ctx.observe_batch(z, blocks=None if own is None else (own, None, None))
    wall = time.perf_counter() - t0
    np.savez(path, index=index, names=np.array(r["names"]), ymin=r["ymin"], ymax=r["ymax"], tmin=r["tmin"], tmax=r["tmax"],
             integral=r["integral"], count=r["count"], nbad=r["nbad"])
    entry = {"rows": int(len(conv)), "nbad_rows": int(np.sum(r["nbad"].sum(axis=1) > 0)), "wall_s": wall, "file": path}
    some = len(conv) > 0
    total = np.zeros((len(conv), len(r["names"])))
    for i in range(r["integral"].shape[1]):                # segment order
        total = total + r["integral"][:, i, :]
    for k, name in enumerate(r["names"]):
        entry[name] = {"min": float(r["ymin"][:, :, k].min()) if some else None, "max": float(r["ymax"][:, :, k].max()) if some else None,
                       "integral_median": float(np.median(total[:, k])) if some else None}
    return entry


def tangent_local(ctx, args, local, lo, rank, params=None):
    """--tangent-out: the sensitivity dz/dtheta (socp_tangent_batch) of this rank's CONVERGED chains to the packed parameter
    --tangent-param, each chain with its own parameter block when the chains have one, written to PATH.rank<r>.npz: index [k] =
    position of the chain in the sweep's start table, dz [k][n], info [k] (0: solved), theta [k] = the chain's value of the parameter,
    z [k][n] = the unknown vectors differentiated.
    Runs after the timed solve.  Returns the record entry of this rank: which roots are stiff in the parameter and which are not."""
    from . import capi
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.tangent_out)
    slot = capi.GODDARD_PARAM_NAMES.index(args.tangent_param)
    theta = np.full(len(conv), ctx.get_params()[slot]) if own is None else own[:, slot].copy()
    t0 = time.perf_counter()
    r = ctx.tangent_batch(z, [(capi.DIR_PARAM, slot)], params=own)
    wall = time.perf_counter() - t0
    dz, info = r["dz"][:, 0, :], r["info"]
    np.savez(path, index=index, dz=dz, info=info, theta=theta, z=z)
    solved = info == 0
    return {"parameter": args.tangent_param, "chains": int(len(conv)), "info_nonzero": int(np.sum(~solved)),
            "median_norm_dz": float(np.median(np.linalg.norm(dz[solved], axis=1))) if solved.any() else None, "wall_s": wall, "file": path}


def sensitivity_local(ctx, args, local, lo, rank, params=None):
    """--sens-out: the EXACT sensitivity dz/dtheta (socp_sensitivity_batch: the exact shooting Jacobian and the exact dF/dtheta of the
    discrete flow, nothing differenced) of this rank's CONVERGED chains to the packed parameter --sens-param, each chain with its own
    parameter block when the chains have one, written to PATH.rank<r>.npz: index [k] = position of the chain in the sweep's start
    table, dz [k][n], info [k] (0: solved), theta [k] = the chain's value of the parameter, z [k][n] = the unknown vectors
    differentiated, g [k][n] = dF/dtheta.  Runs after the timed solve.  Returns the record entry of this rank."""
    from . import capi
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.sens_out)
    slot = capi.GODDARD_PARAM_NAMES.index(args.sens_param)
    theta = np.full(len(conv), ctx.get_params()[slot]) if own is None else own[:, slot].copy()
    r = ctx.sensitivity_batch(z, [(capi.DIR_PARAM, slot)], params=own, g=True)
    dz, info, g = r["dz"][:, 0, :], r["info"], r["g"][:, 0, :]
    np.savez(path, index=index, dz=dz, info=info, theta=theta, z=z, g=g)
    solved = info == 0
    return {"parameter": args.sens_param, "rows": int(len(conv)), "refused": int(np.sum(~solved)),
            "dz_norm_median": float(np.median(np.linalg.norm(dz[solved], axis=1))) if solved.any() else None, "file": path}


def singular_local(ctx, args, local, lo, rank, params=None):
    """--sing-out: the singular values of the shooting Jacobian (socp_singular_batch) at this rank's CONVERGED chains, each with its
    own parameter block when the chains have one; --sing-scale 1 brings the columns to unit norm first.  Written to PATH.rank<r>.npz:
    index [k] = position of the chain in the sweep's start table, sigma [k][n] descending, vmin [k][n] (the right singular vector of
    the smallest one), colnorm [k][n], sweeps [k], info [k] (0: converged).  Runs after the timed solve.  Returns the record entry of
    this rank: how close to singular the roots the sweep found are."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.sing_out)
    t0 = time.perf_counter()
    r = ctx.singular_batch(z, scale=args.sing_scale, max_sweeps=args.sing_sweeps, params=own)
    wall = time.perf_counter() - t0
    np.savez(path, index=index, sigma=r["sigma"], vmin=r["vmin"], colnorm=r["colnorm"], sweeps=r["sweeps"], info=r["info"])
    good = r["info"] == 0
    smin = r["sigma"][good, -1]
    with np.errstate(divide="ignore"):
        cond = r["sigma"][good, 0] / smin
    some = bool(good.any())
    return {"rows": int(len(conv)), "not_converged": int(np.sum(~good)), "sigma_min_min": float(smin.min()) if some else None,
            "sigma_min_median": float(np.median(smin)) if some else None, "cond_median": float(np.median(cond)) if some else None,
            "cond_max": float(cond.max()) if some else None, "scale": args.sing_scale, "max_sweeps": args.sing_sweeps, "wall_s": wall,
            "file": path}


def branch_local(ctx, args, local, lo, rank, params=None):
    """--branch-out: pseudo-arclength continuation (socp_branch_batch) of this rank's CONVERGED chains along the packed parameter
    --branch-param towards --branch-goal, each chain from its own parameter block when the chains have one: the branch is followed by
    its arclength, past folds, until the parameter crosses the goal.  Written to PATH.rank<r>.npz: index [k] = position of the chain
    in the sweep's start table, y [k][cap][n+1] (z then the parameter of every accepted point, unused slots NaN), ttheta, rnorm
    [k][cap], count, nfold, ifold, status [k], zgoal [k][n] (the root at the goal; NaN unless the goal was reached).  Runs after the
    timed solve.  Returns the record entry of this rank: how many branches reach the goal, and how many turn back on the way."""
    from . import capi
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.branch_out)
    slot = capi.GODDARD_PARAM_NAMES.index(args.branch_param)
    theta = np.full(len(conv), ctx.get_params()[slot]) if own is None else own[:, slot].copy()
    # one orientation per call: towards the goal from where most chains stand
    direction = 1 if len(conv) == 0 or args.branch_goal >= float(np.median(theta)) else -1
    r = ctx.branch_batch(z, (capi.DIR_PARAM, slot), params=own, wtheta=args.branch_wtheta, dir=direction, h0=args.branch_h, hmin=1e-6 * args.branch_h,
                         hmax=8.0 * args.branch_h, goal=args.branch_goal, cap=args.branch_points, rounds=args.branch_rounds)
    np.savez(path, index=index, y=r["y"], ttheta=r["ttheta"], rnorm=r["rnorm"], count=r["count"], nfold=r["nfold"], ifold=r["ifold"],
             status=r["status"], zgoal=r["zgoal"])
    status = r["status"]
    return {"rows": int(len(conv)), "reached": int(np.sum(status == capi.BRANCH_REACHED)), "with_fold": int(np.sum(r["nfold"] > 0)),
            "step_too_small": int(np.sum(status == capi.BRANCH_STEP_TOO_SMALL)), "singular": int(np.sum(status == capi.BRANCH_SINGULAR)),
            "points_median": float(np.median(r["count"])) if len(conv) else None}


NEWTON_STATUS_KEYS = ("running", "converged", "small_step", "stalled", "singular", "bad_start")      # by SOCP_NEWTON_* value


def newton_local(ctx, args, local, lo, rank, params=None):
    """--newton-out: damped Newton polish (socp_newton_batch) of this rank's CONVERGED chains, each with its own parameter block when
    the chains have one: the roots hybrd stopped on at xtol are driven towards rounding level, and every row says how far it got.
    --newton-jac 2 (the exact Jacobian) where the context has it, else 0.  Written to PATH.rank<r>.npz: index [k] = position of the
    chain in the sweep's start table, z [k][n] (the polished unknowns), rnorm, dnorm, iters, nhalf, status [k].  Runs after the timed
    solve.  Returns the record entry of this rank: the rows per status and the residual norms reached."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.newton_out)
    jac = args.newton_jac if args.newton_jac is not None else (2 if ctx.has_exact_jacobian() else 0)
    r = ctx.newton_batch(z, params=own, jac=jac, ftol=args.newton_ftol, xtol=args.newton_xtol, rounds=args.newton_rounds,
                         trials=args.newton_trials, residual=False, history=False)
    np.savez(path, index=index, z=r["z"], rnorm=r["rnorm"], dnorm=r["dnorm"], iters=r["iters"], nhalf=r["nhalf"], status=r["status"])
    some = len(conv) > 0
    entry = {"rows": int(len(conv)), "jac": int(jac)}
    for value, key in enumerate(NEWTON_STATUS_KEYS):
        entry[key] = int(np.sum(r["status"] == value))
    entry.update(rnorm_median=float(np.median(r["rnorm"])) if some else None, rnorm_max=float(np.max(r["rnorm"])) if some else None,
                 iters_median=float(np.median(r["iters"])) if some else None)
    return entry


def roots_global(ctx, args, table, n, with_cost=False, leader_blocks=None):
    """--roots-out: the distinct roots of the WHOLE sweep (socp_group_batch), on rank 0 from the gathered table [P][n+3] as it is:
    ld = n + 3, mask = (info == 1), grouping on the unknown vectors z only, greedy in start order.  Written to PATH.npz: label [P]
    indexed by start (the group, or -1 overflow / -2 not finite / -3 not converged), leader [G] = the start that leads group g,
    count [G], radius [G], z [G][n] = the leaders' unknown vectors and -- with_cost: the model has a running-cost kernel and the
    integrator is the fixed-step one -- cost [G] = the integrated running cost (socp_cost_batch) of the G LEADERS, each with its own
    parameter block (leader_blocks(leader) -> [G][nparams + 2]) when chains carry one.  Runs after the timed solve.  Returns the
    record entry."""
    info = table[:, -2].astype(int)
    t0 = time.perf_counter()
    r = ctx.group_batch(table, n=n, mask=(info == 1), atol=args.roots_atol, rtol=args.roots_rtol, max_groups=args.roots_max)
    leader, count, radius = r["leader"], r["count"], r["radius"]
    G = len(leader)
    z = np.ascontiguousarray(table[leader, :n])
    arrays = dict(label=r["label"], leader=leader, count=count, radius=radius, z=z)
    cost = None
    if with_cost:
        cost = ctx.cost_batch(z, params=leader_blocks(leader) if leader_blocks is not None and G else None)["total"] if G else np.zeros(0)
        arrays["cost"] = cost
    wall = time.perf_counter() - t0
    path = args.roots_out + ".npz"
    np.savez(path, **arrays)
    best = int(np.argmin(cost)) if cost is not None and G else None
    entry = {"groups": G, "overflow": int(r["summary"][1]), "largest_count": int(count.max()) if G else 0,
             "radius_max": float(radius.max()) if G else 0.0, "best_cost": float(cost[best]) if best is not None else None, "best_root": best,
             "rtol": args.roots_rtol, "atol": args.roots_atol, "wall_s": wall, "file": path}
    if leader_blocks is not None and args.kd_spread != 0.0:
        entry["note"] = "chains have their own parameter goals (--kd-spread): grouping is on z only, roots of different problems may share a group"
    return entry


def regrid_structure(args):
    """--regrid-segments: time modes of the target structure -- goddard_multiple_shooting_problem(M2)'s (free final time) for a
    multiple-shooting sweep, FIXED end times for single shooting (whose final time is fixed)."""
    from . import capi
    M2 = args.regrid_segments
    return [capi.FIXED] + [capi.CONTINUOUS] * (M2 - 1) + [capi.FIXED if args.segments == 1 else capi.FREE]


def regrid_local(ctx, args, local, lo, rank, params=None):
    """--regrid-out: this rank's CONVERGED chains moved onto --regrid-segments uniform segments between each chain's own first and
    last timeline entry (socp_regrid_batch: Move(tf) of every new node time on the stored solution, each chain with its own parameter
    block when the chains have one), written to PATH.rank<r>.npz: z [k][n2] = the unknown vectors of the new structure, time [k][M2+1]
    and xnode [k][M2+1][14] = its boundary blocks, index [k] = position of the chain in the sweep's start table, source [k][n] = the
    solutions moved.  Runs after the timed solve.  Returns the record entry of this rank."""
    conv, z, own, index, path = converged_rows(local, lo, rank, params, args.regrid_out)
    M2 = args.regrid_segments
    T2 = np.empty((len(conv), M2 + 1))
    for k, zk in enumerate(z):
        tl = ctx.timeline(zk)
        T2[k] = np.linspace(tl[0], tl[-1], M2 + 1)
    t0 = time.perf_counter()
    r = ctx.regrid_batch(z, regrid_structure(args), T2, params=own)
    seconds = time.perf_counter() - t0
    np.savez(path, index=index, z=r["z"], time=r["time"], xnode=r["xnode"], source=z)
    return {"count": int(len(conv)), "n2": int(r["z"].shape[1]), "seconds": seconds}


def interceptor_sweep(args, torch, dist, capi, world, rank, local_rank, dev, record_fd):
    eps = args.eps if args.eps is not None else 1e-3
    ctx, Z0, _kw = interceptor_config5_sweep(args.starts, variant=args.variant, eps=eps, ode_tol=args.ode_tol, fixed_step=args.fixed_step,
                                             device=local_rank)
    n = Z0.shape[1]
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    stats = {}

    def solve_block(Zb):
        r = ctx.chains_solve(Zb, kind=capi.CHAIN_PLAIN, xtol=args.xtol, speculate=args.speculate, max_rounds=args.max_rounds,
                             solver=SOLVERS[args.solver])
        stats.update(r["stats"])
        r["rounds"] = r["stats"]["rounds"]
        return r
    c0 = warm_up(ctx, args, lambda k: solve_block(Z0[:k]))
    stats.clear()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    table, local = run_sweep(Z0, solve_block, dist if world > 1 else None, dev)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    traj = torch.tensor([float(ctx.counters()[0] - c0)], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(traj)
    extra = {"trace_rank%d" % rank: trace_local(ctx, args, local, shard(args.starts, rank, world)[0], rank)} if args.trace_out else {}
    if rank == 0:
        info = table[:, -2].astype(int)
        conv = table[info == 1, :n]
        if args.roots_out:
            extra["roots"] = roots_global(ctx, args, table, n)
        record = json.dumps({**extra, "sweep": "interceptor_config5_M21_n%d_%s" % (n, "rk4" if args.fixed_step else "dopri5_tol%g" % args.ode_tol),
                             "starts": args.starts, "eps": eps, "n_gpus": world, "variant": args.variant, "solver": args.solver, "xtol": args.xtol, "wall_s": wall,
                             "warmup_starts": args.warmup,
                             "converged": int(np.sum(info == 1)), "info_histogram": {str(k): int(np.sum(info == k)) for k in np.unique(info)},
                             "solution_spread_rel": float(np.max(np.abs(conv - np.median(conv, axis=0))) / np.max(np.abs(conv))) if len(conv) else None,
                             "solves_per_s": args.starts / wall, "trajectories": int(traj.item()), "trajectories_per_s": traj.item() / wall,
                             "rounds_rank0": int(local["rounds"]), "mean_nfev": float(np.mean(table[:, -1])), "engine_rank0": stats})
        os.write(record_fd, (record + "\n").encode())
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=4096)
    ap.add_argument("--eps", type=float, default=None,
                    help="relative costate perturbation; default 1e-3 for single shooting, 0.05 for --segments >= 2 "
                         "(single shooting diverges beyond ~0.3 %%, SURVEY 7 hard part 3)")
    ap.add_argument("--segments", type=int, default=1, help="1: single shooting, fixed tf (n = 14); M >= 2: the "
                    "testGoddard layout with M segments and free tf (n = 14 M + 1)")
    ap.add_argument("--rk4-steps", type=int, default=10000)
    ap.add_argument("--xtol", type=float, default=1e-8)
    ap.add_argument("--variant", choices=["exact", "fast"], default="fast")
    ap.add_argument("--continuation", choices=["none", "kd"], default="none",
                    help="kd: every start is a CHAIN of testGoddard's drag continuation, SolveOCP(step, \"KD\", goal) "
                         "(shooting.cpp:695-778), started from the no-drag solution of the test (tests/golden) with node-0 "
                         "costates perturbed by --eps; all chains advance in lock-step (socp_chains_solve)")
    ap.add_argument("--model", choices=["goddard", "interceptor"], default="goddard",
                    help="interceptor: BASELINE config 5 class -- M = 21 segments, n = 253 unknowns, nodes along the converged "
                         "scenario-1 trajectory of the reference's test program (tests/golden), node-0 costates perturbed by --eps "
                         "(default 1e-3), adaptive Dormand-Prince unless --fixed-step; every start is a full Newton solve")
    ap.add_argument("--fixed-step", action="store_true", help="interceptor: the reference's 50 fixed RK4 steps per stage instead of Dormand-Prince")
    ap.add_argument("--ode-tol", type=float, default=1e-8, help="interceptor: tolerance of the adaptive integrator")
    ap.add_argument("--kd-goal", type=float, default=310.0)
    ap.add_argument("--kd-spread", type=float, default=0.0, help="chain p's goal = kd-goal * (1 + spread * xi_p), xi uniform(-1, 1)")
    ap.add_argument("--step", type=float, default=1.0, help="continuationStep of the chains")
    ap.add_argument("--max-rounds", type=int, default=0, help="socp_chain_options.max_rounds: stop chains still solving after "
                    "that many launch rounds (info = -3); 0 = no limit")
    ap.add_argument("--speculate", type=int, default=-1, help="socp_chain_options.speculate: -1 auto, 0 never, 1 always")
    ap.add_argument("--warmup", type=int, default=8, help="starts of one untimed solve before the timed one (what a process pays once: the "
                    "context's second stream ~6 ms, first-launch code-object loads ~9 ms); 0: the timed call includes them")
    ap.add_argument("--solver", choices=sorted(SOLVERS), default="auto", help=SOLVER_HELP)
    ap.add_argument("--trace-stride", type=int, default=100, help="with --trace-out: keep every K-th row of each segment's trace (and the last)")
    ap.add_argument("--trace-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank traces the converged chains of its own block in one batch (socp_trace_batch), with the "
                         "chains' own parameter blocks, and writes PATH.rank<r>.npz (rows, count, index of the chains).  Trajectories are "
                         "NOT gathered across ranks.  Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--cost-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank integrates the running cost of the converged chains of its own block in one batch "
                         "(socp_cost_batch), with the chains' own parameter blocks, writes PATH.rank<r>.npz (cost per segment, total, index "
                         "of the chains, z) and adds cost_rank<r> {chains, min, median, max, best_index, wall_s, file} to the record.  Not "
                         "with --model interceptor.  Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--regrid-segments", type=int, default=0, metavar="M2",
                    help="with --regrid-out: the number of uniform segments the converged chains are moved onto")
    ap.add_argument("--regrid-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank moves the converged chains of its own block onto M2 uniform segments between each "
                         "chain's own first and last node time in one batch (socp_regrid_batch: Move(tf) at every new node, the chains' own "
                         "parameter blocks; the structure of the M2-segment testGoddard layout, FIXED end times for --segments 1), writes "
                         "PATH.rank<r>.npz (index, z, time, xnode, source) and adds regrid_rank<r> {count, n2, seconds} to the record.  Not "
                         "with --model interceptor.  Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--events-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank locates the control-structure events of the converged chains of its own block in "
                         "one batch (socp_events_batch): the crossings of Goddard's switching function through -2 mu2 u_max (saturation) "
                         "and 0 (thrust on / off), the levels from the chains' own parameter blocks; writes PATH.rank<r>.npz (index, t, "
                         "id, count) and adds events_rank<r> {chains, refine, events_per_segment_max, signatures, wall_s, file} to the "
                         "record, signatures = chains per tuple of event ids in time order.  Not with --model interceptor.  Absent: "
                         "the timed wall and the printed record are unchanged")
    ap.add_argument("--tangent-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank computes the sensitivity dz/dtheta of the converged chains of its own block to "
                         "one packed parameter in one batch (socp_tangent_batch), with the chains' own parameter blocks, writes "
                         "PATH.rank<r>.npz (index, dz, info, theta, z) and adds tangent_rank<r> {parameter, chains, info_nonzero, "
                         "median_norm_dz, wall_s, file} to the record.  Not with --model interceptor.  Absent: the timed wall and the "
                         "printed record are unchanged")
    ap.add_argument("--tangent-param", default="KD", metavar="NAME",
                    help="with --tangent-out: the parameter, by its name in the model's packed block (C, b, KD, kr, u_max, mu1, mu2, "
                         "singularControl)")
    ap.add_argument("--sens-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank computes the EXACT sensitivity dz/dtheta of the converged chains of its own block "
                         "to one packed parameter in one batch (socp_sensitivity_batch: exact Jacobian, exact dF/dtheta), with the chains' "
                         "own parameter blocks, writes PATH.rank<r>.npz (index, dz, info, theta, z, g) and adds sensitivity {parameter, "
                         "rows, refused, dz_norm_median, file} to the record.  Not with --model interceptor.  Absent: the timed wall and "
                         "the printed record are unchanged")
    ap.add_argument("--sens-param", default="KD", metavar="NAME",
                    help="with --sens-out: the parameter, by its name in the model's packed block (C, b, KD, kr, u_max, mu1, mu2, "
                         "singularControl)")
    ap.add_argument("--roots-out", default=None, metavar="PATH",
                    help="after the timed solve, rank 0 groups the converged rows of the gathered table into distinct roots in one call "
                         "(socp_group_batch: greedy in start order, a row joins the FIRST leader l with |z_i - l_i| <= atol + rtol |l_i| for "
                         "every i), writes PATH.npz (label per start, leader, count, radius, z of the leaders, and for Goddard cost = the "
                         "integrated running cost of the leaders) and adds roots {groups, overflow, largest_count, radius_max, best_cost, "
                         "best_root, rtol, atol, wall_s, file} to the record.  Both models.  Absent: the timed wall and the printed record "
                         "are unchanged")
    ap.add_argument("--roots-rtol", type=float, default=1e-6, metavar="R", help="with --roots-out: the relative tolerance (finite, >= 0)")
    ap.add_argument("--roots-atol", type=float, default=0.0, metavar="A", help="with --roots-out: the absolute tolerance (finite, >= 0)")
    ap.add_argument("--roots-max", type=int, default=1024, metavar="G",
                    help="with --roots-out: at most G groups (one device round per group); converged rows beyond them are counted as overflow")
    ap.add_argument("--jacobi-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank runs the conjugate-time test of the converged chains of its own block in one "
                         "batch (socp_jacobi_batch): the determinant of dx(t)/dp(t0) along every segment and its sign changes, with the "
                         "chains' own parameter blocks; writes PATH.rank<r>.npz (index, tq, det, count, nchange, tconj) and adds jacobi "
                         "{rows, with_change, tconj_min, tconj_median, stride, skip, wall_s, file} to the record.  Not with --model "
                         "interceptor.  Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--fields-out", default=None, metavar="PATH",
                    help="after the solve, run the conjugate-time test with EXACT Jacobi fields on this rank's converged chains as one "
                         "batch (socp_fields_batch): dx(t)/dp(t0) carried through the RK4 steps on dual numbers, no forward "
                         "difference; writes PATH.rank<r>.npz (index, tq, det, count, nchange, tconj; phi with --fields-phi) and adds "
                         "fields {rows, with_change, tconj_min, tconj_median} to the record.  Not for the interceptor")
    ap.add_argument("--exactjac-out", default=None, metavar="PATH",
                    help="after the solve, take the EXACT shooting Jacobian of this rank's converged chains as one batch "
                         "(socp_exact_jacobian_batch) beside the forward difference (socp_fd_jacobian_multi_dev); writes PATH.rank<r>.npz "
                         "(index, fd_dev = max|J_fd - J| / max|J| per row, sigma = the singular values of the exact matrices where "
                         "n <= 142) and adds exact_jacobian {rows, fd_dev_median, fd_dev_max, sigma_min_min} to the record.  Not for "
                         "the interceptor")
    ap.add_argument("--extrema-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank reduces the trajectories of the converged chains of its own block in one launch "
                         "that stores no row (socp_extrema_batch): the smallest and the largest value of every state and, by "
                         "--extrema-what, control, the Hamiltonian and the switching function over all rows of every segment, with the "
                         "chains' own parameter blocks; writes PATH.rank<r>.npz (index, vmin, vmax, tmin, tmax, count, nbad) and adds "
                         "extrema {rows, h_spread_max, h_spread_median, nbad_rows} to the record.  Not with --model interceptor.  "
                         "Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--observe-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank reduces the model-defined observables along the trajectories of the converged "
                         "chains of its own block in one launch that stores no row (socp_observe_batch): for Goddard r, v, norm_u, drag, "
                         "drag_acc and fuel_rate -- their smallest and largest value over all rows of every segment, when, and their "
                         "trapezoid integral (that of fuel_rate is the burnt mass), with the chains' own parameter blocks; writes "
                         "PATH.rank<r>.npz (index, names, ymin, ymax, tmin, tmax, integral, count, nbad) and adds observe {rows, "
                         "nbad_rows, and per name min, max, integral_median} to the record.  Not with --model interceptor.  Absent: the "
                         "timed wall and the printed record are unchanged")
    ap.add_argument("--extrema-what", type=int, default=7, metavar="N",
                    help="with --extrema-out: 0 .. 7, the sum of 1 (controls), 2 (Hamiltonian), 4 (event channels); the states always")
    ap.add_argument("--gain-out", default=None, metavar="PATH",
                    help="after the solve, compute the neighbouring-extremal feedback gains of this rank's converged chains as one batch "
                         "(socp_gain_batch): dp/dx along the flight, exact for the discrete flow; writes PATH.rank<r>.npz (index, tq, xq, kp, "
                         "info, count) and adds gain {rows, singular_samples, kp_norm_median, stride, wall_s, file} to the record.  With "
                         "--segments > 1 the final time is free: socp_gain_free_batch, kt in the file and with_free_tf in the record.  "
                         "CONTINUOUS interior nodes only; not with --model interceptor.  Absent: the timed wall and the printed "
                         "record are unchanged")
    ap.add_argument("--gain-stride", type=int, default=100, metavar="K",
                    help="with --gain-out and --guide-out: a gain at the start of every K-th step")
    ap.add_argument("--guide-out", default=None, metavar="PATH",
                    help="after the solve, fly --guide-cases dispersed cases per converged chain in closed loop under the sampled "
                         "neighbouring-extremal law (socp_guide_batch), and once more open loop; writes PATH.rank<r>.npz (index, dx0, miss, "
                         "miss_open, nupd, nskip, tf) and adds guide {rows, cases, miss_median, miss_p95, miss_open_median, miss_open_p95, "
                         "skipped_samples, ...} to the record.  The gains are those of --gain-stride.  CONTINUOUS interior nodes only; not "
                         "with --model interceptor.  Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--guide-cases", type=int, default=16, metavar="K", help="with --guide-out: dispersed cases per chain")
    ap.add_argument("--guide-sigma", type=float, default=1e-3, metavar="S",
                    help="with --guide-out: dX0 = S max(1, |x0_c|) N(0, 1) at the first sample")
    ap.add_argument("--guide-every", type=int, default=1, metavar="E", help="with --guide-out: a correction at every E-th sample")
    ap.add_argument("--guide-seed", type=int, default=0, metavar="N", help="with --guide-out: the seed of the deviations (+ the rank)")
    ap.add_argument("--fields-stride", type=int, default=100, metavar="K", help="with --fields-out: sample every K-th step (and the last)")
    ap.add_argument("--fields-skip", type=int, default=0, metavar="S", help="with --fields-out: compare the samples from the S-th on")
    ap.add_argument("--fields-phi", action="store_true",
                    help="with --fields-out: all 2d columns, and the transition matrix of every segment in the file")
    ap.add_argument("--jacobi-stride", type=int, default=100, metavar="K", help="with --jacobi-out: sample every K-th step (and the last)")
    ap.add_argument("--jacobi-skip", type=int, default=1, metavar="S",
                    help="with --jacobi-out: compare the samples from the S-th on (near t0 the difference matrix is singular to rounding)")
    ap.add_argument("--sing-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank computes the singular values of the shooting Jacobian at the converged chains "
                         "of its own block in one batch (socp_singular_batch), with the chains' own parameter blocks; writes "
                         "PATH.rank<r>.npz (index, sigma, vmin, colnorm, sweeps, info) and adds singular {rows, not_converged, "
                         "sigma_min_min, sigma_min_median, cond_median, cond_max, scale, max_sweeps, wall_s, file} to the record.  Not "
                         "with --model interceptor.  Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--sing-scale", type=int, default=1, metavar="0|1",
                    help="with --sing-out: 1 brings the Jacobian's columns to unit norm first (MINPACK's mode 1 scaling), 0 takes it as it is")
    ap.add_argument("--sing-sweeps", type=int, default=60, metavar="N", help="with --sing-out: at most N Jacobi sweeps, 1 .. 1000")
    ap.add_argument("--branch-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank follows the solution branch of the converged chains of its own block along one "
                         "packed parameter by pseudo-arclength continuation in one batch (socp_branch_batch: past folds, where restarting "
                         "the solver at the next parameter value stalls), with the chains' own parameter blocks, until --branch-goal is "
                         "crossed; writes PATH.rank<r>.npz (index, y, ttheta, rnorm, count, nfold, ifold, status, zgoal) and adds branch "
                         "{rows, reached, with_fold, step_too_small, singular, points_median} to the record.  Needs --branch-goal.  Not "
                         "with --model interceptor.  Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--branch-param", default="KD", metavar="NAME", help="with --branch-out: the parameter, by its name in the packed block")
    ap.add_argument("--branch-goal", type=float, default=None, metavar="V", help="with --branch-out: follow until the parameter crosses V")
    ap.add_argument("--branch-wtheta", type=float, default=1.0, metavar="W",
                    help="with --branch-out: the scale of the parameter in the arclength (lambda = theta / W; for KD ~ 310 take 310)")
    ap.add_argument("--branch-h", type=float, default=0.1, metavar="H", help="with --branch-out: the first arclength step (the largest is 8 H)")
    ap.add_argument("--branch-points", type=int, default=64, metavar="C", help="with --branch-out: points kept per row, >= 2")
    ap.add_argument("--branch-rounds", type=int, default=400, metavar="R", help="with --branch-out: rounds, >= 1")
    ap.add_argument("--newton-out", default=None, metavar="PATH",
                    help="after the timed solve, each rank polishes the converged chains of its own block by damped Newton iteration in one "
                         "batch (socp_newton_batch), with the chains' own parameter blocks; writes PATH.rank<r>.npz (index, z, rnorm, dnorm, "
                         "iters, nhalf, status) and adds newton {rows, jac, the rows per status, rnorm_median, rnorm_max, iters_median} to "
                         "the record.  Not with --model interceptor.  Absent: the timed wall and the printed record are unchanged")
    ap.add_argument("--newton-jac", type=int, default=None, metavar="J",
                    help="with --newton-out: 0 forward differences, 1 variational, 2 exact; default 2 where the context has it, else 0")
    ap.add_argument("--newton-ftol", type=float, default=1e-12, metavar="F", help="with --newton-out: CONVERGED when ||F||inf <= F")
    ap.add_argument("--newton-xtol", type=float, default=0.0, metavar="X", help="with --newton-out: SMALL_STEP when the step is <= X ||z||inf; 0: off")
    ap.add_argument("--newton-rounds", type=int, default=20, metavar="R", help="with --newton-out: rounds, >= 1")
    ap.add_argument("--newton-trials", type=int, default=4, metavar="T", help="with --newton-out: step lengths tried per round, 1 .. 8")
    ap.add_argument("--events-refine", type=int, default=2, metavar="R",
                    help="with --events-out: false-position steps per event, 0 .. 8 (0: linear interpolation over the step)")
    args = ap.parse_args()
    if not 0 <= args.events_refine <= 8:
        ap.error("--events-refine must be 0 .. 8")
    if args.events_out and args.model == "interceptor":
        ap.error("--events-out: the interceptor has no event channels (its own ComputeTraj rewrites the costate in mid-trajectory)")
    if args.jacobi_out and args.model == "interceptor":
        ap.error("--jacobi-out: the interceptor has no Jacobi-field kernel (its own ComputeTraj rewrites the costate in mid-trajectory)")
    if args.fields_out and args.model == "interceptor":
        ap.error("--fields-out: the interceptor has no exact-fields kernel (its own ComputeTraj rewrites the costate in mid-trajectory)")
    if args.gain_out and args.model == "interceptor":
        ap.error("--gain-out: the interceptor has no gain entry (its own ComputeTraj and final rows)")
    if args.gain_stride < 1:
        ap.error("--gain-stride must be >= 1")
    if args.guide_out and args.model == "interceptor":
        ap.error("--guide-out: the interceptor has no guide entry (its own ComputeTraj and final rows)")
    if args.guide_cases < 1 or args.guide_every < 0 or not args.guide_sigma >= 0:
        ap.error("--guide-cases must be >= 1, --guide-every >= 0 and --guide-sigma >= 0")
    if args.exactjac_out and args.model == "interceptor":
        ap.error("--exactjac-out: the interceptor has no exact-Jacobian kernel (its own ComputeTraj and final rows)")
    if args.extrema_out and args.model == "interceptor":
        ap.error("--extrema-out is implemented for the Goddard sweeps")
    if args.observe_out and args.model == "interceptor":
        ap.error("--observe-out: the interceptor has no observe entry (a model with its own ComputeTraj)")
    if not 0 <= args.extrema_what <= 7:
        ap.error("--extrema-what must be 0 .. 7")
    if args.fields_stride < 1 or args.fields_skip < 0:
        ap.error("--fields-stride must be >= 1 and --fields-skip >= 0")
    if args.jacobi_stride < 1 or args.jacobi_skip < 0:
        ap.error("--jacobi-stride must be >= 1 and --jacobi-skip >= 0")
    if bool(args.regrid_out) != (args.regrid_segments > 0) or not 0 <= args.regrid_segments <= 255:
        ap.error("--regrid-segments M2 (1 .. 255) and --regrid-out PATH go together")
    if args.regrid_out and args.model == "interceptor":
        ap.error("--regrid-out is implemented for the Goddard sweeps")
    if args.trace_stride < 1:
        ap.error("--trace-stride must be >= 1")
    if args.tangent_out and args.model == "interceptor":
        ap.error("--tangent-out is implemented for the Goddard sweeps")
    if args.tangent_out:
        from .capi import GODDARD_PARAM_NAMES            # (the module only: the library is loaded by the first context)
        if args.tangent_param not in GODDARD_PARAM_NAMES:
            ap.error("--tangent-param: not a name of the packed parameter block (%s)" % ", ".join(GODDARD_PARAM_NAMES))
    if args.sens_out and args.model == "interceptor":
        ap.error("--sens-out: the interceptor has no sensitivity kernel (its own ComputeTraj and final rows)")
    if args.sens_out:
        from .capi import GODDARD_PARAM_NAMES
        if args.sens_param not in GODDARD_PARAM_NAMES:
            ap.error("--sens-param: not a name of the packed parameter block (%s)" % ", ".join(GODDARD_PARAM_NAMES))
    if args.branch_out and args.model == "interceptor":
        ap.error("--branch-out is implemented for the Goddard sweeps")
    if args.branch_out:
        from .capi import GODDARD_PARAM_NAMES
        if args.branch_param not in GODDARD_PARAM_NAMES:
            ap.error("--branch-param: not a name of the packed parameter block (%s)" % ", ".join(GODDARD_PARAM_NAMES))
        if args.branch_goal is None or not np.isfinite(args.branch_goal):
            ap.error("--branch-out needs a finite --branch-goal")
        if not (args.branch_wtheta > 0 and np.isfinite(args.branch_wtheta) and args.branch_h > 0 and np.isfinite(args.branch_h)):
            ap.error("--branch-wtheta and --branch-h must be positive and finite")
        if args.branch_points < 2 or args.branch_rounds < 1:
            ap.error("--branch-points must be >= 2 and --branch-rounds >= 1")
    if args.newton_out and args.model == "interceptor":
        ap.error("--newton-out is implemented for the Goddard sweeps")
    if args.newton_out:
        if args.newton_jac is not None and args.newton_jac not in (0, 1, 2):
            ap.error("--newton-jac must be 0, 1 or 2")
        if not args.newton_ftol > 0 or not args.newton_xtol >= 0:
            ap.error("--newton-ftol must be positive and --newton-xtol >= 0")
        if args.newton_rounds < 1 or not 1 <= args.newton_trials <= 8:
            ap.error("--newton-rounds must be >= 1 and --newton-trials 1 .. 8")
    if args.sing_out and args.model == "interceptor":
        ap.error("--sing-out is implemented for the Goddard sweeps")
    if args.sing_scale not in (0, 1):
        ap.error("--sing-scale must be 0 or 1")
    if not 1 <= args.sing_sweeps <= 1000:
        ap.error("--sing-sweeps must be 1 .. 1000")
    if args.roots_max < 1:
        ap.error("--roots-max must be >= 1")
    if not (np.isfinite(args.roots_rtol) and args.roots_rtol >= 0):
        ap.error("--roots-rtol must be finite and >= 0")
    if not (np.isfinite(args.roots_atol) and args.roots_atol >= 0):
        ap.error("--roots-atol must be finite and >= 0")
    if args.cost_out and args.model == "interceptor":
        ap.error("--cost-out: the interceptor has no running-cost kernel (its chart changes rewrite the costate in mid-trajectory)")

    # stdout carries only the JSON record: RCCL prints a version banner to file descriptor 1 when a process group is created
    import sys
    sys.stdout.flush()
    record_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    from . import capi

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    if args.model == "interceptor":
        return interceptor_sweep(args, torch, dist, capi, world, rank, local_rank, dev, record_fd)
    ctx = capi.Context(capi.MODEL_GODDARD, device=local_rank)
    ctx.set_params(GODDARD_PARAMS)
    ctx.set_step_number(args.rk4_steps)
    ctx.set_variant(capi.VARIANT_LANE_FAST if args.variant == "fast" else capi.VARIANT_LANE_EXACT)
    eps = args.eps if args.eps is not None else (1e-3 if (args.segments == 1 and args.continuation == "none") else 0.05)
    Z0 = goddard_starts(args.starts, eps)
    chain_kw = None
    if args.continuation == "kd":
        args.segments = 6
        Z0, params, goals, _kd = goddard_kd_chains(ctx, args.starts, eps, args.kd_goal, args.kd_spread)
        chain_kw = dict(kind=capi.CHAIN_PARAM, param_index=2, step=args.step, speculate=args.speculate)
    elif args.segments == 1:
        goddard_single_shooting_problem(ctx)
    else:
        goddard_multiple_shooting_problem(ctx, args.segments)
        lo, hi = shard(args.starts, rank, world)
        Zfull = np.zeros((args.starts, 14 * args.segments + 1))
        Zfull[lo:hi] = goddard_multiple_shooting_starts(ctx, Z0[lo:hi], args.segments)     # each rank builds its own rows
        Z0 = Zfull
    n_unknown = Z0.shape[1]

    stats = {}

    solver = SOLVERS[args.solver]

    def solve_block(Zb):
        lo, hi = shard(args.starts, rank, world)
        if chain_kw is not None:
            r = ctx.chains_solve(Zb, goal=goals[lo:hi], params=params[lo:hi], xtol=args.xtol, max_rounds=args.max_rounds, solver=solver, **chain_kw)
        else:
            r = ctx.chains_solve(Zb, kind=capi.CHAIN_PLAIN, xtol=args.xtol, speculate=args.speculate, max_rounds=args.max_rounds, solver=solver)
        stats.update(r["stats"])
        stats["solves"] = int(np.sum(r["solves"]))
        r["rounds"] = r["stats"]["rounds"]
        return r
    lo_w, hi_w = shard(args.starts, rank, world)

    def warm(k):
        # the first k starts of this rank's block through the same call (continuation chains: with their own goals / parameters)
        if chain_kw is not None:
            return ctx.chains_solve(Z0[lo_w:lo_w + k], goal=goals[lo_w:lo_w + k], params=params[lo_w:lo_w + k], xtol=args.xtol, solver=solver, **chain_kw)
        return ctx.chains_solve(Z0[lo_w:lo_w + k], kind=capi.CHAIN_PLAIN, xtol=args.xtol, speculate=args.speculate, max_rounds=args.max_rounds, solver=solver)
    c0 = warm_up(ctx, args, warm)
    stats.clear()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    table, local = run_sweep(Z0, solve_block, dist if world > 1 else None, dev)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    traj = torch.tensor([float(ctx.counters()[0] - c0)], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(traj)
    extra = {}
    blocks = None
    if chain_kw is not None:                            # for the four below: every chain at the KD it reached, then the context's two switching times
        blocks = np.concatenate([params[lo_w:hi_w], np.zeros((hi_w - lo_w, 2))], axis=1)
        blocks[:, 2] = local["param_final"]
    if args.trace_out:
        extra["trace_rank%d" % rank] = trace_local(ctx, args, local, lo_w, rank, blocks)
    if args.cost_out:
        extra["cost_rank%d" % rank] = cost_local(ctx, args, local, lo_w, rank, blocks)
    if args.regrid_out:
        extra["regrid_rank%d" % rank] = regrid_local(ctx, args, local, lo_w, rank, blocks)
    if args.events_out:
        extra["events_rank%d" % rank] = events_local(ctx, args, local, lo_w, rank, blocks)
    if args.tangent_out:
        extra["tangent_rank%d" % rank] = tangent_local(ctx, args, local, lo_w, rank, blocks)
    if args.sens_out:
        extra["sensitivity" if rank == 0 else "sensitivity_rank%d" % rank] = sensitivity_local(ctx, args, local, lo_w, rank, blocks)
    if args.jacobi_out:
        extra["jacobi" if rank == 0 else "jacobi_rank%d" % rank] = jacobi_local(ctx, args, local, lo_w, rank, blocks)
    if args.fields_out:
        extra["fields" if rank == 0 else "fields_rank%d" % rank] = fields_local(ctx, args, local, lo_w, rank, blocks)
    if args.gain_out:
        extra["gain" if rank == 0 else "gain_rank%d" % rank] = gain_local(ctx, args, local, lo_w, rank, blocks)
    if args.guide_out:
        extra["guide" if rank == 0 else "guide_rank%d" % rank] = guide_local(ctx, args, local, lo_w, rank, blocks)
    if args.exactjac_out:
        extra["exact_jacobian" if rank == 0 else "exact_jacobian_rank%d" % rank] = exactjac_local(ctx, args, local, lo_w, rank, blocks)
    if args.extrema_out:
        extra["extrema" if rank == 0 else "extrema_rank%d" % rank] = extrema_local(ctx, args, local, lo_w, rank, blocks)
    if args.observe_out:
        extra["observe" if rank == 0 else "observe_rank%d" % rank] = observe_local(ctx, args, local, lo_w, rank, blocks)
    if args.sing_out:
        extra["singular" if rank == 0 else "singular_rank%d" % rank] = singular_local(ctx, args, local, lo_w, rank, blocks)
    if args.branch_out:
        extra["branch" if rank == 0 else "branch_rank%d" % rank] = branch_local(ctx, args, local, lo_w, rank, blocks)
    if args.newton_out:
        extra["newton" if rank == 0 else "newton_rank%d" % rank] = newton_local(ctx, args, local, lo_w, rank, blocks)
    if rank == 0:
        info = table[:, -2].astype(int)
        conv = table[info == 1, :n_unknown]
        if args.roots_out:                                 # (a converged chain has reached its goal: its own KD is the goal)
            own = None if chain_kw is None else (lambda lead: np.concatenate([params[lead, :2], goals[lead, None], params[lead, 3:], np.zeros((len(lead), 2))], axis=1))
            extra["roots"] = roots_global(ctx, args, table, n_unknown, with_cost=ctx.has_cost(), leader_blocks=own)
        spread = float(np.max(np.abs(conv - np.median(conv, axis=0))) / np.max(np.abs(conv))) if len(conv) else None
        record = json.dumps({**extra, "solution_spread_rel": spread, "max_fnorm_converged": float(np.max(table[info == 1, -3])) if len(conv) else None,
                          "sweep": ("goddard_kd_continuation_chains_M6_n85" if chain_kw is not None else
                                    "goddard_single_shooting_n14" if args.segments == 1 else "goddard_multiple_shooting_M%d_n%d" % (args.segments, n_unknown)),
                          "chains_per_s": (args.starts / wall) if chain_kw is not None else None,
                          "continuation": None if chain_kw is None else {"parameter": "KD", "from": 0.0, "goal": args.kd_goal, "goal_spread": args.kd_spread, "step": args.step},
                          "engine_rank0": stats,
                          "starts": args.starts, "eps": eps, "n_gpus": world, "solver": args.solver,
                          "rk4_steps": args.rk4_steps, "variant": args.variant, "xtol": args.xtol, "wall_s": wall, "warmup_starts": args.warmup, "max_rounds": args.max_rounds,
                          "converged": int(np.sum(info == 1)), "info_histogram": {str(k): int(np.sum(info == k)) for k in np.unique(info)},
                          "trajectories": int(traj.item()), "trajectories_per_s": traj.item() / wall,
                          "solves_per_s": args.starts / wall, "rounds_rank0": int(local["rounds"]),
                          "mean_nfev": float(np.mean(table[:, -1]))})
        os.write(record_fd, (record + "\n").encode())
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
