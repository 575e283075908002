"""ctypes bindings over the C-ABI of libsocp_hip.so (include/socp_hip.h, cminpack.h, socp_solver.h).

Thin plumbing only: every call goes straight to the shared library, which has no CPU path.
If the library is missing, importing the loader raises -- nothing here falls back to NumPy.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SOCP_LIB_PATH") or os.path.join(_HERE, "_build", "libsocp_hip.so")      # (SOCP_LIB_PATH: A/B builds of the library)

OK, ERR_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4
MODEL_GODDARD, MODEL_DOUBLE_INTEGRATOR, MODEL_COVID19, MODEL_INTERCEPTOR = 1, 2, 3, 4
MODEL_VTOLUAV = 5
# packed block of the vtolUAV model: its own nine parameters, then the four scalars of its obstacle map (SOCP_VTOL_NPARAMS)
VTOL_PARAM_NAMES = ["u_max", "a_max", "alphaT", "alphaV", "invSigmaXwp", "Vd", "ca", "nWP_tot", "nWP",
                    "phiObs", "psiWP", "muObs", "sigmaWP"]
MAP_STRIDE, MAX_OBSTACLES = 7, 256      # obstacle table: rows of (type, centre xyz, radii xyz)
INTERCEPTOR_PARAM_NAMES = ["c0", "hr", "d0", "eta", "propellant_mass", "empty_mass", "q", "ve", "alpha_max", "u_max",
                           "a_max", "mu_gft", "muT", "muV", "muC", "R_Earth", "mu0", "chartLimit"]
FIXED, FREE, CONTINUOUS = 0, 1, 2
VARIANT_AUTO, VARIANT_LANE_EXACT, VARIANT_LANE_FAST = 0, 1, 2
EVAL_RHS, EVAL_CONTROL, EVAL_HAMILTONIAN = 0, 1, 2
FIELDS_COSTATE, FIELDS_ALL = 0, 1          # socp_fields_batch: the d costate columns / all s columns
REQ_DONE, REQ_FVEC, REQ_JAC = 0, 1, 2
INT_RK4, INT_DOPRI5 = 0, 1
GODDARD_PARAM_NAMES = ["C", "b", "KD", "kr", "u_max", "mu1", "mu2", "singularControl"]
DIR_PARAM, DIR_TIME, DIR_XNODE = 0, 1, 2      # what a direction of tangent_batch addresses (SOCP_DIR_*)
BRANCH_RUNNING, BRANCH_REACHED, BRANCH_FULL, BRANCH_STEP_TOO_SMALL, BRANCH_SINGULAR, BRANCH_BAD_START = range(6)      # status of branch_batch (SOCP_BRANCH_*)
NEWTON_RUNNING, NEWTON_CONVERGED, NEWTON_SMALL_STEP, NEWTON_STALLED, NEWTON_SINGULAR, NEWTON_BAD_START = range(6)      # status of newton_batch (SOCP_NEWTON_*)
GROUP_OVERFLOW, GROUP_NOTFINITE, GROUP_MASKED = -1, -2, -3      # the negative labels of group_batch (SOCP_GROUP_*)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

FCN = C.CFUNCTYPE(C.c_int, _vp, C.c_int, _dp, _dp, C.c_int)
FCNDER = C.CFUNCTYPE(C.c_int, _vp, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int)
FDJAC = C.CFUNCTYPE(C.c_int, _vp, C.c_int, _dp, _dp, C.c_double, _dp, C.c_int)

_lib = None


CHAIN_PLAIN, CHAIN_PARAM, CHAIN_DATA = 0, 1, 2
SOLVER_AUTO, SOLVER_HOST, SOLVER_DEVICE, SOLVER_DEVICE_FAST = 0, 1, 2, 3
FACTOR_EXACT, FACTOR_FAST = 0, 1


class ChainOptions(C.Structure):
    """socp_chain_options (include/socp_solver.h)."""
    _fields_ = [("kind", C.c_int), ("param_index", C.c_int), ("step", C.c_double), ("step_min", C.c_double),
                ("xtol", C.c_double), ("maxfev", C.c_int), ("epsfcn", C.c_double), ("factor", C.c_double),
                ("dedup", C.c_int), ("speculate", C.c_int), ("max_rounds", C.c_int), ("analytic_jac", C.c_int),
                ("solver", C.c_int)]


class BranchOptions(C.Structure):
    """socp_branch_options (include/socp_hip.h)."""
    _fields_ = [("epsfcn", C.c_double), ("jac", C.c_int), ("wtheta", C.c_double), ("dir", C.c_int), ("h0", C.c_double),
                ("hmin", C.c_double), ("hmax", C.c_double), ("grow", C.c_double), ("kfast", C.c_int), ("max_corr", C.c_int),
                ("ftol", C.c_double), ("have_goal", C.c_int), ("goal", C.c_double), ("cap", C.c_int), ("rounds", C.c_int)]


def branch_options(epsfcn=1e-15, jac=0, wtheta=1.0, dir=1, h0=0.1, hmin=1e-8, hmax=1.0, grow=2.0, kfast=2, max_corr=6, ftol=1e-10,
                   goal=None, cap=64, rounds=200):
    """A BranchOptions with the defaults of branch_batch; goal=None: no goal."""
    return BranchOptions(float(epsfcn), int(jac), float(wtheta), int(dir), float(h0), float(hmin), float(hmax), float(grow), int(kfast),
                         int(max_corr), float(ftol), 0 if goal is None else 1, 0.0 if goal is None else float(goal), int(cap), int(rounds))


class NewtonOptions(C.Structure):
    """socp_newton_options (include/socp_hip.h)."""
    _fields_ = [("jac", C.c_int), ("epsfcn", C.c_double), ("ftol", C.c_double), ("xtol", C.c_double), ("trials", C.c_int), ("rounds", C.c_int)]


def newton_options(jac=2, epsfcn=1e-15, ftol=1e-12, xtol=0.0, trials=4, rounds=20):
    """A NewtonOptions with the defaults of newton_batch."""
    return NewtonOptions(int(jac), float(epsfcn), float(ftol), float(xtol), int(trials), int(rounds))


class ChainStats(C.Structure):
    _fields_ = [("rounds", C.c_longlong), ("jacobians_launched", C.c_longlong), ("jacobians_from_cache", C.c_longlong),
                ("speculative_rounds", C.c_longlong), ("restarts", C.c_longlong), ("wall_ms", C.c_double)]


class SocpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libsocp_hip error %d: %s" % (code, msg))
        self.code = code


def lib():
    """Load libsocp_hip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            # a source-only checkout: compile the HIP library now (hipcc cross-compiles gfx950 anywhere)
            import subprocess
            try:
                subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])
            except Exception as exc:
                raise ImportError("%s is not built and building it failed (%s): run "
                                  "`python -c 'import __graft_entry__ as g; g.build()'`" % (LIB_PATH, exc))
        # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64 (same soname as
        # /opt/rocm's).  Importing torch FIRST makes the loader bind this library to that copy, so
        # torch tensors/streams and our kernels share one runtime; the other order gives two runtimes
        # and torch then reports "No HIP GPUs are available".  Without torch, /opt/rocm's is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.socp_last_error.restype = C.c_char_p
        L.socp_last_error.argtypes = [_vp]
        L.socp_ctx_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int]
        for name in ("socp_ctx_destroy", "socp_ctx_synchronize", "socp_ctx_warm_up"):
            getattr(L, name).argtypes = [_vp]
        L.socp_ctx_set_params.argtypes = [_vp, _dp, C.c_int]
        L.socp_ctx_get_params.argtypes = [_vp, _dp, C.c_int]
        L.socp_ctx_set_step_number.argtypes = [_vp, C.c_int]
        L.socp_ctx_set_map.argtypes = [_vp, C.c_int, _dp]
        L.socp_ctx_get_map.argtypes = [_vp, _ip, _dp, C.c_int]
        L.socp_ctx_set_integrator.argtypes = [_vp, C.c_int, C.c_double]
        L.socp_ctx_get_integrator.argtypes = [_vp, _ip, _ip, _dp]
        L.socp_ctx_set_switching_times.argtypes = [_vp, _dp, C.c_int]
        L.socp_ctx_set_variant.argtypes = [_vp, C.c_int]
        L.socp_ctx_set_exact_hooks.argtypes = [_vp, C.c_int]
        L.socp_ctx_set_stream.argtypes = [_vp, _vp, C.c_int]
        L.socp_ctx_aux_stream.argtypes = [_vp, C.POINTER(C.c_void_p)]
        L.socp_ctx_dims.argtypes = [_vp, _ip, _ip, _ip]
        L.socp_ctx_control_dim.argtypes = [_vp]
        L.socp_ctx_device.argtypes = [_vp]
        L.socp_ctx_num_params.argtypes = [_vp]
        L.socp_ctx_model_id.argtypes = [_vp]
        L.socp_ctx_has_variational.argtypes = [_vp]
        L.socp_ctx_counters.argtypes = [_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.socp_integrate_batch.argtypes = [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp, C.c_int]
        L.socp_integrate_batch_dev.argtypes = [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int]
        L.socp_integrate_dense.argtypes = [_vp, C.c_double, C.c_double, _dp, _dp, _dp, _dp, C.c_int, _ip]
        L.socp_integrate_dense_aux.argtypes = [_vp, C.c_double, C.c_double, _dp, _dp, _dp, _dp, _dp, C.c_int, _ip]
        L.socp_eval_batch.argtypes = [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _dp, C.c_int]
        L.socp_problem_set.argtypes = [_vp, C.c_int, _ip, _ip, _dp, _dp]
        L.socp_problem_num_param.argtypes = [_vp]
        L.socp_timeline.argtypes = [_vp, _dp, _dp]
        L.socp_residual_batch.argtypes = [_vp, C.c_int, _dp, _dp]
        L.socp_residual_batch_dev.argtypes = [_vp, C.c_int, _vp, _vp]
        L.socp_fd_jacobian.argtypes = [_vp, _dp, _dp, C.c_double, _dp, C.c_int]
        L.socp_fd_jacobian_dev.argtypes = [_vp, _vp, _vp, C.c_double, _vp, C.c_int]
        L.socp_var_jacobian.argtypes = [_vp, _dp, _dp]
        L.socp_fd_jacobian_multi_dev.argtypes = [_vp, C.c_int, _vp, _vp, C.c_double, _vp, C.c_int]
        L.socp_fd_rows_dev.argtypes = [_vp, C.c_int, _vp, C.c_double, _vp]
        L.socp_fd_rows.argtypes = [_vp, C.c_int, _dp, C.c_double, _dp]
        L.socp_fd_diff_dev.argtypes = [_vp, C.c_int, _vp, C.c_double, _vp, _vp]
        L.socp_plugin_load.argtypes = [C.c_char_p]
        L.socp_problem_set_blocks_dev.argtypes = [_vp, _vp, C.c_int, _vp, _vp]
        L.socp_residual_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp]
        L.socp_problem_num_nodes.argtypes = [_vp]
        L.socp_trace_width.argtypes = [_vp]
        L.socp_trace_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]
        L.socp_trace_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _ip]
        L.socp_trace_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _ip]
        L.socp_ctx_has_cost.argtypes = [_vp]
        L.socp_cost_batch_dev.argtypes = [_vp, C.c_int, _vp, _vp, _vp, _vp]
        L.socp_cost_batch.argtypes = [_vp, C.c_int, _dp, _dp, _dp, _dp]
        L.socp_cost_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp]
        L.socp_ctx_event_channels.argtypes = [_vp]
        L.socp_extrema_width.argtypes = [_vp]
        L.socp_ctx_has_extrema.argtypes = [_vp]
        L.socp_extrema_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
        L.socp_extrema_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip]
        L.socp_extrema_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip]
        L.socp_ctx_has_observe.argtypes = [_vp]
        L.socp_ctx_observables.argtypes = [_vp]
        L.socp_ctx_observable_name.argtypes = [_vp, C.c_int]
        L.socp_ctx_observable_name.restype = C.c_char_p
        L.socp_observe_batch_dev.argtypes = [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.socp_observe_batch.argtypes = [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip]
        L.socp_observe_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip]
        L.socp_events_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, _ip, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]
        L.socp_events_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, _ip, _dp, C.c_int, C.c_int, _dp, _ip, _ip, _dp]
        L.socp_events_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _ip, _dp, C.c_int, C.c_int, _dp, _ip,
                                               _ip, _dp]
        L.socp_ctx_has_jacobi.argtypes = [_vp]
        L.socp_jacobi_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_double, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
        L.socp_jacobi_batch.argtypes = [_vp, C.c_int, _dp, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp, _dp]
        L.socp_ctx_has_fields.argtypes = [_vp]
        L.socp_fields_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
        L.socp_fields_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp, _dp]
        L.socp_fields_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip,
                                               _ip, _dp, _dp]
        L.socp_jacobi_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip,
                                               _ip, _dp, _dp]
        L.socp_ctx_has_exact_jacobian.argtypes = [_vp]
        L.socp_exact_jacobian_batch_dev.argtypes = [_vp, C.c_int, _vp, _vp, _vp]
        L.socp_exact_jacobian_batch.argtypes = [_vp, C.c_int, _dp, _dp, _dp]
        L.socp_exact_jacobian_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp]
        L.socp_move_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp]
        L.socp_move_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp]
        L.socp_move_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp]
        L.socp_regrid_num_param.argtypes = [_vp, C.c_int, _ip]
        L.socp_regrid_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, _ip, _vp, _vp, _vp]
        L.socp_regrid_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp]
        L.socp_tangent_work_bytes.argtypes = [_vp, C.c_int, C.c_int]
        L.socp_tangent_work_bytes.restype = C.c_size_t
        L.socp_tangent_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, _ip, _ip, C.c_double, C.c_int, _vp, C.c_size_t, _vp, _vp, _vp]
        L.socp_tangent_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, _ip, _ip, C.c_double, C.c_int, _dp, _ip, _dp]
        L.socp_tangent_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _ip, _ip, C.c_double, C.c_int, _dp, _ip,
                                                _dp]
        L.socp_ctx_has_sensitivity.argtypes = [_vp]
        L.socp_sensitivity_work_bytes.argtypes = [_vp, C.c_int, C.c_int]
        L.socp_sensitivity_work_bytes.restype = C.c_size_t
        L.socp_sensitivity_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, _ip, _ip, _vp, C.c_size_t, _vp, _vp, _vp]
        L.socp_sensitivity_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, _ip, _ip, _dp, _ip, _dp]
        L.socp_sensitivity_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _ip, _ip, _dp, _ip, _dp]
        L.socp_ctx_has_gain.argtypes = [_vp]
        L.socp_gain_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.socp_gain_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp, _dp, _dp]
        L.socp_gain_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp, _dp, _dp]
        L.socp_ctx_has_gain_free.argtypes = [_vp]
        L.socp_gain_free_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.socp_gain_free_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _dp]
        L.socp_gain_free_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _dp]
        L.socp_ctx_has_guide.argtypes = [_vp]
        L.socp_guide_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.socp_guide_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _ip, C.c_int, _dp, C.c_int, _dp, _dp, _ip, _ip, _dp, _dp, _dp]
        L.socp_guide_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _ip, C.c_int, _dp, C.c_int,
                                              _dp, _dp, _ip, _ip, _dp, _dp, _dp]
        L.socp_ctx_has_hamiltonian_gradient.argtypes = [_vp]
        L.socp_hamiltonian_gradient_batch_dev.argtypes = [_vp, C.c_int, _vp, _vp, _vp, _vp]
        L.socp_hamiltonian_gradient_batch.argtypes = [_vp, C.c_int, _dp, _dp, _dp, _dp]
        L.socp_ctx_has_hamiltonian_jacobian.argtypes = [_vp]
        L.socp_hamiltonian_jacobian_batch_dev.argtypes = [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp]
        L.socp_hamiltonian_jacobian_batch.argtypes = [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp]
        L.socp_linsolve_batch_dev.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]
        L.socp_svd_batch_dev.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp]
        L.socp_branch_work_bytes.argtypes = [_vp, C.c_int]
        L.socp_branch_work_bytes.restype = C.c_size_t
        _bo = C.POINTER(BranchOptions)
        L.socp_branch_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, _bo, _vp, C.c_size_t] + [_vp] * 10
        L.socp_branch_batch.argtypes = [_vp, C.c_int, _dp, C.c_int, C.c_int, _bo, _dp, _dp, _dp, _ip, _ip, _ip, _ip, _ip, _dp, _dp]
        L.socp_branch_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, _bo, _dp, _dp, _dp, _ip, _ip,
                                               _ip, _ip, _ip, _dp, _dp]
        _no = C.POINTER(NewtonOptions)
        L.socp_newton_work_bytes.argtypes = [_vp, C.c_int, _no]
        L.socp_newton_work_bytes.restype = C.c_size_t
        L.socp_newton_batch_dev.argtypes = [_vp, C.c_int, _vp, _no, _vp, C.c_size_t] + [_vp] * 8
        L.socp_newton_batch.argtypes = [_vp, C.c_int, _dp, _no, _dp, _dp, _dp, _dp, _ip, _ip, _ip, _dp]
        L.socp_newton_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _no, _dp, _dp, _dp, _dp, _ip, _ip, _ip, _dp]
        L.socp_singular_work_bytes.argtypes = [_vp, C.c_int]
        L.socp_singular_work_bytes.restype = C.c_size_t
        L.socp_singular_batch_dev.argtypes = [_vp, C.c_int, _vp, C.c_double, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp]
        L.socp_singular_batch.argtypes = [_vp, C.c_int, _dp, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip]
        L.socp_singular_batch_blocks.argtypes = [_vp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp,
                                                 _ip, _ip]
        L.socp_group_batch_dev.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp]
        L.socp_group_batch.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _dp, _ip, C.c_double, C.c_double, C.c_int, _ip, _ip, _ip, _dp, _ip]
        L.socp_ctx_get_switching_times.argtypes = [_vp, _dp]
        L.socp_chains_solve.argtypes = [_vp, C.c_int, C.POINTER(ChainOptions), _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip,
                                        _ip, _dp, _dp, _dp, C.POINTER(ChainStats)]
        L.socp_chains_solve_ex.argtypes = [_vp, C.c_int, C.POINTER(ChainOptions), _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip,
                                           _ip, _ip, _dp, _dp, _dp, C.POINTER(ChainStats)]
        L.socp_var_jacobian_multi_dev.argtypes = [_vp, C.c_int, _vp, _vp]
        L.socp_multistart_solve.argtypes = [_vp, C.c_int, _dp, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int,
                                            _dp, _ip, _ip, _dp, C.POINTER(C.c_longlong)]
        L.hybrd.argtypes = [FCN, _vp, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double,
                            _dp, C.c_int, C.c_double, C.c_int, _ip, _dp, C.c_int, _dp, C.c_int, _dp,
                            _dp, _dp, _dp, _dp]
        L.socp_hybrd_batched.argtypes = [FCN, FDJAC] + L.hybrd.argtypes[1:]
        L.hybrj.argtypes = [FCNDER, _vp, C.c_int, _dp, _dp, _dp, C.c_int, C.c_double, C.c_int, _dp, C.c_int,
                            C.c_double, C.c_int, _ip, _ip, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp]
        L.socp_hybr_create.restype = _vp
        L.socp_hybr_create.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int]
        L.socp_hybr_destroy.argtypes = [_vp]
        L.socp_hybr_start.argtypes = [_vp, _dp, _dp]
        L.socp_hybr_advance.argtypes = [_vp, C.c_int, C.POINTER(_dp), C.POINTER(_dp)]
        for name in ("socp_hybr_info", "socp_hybr_nfev", "socp_hybr_njev"):
            getattr(L, name).argtypes = [_vp]
        for name in ("socp_hybr_x", "socp_hybr_fvec"):
            getattr(L, name).argtypes = [_vp]
            getattr(L, name).restype = _dp
        L.socp_hybr_trust_region.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.socp_hybr_trust_region.restype = None
        L.socp_workspace_release.argtypes = [C.c_int]
        L.socp_workspace_release.restype = C.c_double
        L.socp_workspace_cached_bytes.argtypes = [C.c_int]
        L.socp_workspace_cached_bytes.restype = C.c_double
        L.socp_qr_factor_batch.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, C.POINTER(C.c_double)]
        L.socp_ctx_get_variant.argtypes = [_vp]
        _lib = L
    return _lib


def workspace_release(device=-1):
    """socp_workspace_release (include/socp_solver.h): frees the device engine's kept arenas of `device` (< 0: all); bytes freed."""
    return lib().socp_workspace_release(int(device))


def workspace_cached_bytes(device=-1):
    """socp_workspace_cached_bytes: device + pinned bytes the device engine keeps for its next call on `device` (< 0: all)."""
    return lib().socp_workspace_cached_bytes(int(device))


def qr_factor_batch(J, b, flavour=FACTOR_FAST, reps=1, device=-1, outputs=True):
    """socp_qr_factor_batch (include/socp_solver.h): J[count][n][n] as matrices J[k][i][j] = J_k(i, j), b[count][n].
    Returns dict(Q[count][n][n], R[count][n][n] (upper triangular, unpacked), qtb, rdiag, acnorm, sing, kernel_ms)."""
    L = lib()
    J = _f64(J)
    count, n = J.shape[0], J.shape[1]
    Jcm = np.ascontiguousarray(np.transpose(J, (0, 2, 1)))                   # column-major per problem
    b = _f64(b).reshape(count, n)
    ms = C.c_double(0)
    if not outputs:
        rc = L.socp_qr_factor_batch(int(device), n, count, _d(Jcm), _d(b), int(flavour), int(reps), None, None, None, None, None, None, C.byref(ms))
        if rc != OK:
            raise RuntimeError("socp_qr_factor_batch: %d" % rc)
        return {"kernel_ms": ms.value}
    Q = np.empty((count, n, n))
    Rp = np.empty((count, n * (n + 1) // 2))
    qtb, rdiag, acnorm = np.empty((count, n)), np.empty((count, n)), np.empty((count, n))
    sing = np.zeros(count, dtype=np.int32)
    rc = L.socp_qr_factor_batch(int(device), n, count, _d(Jcm), _d(b), int(flavour), int(reps), _d(Q), _d(Rp), _d(qtb), _d(rdiag), _d(acnorm),
                                sing.ctypes.data_as(_ip), C.byref(ms))
    if rc != OK:
        raise RuntimeError("socp_qr_factor_batch: %d" % rc)
    R = np.zeros((count, n, n))
    iu = np.triu_indices(n)
    R[:, iu[0], iu[1]] = Rp                                                  # packed by rows = row-major order of the upper triangle
    return {"Q": Q, "R": R, "qtb": qtb, "rdiag": rdiag, "acnorm": acnorm, "sing": sing, "kernel_ms": ms.value}


def plugin_load(path):
    """Load an out-of-tree device model (include/socp_plugin.h); afterwards Context(model_id) works."""
    rc = lib().socp_plugin_load(os.fsencode(path))
    if rc != OK:
        raise SocpError(rc, lib().socp_last_error(None).decode())


def trace_kept_rows(R, stride):
    """Indices of the rows a batched trace keeps of the R rows integrate_dense_aux reports for a segment: every stride-th from
    row 0, and the last one (socp_trace_batch_dev).  The definition callers and tests share."""
    R, stride = int(R), int(stride)
    if R < 1 or stride < 1:
        raise ValueError("trace_kept_rows: R >= 1 and stride >= 1 are required")
    kept = list(range(0, R, stride))
    if kept[-1] != R - 1:
        kept.append(R - 1)
    return kept


EXTREMA_CONTROL, EXTREMA_HAMILTONIAN, EXTREMA_EVENTS = 1, 2, 4


def extrema_channel_names(dim, control_dim, event_channels=0):
    """Names of the C = 2 dim + control_dim + 1 + event_channels channels of extrema_batch, in their order: x0.., p0.. (the state
    and the costate), u0.., H, g0.. (the model's event channels)."""
    return (["x%d" % k for k in range(dim)] + ["p%d" % k for k in range(dim)] + ["u%d" % k for k in range(control_dim)] + ["H"]
            + ["g%d" % k for k in range(event_channels)])


def merge_events(t, id, count):
    """The events of all segments of every row, sorted by time: from what events_batch returns (t[B][M][cap], id[B][M][cap],
    count[B][M]) a list of B pairs (times, ids).  Only the stored events take part (min(count, cap) per segment); events at equal
    times keep their (segment, step, watch) order."""
    t, id, count = np.asarray(t), np.asarray(id), np.asarray(count)
    B, M, cap = t.shape
    out = []
    for b in range(B):
        tt = np.concatenate([t[b, i, :min(int(count[b, i]), cap)] for i in range(M)]) if M else np.empty(0)
        ii = np.concatenate([id[b, i, :min(int(count[b, i]), cap)] for i in range(M)]) if M else np.empty(0, dtype=np.int32)
        order = np.argsort(tt, kind="stable")
        out.append((tt[order], ii[order]))
    return out


def move_segment(tl, q):
    """The selection rule of shooting::Move(tf) (shooting.cpp:407-424) as the batched move applies it: for a timeline tl[0 .. M] and a
    query time q, returns (seg, target) -- the query clamped to [tl[0], tl[M]] the reference's way (out of range and NaN go to tl[M]) and
    the segment whose start node the integration tl[seg] -> target starts from.  The definition callers and tests share."""
    tl = [float(t) for t in tl]
    M = len(tl) - 1
    if M < 1:
        raise ValueError("move_segment: a timeline has at least two entries")
    q = float(q)
    target = q if (q >= tl[0] and q <= tl[M]) else tl[M]
    seg = 0
    while seg < M - 1 and tl[seg + 1] < target:
        seg += 1
    return seg, target


def _d(a):
    """double* of a float64 array (the pointer keeps the array alive); None stays None: an optional argument that is absent."""
    return a.ctypes.data_as(_dp) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _block_args(B, params, time, xnode):
    """The (params, param_stride, time, xnode) arguments of a _blocks entry point from per-row blocks of B rows each (None: absent)."""
    pp, tt, xx = (_f64(a).reshape(B, -1) if a is not None else None for a in (params, time, xnode))
    return _d(pp), pp.shape[1] if pp is not None else 0, _d(tt), _d(xx)


def _dirs(dirs):
    """(kind[K], index[K]) int32 arrays from a list of (kind, index) pairs."""
    d = np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 2)
    return np.ascontiguousarray(d[:, 0]), np.ascontiguousarray(d[:, 1])


def _call_with_enough_cap(call, cap):
    """call(cap) -> (count[B][M], result) of an entry point that stores at most `cap` items per segment and counts them all: called
    with `cap` and, when a segment had more, once more with cap = count.max().  Returns the last result."""
    cap = int(cap)
    count, result = call(cap)
    if count.size and count.max() > cap:
        count, result = call(int(count.max()))
    return result


class Context:
    """One device context = one model object with its packed parameters (socp_ctx)."""

    def __init__(self, model_id, device=-1, nparams=None):
        self.L = lib()
        self.h = _vp()
        rc = self.L.socp_ctx_create(C.byref(self.h), int(model_id), int(device))
        if rc != OK:
            raise SocpError(rc, self.L.socp_last_error(None).decode())
        dim, s, sj = C.c_int(), C.c_int(), C.c_int()
        self.L.socp_ctx_dims(self.h, C.byref(dim), C.byref(s), C.byref(sj))
        self.model_id, self.dim, self.s, self.s_jac = model_id, dim.value, s.value, sj.value
        self.nu = self.L.socp_ctx_control_dim(self.h)
        self.n = None
        self.nparams = nparams
        if nparams is None and model_id == MODEL_INTERCEPTOR:
            self.nparams = len(INTERCEPTOR_PARAM_NAMES)
        if nparams is None and model_id == MODEL_VTOLUAV:
            self.nparams = len(VTOL_PARAM_NAMES)

    def close(self):
        if self.h:
            self.L.socp_ctx_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            raise SocpError(rc, self.L.socp_last_error(self.h).decode())

    # -- configuration
    def aux_stream(self):
        """The context's second stream (socp_ctx_aux_stream): created on the first call (~6 ms), then kept."""
        st = C.c_void_p()
        self._chk(self.L.socp_ctx_aux_stream(self.h, C.byref(st)))
        return st.value

    def warm_up(self):
        """socp_ctx_warm_up: the process's one-time costs now (second stream, copy-engine start-up)."""
        self._chk(self.L.socp_ctx_warm_up(self.h))

    def has_variational(self):
        return self.L.socp_ctx_has_variational(self.h) == 1

    def set_params(self, params):
        p = _f64(params)
        self._chk(self.L.socp_ctx_set_params(self.h, _d(p), len(p)))

    def get_params(self):
        n = self.nparams if self.nparams is not None else (3 if self.model_id == MODEL_DOUBLE_INTEGRATOR else 8)
        p = np.empty(n)
        self._chk(self.L.socp_ctx_get_params(self.h, _d(p), n))
        return p

    def set_param(self, name, value):
        p = self.get_params()
        names = {MODEL_INTERCEPTOR: INTERCEPTOR_PARAM_NAMES, MODEL_VTOLUAV: VTOL_PARAM_NAMES}.get(self.model_id, GODDARD_PARAM_NAMES)
        p[names.index(name)] = value
        self.set_params(p)

    def set_map(self, table):
        """Obstacle table of the vtolUAV model (socp_ctx_set_map): rows of (type, centre xyz, radii xyz); an empty table is free space."""
        t = _f64(table).reshape(-1, MAP_STRIDE)
        self._chk(self.L.socp_ctx_set_map(self.h, t.shape[0], _d(t) if t.shape[0] else None))

    def get_map(self):
        """The table in force, read back from the device: array [n_obs][7]."""
        n = C.c_int()
        self._chk(self.L.socp_ctx_get_map(self.h, C.byref(n), None, 0))
        t = np.empty((n.value, MAP_STRIDE))
        if n.value:
            self._chk(self.L.socp_ctx_get_map(self.h, C.byref(n), _d(t), n.value))
        return t

    def set_step_number(self, n):
        self._chk(self.L.socp_ctx_set_step_number(self.h, int(n)))

    def set_integrator(self, kind, tol=1e-8):
        """kind: 0 = fixed-step RK4, 1 = adaptive Dormand-Prince 5(4) with abs = rel tolerance tol."""
        self._chk(self.L.socp_ctx_set_integrator(self.h, int(kind), float(tol)))

    def set_switching_times(self, sw):
        sw = _f64(sw)
        self._chk(self.L.socp_ctx_set_switching_times(self.h, _d(sw), len(sw)))

    def set_variant(self, v):
        self._chk(self.L.socp_ctx_set_variant(self.h, int(v)))

    def set_exact_hooks(self, on=True):
        """vtolUAV only: switch the context's exact fields / exact Jacobian / Newton jac = 2 on (they are off in a new context, which
        then answers as before the model had them: socp_ctx_set_exact_hooks)."""
        self._chk(self.L.socp_ctx_set_exact_hooks(self.h, int(bool(on))))

    def get_variant(self):
        return int(self.L.socp_ctx_get_variant(self.h))

    def set_stream(self, stream_ptr, use_own=False):
        """stream_ptr: hipStream_t as int (0 = the default stream); use_own=True: context's own stream."""
        self._chk(self.L.socp_ctx_set_stream(self.h, _vp(stream_ptr), int(bool(use_own))))

    def synchronize(self):
        self._chk(self.L.socp_ctx_synchronize(self.h))

    def counters(self):
        a, b = C.c_longlong(), C.c_longlong()
        self._chk(self.L.socp_ctx_counters(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- trajectories (host buffers)
    def integrate_batch(self, t0, tf, X0, sw=None, is_jac=0):
        X0 = _f64(X0)
        B = X0.shape[0]
        t0 = _f64(np.broadcast_to(t0, (B,)))
        tf = _f64(np.broadcast_to(tf, (B,)))
        Xf = np.empty_like(X0)
        swp = None
        if sw is not None:
            sw = _f64(sw)
            swp = _d(sw)
        self._chk(self.L.socp_integrate_batch(self.h, B, _d(t0), _d(tf), swp, _d(X0), _d(Xf), int(is_jac)))
        return Xf

    def integrate_batch_dev(self, B, d_t0, d_tf, d_sw, d_X0, d_Xf, is_jac=0):
        """Device pointers (ints); enqueue only."""
        self._chk(self.L.socp_integrate_batch_dev(self.h, int(B), _vp(d_t0), _vp(d_tf), _vp(d_sw), _vp(d_X0),
                                                  _vp(d_Xf), int(is_jac)))

    def integrate_dense(self, t0, tf, X0, sw=None, cap=None):
        """One trajectory, state after every step: returns (times[rows], X[rows][s])."""
        X0 = _f64(X0)
        cap = cap or 20000
        dense = np.empty((cap, len(X0)))
        times = np.empty(cap)
        rows = C.c_int(0)
        swp = _d(_f64(sw)) if sw is not None else None
        self._chk(self.L.socp_integrate_dense(self.h, float(t0), float(tf), swp, _d(X0), _d(dense), _d(times), cap,
                                              C.byref(rows)))
        k = min(rows.value, cap)
        return times[:k].copy(), dense[:k].copy()

    def integrate_dense_aux(self, t0, tf, X0, sw=None, cap=None):
        """As integrate_dense, plus each row's two auxiliary scalars: (times, X[rows][s], aux[rows][2])."""
        X0 = _f64(X0)
        cap = cap or 20000
        dense = np.empty((cap, len(X0)))
        times = np.empty(cap)
        aux = np.empty((cap, 2))
        rows = C.c_int(0)
        swp = _d(_f64(sw)) if sw is not None else None
        self._chk(self.L.socp_integrate_dense_aux(self.h, float(t0), float(tf), swp, _d(X0), _d(dense), _d(times),
                                                  _d(aux), cap, C.byref(rows)))
        k = min(rows.value, cap)
        return times[:k].copy(), dense[:k].copy(), aux[:k].copy()

    def eval_batch(self, what, t, X, sw=None, is_jac=0):
        X = _f64(X)
        B = X.shape[0]
        t = _f64(np.broadcast_to(t, (B,)))
        out_len = {EVAL_RHS: X.shape[1], EVAL_CONTROL: self.nu, EVAL_HAMILTONIAN: (self.s + 1) if is_jac else 1}[what]
        out = np.empty((B, out_len))
        swp = None
        if sw is not None:
            sw = _f64(sw)
            swp = _d(sw)
        self._chk(self.L.socp_eval_batch(self.h, what, B, _d(t), swp, _d(X), X.shape[1], _d(out), int(is_jac)))
        return out

    # -- Hamiltonian gradient
    def has_hamiltonian_gradient(self):
        """Whether this model has the Hamiltonian-gradient kernel (socp_ctx_has_hamiltonian_gradient): any model with the
        hamiltonian_t trait -- the in-tree Goddard, double integrator and covid19, a plugin that brings it."""
        return self.L.socp_ctx_has_hamiltonian_gradient(self.h) == 1

    def hamiltonian_gradient_batch_dev(self, B, d_t, d_sw, d_X, d_G):
        """Device pointers (ints; d_sw may be None): t[B], sw[B][2], X[B][S] -> G[B][S]; one launch, enqueue only, no allocation, no
        copy, no synchronise (socp_hamiltonian_gradient_batch_dev)."""
        self._chk(self.L.socp_hamiltonian_gradient_batch_dev(self.h, int(B), _vp(d_t), _vp(d_sw), _vp(d_X), _vp(d_G)))

    def hamiltonian_gradient_batch(self, t, X, sw=None):
        """G[B][S] = (dH/dp, -dH/dx) of the model's Hamiltonian text at the points (t, X[B][S]), by dual numbers through
        hamiltonian_t, the control law inside (include/socp_hip.h has the definition and says when this equals the costate
        equations).  Takes t, X and sw as eval_batch does; directly comparable with eval_batch(EVAL_RHS, t, X, sw)."""
        X = _f64(X).reshape(-1, self.s)
        B = X.shape[0]
        t = _f64(np.broadcast_to(t, (B,)))
        G = np.full((B, self.s), np.nan)
        swp = None
        if sw is not None:
            sw = _f64(sw)
            swp = _d(sw)
        self._chk(self.L.socp_hamiltonian_gradient_batch(self.h, B, _d(t), swp, _d(X), _d(G)))
        return G

    # -- Jacobian of the Hamiltonian vector field
    def has_hamiltonian_jacobian(self):
        """Whether this model has the Hamiltonian-Jacobian kernel (socp_ctx_has_hamiltonian_jacobian): any model whose hamiltonian_t
        takes nested dual numbers -- the in-tree Goddard, double integrator and covid19, a plugin that brings such a text."""
        return self.L.socp_ctx_has_hamiltonian_jacobian(self.h) == 1

    def hamiltonian_jacobian_batch_dev(self, B, d_t, d_sw, d_X, d_A, d_G=None):
        """Device pointers (ints; d_sw and d_G may be None): t[B], sw[B][2], X[B][S] -> A[B][S * S] column-major and G[B][S]; one
        launch, enqueue only, no allocation, no copy, no synchronise (socp_hamiltonian_jacobian_batch_dev)."""
        self._chk(self.L.socp_hamiltonian_jacobian_batch_dev(self.h, int(B), _vp(d_t), _vp(d_sw), _vp(d_X), _vp(d_A), _vp(d_G)))

    def hamiltonian_jacobian_batch(self, t, X, sw=None, gradient=False):
        """A[B][S][S] with A[b, i, j] = dG_i/dX_j, G = hamiltonian_gradient_batch's gradient of the model's Hamiltonian text: the
        TOTAL second derivative of X -> H(X, u(X)) by nested dual numbers (include/socp_hip.h, "NESTED DUAL NUMBERS").  Takes t, X
        and sw as hamiltonian_gradient_batch does.  gradient=True: returns (A, G), G[B][S] the value parts."""
        X = _f64(X).reshape(-1, self.s)
        B = X.shape[0]
        t = _f64(np.broadcast_to(t, (B,)))
        A = np.full((B, self.s * self.s), np.nan)
        G = np.full((B, self.s), np.nan) if gradient else None
        swp = None
        if sw is not None:
            sw = _f64(sw)
            swp = _d(sw)
        self._chk(self.L.socp_hamiltonian_jacobian_batch(self.h, B, _d(t), swp, _d(X), _d(A), _d(G) if gradient else None))
        A = A.reshape(B, self.s, self.s).transpose(0, 2, 1).copy()        # column-major per point -> [row i][column j]
        return (A, G) if gradient else A

    def var_jacobian(self, z):
        """Analytic (variational) shooting Jacobian J[row, col] (hybrj path)."""
        z = _f64(z)
        Jcm = np.empty((self.n, self.n))
        self._chk(self.L.socp_var_jacobian(self.h, _d(z), _d(Jcm)))
        return Jcm.T.copy()

    # -- shooting problem
    def problem_set(self, mode_t, mode_x, time, xnode):
        mode_t = np.ascontiguousarray(mode_t, dtype=np.int32)
        M = len(mode_t) - 1
        mode_x = np.ascontiguousarray(mode_x, dtype=np.int32).reshape(M + 1, self.dim)
        time = _f64(time)
        xnode = _f64(xnode).reshape(M + 1, self.s)
        self._chk(self.L.socp_problem_set(self.h, M, mode_t.ctypes.data_as(_ip), mode_x.ctypes.data_as(_ip),
                                          _d(time), _d(xnode)))
        self.M = M
        self.n = self.L.socp_problem_num_param(self.h)
        return self.n

    def timeline(self, z):
        z = _f64(z)
        tl = np.empty(self.M + 1)
        self._chk(self.L.socp_timeline(self.h, _d(z), _d(tl)))
        return tl

    def residual_batch(self, Z):
        Z = _f64(Z)
        assert Z.ndim == 2 and Z.shape[1] == self.n
        F = np.empty_like(Z)
        self._chk(self.L.socp_residual_batch(self.h, Z.shape[0], _d(Z), _d(F)))
        return F

    def residual(self, z):
        return self.residual_batch(_f64(z)[None, :])[0]

    def residual_batch_dev(self, B, d_Z, d_F):
        self._chk(self.L.socp_residual_batch_dev(self.h, int(B), _vp(d_Z), _vp(d_F)))

    def fd_jacobian(self, z, fvec, epsfcn=1e-15, dedup=False):
        """Returns J[row, col] (the C side is column-major)."""
        z, fvec = _f64(z), _f64(fvec)
        Jcm = np.empty((self.n, self.n))
        self._chk(self.L.socp_fd_jacobian(self.h, _d(z), _d(fvec), float(epsfcn), _d(Jcm), int(bool(dedup))))
        return Jcm.T.copy()

    def fd_rows(self, Z, epsfcn=1e-15):
        """Rows[np][n+1][n]: F(z) and the n forward-difference residuals, one launch."""
        Z = _f64(Z).reshape(-1, self.n)
        rows = np.empty((Z.shape[0], self.n + 1, self.n))
        self._chk(self.L.socp_fd_rows(self.h, Z.shape[0], _d(Z), float(epsfcn), _d(rows)))
        return rows

    def fd_rows_dev(self, np_, d_Z, epsfcn, d_rows):
        self._chk(self.L.socp_fd_rows_dev(self.h, int(np_), _vp(d_Z), float(epsfcn), _vp(d_rows)))

    def fd_diff_dev(self, np_, d_Z, epsfcn, d_rows, d_fjac):
        self._chk(self.L.socp_fd_diff_dev(self.h, int(np_), _vp(d_Z), float(epsfcn), _vp(d_rows), _vp(d_fjac)))

    def fd_jacobian_multi_dev(self, np_, d_Z, d_Fvec, epsfcn, d_Fjac, dedup=False):
        self._chk(self.L.socp_fd_jacobian_multi_dev(self.h, int(np_), _vp(d_Z), _vp(d_Fvec), float(epsfcn),
                                                    _vp(d_Fjac), int(bool(dedup))))

    def multistart_solve(self, Z0, xtol=1e-8, maxfev=10000, epsfcn=1e-15, factor=1.0, dedup=True):
        """Lock-step hybrd solves of the rows of Z0.  Returns dict(z, info, nfev, fnorm, rounds)."""
        Z0 = _f64(Z0).reshape(-1, self.n)
        P = Z0.shape[0]
        Z = np.empty_like(Z0)
        info = np.zeros(P, dtype=np.int32)
        nfev = np.zeros(P, dtype=np.int32)
        fnorm = np.zeros(P)
        rounds = C.c_longlong(0)
        self._chk(self.L.socp_multistart_solve(self.h, P, _d(Z0), float(xtol), int(maxfev), float(epsfcn), float(factor),
                                               int(bool(dedup)), _d(Z), info.ctypes.data_as(_ip),
                                               nfev.ctypes.data_as(_ip), _d(fnorm), C.byref(rounds)))
        return dict(z=Z, info=info, nfev=nfev, fnorm=fnorm, rounds=rounds.value)

    def residual_batch_blocks(self, Z, params=None, time=None, xnode=None):
        """Residual of every row of Z with that row's OWN parameter block [B][nparams + 2] (parameters, sw0, sw1) and / or
        boundary tables time [B][M+1], xnode [B][(M+1)*2d] (None: the shared ones)."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        F = np.empty_like(Z)
        self._chk(self.L.socp_residual_batch_blocks(self.h, B, _d(Z), *_block_args(B, params, time, xnode), _d(F)))
        return F

    # -- batched trace
    def trace_width(self):
        """Doubles per trace row of this model: t, X[2d], u[NU], H, aux0, aux1 (socp_trace_width)."""
        return self.L.socp_trace_width(self.h)

    def trace_batch_dev(self, B, d_Z, stride, cap, d_rows, d_count):
        """Device pointers (ints); enqueue only, no copy, no synchronise (socp_trace_batch_dev)."""
        self._chk(self.L.socp_trace_batch_dev(self.h, int(B), _vp(d_Z), int(stride), int(cap), _vp(d_rows), _vp(d_count)))

    def trace_batch(self, Z, stride=1, cap=None, params=None, time=None, xnode=None, fill=None):
        """Sampled trace rows of every segment of every row of Z: returns (rows[B][M][cap][W], count[B][M]); rows[b][i][k] for
        k < count[b][i] are row trace_kept_rows(R, stride)[k] of segment i (t, X, u, H, aux0, aux1), the rest holds `fill` (NaN).
        params / time / xnode: per-row blocks as in residual_batch_blocks.  cap=None runs the two-call protocol: a first call with
        step_nbr // stride + 3 rows per segment (64 under the adaptive integrator, whose row count is only known afterwards), and
        one more with cap = count.max() when a segment had more."""
        Z = _f64(Z).reshape(-1, self.n)
        B, W = Z.shape[0], self.trace_width()
        blocks = _block_args(B, params, time, xnode)

        def call(c):
            rows = np.full((B, self.M, c, W), np.nan if fill is None else fill)
            count = np.zeros((B, self.M), dtype=np.int32)
            self._chk(self.L.socp_trace_batch_blocks(self.h, B, _d(Z), *blocks, int(stride), c, _d(rows), count.ctypes.data_as(_ip)))
            return count, (rows, count)
        if cap is not None:
            return call(int(cap))[1]
        step_nbr, integrator = C.c_int(), C.c_int()
        self._chk(self.L.socp_ctx_get_integrator(self.h, C.byref(step_nbr), C.byref(integrator), None))
        return _call_with_enough_cap(call, 64 if integrator.value == INT_DOPRI5 else step_nbr.value // int(stride) + 3)

    # -- batched cost
    def has_cost(self):
        """Whether this model has a running-cost kernel (socp_ctx_has_cost); the interceptor has none."""
        return self.L.socp_ctx_has_cost(self.h) == 1

    def cost_batch_dev(self, B, d_Z, d_cost, d_total=None, d_Xend=None):
        """Device pointers (ints; d_total / d_Xend may be None); enqueue only, no copy, no synchronise (socp_cost_batch_dev)."""
        self._chk(self.L.socp_cost_batch_dev(self.h, int(B), _vp(d_Z), _vp(d_cost), _vp(d_total), _vp(d_Xend)))

    def cost_batch(self, Z, params=None, time=None, xnode=None, total=True, xend=False):
        """Integrated running cost L = H - <p, f_x> of every segment of every row of Z, along the residual's fixed RK4 steps:
        returns dict(cost[B][M], total[B] or None, xend[B][M][2d] or None).  params / time / xnode: per-row blocks as in
        residual_batch_blocks.  Fixed-step integrator only; not for the interceptor (has_cost)."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        blocks = _block_args(B, params, time, xnode)
        cost = np.empty((B, self.M))
        tot = np.empty(B) if total else None
        xe = np.empty((B, self.M, self.s)) if xend else None
        self._chk(self.L.socp_cost_batch_blocks(self.h, B, _d(Z), *blocks, _d(cost), _d(tot), _d(xe)))
        return dict(cost=cost, total=tot, xend=xe)

    # -- batched extrema
    def has_extrema(self):
        """Whether this model's launch table has an extrema entry (socp_ctx_has_extrema): every model with a trace entry."""
        return self.L.socp_ctx_has_extrema(self.h) == 1

    def extrema_width(self):
        """Channels of extrema_batch: X[2d], u[NU], H, g[event channels] (socp_extrema_width)."""
        return self.L.socp_extrema_width(self.h)

    def extrema_channels(self):
        """The channels' names, in their order (extrema_channel_names)."""
        return extrema_channel_names(self.dim, self.nu, self.event_channels())

    def extrema_batch_dev(self, B, d_Z, what, d_vmin, d_vmax, d_tmin, d_tmax, d_count, d_nbad=None):
        """Device pointers (ints; d_tmin / d_tmax / d_nbad may be None); enqueue only, no copy, no synchronise
        (socp_extrema_batch_dev)."""
        self._chk(self.L.socp_extrema_batch_dev(self.h, int(B), _vp(d_Z), int(what), _vp(d_vmin), _vp(d_vmax), _vp(d_tmin), _vp(d_tmax),
                                                _vp(d_count), _vp(d_nbad)))

    def extrema_batch(self, Z, what=7, blocks=None):
        """Per-segment extrema over the rows trace_batch keeps with stride = 1, in one launch that stores no row (include/socp_hip.h):
        returns dict(vmin, vmax, tmin, tmax [B][M][C], count[B][M], nbad[B][M], channels) -- the smallest and the largest value of
        every channel (extrema_channels), the time of the row that first attains it, the number of rows and the number of rows with
        a value that is not finite.  what: EXTREMA_CONTROL | EXTREMA_HAMILTONIAN | EXTREMA_EVENTS select u, H and the event channels
        beside the state; the columns of a group that is not selected hold NaN.  blocks = (params, time, xnode): per-row blocks as in
        residual_batch_blocks, host arrays or None."""
        Z = _f64(Z).reshape(-1, self.n)
        B, Cw = Z.shape[0], self.extrema_width()
        out = {k: np.full((B, self.M, Cw), np.nan) for k in ("vmin", "vmax", "tmin", "tmax")}
        count = np.zeros((B, self.M), dtype=np.int32)
        nbad = np.zeros((B, self.M), dtype=np.int32)
        self._chk(self.L.socp_extrema_batch_blocks(self.h, B, _d(Z), *_block_args(B, *(blocks if blocks is not None else (None, None, None))),
                                                   int(what), _d(out["vmin"]), _d(out["vmax"]), _d(out["tmin"]), _d(out["tmax"]),
                                                   count.ctypes.data_as(_ip), nbad.ctypes.data_as(_ip)))
        out.update(count=count, nbad=nbad, channels=self.extrema_channels())
        return out

    # -- batched observables
    def has_observe(self):
        """Whether this model's launch table has an observe entry (socp_ctx_has_observe): a model with the observables trait and
        without its own ComputeTraj."""
        return self.L.socp_ctx_has_observe(self.h) == 1

    def observable_names(self):
        """The names of the model's observables, in their order (socp_ctx_observables / socp_ctx_observable_name); [] without the
        entry."""
        return [self.L.socp_ctx_observable_name(self.h, k).decode() for k in range(max(0, self.L.socp_ctx_observables(self.h)))]

    def observe_batch_dev(self, B, d_Z, d_ymin, d_ymax, d_tmin, d_tmax, d_integral, d_count, d_nbad=None):
        """Device pointers (ints; d_tmin / d_tmax / d_integral / d_nbad may be None); enqueue only, no copy, no synchronise
        (socp_observe_batch_dev)."""
        self._chk(self.L.socp_observe_batch_dev(self.h, int(B), _vp(d_Z), _vp(d_ymin), _vp(d_ymax), _vp(d_tmin), _vp(d_tmax),
                                                _vp(d_integral), _vp(d_count), _vp(d_nbad)))

    def observe_batch(self, Z, blocks=None):
        """Extrema and trapezoid integrals of the model's observables over the rows trace_batch keeps with stride = 1, in one launch
        that stores no row (include/socp_hip.h): returns dict(ymin, ymax, tmin, tmax, integral [B][M][NO], count[B][M], nbad[B][M],
        names) -- per segment and observable (observable_names) the smallest and the largest value, the time of the row that first
        attains it and the integral over the segment; the number of rows and the number of rows with a value that is not finite.
        blocks = (params, time, xnode): per-row blocks as in residual_batch_blocks, host arrays or None."""
        Z = _f64(Z).reshape(-1, self.n)
        names = self.observable_names()
        B, NO = Z.shape[0], len(names)
        out = {k: np.full((B, self.M, NO), np.nan) for k in ("ymin", "ymax", "tmin", "tmax", "integral")}
        count = np.zeros((B, self.M), dtype=np.int32)
        nbad = np.zeros((B, self.M), dtype=np.int32)
        self._chk(self.L.socp_observe_batch_blocks(self.h, B, _d(Z), *_block_args(B, *(blocks if blocks is not None else (None, None, None))),
                                                   _d(out["ymin"]), _d(out["ymax"]), _d(out["tmin"]), _d(out["tmax"]), _d(out["integral"]),
                                                   count.ctypes.data_as(_ip), nbad.ctypes.data_as(_ip)))
        out.update(count=count, nbad=nbad, names=names)
        return out

    # -- batched events
    def event_channels(self):
        """Number of event channels of this model (socp_ctx_event_channels); 0: it has none (interceptor, vtolUAV)."""
        return self.L.socp_ctx_event_channels(self.h)

    def events_batch_dev(self, B, d_Z, chan, d_levels, refine, cap, d_tev, d_id, d_count, d_Xev=None):
        """Device pointers (ints; d_Xev may be None), chan a host sequence; enqueue only, no copy, no synchronise
        (socp_events_batch_dev)."""
        ch = np.ascontiguousarray(chan, dtype=np.int32).ravel()
        self._chk(self.L.socp_events_batch_dev(self.h, int(B), _vp(d_Z), len(ch), ch.ctypes.data_as(_ip), _vp(d_levels), int(refine), int(cap),
                                               _vp(d_tev), _vp(d_id), _vp(d_count), _vp(d_Xev)))

    def events_batch(self, Z, chan, levels, refine=2, cap=4, params=None, time=None, xnode=None, xev=False):
        """Every crossing of channel chan[e] through levels[b][e] (a 1-D levels: the same for all rows) along the residual's fixed
        RK4 steps of every segment of every row of Z, each refined inside its step by `refine` false-position steps (include/socp_hip.h).
        Returns (t[B][M][cap], id[B][M][cap], count[B][M]) and Xev[B][M][cap][2d] with xev=True; id = +(e+1) rising, -(e+1) falling;
        the slots at or beyond count hold NaN / 0.  When a segment has more than `cap` events the call is repeated with the largest
        count.  params / time / xnode: per-row blocks as in residual_batch_blocks.  merge_events sorts a row's events by time."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        ch = np.ascontiguousarray(chan, dtype=np.int32).ravel()
        E = len(ch)
        lv = np.asarray(levels, dtype=np.float64)
        lv = np.array(np.broadcast_to(lv, (B, E)) if lv.ndim == 1 else lv.reshape(B, E), dtype=np.float64, order="C")
        blocks = _block_args(B, params, time, xnode)

        def call(c):
            t = np.full((B, self.M, c), np.nan)
            ident = np.zeros((B, self.M, c), dtype=np.int32)
            count = np.zeros((B, self.M), dtype=np.int32)
            X = np.full((B, self.M, c, self.s), np.nan) if xev else None
            self._chk(self.L.socp_events_batch_blocks(self.h, B, _d(Z), *blocks, E, ch.ctypes.data_as(_ip), _d(lv), int(refine), c, _d(t),
                                                      ident.ctypes.data_as(_ip), count.ctypes.data_as(_ip), _d(X)))
            return count, ((t, ident, count, X) if xev else (t, ident, count))
        return _call_with_enough_cap(call, cap)

    # -- batched Jacobi fields
    def has_jacobi(self):
        """Whether this model has a Jacobi-field kernel (socp_ctx_has_jacobi); the interceptor and vtolUAV have none."""
        return self.L.socp_ctx_has_jacobi(self.h) == 1

    def jacobi_batch_dev(self, B, d_Z, epsfcn, stride, skip, cap, d_tq, d_det, d_count, d_nchange, d_tconj, d_Jend=None):
        """Device pointers (ints; d_Jend may be None); enqueue only, no copy, no synchronise (socp_jacobi_batch_dev)."""
        self._chk(self.L.socp_jacobi_batch_dev(self.h, int(B), _vp(d_Z), float(epsfcn), int(stride), int(skip), int(cap), _vp(d_tq), _vp(d_det),
                                               _vp(d_count), _vp(d_nchange), _vp(d_tconj), _vp(d_Jend)))

    def jacobi_batch(self, Z, stride=1, skip=0, cap=64, epsfcn=0.0, jend=False, blocks=None):
        """Conjugate-time test of every segment of every row of Z (include/socp_hip.h): the determinant of J(t) = dx(t)/dp(t0), formed
        from d + 1 trajectories along the residual's fixed RK4 steps and sampled every `stride` steps and after the last; sign changes
        between consecutive samples from sample `skip` on.  Z: a host array or a torch tensor on the device.  Returns a dict of
        DEVICE tensors, the work of the context's stream synchronised: tq[B][M][cap], det[B][M][cap] (NaN at or beyond count),
        count[B][M], nchange[B][M], tconj[B][M] (NaN: no change) and, with jend=True, jend[B][M][d][d].  When a segment has more
        than `cap` samples the call is repeated with the largest count.  blocks = (params, time, xnode): per-row blocks as in
        residual_batch_blocks, each a host array, a device tensor or None; they replace blocks set with socp_problem_set_blocks_dev and are cleared afterwards.
        A measuring instrument: the classical statement is for M = 1 with a fixed initial state; see the header for the rest."""
        import torch
        dev = torch.device("cuda")
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
        Zd = up(Z).reshape(-1, self.n)
        B, M, d = Zd.shape[0], self.M, self.dim
        held = [up(a).reshape(B, -1) if a is not None else None for a in (blocks if blocks is not None else ())]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731

        def call(c):
            out = dict(tq=torch.full((B, M, c), float("nan"), dtype=torch.float64, device=dev),
                       det=torch.full((B, M, c), float("nan"), dtype=torch.float64, device=dev),
                       count=torch.zeros((B, M), dtype=torch.int32, device=dev), nchange=torch.zeros((B, M), dtype=torch.int32, device=dev),
                       tconj=torch.full((B, M), float("nan"), dtype=torch.float64, device=dev))
            if jend:
                out["jend"] = torch.zeros((B, M, d, d), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            if B:
                self.jacobi_batch_dev(B, Zd.data_ptr(), epsfcn, stride, skip, c, out["tq"].data_ptr(), out["det"].data_ptr(), out["count"].data_ptr(),
                                      out["nchange"].data_ptr(), out["tconj"].data_ptr(), out["jend"].data_ptr() if jend else None)
            self.synchronize()
            return out["count"].cpu().numpy(), out

        if not held:
            return _call_with_enough_cap(call, cap)
        pp, tt, xx = held
        self._chk(self.L.socp_problem_set_blocks_dev(self.h, ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx)))
        try:
            return _call_with_enough_cap(call, cap)
        finally:
            self.L.socp_problem_set_blocks_dev(self.h, None, 0, None, None)

    # -- batched exact fields
    def has_fields(self):
        """Whether this model has an exact-fields kernel (socp_ctx_has_fields): the in-tree Goddard, double integrator and covid19,
        vtolUAV after set_exact_hooks() (both flavours read one reference-order object), and a plugin with the rhs_t trait; not the interceptor."""
        return self.L.socp_ctx_has_fields(self.h) == 1

    def fields_batch_dev(self, B, d_Z, cols, stride, skip, cap, d_tq, d_det, d_count, d_nchange, d_tconj, d_Phi=None):
        """Device pointers (ints; d_Phi may be None); enqueue only, no copy, no synchronise (socp_fields_batch_dev)."""
        self._chk(self.L.socp_fields_batch_dev(self.h, int(B), _vp(d_Z), int(cols), int(stride), int(skip), int(cap), _vp(d_tq), _vp(d_det),
                                               _vp(d_count), _vp(d_nchange), _vp(d_tconj), _vp(d_Phi)))

    def fields_batch(self, Z, cols=0, stride=1, skip=0, cap=64, phi=False, blocks=None):
        """The conjugate-time test of jacobi_batch with EXACT Jacobi fields (include/socp_hip.h): J(t) = dx(t)/dp(t0) carried through the
        residual's fixed RK4 steps on dual numbers -- the derivative of the discrete flow, no epsfcn.  cols = FIELDS_COSTATE (0): the
        d costate columns; FIELDS_ALL (1): all s columns, the whole transition matrix.  Returns a dict of DEVICE tensors like
        jacobi_batch: tq, det [B][M][cap], count, nchange, tconj [B][M] and, with phi=True, phi[B][M][s][C] and jend[B][M][d][d] = the
        x-rows of the costate columns of phi (a view).  Repeated with the largest count when a segment has more than `cap` samples.
        blocks = (params, time, xnode) as in jacobi_batch.  The same bits on a throughput-flavour context."""
        import torch
        dev = torch.device("cuda")
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
        Zd = up(Z).reshape(-1, self.n)
        B, M, d = Zd.shape[0], self.M, self.dim
        ncol = 2 * d if int(cols) == FIELDS_ALL else d
        held = [up(a).reshape(B, -1) if a is not None else None for a in (blocks if blocks is not None else ())]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731

        def call(c):
            out = dict(tq=torch.full((B, M, c), float("nan"), dtype=torch.float64, device=dev),
                       det=torch.full((B, M, c), float("nan"), dtype=torch.float64, device=dev),
                       count=torch.zeros((B, M), dtype=torch.int32, device=dev), nchange=torch.zeros((B, M), dtype=torch.int32, device=dev),
                       tconj=torch.full((B, M), float("nan"), dtype=torch.float64, device=dev))
            if phi:
                out["phi"] = torch.zeros((B, M, 2 * d, ncol), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            if B:
                self.fields_batch_dev(B, Zd.data_ptr(), cols, stride, skip, c, out["tq"].data_ptr(), out["det"].data_ptr(), out["count"].data_ptr(),
                                      out["nchange"].data_ptr(), out["tconj"].data_ptr(), out["phi"].data_ptr() if phi else None)
            self.synchronize()
            if phi:
                out["jend"] = out["phi"][:, :, :d, ncol - d:]
            return out["count"].cpu().numpy(), out

        if not held:
            return _call_with_enough_cap(call, cap)
        pp, tt, xx = held
        self._chk(self.L.socp_problem_set_blocks_dev(self.h, ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx)))
        try:
            return _call_with_enough_cap(call, cap)
        finally:
            self.L.socp_problem_set_blocks_dev(self.h, None, 0, None, None)

    # -- batched neighbouring-extremal gains
    def has_gain(self):
        """Whether this model has the gain kernels (socp_ctx_has_gain): the in-tree Goddard, double integrator and covid19, and a plugin
        with the rhs_t trait and no switching_state hook, custom final rows or ComputeTraj of its own; not the interceptor, not vtolUAV."""
        return self.L.socp_ctx_has_gain(self.h) == 1

    def gain_batch_dev(self, B, d_Z, stride, cap, d_tq, d_Kp, d_info, d_count, d_Xq=None, d_Wq=None, d_Psi=None):
        """Device pointers (ints; d_Xq, d_Wq, d_Psi may be None); enqueue only, no copy, no synchronise (socp_gain_batch_dev)."""
        self._chk(self.L.socp_gain_batch_dev(self.h, int(B), _vp(d_Z), int(stride), int(cap), _vp(d_tq), _vp(d_Kp), _vp(d_info), _vp(d_count),
                                             _vp(d_Xq), _vp(d_Wq), _vp(d_Psi)))

    def gain_batch(self, Z, stride=1, cap=None, xq=True, wq=False, psi=False, blocks=None):
        """The neighbouring-extremal feedback gains along every row of Z (include/socp_hip.h): at sample q of segment i, the start of
        step q * stride, kp[b][i][q] is the d x d matrix dp/dx (COLUMN-major: kp[b][i][q][c][r] = dp_r/dx_c, so kp[b][i][q].T is K) with
        which the costate correction dp = K dx keeps the final boundary rows satisfied to first order -- exact for the discrete flow.
        Returns a dict of DEVICE tensors: tq[B][M][cap], kp[B][M][cap][d][d], info[B][M][cap] (the elimination's code, 0 = solved),
        count[B][M] and, when asked for, xq[B][M][cap][s], wq[B][M][cap][d][s] (the final rows' sensitivity to the state at the sample)
        and psi[B][M][cap][s][s] (the blocks, row-major).  cap defaults to ceil(step_nbr / stride); the slots at or beyond count keep
        NaN (info -1).  blocks = (params, time, xnode) as in fields_batch.  The same bits on a throughput-flavour context."""
        import torch
        dev = torch.device("cuda")
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
        Zd = up(Z).reshape(-1, self.n)
        B, M, d = Zd.shape[0], self.M, self.dim
        stride = int(stride)
        step_nbr = C.c_int()
        self._chk(self.L.socp_ctx_get_integrator(self.h, C.byref(step_nbr), None, None))
        c = int(cap) if cap is not None else max(1, -(-step_nbr.value // max(1, stride)))
        held = [up(a).reshape(B, -1) if a is not None else None for a in (blocks if blocks is not None else ())]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        nan = float("nan")
        out = dict(tq=torch.full((B, M, c), nan, dtype=torch.float64, device=dev),
                   kp=torch.full((B, M, c, d, d), nan, dtype=torch.float64, device=dev),
                   info=torch.full((B, M, c), -1, dtype=torch.int32, device=dev), count=torch.zeros((B, M), dtype=torch.int32, device=dev))
        if xq:
            out["xq"] = torch.full((B, M, c, 2 * d), nan, dtype=torch.float64, device=dev)
        if wq:
            out["wq"] = torch.full((B, M, c, d, 2 * d), nan, dtype=torch.float64, device=dev)
        if psi:
            out["psi"] = torch.full((B, M, c, 2 * d, 2 * d), nan, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        if held:
            pp, tt, xx = held
            self._chk(self.L.socp_problem_set_blocks_dev(self.h, ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx)))
        try:
            self.gain_batch_dev(B, Zd.data_ptr(), stride, c, out["tq"].data_ptr(), out["kp"].data_ptr(), out["info"].data_ptr(),
                                out["count"].data_ptr(), ptr(out.get("xq")), ptr(out.get("wq")), ptr(out.get("psi")))
            self.synchronize()
        finally:
            if held:
                self.L.socp_problem_set_blocks_dev(self.h, None, 0, None, None)
        return out

    # -- batched neighbouring-extremal gains with a free final time
    def has_gain_free(self):
        """Whether this model has the free-final-time gain kernels (socp_ctx_has_gain_free): has_gain()'s condition and the hamiltonian_t
        trait -- the in-tree Goddard, double integrator and covid19, and a plugin with both traits."""
        return self.L.socp_ctx_has_gain_free(self.h) == 1

    def gain_free_batch_dev(self, B, d_Z, stride, cap, d_tq, d_Ke, d_info, d_count, d_Xq=None, d_Wq=None, d_Psi=None, d_Len=None):
        """Device pointers (ints; d_Xq, d_Wq, d_Psi, d_Len may be None); enqueue only, no copy, no synchronise (socp_gain_free_batch_dev)."""
        self._chk(self.L.socp_gain_free_batch_dev(self.h, int(B), _vp(d_Z), int(stride), int(cap), _vp(d_tq), _vp(d_Ke), _vp(d_info),
                                                  _vp(d_count), _vp(d_Xq), _vp(d_Wq), _vp(d_Psi), _vp(d_Len)))

    def gain_free_batch(self, Z, stride=1, cap=None, xq=True, wq=False, psi=False, length=False, blocks=None):
        """The neighbouring-extremal feedback gains along every row of Z of a problem whose FINAL TIME IS FREE (include/socp_hip.h): at
        sample q of segment i, kp[b][i][q] is the d x d matrix dp/dx in gain_batch's layout (kp[b][i][q][c][r] = dp_r/dx_c) and
        kt[b][i][q][c] = dt_f/dx_c, with which dp = K_p dx and dt_f = k_t . dx keep the final boundary rows AND H(t_f) = 0 satisfied to
        first order -- exact for the discrete flow; dx is measured at the sample index and the remaining steps are re-timed with the
        new t_f.  Returns a dict of DEVICE tensors: tq, kp, kt[B][M][cap][d], ke[B][M][cap][d][d+1] (the call's own layout, of which kp
        and kt are views), info, count and, when asked for, xq[B][M][cap][s], wq[B][M][cap][d+1][s+1], psi[B][M][cap][s][s],
        len[B][M][cap][s].  cap, the slots at or beyond count and blocks as in gain_batch.  The same bits on a throughput-flavour context."""
        import torch
        dev = torch.device("cuda")
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
        Zd = up(Z).reshape(-1, self.n)
        B, M, d = Zd.shape[0], self.M, self.dim
        stride = int(stride)
        step_nbr = C.c_int()
        self._chk(self.L.socp_ctx_get_integrator(self.h, C.byref(step_nbr), None, None))
        c = int(cap) if cap is not None else max(1, -(-step_nbr.value // max(1, stride)))
        held = [up(a).reshape(B, -1) if a is not None else None for a in (blocks if blocks is not None else ())]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        nan = float("nan")
        out = dict(tq=torch.full((B, M, c), nan, dtype=torch.float64, device=dev),
                   ke=torch.full((B, M, c, d, d + 1), nan, dtype=torch.float64, device=dev),
                   info=torch.full((B, M, c), -1, dtype=torch.int32, device=dev), count=torch.zeros((B, M), dtype=torch.int32, device=dev))
        if xq:
            out["xq"] = torch.full((B, M, c, 2 * d), nan, dtype=torch.float64, device=dev)
        if wq:
            out["wq"] = torch.full((B, M, c, d + 1, 2 * d + 1), nan, dtype=torch.float64, device=dev)
        if psi:
            out["psi"] = torch.full((B, M, c, 2 * d, 2 * d), nan, dtype=torch.float64, device=dev)
        if length:
            out["len"] = torch.full((B, M, c, 2 * d), nan, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        if held:
            pp, tt, xx = held
            self._chk(self.L.socp_problem_set_blocks_dev(self.h, ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx)))
        try:
            self.gain_free_batch_dev(B, Zd.data_ptr(), stride, c, out["tq"].data_ptr(), out["ke"].data_ptr(), out["info"].data_ptr(),
                                     out["count"].data_ptr(), ptr(out.get("xq")), ptr(out.get("wq")), ptr(out.get("psi")), ptr(out.get("len")))
            self.synchronize()
        finally:
            if held:
                self.L.socp_problem_set_blocks_dev(self.h, None, 0, None, None)
        out["kp"] = out["ke"][..., :d]
        out["kt"] = out["ke"][..., d]
        return out

    # -- closed-loop flight under the sampled neighbouring-extremal law
    def has_guide(self):
        """Whether this model has the closed-loop flight kernel (socp_ctx_has_guide): every model without a switching_state hook, custom
        final rows or ComputeTraj of its own -- the in-tree Goddard, double integrator and covid19, and such plugins; not the interceptor,
        not vtolUAV.  guide_batch also needs the gain entry of the problem's structure (has_gain / has_gain_free)."""
        return self.L.socp_ctx_has_guide(self.h) == 1

    def guide_batch_dev(self, B, d_Z, stride, cap, d_Xq, d_Kg, d_info, d_count, K, d_dX0, every, d_Xf, d_miss, d_nupd, d_nskip, d_tf=None,
                        d_dxmax=None, d_Xs=None):
        """Device pointers (ints; d_tf, d_dxmax, d_Xs may be None); enqueue only, no copy, no synchronise (socp_guide_batch_dev)."""
        self._chk(self.L.socp_guide_batch_dev(self.h, int(B), _vp(d_Z), int(stride), int(cap), _vp(d_Xq), _vp(d_Kg), _vp(d_info), _vp(d_count),
                                              int(K), _vp(d_dX0), int(every), _vp(d_Xf), _vp(d_miss), _vp(d_nupd), _vp(d_nskip), _vp(d_tf),
                                              _vp(d_dxmax), _vp(d_Xs)))

    def guide_batch(self, Z, dx0, stride=1, every=1, tables=None, blocks=None, xs=False):
        """K dispersed cases per row of Z flown in closed loop under the sampled neighbouring-extremal law (include/socp_hip.h): case
        (b, k) starts from x = z_x + dx0[b][k] with the nominal costate, takes the residual's steps through all M segments and, at every
        `every`-th sample whose table entry has info == 0, RESETS its costate to p_nom + K_p (x - x_nom) -- and re-times the rest of the
        flight with t_f + k_t . (x - x_nom) when the final time is FREE.  every = 0: open loop.  dx0: [B][K][d].  tables: the dict
        gain_batch / gain_free_batch returned for the same Z, stride and blocks (with xq); None: that call is made here.  A caller may
        disable samples by writing a nonzero info into the tables.  Returns a dict of DEVICE tensors: xf[B][K][s], miss[B][K][d]
        ([d + 1] with a free final time: the final rows, then H), nupd, nskip[B][K] (int32), tf[B][K], dxmax[B][K], the tables, and with
        xs=True xs[B][K][M][cap][s], the state at every sample after its correction (NaN where there is no sample)."""
        import torch
        dev = torch.device("cuda")
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
        Zd = up(Z).reshape(-1, self.n)
        B, M, d = Zd.shape[0], self.M, self.dim
        free = self.n > 2 * d * M
        stride = int(stride)
        if tables is None:
            tables = (self.gain_free_batch if free else self.gain_batch)(Zd, stride=stride, xq=True, blocks=blocks)
        kg = tables["ke" if free else "kp"].contiguous()
        xq, info, count = tables["xq"].contiguous(), tables["info"].contiguous(), tables["count"].contiguous()
        c = int(info.shape[2])
        D0 = up(dx0)
        K = int(D0.shape[1]) if D0.dim() == 3 else int(D0.numel() // max(1, B * d))
        D0 = D0.reshape(B, K, d)
        held = [up(a).reshape(B, -1) if a is not None else None for a in (blocks if blocks is not None else ())]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        nan = float("nan")
        out = dict(xf=torch.full((B, K, 2 * d), nan, dtype=torch.float64, device=dev),
                   miss=torch.full((B, K, d + 1 if free else d), nan, dtype=torch.float64, device=dev),
                   nupd=torch.zeros((B, K), dtype=torch.int32, device=dev), nskip=torch.zeros((B, K), dtype=torch.int32, device=dev),
                   tf=torch.full((B, K), nan, dtype=torch.float64, device=dev), dxmax=torch.full((B, K), nan, dtype=torch.float64, device=dev))
        if xs:
            out["xs"] = torch.full((B, K, M, c, 2 * d), nan, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        if held:
            pp, tt, xx = held
            self._chk(self.L.socp_problem_set_blocks_dev(self.h, ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx)))
        try:
            self.guide_batch_dev(B, Zd.data_ptr(), stride, c, xq.data_ptr(), kg.data_ptr(), info.data_ptr(), count.data_ptr(), K, D0.data_ptr(),
                                 int(every), out["xf"].data_ptr(), out["miss"].data_ptr(), out["nupd"].data_ptr(), out["nskip"].data_ptr(),
                                 out["tf"].data_ptr(), out["dxmax"].data_ptr(), ptr(out.get("xs")))
            self.synchronize()
        finally:
            if held:
                self.L.socp_problem_set_blocks_dev(self.h, None, 0, None, None)
        out["tables"] = tables
        return out

    # -- batched exact shooting Jacobian
    def has_exact_jacobian(self):
        """Whether this model has the exact shooting-Jacobian kernel (socp_ctx_has_exact_jacobian): the in-tree Goddard, double integrator
        and covid19, vtolUAV after set_exact_hooks() (custom final rows and switching_state rows through final_row_t / switching_state_t), and a plugin with the
        rhs_t, hamiltonian_t and switching_fn_t traits; not the interceptor."""
        return self.L.socp_ctx_has_exact_jacobian(self.h) == 1

    def exact_jacobian_batch_dev(self, B, d_Z, d_Fjac, d_F=None):
        """Device pointers (ints; d_F may be None); enqueue only, no copy, no synchronise (socp_exact_jacobian_batch_dev)."""
        self._chk(self.L.socp_exact_jacobian_batch_dev(self.h, int(B), _vp(d_Z), _vp(d_Fjac), _vp(d_F)))

    def exact_jacobian_batch(self, Z, residual=False, blocks=None):
        """The exact Jacobian dF/dz of the shooting function for every row of Z (include/socp_hip.h): dual numbers carried through the
        residual's RK4 steps and its boundary, continuity, Hamiltonian and switching rows, with the free-time columns.  Returns the
        DEVICE tensor J[B][n][n] holding each matrix COLUMN-major (J[b][j][r] = dF_r/dz_j: J[b].T is the matrix), the layout
        socp_linsolve_batch_dev and socp_svd_batch_dev take; with residual=True (J, F[B][n]).  blocks = (params, time, xnode) as in
        fields_batch.  The same bits on a throughput-flavour context."""
        import torch
        dev = torch.device("cuda")
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
        Zd = up(Z).reshape(-1, self.n)
        B, n = Zd.shape[0], self.n
        held = [up(a).reshape(B, -1) if a is not None else None for a in (blocks if blocks is not None else ())]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        J = torch.empty((B, n, n), dtype=torch.float64, device=dev)
        F = torch.empty((B, n), dtype=torch.float64, device=dev) if residual else None
        torch.cuda.synchronize()
        if held:
            pp, tt, xx = held
            self._chk(self.L.socp_problem_set_blocks_dev(self.h, ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt), ptr(xx)))
        try:
            self.exact_jacobian_batch_dev(B, Zd.data_ptr(), J.data_ptr(), ptr(F))
            self.synchronize()
        finally:
            if held:
                self.L.socp_problem_set_blocks_dev(self.h, None, 0, None, None)
        return (J, F) if residual else J

    # -- batched Move(tf) / re-grid
    def move_batch_dev(self, B, d_Z, K, d_tq, d_Xq, d_tout=None):
        """Device pointers (ints; d_tout may be None); enqueue only, no copy, no synchronise (socp_move_batch_dev)."""
        self._chk(self.L.socp_move_batch_dev(self.h, int(B), _vp(d_Z), int(K), _vp(d_tq), _vp(d_Xq), _vp(d_tout)))

    def move_batch(self, Z, tq, params=None, time=None, xnode=None, tout=False):
        """shooting::Move(tf) for a whole batch: the state on the stored solution Z[b] at every query time tq[b][k] (move_segment says
        from which node it is integrated).  Returns Xq[B][K][2d], or (Xq, tout[B][K]) with tout=True: the times actually reached.
        params / time / xnode: per-row blocks as in residual_batch_blocks."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        tq = _f64(tq)
        K = tq.size // B if B else (tq.shape[-1] if tq.ndim >= 2 else 0)
        tq = tq.reshape(B, K)
        blocks = _block_args(B, params, time, xnode)
        Xq = np.full((B, K, self.s), np.nan)
        to = np.full((B, K), np.nan) if tout else None
        self._chk(self.L.socp_move_batch_blocks(self.h, B, _d(Z), *blocks, K, _d(tq), _d(Xq), _d(to)))
        return (Xq, to) if tout else Xq

    def regrid_num_param(self, mode_t2):
        """Number of unknowns of a re-grid's target structure: 2d M2 + #FREE(mode_t2) (socp_regrid_num_param)."""
        mt = np.ascontiguousarray(mode_t2, dtype=np.int32)
        n2 = self.L.socp_regrid_num_param(self.h, len(mt) - 1, mt.ctypes.data_as(_ip))
        if n2 < 0:
            raise SocpError(n2, "regrid_num_param: 1 <= M2 <= 255 and time modes FIXED / FREE / CONTINUOUS are required")
        return n2

    def regrid_batch_dev(self, B, d_Z, mode_t2, d_T2, d_Z2, d_xnode2=None):
        """Device pointers (ints; d_xnode2 may be None), mode_t2 a host sequence; enqueue only (socp_regrid_batch_dev)."""
        mt = np.ascontiguousarray(mode_t2, dtype=np.int32)
        self._chk(self.L.socp_regrid_batch_dev(self.h, int(B), _vp(d_Z), len(mt) - 1, mt.ctypes.data_as(_ip), _vp(d_T2), _vp(d_Z2),
                                               _vp(d_xnode2)))

    def regrid_batch(self, Z, mode_t2, T2, params=None, time=None, xnode=None, want_xnode=True):
        """B solutions onto a new structure (time modes mode_t2[M2+1], node times T2[B][M2+1]): what testGoddard.cpp:119-145 does with
        Move + InitShooting(vt, vX).  Returns dict(z[B][n2], time = T2, xnode[B][M2+1][2d] or None): the start vectors of the next
        stage and the blocks chains_solve takes as time_goal / x_goal.  params / time / xnode: per-row blocks of THIS context's problem."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        mt = np.ascontiguousarray(mode_t2, dtype=np.int32)
        M2 = len(mt) - 1
        T2 = np.array(np.broadcast_to(np.asarray(T2, dtype=np.float64), (B, M2 + 1)), order="C")       # the caller's own times: returned as `time`
        blocks = _block_args(B, params, time, xnode)
        n2 = self.L.socp_regrid_num_param(self.h, M2, mt.ctypes.data_as(_ip))
        Z2 = np.full((B, max(n2, 0)), np.nan)
        X2 = np.full((B, M2 + 1, self.s), np.nan) if want_xnode else None
        self._chk(self.L.socp_regrid_batch_blocks(self.h, B, _d(Z), *blocks, M2, mt.ctypes.data_as(_ip), _d(T2), _d(Z2), _d(X2)))
        return dict(z=Z2, time=T2, xnode=X2)

    # -- batched tangent
    def tangent_work_bytes(self, B, K):
        """Bytes of the workspace tangent_batch_dev needs for B rows and K directions (socp_tangent_work_bytes)."""
        return int(self.L.socp_tangent_work_bytes(self.h, int(B), int(K)))

    def tangent_batch_dev(self, B, d_Z, dirs, epsfcn, jac, d_work, work_bytes, d_dZ, d_info, d_Fp=None):
        """Device pointers (ints; d_Fp may be None), dirs a host list of (kind, index); enqueue only, no allocation, no copy, no
        synchronise (socp_tangent_batch_dev)."""
        kinds, index = _dirs(dirs)
        self._chk(self.L.socp_tangent_batch_dev(self.h, int(B), _vp(d_Z), len(kinds), kinds.ctypes.data_as(_ip), index.ctypes.data_as(_ip),
                                                float(epsfcn), int(jac), _vp(d_work), int(work_bytes), _vp(d_dZ), _vp(d_info), _vp(d_Fp)))

    def tangent_batch(self, Z, dirs, epsfcn=1e-15, jac=0, params=None, time=None, xnode=None, fp=False):
        """dz/dtheta of every row of Z for the K directions dirs = [(kind, index), ...] (DIR_PARAM: slot of the packed block,
        DIR_TIME: node, DIR_XNODE: node * 2d + component): the solution of J dz = -dF/dtheta, J the forward-difference (jac=0) or
        variational (jac=1) shooting Jacobian (include/socp_hip.h has the definition).  Returns dict(dz[B][K][n], info[B] (0: solved,
        k + 1: no pivot at step k, n + 1: a solution entry is not finite), fp[B][K][n] = dF/dtheta or None).  params / time / xnode:
        per-row blocks as in residual_batch_blocks."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        kinds, index = _dirs(dirs)
        K = len(kinds)
        blocks = _block_args(B, params, time, xnode)
        dz = np.full((B, K, self.n), np.nan)
        info = np.zeros(B, dtype=np.int32)
        G = np.full((B, K, self.n), np.nan) if fp else None
        self._chk(self.L.socp_tangent_batch_blocks(self.h, B, _d(Z), *blocks, K, kinds.ctypes.data_as(_ip), index.ctypes.data_as(_ip),
                                                   float(epsfcn), int(jac), _d(dz), info.ctypes.data_as(_ip), _d(G)))
        return dict(dz=dz, info=info, fp=G)

    # -- batched exact sensitivities
    def has_sensitivity(self):
        """Whether this model has the exact-sensitivities kernel (socp_ctx_has_sensitivity): the in-tree Goddard, double integrator
        and covid19, and a plugin whose rhs_t / hamiltonian_t / switching_fn_t are generic in the parameter view."""
        return self.L.socp_ctx_has_sensitivity(self.h) == 1

    def sensitivity_work_bytes(self, B, K):
        """Bytes of the workspace sensitivity_batch_dev needs for B rows and K directions (socp_sensitivity_work_bytes)."""
        return int(self.L.socp_sensitivity_work_bytes(self.h, int(B), int(K)))

    def sensitivity_batch_dev(self, B, d_Z, dirs, d_work, work_bytes, d_dZ, d_info, d_Gp=None):
        """Device pointers (ints; d_Gp may be None), dirs a host list of (kind, index); enqueue only, no allocation, no copy, no
        synchronise (socp_sensitivity_batch_dev)."""
        kinds, index = _dirs(dirs)
        self._chk(self.L.socp_sensitivity_batch_dev(self.h, int(B), _vp(d_Z), len(kinds), kinds.ctypes.data_as(_ip), index.ctypes.data_as(_ip),
                                                    _vp(d_work), int(work_bytes), _vp(d_dZ), _vp(d_info), _vp(d_Gp)))

    def sensitivity_batch(self, Z, dirs, params=None, time=None, xnode=None, g=False):
        """The exact dz/dtheta of every row of Z for the K directions dirs = [(kind, index), ...] (as tangent_batch; a DIR_PARAM index
        must be below nparams): the solution of J dz = -dF/dtheta with the exact shooting Jacobian and the exact dF/dtheta of the
        discrete flow (include/socp_hip.h has the definition).  Returns dict(dz[B][K][n], info[B] as tangent_batch,
        g[B][K][n] = dF/dtheta or None).  params / time / xnode: per-row blocks as in residual_batch_blocks."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        kinds, index = _dirs(dirs)
        K = len(kinds)
        blocks = _block_args(B, params, time, xnode)
        dz = np.full((B, K, self.n), np.nan)
        info = np.zeros(B, dtype=np.int32)
        G = np.full((B, K, self.n), np.nan) if g else None
        self._chk(self.L.socp_sensitivity_batch_blocks(self.h, B, _d(Z), *blocks, K, kinds.ctypes.data_as(_ip), index.ctypes.data_as(_ip),
                                                       _d(dz), info.ctypes.data_as(_ip), _d(G)))
        return dict(dz=dz, info=info, g=G)

    def linsolve_batch_dev(self, B, n, K, d_A, d_Y, d_info):
        """Device pointers (ints): A[B][n*n] column-major, Y[B][K][n] overwritten by the solutions, info[B]; enqueue only
        (socp_linsolve_batch_dev)."""
        self._chk(self.L.socp_linsolve_batch_dev(self.h, int(B), int(n), int(K), _vp(d_A), _vp(d_Y), _vp(d_info)))

    # -- batched singular values
    def svd_batch_dev(self, B, n, d_A, max_sweeps, d_sigma, d_Vt, d_sweeps, d_info):
        """Device pointers (ints; d_Vt may be None): A[B][n*n] column-major (left as it was) -> sigma[B][n] descending, Vt[B][n][n],
        sweeps[B], info[B] (0: converged, 1: max_sweeps reached, 2: an entry is not finite); one launch, enqueue only
        (socp_svd_batch_dev).  Needs no problem."""
        self._chk(self.L.socp_svd_batch_dev(self.h, int(B), int(n), _vp(d_A), int(max_sweeps), _vp(d_sigma), _vp(d_Vt), _vp(d_sweeps),
                                            _vp(d_info)))

    def singular_work_bytes(self, B):
        """Bytes of the workspace singular_batch_dev needs for B rows (socp_singular_work_bytes)."""
        return int(self.L.socp_singular_work_bytes(self.h, int(B)))

    def singular_batch_dev(self, B, d_Z, epsfcn, jac, scale, max_sweeps, d_work, work_bytes, d_sigma, d_vmin, d_colnorm, d_sweeps, d_info):
        """Device pointers (ints; d_colnorm may be None); enqueue only, no allocation, no copy, no synchronise
        (socp_singular_batch_dev)."""
        self._chk(self.L.socp_singular_batch_dev(self.h, int(B), _vp(d_Z), float(epsfcn), int(jac), int(scale), int(max_sweeps), _vp(d_work),
                                                 int(work_bytes), _vp(d_sigma), _vp(d_vmin), _vp(d_colnorm), _vp(d_sweeps), _vp(d_info)))

    def singular_batch(self, Z, epsfcn=1e-15, jac=0, scale=1, max_sweeps=60, params=None, time=None, xnode=None):
        """The singular values of the shooting Jacobian at every row of Z (jac=0 forward differences, jac=1 variational), its columns
        brought to unit norm first when scale=1 (include/socp_hip.h has the definition).  Returns dict(sigma[B][n] descending,
        vmin[B][n] (the right singular vector of the smallest one), colnorm[B][n], sweeps[B], info[B] (0: converged, 1: max_sweeps
        reached, 2: a Jacobian entry is not finite)).  params / time / xnode: per-row blocks as in residual_batch_blocks."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        blocks = _block_args(B, params, time, xnode)
        sigma, vmin, colnorm = (np.full((B, self.n), np.nan) for _ in range(3))
        sweeps, info = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        self._chk(self.L.socp_singular_batch_blocks(self.h, B, _d(Z), *blocks, float(epsfcn), int(jac), int(scale), int(max_sweeps), _d(sigma),
                                                    _d(vmin), _d(colnorm), sweeps.ctypes.data_as(_ip), info.ctypes.data_as(_ip)))
        return dict(sigma=sigma, vmin=vmin, colnorm=colnorm, sweeps=sweeps, info=info)

    # -- batched branch following
    def branch_work_bytes(self, B):
        """Bytes of the workspace branch_batch_dev needs for B rows (socp_branch_work_bytes)."""
        return int(self.L.socp_branch_work_bytes(self.h, int(B)))

    def branch_batch_dev(self, B, d_Z, direction, opts, d_work, work_bytes, d_Y, d_ttheta, d_rnorm, d_count, d_nfold, d_ifold, d_status,
                         d_nreject, d_hlast, d_zgoal=None):
        """Device pointers (ints; d_zgoal may be None), direction = (kind, index), opts a BranchOptions; enqueues exactly opts.rounds
        rounds, no allocation, no copy, no synchronise (socp_branch_batch_dev)."""
        self._chk(self.L.socp_branch_batch_dev(self.h, int(B), _vp(d_Z), int(direction[0]), int(direction[1]), C.byref(opts), _vp(d_work),
                                               int(work_bytes), _vp(d_Y), _vp(d_ttheta), _vp(d_rnorm), _vp(d_count), _vp(d_nfold), _vp(d_ifold),
                                               _vp(d_status), _vp(d_nreject), _vp(d_hlast), _vp(d_zgoal)))

    def branch_batch(self, Z, direction, opts=None, params=None, time=None, xnode=None, **kw):
        """Pseudo-arclength continuation of every row of Z along direction = (kind, index) (DIR_PARAM / DIR_TIME / DIR_XNODE as
        tangent_batch): theta is that entry of the row's blocks, followed past folds (include/socp_hip.h has the definition).  opts: a
        BranchOptions, or keyword arguments of branch_options().  Returns dict(y[B][cap][n+1] (z then theta of every accepted point,
        unused slots NaN), ttheta[B][cap], rnorm[B][cap], count[B], nfold[B], ifold[B], status[B] (BRANCH_*), nreject[B], hlast[B],
        zgoal[B][n] (NaN unless BRANCH_REACHED)).  params / time / xnode: per-row blocks as in residual_batch_blocks."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        if opts is not None and kw:
            raise TypeError("branch_batch: give a BranchOptions or keyword options, not both (%s)" % ", ".join(sorted(kw)))
        opts = branch_options(**kw) if opts is None else opts
        blocks = _block_args(B, params, time, xnode)
        cap = max(int(opts.cap), 0)
        Y = np.full((B, cap, self.n + 1), np.nan)
        tth, rn = np.full((B, cap), np.nan), np.full((B, cap), np.nan)
        hlast, zgoal = np.full(B, np.nan), np.full((B, self.n), np.nan)
        count, nfold, ifold, status, nreject = (np.zeros(B, dtype=np.int32) for _ in range(5))
        self._chk(self.L.socp_branch_batch_blocks(self.h, B, _d(Z), *blocks, int(direction[0]), int(direction[1]), C.byref(opts), _d(Y), _d(tth),
                                                  _d(rn), *(a.ctypes.data_as(_ip) for a in (count, nfold, ifold, status, nreject)), _d(hlast),
                                                  _d(zgoal)))
        return dict(y=Y, ttheta=tth, rnorm=rn, count=count, nfold=nfold, ifold=ifold, status=status, nreject=nreject, hlast=hlast, zgoal=zgoal)

    # -- batched Newton polish
    def newton_work_bytes(self, B, opts):
        """Bytes of the workspace newton_batch_dev needs for B rows and opts.trials (socp_newton_work_bytes)."""
        return int(self.L.socp_newton_work_bytes(self.h, int(B), C.byref(opts)))

    def newton_batch_dev(self, B, d_Z, opts, d_work, work_bytes, d_Zout, d_Fout, d_rnorm, d_dnorm, d_iters, d_nhalf, d_status, d_rhist=None):
        """Device pointers (ints; d_Fout and d_rhist may be None), opts a NewtonOptions; enqueues exactly opts.rounds rounds on all B
        slots, no allocation, no copy, no synchronise (socp_newton_batch_dev)."""
        self._chk(self.L.socp_newton_batch_dev(self.h, int(B), _vp(d_Z), C.byref(opts), _vp(d_work), int(work_bytes), _vp(d_Zout), _vp(d_Fout),
                                               _vp(d_rnorm), _vp(d_dnorm), _vp(d_iters), _vp(d_nhalf), _vp(d_status), _vp(d_rhist)))

    def newton_batch(self, Z, opts=None, params=None, time=None, xnode=None, residual=True, history=True, **kw):
        """Damped Newton polish of every row of Z with the exact (jac=2), variational (1) or forward-difference (0) Jacobian
        (include/socp_hip.h has the definition).  opts: a NewtonOptions, or keyword arguments of newton_options().  Returns dict(z[B][n],
        f[B][n] (None unless residual), rnorm[B], dnorm[B], iters[B], nhalf[B], status[B] (NEWTON_*), rhist[B][rounds + 1] (None unless
        history; unused slots NaN)).  params / time / xnode: per-row blocks as in residual_batch_blocks."""
        Z = _f64(Z).reshape(-1, self.n)
        B = Z.shape[0]
        if opts is not None and kw:
            raise TypeError("newton_batch: give a NewtonOptions or keyword options, not both (%s)" % ", ".join(sorted(kw)))
        opts = newton_options(**kw) if opts is None else opts
        blocks = _block_args(B, params, time, xnode)
        Zout, F = np.full((B, self.n), np.nan), (np.full((B, self.n), np.nan) if residual else None)
        rn, dn = np.full(B, np.nan), np.full(B, np.nan)
        rhist = np.full((B, max(int(opts.rounds), 0) + 1), np.nan) if history else None
        iters, nhalf, status = (np.zeros(B, dtype=np.int32) for _ in range(3))
        self._chk(self.L.socp_newton_batch_blocks(self.h, B, _d(Z), *blocks, C.byref(opts), _d(Zout), _d(F), _d(rn), _d(dn),
                                                  *(a.ctypes.data_as(_ip) for a in (iters, nhalf, status)), _d(rhist)))
        return dict(z=Zout, f=F, rnorm=rn, dnorm=dn, iters=iters, nhalf=nhalf, status=status, rhist=rhist)

    # -- row grouping
    def group_batch_dev(self, B, n, ld, d_V, d_mask, atol, rtol, max_groups, d_label, d_leader, d_count, d_radius, d_summary):
        """Device pointers (ints; d_mask may be None): V[B][ld], label[B], leader / count / radius[max_groups], summary[4].  Enqueues on
        the context's stream and synchronises it once per chunk of rounds (socp_group_batch_dev)."""
        self._chk(self.L.socp_group_batch_dev(self.h, int(B), int(n), int(ld), _vp(d_V), _vp(d_mask), float(atol), float(rtol), int(max_groups),
                                              _vp(d_label), _vp(d_leader), _vp(d_count), _vp(d_radius), _vp(d_summary)))

    def group_batch(self, V, n=None, mask=None, atol=0.0, rtol=1e-6, max_groups=1024):
        """The distinct rows of the table V[B][ld], compared on their first n entries (default: all): greedy leader grouping in row
        order -- a row joins the FIRST leader l with |v_i - l_i| <= atol + rtol |l_i| for every i < n, or becomes the next leader
        (include/socp_hip.h has the definition).  mask[B]: rows with mask == 0 take no part.  Returns dict(label[B] (the group, or
        GROUP_OVERFLOW / GROUP_NOTFINITE / GROUP_MASKED), leader[G] (row indices, ascending), count[G], radius[G] (max |v_i - l_i|
        over a group), summary = [G, overflow rows, non-finite rows, masked rows]).  Needs no problem."""
        V = _f64(V)
        V = V.reshape(-1, V.shape[-1]) if V.ndim >= 2 else V.reshape(-1, 1)
        B, ld = V.shape
        n = ld if n is None else int(n)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).ravel() != 0, dtype=np.int32)
            if m.size != B:
                raise ValueError("group_batch: mask must have one entry per row")
        cap = max(int(max_groups), 1)
        label = np.empty(B, dtype=np.int32)
        leader, count, radius = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32), np.empty(cap)
        summary = np.zeros(4, dtype=np.int32)
        ip_ = lambda a: a.ctypes.data_as(_ip) if a is not None else None      # noqa: E731
        self._chk(self.L.socp_group_batch(self.h, B, n, ld, _d(V), ip_(m), float(atol), float(rtol), int(max_groups), ip_(label), ip_(leader),
                                          ip_(count), _d(radius), ip_(summary)))
        G = int(summary[0])
        return dict(label=label, leader=leader[:G].copy(), count=count[:G].copy(), radius=radius[:G].copy(), summary=summary)

    def chains_solve(self, Z0, kind=CHAIN_PLAIN, param_index=0, step=1.0, step_min=1e-12, goal=None, params=None,
                     time_prev=None, x_prev=None, time_goal=None, x_goal=None, xtol=1e-8, maxfev=10000, epsfcn=1e-15,
                     factor=1.0, dedup=True, speculate=-1, max_rounds=0, analytic_jac=False, solver=SOLVER_AUTO):
        """Lock-step continuation chains (socp_chains_solve).  Returns a dict of per-chain arrays + 'stats'."""
        Z0 = _f64(Z0).reshape(-1, self.n)
        P = Z0.shape[0]
        opt = ChainOptions(int(kind), int(param_index), float(step), float(step_min), float(xtol), int(maxfev), float(epsfcn),
                           float(factor), int(bool(dedup)), int(speculate), int(max_rounds), int(bool(analytic_jac)), int(solver))
        keep = []

        def arr(a, width=None):
            if a is None:
                return None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (P,) if width is None else (P, width)))
            keep.append(a)
            return _d(a)
        nodes = self.L.socp_problem_num_nodes(self.h)
        Z = np.empty_like(Z0)
        info = np.zeros(P, dtype=np.int32)
        nfev_last = np.zeros(P, dtype=np.int32)
        nfev_total = np.zeros(P, dtype=np.int32)
        solves = np.zeros(P, dtype=np.int32)
        njev = np.zeros(P, dtype=np.int32)
        b = np.zeros(P)
        pf = np.zeros(P)
        fn = np.zeros(P)
        st = ChainStats()
        ip = lambda a: a.ctypes.data_as(_ip)  # noqa: E731
        self._chk(self.L.socp_chains_solve_ex(self.h, P, C.byref(opt), _d(Z0), arr(params, len(self.get_params())), arr(goal),
                                              arr(time_prev, nodes), arr(x_prev, nodes * self.s), arr(time_goal, nodes),
                                              arr(x_goal, nodes * self.s), _d(Z), ip(info), ip(nfev_last), ip(nfev_total), ip(njev),
                                              ip(solves), _d(b), _d(pf), _d(fn), C.byref(st)))
        return dict(z=Z, info=info, nfev=nfev_last, nfev_total=nfev_total, njev=njev, solves=solves, b_reached=b, param_final=pf, fnorm=fn,
                    stats={k: getattr(st, k) for k, _ in ChainStats._fields_})

    def fd_jacobian_dev(self, d_z, d_fvec, epsfcn, d_fjac, dedup=False):
        self._chk(self.L.socp_fd_jacobian_dev(self.h, _vp(d_z), _vp(d_fvec), float(epsfcn), _vp(d_fjac),
                                              int(bool(dedup))))


# ---------------------------------------------------------------------------------------------
# MINPACK entry points (host code inside the same library)
# ---------------------------------------------------------------------------------------------

def _workspace(n):
    return dict(fvec=np.zeros(n), diag=np.ones(n), fjac=np.zeros((n, n)), r=np.zeros(n * (n + 1) // 2),
                qtf=np.zeros(n), wa1=np.zeros(n), wa2=np.zeros(n), wa3=np.zeros(n), wa4=np.zeros(n))


def hybrd(func, x0, xtol=1e-8, maxfev=10000, ml=None, mu=None, epsfcn=1e-15, mode=1, factor=1.0,
          diag=None, fdjac=None):
    """Drive the library's hybrd (or socp_hybrd_batched when `fdjac` is given) with Python callables.

    func(x) -> F(x) (or None to abort);  fdjac(x, fvec, epsfcn) -> J[row, col].
    Returns dict(x, fvec, info, nfev, fjac (Q, column-major as MINPACK leaves it), r, qtf, diag).
    """
    L = lib()
    x = _f64(np.array(x0, dtype=np.float64))
    n = len(x)
    ws = _workspace(n)
    if diag is not None:
        ws["diag"][:] = diag
    ml = n - 1 if ml is None else ml
    mu = n - 1 if mu is None else mu
    nfev = C.c_int(0)

    def _fcn(p, nn, xp, fp, iflag):
        out = func(np.ctypeslib.as_array(xp, shape=(nn,)).copy())
        if out is None:
            return -1
        np.ctypeslib.as_array(fp, shape=(nn,))[:] = out
        return 0

    def _jac(p, nn, xp, fp, eps, jp, ld):
        J = fdjac(np.ctypeslib.as_array(xp, shape=(nn,)).copy(), np.ctypeslib.as_array(fp, shape=(nn,)).copy(), eps)
        if J is None:
            return -1
        np.ctypeslib.as_array(jp, shape=(nn, ld))[:, :nn] = np.asarray(J).T   # column-major
        return 0

    cb = FCN(_fcn)
    args = [None, n, _d(x), _d(ws["fvec"]), xtol, maxfev, ml, mu, epsfcn, _d(ws["diag"]), mode, factor, 0,
            C.byref(nfev), _d(ws["fjac"]), n, _d(ws["r"]), len(ws["r"]), _d(ws["qtf"]),
            _d(ws["wa1"]), _d(ws["wa2"]), _d(ws["wa3"]), _d(ws["wa4"])]
    if fdjac is None:
        info = L.hybrd(cb, *args)
    else:
        info = L.socp_hybrd_batched(cb, FDJAC(_jac), *args)
    return dict(x=x, fvec=ws["fvec"], info=info, nfev=nfev.value, fjac=ws["fjac"], r=ws["r"], qtf=ws["qtf"],
                diag=ws["diag"])


def hybrj(func, jac, x0, xtol=1e-8, maxfev=10000, mode=1, factor=1.0, diag=None):
    """Drive the library's hybrj.  func(x) -> F, jac(x) -> J[row, col]."""
    L = lib()
    x = _f64(np.array(x0, dtype=np.float64))
    n = len(x)
    ws = _workspace(n)
    if diag is not None:
        ws["diag"][:] = diag
    nfev, njev = C.c_int(0), C.c_int(0)

    def _fcn(p, nn, xp, fp, jp, ld, iflag):
        xx = np.ctypeslib.as_array(xp, shape=(nn,)).copy()
        if iflag == 1:
            out = func(xx)
            if out is None:
                return -1
            np.ctypeslib.as_array(fp, shape=(nn,))[:] = out
        else:
            J = jac(xx)
            if J is None:
                return -1
            np.ctypeslib.as_array(jp, shape=(nn, ld))[:, :nn] = np.asarray(J).T
        return 0

    cb = FCNDER(_fcn)
    info = L.hybrj(cb, None, n, _d(x), _d(ws["fvec"]), _d(ws["fjac"]), n, xtol, maxfev, _d(ws["diag"]), mode,
                   factor, 0, C.byref(nfev), C.byref(njev), _d(ws["r"]), len(ws["r"]), _d(ws["qtf"]),
                   _d(ws["wa1"]), _d(ws["wa2"]), _d(ws["wa3"]), _d(ws["wa4"]))
    return dict(x=x, fvec=ws["fvec"], info=info, nfev=nfev.value, njev=njev.value, fjac=ws["fjac"], r=ws["r"],
                qtf=ws["qtf"], diag=ws["diag"])


class HybrSolver:
    """Resumable solver object (socp_hybr_*)."""

    def __init__(self, n, xtol=1e-8, maxfev=10000, epsfcn=1e-15, mode=1, factor=1.0, analytic_jac=False):
        self.L = lib()
        self.n = n
        self.h = _vp(self.L.socp_hybr_create(n, xtol, maxfev, epsfcn, mode, factor, int(analytic_jac)))
        self._xe = _dp()
        self._out = _dp()

    def __del__(self):
        try:
            self.L.socp_hybr_destroy(self.h)
        except Exception:
            pass

    def start(self, x0, diag=None):
        x0 = _f64(x0)
        self.L.socp_hybr_start(self.h, _d(x0), _d(_f64(diag)) if diag is not None else None)

    def advance(self, flag=0):
        """Returns (request, x_eval view, out view)."""
        req = self.L.socp_hybr_advance(self.h, int(flag), C.byref(self._xe), C.byref(self._out))
        if req == REQ_DONE:
            return req, None, None
        xe = np.ctypeslib.as_array(self._xe, shape=(self.n,))
        out = np.ctypeslib.as_array(self._out, shape=(self.n,) if req == REQ_FVEC else (self.n * self.n,))
        return req, xe, out

    @property
    def info(self):
        return self.L.socp_hybr_info(self.h)

    @property
    def nfev(self):
        return self.L.socp_hybr_nfev(self.h)

    @property
    def njev(self):
        return self.L.socp_hybr_njev(self.h)

    @property
    def trust_region(self):
        """(delta, |diag x|, |F|) of the current iterate."""
        d, xn, fn = C.c_double(0), C.c_double(0), C.c_double(0)
        self.L.socp_hybr_trust_region(self.h, C.byref(d), C.byref(xn), C.byref(fn))
        return d.value, xn.value, fn.value

    @property
    def x(self):
        return np.ctypeslib.as_array(self.L.socp_hybr_x(self.h), shape=(self.n,)).copy()

    @property
    def fvec(self):
        return np.ctypeslib.as_array(self.L.socp_hybr_fvec(self.h), shape=(self.n,)).copy()
