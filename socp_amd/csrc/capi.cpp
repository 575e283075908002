// capi.cpp -- implementation of include/socp_hip.h (context, device tables, launch dispatch).
// Host logic only: every number the caller receives was computed by a gfx950 kernel.
#include "../../include/socp_hip.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <dlfcn.h>

#include <map>
#include <mutex>

#include "../../include/socp_plugin.h"
#include "launch.hpp"

using namespace socp;

static_assert(socp::kMaxObstacles == SOCP_MAX_OBSTACLES && socp::kMapStride == SOCP_MAP_STRIDE && SOCP_VTOL_NPARAMS <= socp::kMaxParams, "socp_hip.h and dev_common.hpp disagree");

namespace {

// socp_last_error(NULL) reports the calling thread's last creation failure: concurrent socp_ctx_create calls may fail at once
thread_local std::string g_create_error;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        size_t want = bytes < 4096 ? 4096 : bytes + bytes / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

}  // namespace

struct socp_ctx {
    int model_id = 0;
    // vtolUAV: its fields / exact_jacobian entries count only once the context asked for them (socp_ctx_set_exact_hooks); before
    // that the context answers as it did when the model had neither entry
    bool exact_hooks = false;
    const ModelLaunchers *vt = nullptr;   // the model's launch table (in-tree model or out-of-tree plugin), reference operation order
    const ModelLaunchers *vt_fast = nullptr;   // the same model's throughput flavour, when it has one
    int device = 0;
    int dim = 0, S = 0, nu = 3;
    int nparams = 0;
    int variant = SOCP_VARIANT_AUTO;
    ModelParams P{};
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    // shooting problem (host copy + device tables)
    bool has_problem = false;
    int M = 0, n = 0;
    std::vector<int> mode_t, mode_x, node_kind, lo, hi, ft_row;
    std::vector<double> time, xnode;
    int sw_node0 = -1, sw_node1 = -1;
    DevBuf d_tables;                 // one allocation holding every table
    ProblemDev pb{};
    DevBuf d_pairs_full, d_pairs_dedup;
    int T_full = 0, T_dedup = 0;

    // obstacle table of the vtolUAV model (socp_ctx_set_map): host copy + the device buffer P.map points into
    std::vector<double> map_table;
    DevBuf d_map;

    // grow-only staging for the host-pointer entry points
    DevBuf s_t0, s_tf, s_sw, s_in, s_out, s_aux, s_var;
    DevBuf s_gain;                    // workspace arena of socp_gain_batch_dev and socp_gain_free_batch_dev: the blocks (unless the caller takes them) and the elimination's matrices

    hipStream_t aux_stream = nullptr; // socp_ctx_aux_stream: created on first use
    bool blocks_smooth_hint = false;  // socp_problem_blocks_all_smooth: every per-problem parameter block has mu2 > 0
    long long n_traj = 0, n_launch = 0;
    std::string err;
};

namespace {

// Registered plugin models.  Contexts keep a pointer to their entry (map nodes do not move; an id registered twice keeps its
// node); registration and look-up may come from different threads.
std::map<int, ModelLaunchers> &plugins()
{
    static std::map<int, ModelLaunchers> table;
    return table;
}
std::mutex &plugins_lock()
{
    static std::mutex m;
    return m;
}

int fail(socp_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

int hip_fail(socp_ctx *c, hipError_t e, const char *what)
{
    return fail(c, SOCP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(c, call)                                                 \
    do {                                                                 \
        hipError_t e__ = (call);                                         \
        if (e__ != hipSuccess) return hip_fail((c), e__, #call);         \
    } while (0)

// launch table for the current variant.  AUTO keeps the reference operation order: it is the variant every parity claim is made
// on.  (A table carries its own adaptive-integrator instantiations, so the throughput table serves both integrators.)
const ModelLaunchers *table_of(const socp_ctx *c)
{
    return (c->variant == SOCP_VARIANT_LANE_FAST && c->vt_fast) ? c->vt_fast : c->vt;
}

hipError_t run_traj(socp_ctx *c, int B, const double *t0, const double *tf, const double *sw,
                    const double *X0, double *Xf)
{
    c->n_traj += B; c->n_launch += 1;
    return table_of(c)->traj(c->stream, c->P, B, t0, tf, sw, X0, Xf);
}

hipError_t run_residual(socp_ctx *c, int B, const double *Z, double *F)
{
    c->n_traj += (long long)B * c->M; c->n_launch += 1;
    return table_of(c)->residual(c->stream, c->P, c->pb, B, Z, F);
}

hipError_t run_fdjac(socp_ctx *c, int np, int T, const int2 *pairs, const double *z, const double *fvec,
                     double eps, double *fjac)
{
    c->n_traj += (long long)np * T; c->n_launch += 1;
    return table_of(c)->fdjac(c->stream, c->P, c->pb, np, T, pairs, z, fvec, eps, fjac);
}

hipError_t run_fdrows(socp_ctx *c, int np, const double *z, double eps, double *rows)
{
    c->n_traj += (long long)np * (c->n + 1) * c->M; c->n_launch += 1;
    return table_of(c)->fdrows(c->stream, c->P, c->pb, np, z, eps, rows);
}

// variational equations on the device: a model whose table carries them (in-tree: the double integrator); always reference order
bool has_var(const socp_ctx *c) { return c->vt->var_traj && c->vt->var_jacobian && c->vt->var_eval; }

double fd_eps(double epsfcn) { return std::sqrt(epsfcn > DBL_EPSILON ? epsfcn : DBL_EPSILON); }

// the variational Jacobian of np problems (socp_var_jacobian_multi_dev, socp_tangent_batch_dev with jac = 1): what it integrates in
// -- the augmented start and end states of the np M trajectories, their start and end times -- and its launch
size_t var_work_doubles(const socp_ctx *c, size_t np)
{
    const size_t segs = np * c->M, L = (size_t)(c->S + 1) * c->S;
    return 2 * segs * L + 2 * segs;
}

hipError_t run_var_jacobian(socp_ctx *c, int np, const double *d_Z, double *work, double *d_Fjac)
{
    const size_t segs = (size_t)np * c->M, L = (size_t)(c->S + 1) * c->S;
    double *Xaug = work, *Xtf = Xaug + segs * L, *t0 = Xtf + segs * L, *tf = t0 + segs;
    c->n_traj += (long long)segs; c->n_launch += 3;
    return c->vt->var_jacobian(c->stream, c->P, c->pb, np, d_Z, Xaug, Xtf, t0, tf, d_Fjac);
}

// ---- staging of the host-pointer entry points: copies travel on the context's stream, the entry point synchronises once at its end
template <class T> hipError_t copy_up(socp_ctx *c, T *dev, const T *host, size_t count)
{
    return hipMemcpyAsync(dev, host, sizeof(T) * count, hipMemcpyHostToDevice, c->stream);
}

template <class T> hipError_t copy_down(socp_ctx *c, T *host, const T *dev, size_t count)
{
    return hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream);
}

// reserve `buf` for `room` elements of T and copy the first `count` of them up; dev: the buffer
template <class T> hipError_t stage_up(socp_ctx *c, DevBuf &buf, const T *host, size_t count, T *&dev, size_t room = 0)
{
    const hipError_t e = buf.reserve(sizeof(T) * (room > count ? room : count));
    if (e != hipSuccess) return e;
    dev = buf.as<T>();
    return copy_up(c, dev, host, count);
}

// ---- refusals the batched entry points over the shooting problem share; every refusal comes before anything is counted, reserved
// or enqueued: an error leaves the context as it was.  args_head first, args_tail behind the entry point's own checks.
int args_head(socp_ctx *c, const std::string &who, bool sizes_ok, const char *sizes)
{
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, who + ": no problem set");
    if (!sizes_ok) return fail(c, SOCP_ERR_ARG, who + ": " + sizes);
    return SOCP_OK;
}

// entry: what the launch table must hold; fixed_only: null, or what the entry does along the fixed-step integrator only
int args_tail(socp_ctx *c, const std::string &who, bool has_entry, const char *entry, const char *fixed_only)
{
    if (!has_entry) return fail(c, SOCP_ERR_UNSUPPORTED, who + ": this model's launch table has no " + entry);
    if (fixed_only && c->P.integrator == SOCP_INT_DOPRI5)
        return fail(c, SOCP_ERR_UNSUPPORTED, who + ": " + fixed_only + " the fixed-step integrator only (this context is set to SOCP_INT_DOPRI5)");
    return SOCP_OK;
}

// ---- the blocks path: what the six _blocks entry points do with the caller's per-row blocks ("Per-row blocks")
// before anything is sized or copied from the blocks: a wrong stride would read past the caller's array
int blocks_stride(socp_ctx *c, const char *what, const double *params, int stride)
{
    if (params && stride != c->nparams + 2)
        return fail(c, SOCP_ERR_ARG, std::string(what) + " must be nparams + 2 (parameters, then two switching times)");
    return SOCP_OK;
}

// the blocks staged through s_aux and put in force
int stage_blocks(socp_ctx *c, int B, const double *params, int pstride, const double *time, const double *xnode)
{
    const size_t nodes = (size_t)c->M + 1;
    const size_t nP = params ? (size_t)B * pstride : 0, nT = time ? B * nodes : 0, nX = xnode ? B * nodes * c->S : 0;
    HIP_TRY(c, c->s_aux.reserve(sizeof(double) * (nP + nT + nX) + 64));
    double *dP = c->s_aux.as<double>(), *dT = dP + nP, *dX = dT + nT;
    if (nP) HIP_TRY(c, copy_up(c, dP, params, nP));
    if (nT) HIP_TRY(c, copy_up(c, dT, time, nT));
    if (nX) HIP_TRY(c, copy_up(c, dX, xnode, nX));
    return socp_problem_set_blocks_dev(c, params ? dP : nullptr, pstride, time ? dT : nullptr, xnode ? dX : nullptr);
}

// the context's own blocks, saved here and back in force when the scope is left, by whatever return
struct BlocksGuard {
    socp_ctx *c;
    const ProblemDev saved;
    explicit BlocksGuard(socp_ctx *ctx) : c(ctx), saved(ctx->pb) {}
    ~BlocksGuard() { c->pb = saved; }
    BlocksGuard(const BlocksGuard &) = delete;
    BlocksGuard &operator=(const BlocksGuard &) = delete;
};

// `call` (the entry point's other form) with the caller's blocks in force; for a batch that is not empty and already checked
template <class Call>
int with_blocks(socp_ctx *c, int B, const double *params, int pstride, const double *time, const double *xnode, Call call)
{
    HIP_TRY(c, hipSetDevice(c->device));
    BlocksGuard guard(c);
    const int rc = stage_blocks(c, B, params, pstride, time, xnode);
    return rc == SOCP_OK ? call() : rc;
}

}  // namespace

extern "C" {

const char *socp_last_error(const socp_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int socp_ctx_create(socp_ctx **out, int model_id, int device)
{
    if (!out) return fail(nullptr, SOCP_ERR_ARG, "socp_ctx_create: null output pointer");
    *out = nullptr;
    const ModelLaunchers *vt = nullptr;
    if (model_id >= SOCP_PLUGIN_ID_MIN) {
        std::lock_guard<std::mutex> guard(plugins_lock());
        auto it = plugins().find(model_id);
        if (it != plugins().end()) vt = &it->second;
    }
    // in-tree models: kernels_interceptor.hip, kernels_vtol.hip, kernels_exact.hip
    if (model_id == SOCP_MODEL_INTERCEPTOR) vt = interceptor_launchers();
    else if (model_id == SOCP_MODEL_VTOLUAV) vt = vtol_launchers();
    else if (!vt) vt = builtin_launchers(model_id);                         // null for an id that is not theirs
    if (!vt)
        return fail(nullptr, SOCP_ERR_UNSUPPORTED, "socp_ctx_create: unknown model id (no device dynamics; plugins: socp_plugin_load)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, SOCP_ERR_NO_DEVICE,
                    "socp_ctx_create: no HIP device visible -- this library has no CPU path");
    if (device < 0) { e = hipGetDevice(&device); if (e != hipSuccess) return hip_fail(nullptr, e, "hipGetDevice"); }
    if (device >= ndev) return fail(nullptr, SOCP_ERR_ARG, "socp_ctx_create: device index out of range");
    e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipSetDevice");

    socp_ctx *c = new socp_ctx;
    c->model_id = model_id;
    c->vt = vt;
    if (model_id == SOCP_MODEL_INTERCEPTOR) c->vt_fast = interceptor_launchers_fast();
    else if (model_id == SOCP_MODEL_VTOLUAV) c->vt_fast = vtol_launchers_fast();
    else c->vt_fast = builtin_launchers_fast(model_id);
    c->device = device;
    c->dim = vt->dim; c->nparams = vt->nparams; c->nu = vt->control_dim;
    std::memcpy(c->P.p, vt->default_params, sizeof(double) * kMaxParams);
    c->P.sw0 = c->P.sw1 = 0.0; c->P.step_nbr = vt->default_step_nbr;
    // the table has no slot for the auxiliary scalars.  Interceptor: they are (stageMode, currentChart), and a fresh object has
    // (0, 1) (interceptor.cpp:62-64); Goddard: the switching times of goddard.cpp:23-40
    if (model_id == SOCP_MODEL_INTERCEPTOR) c->P.sw1 = 1.0;
    if (model_id == SOCP_MODEL_GODDARD) { c->P.sw0 = 0.0227; c->P.sw1 = 0.08; }
    c->S = 2 * c->dim;
    // default arithmetic flavour can be chosen from the environment (host programs that do not call
    // socp_ctx_set_variant): SOCP_VARIANT=exact|fast
    if (const char *v = std::getenv("SOCP_VARIANT")) {
        if (std::strcmp(v, "fast") == 0) c->variant = SOCP_VARIANT_LANE_FAST;
        else if (std::strcmp(v, "exact") == 0) c->variant = SOCP_VARIANT_LANE_EXACT;
    }
    e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return hip_fail(nullptr, e, "hipStreamCreate"); }
    c->stream = c->own_stream;
    *out = c;
    return SOCP_OK;
}

int socp_ctx_clone(const socp_ctx *proto, int device, socp_ctx **out)
{
    if (!proto || !out) return fail(nullptr, SOCP_ERR_ARG, "socp_ctx_clone: null argument");
    *out = nullptr;
    socp_ctx *c = nullptr;
    int rc = socp_ctx_create(&c, proto->model_id, device);
    if (rc != SOCP_OK) return rc;
    c->P = proto->P;                                   // parameters, switching times, step number, integrator, tolerance
    c->P.map = nullptr; c->P.n_map = 0;                // the table pointer is the prototype's: the clone gets its own copy
    c->variant = proto->variant;
    c->exact_hooks = proto->exact_hooks;
    if (!proto->map_table.empty())
        rc = socp_ctx_set_map(c, (int)(proto->map_table.size() / kMapStride), proto->map_table.data());
    if (rc != SOCP_OK) { g_create_error = c->err; socp_ctx_destroy(c); return rc; }
    if (proto->has_problem)
        rc = socp_problem_set(c, proto->M, proto->mode_t.data(), proto->mode_x.data(), proto->time.data(), proto->xnode.data());
    if (rc != SOCP_OK) { g_create_error = c->err; socp_ctx_destroy(c); return rc; }
    *out = c;
    return SOCP_OK;
}

int socp_ctx_destroy(socp_ctx *c)
{
    if (!c) return SOCP_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->d_tables.release(); c->d_pairs_full.release(); c->d_pairs_dedup.release(); c->d_map.release();
    c->s_t0.release(); c->s_tf.release(); c->s_sw.release(); c->s_in.release(); c->s_out.release(); c->s_aux.release(); c->s_var.release(); c->s_gain.release();
    if (c->aux_stream) { (void)hipStreamSynchronize(c->aux_stream); (void)hipStreamDestroy(c->aux_stream); }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return SOCP_OK;
}

int socp_ctx_set_params(socp_ctx *c, const double *params, int nparams)
{
    if (!c || !params) return fail(c, SOCP_ERR_ARG, "set_params: null argument");
    if (nparams != c->nparams) return fail(c, SOCP_ERR_ARG, "set_params: wrong parameter count for this model");
    std::memcpy(c->P.p, params, sizeof(double) * nparams);
    return SOCP_OK;
}

int socp_ctx_get_params(const socp_ctx *c, double *params, int nparams)
{
    if (!c || !params || nparams != c->nparams) return SOCP_ERR_ARG;
    std::memcpy(params, c->P.p, sizeof(double) * nparams);
    return SOCP_OK;
}

int socp_ctx_num_params(const socp_ctx *c) { return c ? c->nparams : SOCP_ERR_ARG; }

int socp_ctx_set_map(socp_ctx *c, int n_obs, const double *table)
{
    if (!c) return SOCP_ERR_ARG;
    if (c->model_id != SOCP_MODEL_VTOLUAV) return fail(c, SOCP_ERR_UNSUPPORTED, "set_map: this model reads no map");
    if (n_obs < 0 || (n_obs > 0 && !table)) return fail(c, SOCP_ERR_ARG, "set_map: null table / negative count");
    if (n_obs > kMaxObstacles)
        return fail(c, SOCP_ERR_ARG, "set_map: too many obstacles (" + std::to_string(n_obs) + " > SOCP_MAX_OBSTACLES = " + std::to_string(kMaxObstacles) + ")");
    const size_t count = (size_t)n_obs * kMapStride;
    if (count == c->map_table.size() && (count == 0 || std::memcmp(c->map_table.data(), table, sizeof(double) * count) == 0)) return SOCP_OK;
    if (n_obs > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        // one buffer of the full capacity, overwritten in place: in order behind everything on the context's stream; what an engine
        // may still have in flight on the context's second stream is waited for first
        if (c->aux_stream) HIP_TRY(c, hipStreamSynchronize(c->aux_stream));
        HIP_TRY(c, c->d_map.reserve(sizeof(double) * kMaxObstacles * kMapStride));
        HIP_TRY(c, hipMemcpyAsync(c->d_map.p, table, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->map_table.assign(table, table + count);
    c->P.map = n_obs > 0 ? c->d_map.as<double>() : nullptr;
    c->P.n_map = n_obs;
    return SOCP_OK;
}

int socp_ctx_get_map(const socp_ctx *c, int *n_obs, double *table, int cap_obs)
{
    if (!c || !n_obs) return SOCP_ERR_ARG;
    *n_obs = c->P.n_map;
    if (!table) return SOCP_OK;
    if (cap_obs < c->P.n_map) return SOCP_ERR_ARG;
    if (c->P.n_map > 0) {
        // read back what the kernels read, not the host copy
        if (hipSetDevice(c->device) != hipSuccess ||
            hipMemcpy(table, c->P.map, sizeof(double) * c->P.n_map * kMapStride, hipMemcpyDeviceToHost) != hipSuccess)
            return SOCP_ERR_HIP;
    }
    return SOCP_OK;
}

int socp_ctx_set_step_number(socp_ctx *c, int step_nbr)
{
    if (!c) return SOCP_ERR_ARG;
    if (step_nbr < 1) return fail(c, SOCP_ERR_ARG, "set_step_number: step number must be >= 1");
    c->P.step_nbr = step_nbr;
    return SOCP_OK;
}

int socp_ctx_set_integrator(socp_ctx *c, int kind, double tol)
{
    if (!c) return SOCP_ERR_ARG;
    if (kind != SOCP_INT_RK4 && kind != SOCP_INT_DOPRI5) return fail(c, SOCP_ERR_ARG, "set_integrator: unknown integrator");
    if (kind == SOCP_INT_DOPRI5 && !(tol > 0)) return fail(c, SOCP_ERR_ARG, "set_integrator: tolerance must be positive");
    c->P.integrator = kind;
    c->P.tol = tol;
    return SOCP_OK;
}

int socp_ctx_get_integrator(const socp_ctx *c, int *step_nbr, int *kind, double *tol)
{
    if (!c) return SOCP_ERR_ARG;
    if (step_nbr) *step_nbr = c->P.step_nbr;
    if (kind) *kind = c->P.integrator;
    if (tol) *tol = c->P.tol;
    return SOCP_OK;
}

int socp_ctx_set_switching_times(socp_ctx *c, const double *sw, int nsw)
{
    if (!c || (nsw > 0 && !sw)) return fail(c, SOCP_ERR_ARG, "set_switching_times: null argument");
    // the control law reads entries [0] and [1] only (goddard.cpp:148-151); a missing entry is an
    // out-of-bounds read in the reference -- here it is NaN, so every comparison is false.
    c->P.sw0 = nsw > 0 ? sw[0] : NAN;
    c->P.sw1 = nsw > 1 ? sw[1] : NAN;
    return SOCP_OK;
}

int socp_ctx_get_switching_times(const socp_ctx *c, double *sw2)
{
    if (!c || !sw2) return SOCP_ERR_ARG;
    sw2[0] = c->P.sw0; sw2[1] = c->P.sw1;
    return SOCP_OK;
}

int socp_ctx_set_variant(socp_ctx *c, int variant)
{
    if (!c) return SOCP_ERR_ARG;
    if (variant < SOCP_VARIANT_AUTO || variant > SOCP_VARIANT_LANE_FAST) return fail(c, SOCP_ERR_ARG, "set_variant: unknown variant");
    c->variant = variant;
    return SOCP_OK;
}

int socp_ctx_set_exact_hooks(socp_ctx *c, int on)
{
    if (!c) return SOCP_ERR_ARG;
    if (c->model_id != SOCP_MODEL_VTOLUAV)
        return fail(c, SOCP_ERR_UNSUPPORTED, "set_exact_hooks: only vtolUAV's exact entries are switched per context");
    c->exact_hooks = on != 0;
    return SOCP_OK;
}

int socp_ctx_set_stream(socp_ctx *c, void *hip_stream, int use_own)
{
    if (!c) return SOCP_ERR_ARG;
    // a null hipStream_t is a real stream (the device's default stream), so "own" is explicit
    c->stream = use_own ? c->own_stream : static_cast<hipStream_t>(hip_stream);
    return SOCP_OK;
}

int socp_ctx_get_stream(const socp_ctx *c, void **hip_stream)
{
    if (!c || !hip_stream) return SOCP_ERR_ARG;
    *hip_stream = static_cast<void *>(c->stream);
    return SOCP_OK;
}

int socp_ctx_aux_stream(socp_ctx *c, void **hip_stream)
{
    if (!c || !hip_stream) return SOCP_ERR_ARG;
    if (!c->aux_stream) {
        HIP_TRY(c, hipSetDevice(c->device));
        // Streams of one priority share a few hardware queues, and two streams on one queue run their kernels one after the other
        // (measured: the residual and Jacobian launches of a round took 0.90 s of launches instead of 0.64 s).  Streams of
        // another priority come from their own queue pool.
        int least = 0, greatest = 0;
        hipStream_t st = nullptr;
        if (!(hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least &&
              hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest) == hipSuccess)) {
            (void)hipGetLastError();
            HIP_TRY(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        }
        c->aux_stream = st;
    }
    *hip_stream = static_cast<void *>(c->aux_stream);
    return SOCP_OK;
}

int socp_ctx_warm_up(socp_ctx *c)
{
    if (!c) return SOCP_ERR_ARG;
    void *aux = nullptr;
    const int rc = socp_ctx_aux_stream(c, &aux);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = 256 * 1024;
    void *h = nullptr, *d = nullptr;
    HIP_TRY(c, hipHostMalloc(&h, bytes, hipHostMallocDefault));
    hipError_t e = hipMalloc(&d, bytes);
    if (e == hipSuccess) {
        std::memset(h, 0, bytes);
        e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d);
    }
    (void)hipHostFree(h);
    if (e != hipSuccess) return hip_fail(c, e, "socp_ctx_warm_up");
    return SOCP_OK;
}

int socp_ctx_synchronize(socp_ctx *c)
{
    if (!c) return SOCP_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_ctx_dims(const socp_ctx *c, int *dim, int *state_len, int *state_len_jac)
{
    if (!c) return SOCP_ERR_ARG;
    if (dim) *dim = c->dim;
    if (state_len) *state_len = c->S;
    if (state_len_jac) *state_len_jac = (c->S + 1) * c->S;
    return SOCP_OK;
}

int socp_ctx_control_dim(const socp_ctx *c) { return c ? c->nu : SOCP_ERR_ARG; }
int socp_ctx_device(const socp_ctx *c) { return c ? c->device : SOCP_ERR_ARG; }
int socp_ctx_get_variant(const socp_ctx *c) { return c ? c->variant : SOCP_ERR_ARG; }
int socp_ctx_model_id(const socp_ctx *c) { return c ? c->model_id : SOCP_ERR_ARG; }
int socp_ctx_has_variational(const socp_ctx *c) { return c ? (has_var(c) ? 1 : 0) : SOCP_ERR_ARG; }

int socp_ctx_counters(const socp_ctx *c, long long *trajectories, long long *launches)
{
    if (!c) return SOCP_ERR_ARG;
    if (trajectories) *trajectories = c->n_traj;
    if (launches) *launches = c->n_launch;
    return SOCP_OK;
}

// batchsolve.cpp: what a clone of `c` integrated on its behalf (chain groups) counts as c's
void socp_ctx_add_counters(socp_ctx *c, long long trajectories, long long launches)
{
    if (c) { c->n_traj += trajectories; c->n_launch += launches; }
}

/* ---- trajectories ------------------------------------------------------------------------ */

int socp_integrate_batch_dev(socp_ctx *c, int B, const double *d_t0, const double *d_tf,
                             const double *d_sw, const double *d_X0, double *d_Xf, int is_jac)
{
    if (!c) return SOCP_ERR_ARG;
    if (B < 0 || (B > 0 && (!d_t0 || !d_tf || !d_X0 || !d_Xf))) return fail(c, SOCP_ERR_ARG, "integrate_batch: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (is_jac) {
        // variational state: one wavefront per trajectory (doubleIntegrator; goddard has modelOrder 0 only)
        if (!has_var(c))
            return fail(c, SOCP_ERR_UNSUPPORTED, "integrate_batch: this model has no variational equations (modelOrder 0)");
        if (d_Xf == d_X0) return fail(c, SOCP_ERR_ARG, "integrate_batch: is_jac=1 needs distinct input and output");
        c->n_traj += B; c->n_launch += 1;
        HIP_TRY(c, c->vt->var_traj(c->stream, c->P, B, d_t0, d_tf, d_X0, d_Xf));
        return SOCP_OK;
    }
    HIP_TRY(c, run_traj(c, B, d_t0, d_tf, d_sw, d_X0, d_Xf));
    return SOCP_OK;
}

int socp_integrate_batch(socp_ctx *c, int B, const double *t0, const double *tf, const double *sw,
                         const double *X0, double *Xf, int is_jac)
{
    if (!c) return SOCP_ERR_ARG;
    if (B < 0 || (B > 0 && (!t0 || !tf || !X0 || !Xf))) return fail(c, SOCP_ERR_ARG, "integrate_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nX = (is_jac ? (size_t)(c->S + 1) * c->S : (size_t)c->S) * B;
    double *d_t0, *d_tf, *d_X0, *d_sw = nullptr;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * nX));
    HIP_TRY(c, stage_up(c, c->s_t0, t0, B, d_t0));
    HIP_TRY(c, stage_up(c, c->s_tf, tf, B, d_tf));
    HIP_TRY(c, stage_up(c, c->s_in, X0, nX, d_X0));
    if (sw) HIP_TRY(c, stage_up(c, c->s_sw, sw, (size_t)2 * B, d_sw));
    int rc = socp_integrate_batch_dev(c, B, d_t0, d_tf, d_sw, d_X0, c->s_out.as<double>(), is_jac);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, Xf, c->s_out.as<double>(), nX));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_integrate_dense(socp_ctx *c, double t0, double tf, const double *sw, const double *X0,
                         double *dense, double *times, int cap, int *rows)
{
    return socp_integrate_dense_aux(c, t0, tf, sw, X0, dense, times, nullptr, cap, rows);
}

int socp_integrate_dense_aux(socp_ctx *c, double t0, double tf, const double *sw, const double *X0,
                             double *dense, double *times, double *aux, int cap, int *rows)
{
    if (!c) return SOCP_ERR_ARG;
    if (!X0 || !dense || !times || !rows || cap < 1) return fail(c, SOCP_ERR_ARG, "integrate_dense: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t S = c->S;
    HIP_TRY(c, c->s_in.reserve(sizeof(double) * S));
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * S * cap));
    HIP_TRY(c, c->s_t0.reserve(sizeof(double) * cap));
    HIP_TRY(c, c->s_aux.reserve(sizeof(int) * 4));
    HIP_TRY(c, c->s_tf.reserve(sizeof(double) * 2 * cap));
    double *d_aux = aux ? c->s_tf.as<double>() : nullptr;
    HIP_TRY(c, hipMemcpyAsync(c->s_in.p, X0, sizeof(double) * S, hipMemcpyHostToDevice, c->stream));
    const double s0 = sw ? sw[0] : c->P.sw0, s1 = sw ? sw[1] : c->P.sw1;
    c->n_traj += 1; c->n_launch += 1;
    hipError_t e = table_of(c)->dense(c->stream, c->P, t0, tf, s0, s1, c->s_in.as<double>(), c->s_out.as<double>(), c->s_t0.as<double>(), cap, c->s_aux.as<int>(), d_aux);
    HIP_TRY(c, e);
    HIP_TRY(c, hipMemcpyAsync(rows, c->s_aux.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int kept = *rows < cap ? *rows : cap;
    HIP_TRY(c, hipMemcpy(dense, c->s_out.p, sizeof(double) * S * kept, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(times, c->s_t0.p, sizeof(double) * kept, hipMemcpyDeviceToHost));
    if (aux) HIP_TRY(c, hipMemcpy(aux, d_aux, sizeof(double) * 2 * kept, hipMemcpyDeviceToHost));
    return SOCP_OK;
}

int socp_eval_batch(socp_ctx *c, int what, int B, const double *t, const double *sw,
                    const double *X, int len, double *out, int is_jac)
{
    if (!c) return SOCP_ERR_ARG;
    if (B < 0 || (B > 0 && (!t || !X || !out))) return fail(c, SOCP_ERR_ARG, "eval_batch: null argument");
    if (what < SOCP_EVAL_RHS || what > SOCP_EVAL_HAMILTONIAN) return fail(c, SOCP_ERR_ARG, "eval_batch: unknown quantity");
    const int L = (c->S + 1) * c->S;
    const bool var = is_jac && what != SOCP_EVAL_CONTROL;
    if (var && !has_var(c))
        return fail(c, SOCP_ERR_UNSUPPORTED, "eval_batch: this model has no variational equations (modelOrder 0)");
    if (var && what == SOCP_EVAL_RHS && len != L) return fail(c, SOCP_ERR_ARG, "eval_batch: augmented state length must be (2*dim+1)*2*dim");
    if (!(var && what == SOCP_EVAL_RHS) && len < c->S) return fail(c, SOCP_ERR_ARG, "eval_batch: state length must be at least 2*dim");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int out_len = var ? (what == SOCP_EVAL_RHS ? L : c->S + 1)
                            : (what == SOCP_EVAL_RHS ? c->S : (what == SOCP_EVAL_CONTROL ? c->nu : 1));
    if (!var && len != c->S) {
        // a longer (augmented) vector may be passed for Control / Hamiltonian: only the state part is read
        return fail(c, SOCP_ERR_ARG, "eval_batch: pass the 2*dim state part for is_jac=0 evaluations");
    }
    double *d_t, *d_X, *d_sw = nullptr, *d_out;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (size_t)B * out_len));
    d_out = c->s_out.as<double>();
    HIP_TRY(c, stage_up(c, c->s_t0, t, B, d_t));
    HIP_TRY(c, stage_up(c, c->s_in, X, (size_t)B * len, d_X));
    if (sw) HIP_TRY(c, stage_up(c, c->s_sw, sw, (size_t)2 * B, d_sw));
    c->n_launch += 1;
    hipError_t e = var ? c->vt->var_eval(c->stream, c->P, what == SOCP_EVAL_RHS ? 0 : 1, B, d_t, d_X, len, d_out)
                       : table_of(c)->eval(c->stream, c->P, what, B, d_t, d_sw, d_X, d_out);
    HIP_TRY(c, e);
    HIP_TRY(c, copy_down(c, out, d_out, (size_t)B * out_len));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

/* ---- Hamiltonian gradient: (dH/dp, -dH/dx) of the model's hamiltonian_t by dual numbers ------ */

int socp_ctx_has_hamiltonian_gradient(const socp_ctx *c) { return c ? (table_of(c)->hamiltonian_gradient ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
// every refusal comes before anything is counted, reserved or enqueued
int hamiltonian_gradient_args(socp_ctx *c, int B, const void *t, const void *X, const void *G)
{
    if (B < 0 || (B > 0 && (!t || !X || !G))) return fail(c, SOCP_ERR_ARG, "hamiltonian_gradient_batch: B >= 0 and non-null t, X, G are required");
    if (!table_of(c)->hamiltonian_gradient)
        return fail(c, SOCP_ERR_UNSUPPORTED, "hamiltonian_gradient_batch: this model's launch table has no hamiltonian_gradient entry (a model "
                                             "without the hamiltonian_t trait)");
    return SOCP_OK;
}
}  // namespace

int socp_hamiltonian_gradient_batch_dev(socp_ctx *c, int B, const double *d_t, const double *d_sw, const double *d_X, double *d_G)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = hamiltonian_gradient_args(c, B, d_t, d_X, d_G)) return rc;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_launch += 1;
    HIP_TRY(c, table_of(c)->hamiltonian_gradient(c->stream, c->P, B, d_t, d_sw, d_X, d_G));
    return SOCP_OK;
}

int socp_hamiltonian_gradient_batch(socp_ctx *c, int B, const double *t, const double *sw, const double *X, double *G)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = hamiltonian_gradient_args(c, B, t, X, G)) return rc;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nX = (size_t)B * c->S;
    double *d_t, *d_X, *d_sw = nullptr;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * nX));
    HIP_TRY(c, stage_up(c, c->s_t0, t, B, d_t));
    HIP_TRY(c, stage_up(c, c->s_in, X, nX, d_X));
    if (sw) HIP_TRY(c, stage_up(c, c->s_sw, sw, (size_t)2 * B, d_sw));
    const int rc = socp_hamiltonian_gradient_batch_dev(c, B, d_t, d_sw, d_X, c->s_out.as<double>());
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, G, c->s_out.as<double>(), nX));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

/* ---- Jacobian of the Hamiltonian vector field: dG/dX of the gradient above by nested dual numbers ------ */

int socp_ctx_has_hamiltonian_jacobian(const socp_ctx *c) { return c ? (table_of(c)->hamiltonian_jacobian ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
// every refusal comes before anything is counted, reserved or enqueued
int hamiltonian_jacobian_args(socp_ctx *c, int B, const void *t, const void *X, const void *A)
{
    if (B < 0 || (B > 0 && (!t || !X || !A))) return fail(c, SOCP_ERR_ARG, "hamiltonian_jacobian_batch: B >= 0 and non-null t, X, A are required");
    if (!table_of(c)->hamiltonian_jacobian)
        return fail(c, SOCP_ERR_UNSUPPORTED, "hamiltonian_jacobian_batch: this model's launch table has no hamiltonian_jacobian entry (a model "
                                             "whose hamiltonian_t does not take nested dual numbers, or without the trait)");
    return SOCP_OK;
}
}  // namespace

int socp_hamiltonian_jacobian_batch_dev(socp_ctx *c, int B, const double *d_t, const double *d_sw, const double *d_X, double *d_A, double *d_G)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = hamiltonian_jacobian_args(c, B, d_t, d_X, d_A)) return rc;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_launch += 1;
    HIP_TRY(c, table_of(c)->hamiltonian_jacobian(c->stream, c->P, B, d_t, d_sw, d_X, d_A, d_G));
    return SOCP_OK;
}

int socp_hamiltonian_jacobian_batch(socp_ctx *c, int B, const double *t, const double *sw, const double *X, double *A, double *G)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = hamiltonian_jacobian_args(c, B, t, X, A)) return rc;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nX = (size_t)B * c->S, nA = nX * c->S;
    double *d_t, *d_X, *d_sw = nullptr;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (nA + nX)));      // A, then G
    HIP_TRY(c, stage_up(c, c->s_t0, t, B, d_t));
    HIP_TRY(c, stage_up(c, c->s_in, X, nX, d_X));
    if (sw) HIP_TRY(c, stage_up(c, c->s_sw, sw, (size_t)2 * B, d_sw));
    double *const d_A = c->s_out.as<double>();
    const int rc = socp_hamiltonian_jacobian_batch_dev(c, B, d_t, d_sw, d_X, d_A, G ? d_A + nA : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, A, d_A, nA));
    if (G) HIP_TRY(c, copy_down(c, G, d_A + nA, nX));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

/* ---- shooting problem --------------------------------------------------------------------- */

int socp_problem_set(socp_ctx *c, int M, const int *mode_t, const int *mode_x, const double *time, const double *xnode)
{
    if (!c) return SOCP_ERR_ARG;
    if (M < 1 || !mode_t || !mode_x || !time || !xnode) return fail(c, SOCP_ERR_ARG, "problem_set: bad argument");
    if (M + 1 > kMaxNodes) return fail(c, SOCP_ERR_ARG, "problem_set: too many shooting nodes");
    const int d = c->dim, S = c->S;
    for (int j = 0; j <= M; j++)
        if (mode_t[j] < SOCP_FIXED || mode_t[j] > SOCP_CONTINUOUS) return fail(c, SOCP_ERR_ARG, "problem_set: bad time mode");
    // a CONTINUOUS end node would leave the tail of the timeline unset in the reference
    // (shooting.cpp:1586-1613 only closes an interval at a FIXED/FREE node)
    if (mode_t[0] == SOCP_CONTINUOUS || mode_t[M] == SOCP_CONTINUOUS)
        return fail(c, SOCP_ERR_ARG, "problem_set: first and last time must be FIXED or FREE");
    for (int k = 0; k <= M; k++)
        for (int j = 0; j < d; j++) {
            const int m = mode_x[k * d + j];
            if (m < SOCP_FIXED || m > SOCP_CONTINUOUS) return fail(c, SOCP_ERR_ARG, "problem_set: bad state mode");
            // (interior FREE states go to the model's SwitchingStateFunction -- shooting.cpp:1535-1538, model.hpp:339-341 -- i.e. to
            // the optional device trait switching_state; a model without it gets the default hook's zero rows)
            if ((k == 0 || k == M) && m == SOCP_CONTINUOUS)
                return fail(c, SOCP_ERR_ARG, "problem_set: CONTINUOUS state mode at a boundary node");
        }

    c->M = M;
    c->mode_t.assign(mode_t, mode_t + M + 1);
    c->mode_x.assign(mode_x, mode_x + (size_t)(M + 1) * d);
    c->time.assign(time, time + M + 1);
    c->xnode.assign(xnode, xnode + (size_t)(M + 1) * S);
    c->node_kind.assign(M + 1, -2); c->lo.assign(M + 1, 0); c->hi.assign(M + 1, 0); c->ft_row.assign(M + 1, -1);

    // unknown / residual layout (shooting.cpp:228-243, 945-990)
    int nbr = S * M;
    c->sw_node0 = c->sw_node1 = -1;
    for (int j = 0; j <= M; j++) {
        if (mode_t[j] == SOCP_FIXED) c->node_kind[j] = -1;
        if (mode_t[j] == SOCP_FREE) {
            c->node_kind[j] = nbr;           // index of the time unknown in z ...
            c->ft_row[j] = nbr;              // ... and of its residual row in F
            nbr++;
            if (j < M) { if (c->sw_node0 < 0) c->sw_node0 = j; else if (c->sw_node1 < 0) c->sw_node1 = j; }
        }
    }
    c->n = nbr;
    int cur = 0;
    for (int j = 0; j <= M; j++) {
        if (c->node_kind[j] != -2) {
            for (int k = cur + 1; k < j; k++) { c->lo[k] = cur; c->hi[k] = j; }
            c->lo[j] = c->hi[j] = j;
            cur = j;
        }
    }

    // FD column -> segments to integrate
    std::vector<int2> full, dedup;
    for (int j = 0; j < c->n; j++)
        for (int i = 0; i < M; i++) full.push_back(make_int2(j, i));
    for (int j = 0; j < c->n; j++) {
        if (j < S * M) {
            const int k = j / S;
            if (k >= 1) dedup.push_back(make_int2(j, k - 1));
            dedup.push_back(make_int2(j, k));
        } else {
            int q = 0;
            for (int k = 0; k <= M; k++) if (c->node_kind[k] == j) q = k;
            if (q == c->sw_node0 || q == c->sw_node1) {
                for (int i = 0; i < M; i++) dedup.push_back(make_int2(j, i));   // control law reads it everywhere
            } else {
                int a = q, b = q;
                while (a > 0 && c->node_kind[a - 1] == -2) a--;
                if (a > 0) a--;                                // previous junction
                while (b < M && c->node_kind[b + 1] == -2) b++;
                if (b < M) b++;                                // next junction
                for (int i = a; i < b; i++) dedup.push_back(make_int2(j, i));
            }
        }
    }
    c->T_full = (int)full.size();
    c->T_dedup = (int)dedup.size();

    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));     // tables may still be in use by enqueued work
    const size_t nI = (size_t)(M + 1), off_kind = 0, off_lo = nI, off_hi = 2 * nI, off_ft = 3 * nI, off_mx = 4 * nI;
    const size_t n_int = 4 * nI + nI * d;
    const size_t int_bytes = ((n_int * sizeof(int) + 15) / 16) * 16;
    const size_t n_dbl = nI + nI * S;
    HIP_TRY(c, c->d_tables.reserve(int_bytes + n_dbl * sizeof(double)));
    std::vector<char> blob(int_bytes + n_dbl * sizeof(double));
    int *bi = reinterpret_cast<int *>(blob.data());
    double *bd = reinterpret_cast<double *>(blob.data() + int_bytes);
    std::memcpy(bi + off_kind, c->node_kind.data(), nI * sizeof(int));
    std::memcpy(bi + off_lo, c->lo.data(), nI * sizeof(int));
    std::memcpy(bi + off_hi, c->hi.data(), nI * sizeof(int));
    std::memcpy(bi + off_ft, c->ft_row.data(), nI * sizeof(int));
    std::memcpy(bi + off_mx, c->mode_x.data(), nI * d * sizeof(int));
    std::memcpy(bd, c->time.data(), nI * sizeof(double));
    std::memcpy(bd + nI, c->xnode.data(), nI * S * sizeof(double));
    HIP_TRY(c, hipMemcpy(c->d_tables.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    HIP_TRY(c, c->d_pairs_full.reserve(sizeof(int2) * full.size()));
    HIP_TRY(c, c->d_pairs_dedup.reserve(sizeof(int2) * dedup.size()));
    HIP_TRY(c, hipMemcpy(c->d_pairs_full.p, full.data(), sizeof(int2) * full.size(), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_pairs_dedup.p, dedup.data(), sizeof(int2) * dedup.size(), hipMemcpyHostToDevice));

    const int *di = c->d_tables.as<int>();
    const double *dd = reinterpret_cast<const double *>(c->d_tables.as<char>() + int_bytes);
    c->pb.dim = d; c->pb.M = M; c->pb.n = c->n;
    c->pb.sw_node0 = c->sw_node0; c->pb.sw_node1 = c->sw_node1;
    c->pb.node_kind = di + off_kind; c->pb.lo = di + off_lo; c->pb.hi = di + off_hi;
    c->pb.ft_row = di + off_ft; c->pb.mode_x = di + off_mx;
    c->pb.time = dd; c->pb.xnode = dd + nI;
    c->pb.pp_params = c->pb.pp_time = c->pb.pp_xnode = nullptr; c->pb.pp_stride = 0; c->pb.pp_smooth = 0;   // a new problem starts without per-problem blocks
    c->blocks_smooth_hint = false;
    c->has_problem = true;
    return SOCP_OK;
}

int socp_problem_set_blocks_dev(socp_ctx *c, const double *d_params, int stride, const double *d_time, const double *d_xnode)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "problem_set_blocks: no problem set");
    if (const int rc = blocks_stride(c, "problem_set_blocks: stride", d_params, stride)) return rc;
    if (d_params && c->nparams > kMaxParams) return fail(c, SOCP_ERR_ARG, "problem_set_blocks: too many parameters");
    c->pb.pp_params = d_params;
    c->pb.pp_stride = d_params ? stride : 0;
    c->pb.pp_time = d_time;
    c->pb.pp_xnode = d_xnode;
    c->pb.pp_smooth = (d_params && c->blocks_smooth_hint) ? 1 : 0;
    return SOCP_OK;
}

int socp_problem_blocks_all_smooth(socp_ctx *c, int all_smooth)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "problem_blocks_all_smooth: no problem set");
    c->blocks_smooth_hint = all_smooth != 0;
    c->pb.pp_smooth = (c->pb.pp_params && c->blocks_smooth_hint) ? 1 : 0;
    return SOCP_OK;
}

int socp_residual_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int stride, const double *time,
                               const double *xnode, double *F)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "residual_batch_blocks: no problem set");
    if (B < 0 || (B > 0 && (!Z || !F))) return fail(c, SOCP_ERR_ARG, "residual_batch_blocks: null argument");
    if (const int rc = blocks_stride(c, "residual_batch_blocks: stride", params, stride)) return rc;
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, stride, time, xnode, [&] { return socp_residual_batch(c, B, Z, F); });
}

int socp_problem_num_nodes(const socp_ctx *c) { return (c && c->has_problem) ? c->M + 1 : SOCP_ERR_ARG; }
int socp_problem_num_param(const socp_ctx *c) { return (c && c->has_problem) ? c->n : SOCP_ERR_ARG; }

int socp_timeline(socp_ctx *c, const double *z, double *tl)
{
    // Pure index/interpolation logic on host data (no RHS arithmetic): shooting.cpp:1579-1617.
    if (!c || !z || !tl) return fail(c, SOCP_ERR_ARG, "timeline: null argument");
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "timeline: no problem set");
    auto jt = [&](int j) { return c->node_kind[j] >= 0 ? z[c->node_kind[j]] : c->time[j]; };
    for (int k = 0; k <= c->M; k++) {
        if (c->node_kind[k] >= -1) tl[k] = jt(k);
        else {
            const int a = c->lo[k], b = c->hi[k];
            const double ta = jt(a), tb = jt(b);
            tl[k] = ta + (k - a) * (tb - ta) / (b - a);
        }
    }
    return SOCP_OK;
}

int socp_residual_batch_dev(socp_ctx *c, int B, const double *d_Z, double *d_F)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "residual_batch: no problem set");
    if (B < 0 || (B > 0 && (!d_Z || !d_F))) return fail(c, SOCP_ERR_ARG, "residual_batch: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, run_residual(c, B, d_Z, d_F));
    return SOCP_OK;
}

int socp_residual_batch(socp_ctx *c, int B, const double *Z, double *F)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "residual_batch: no problem set");
    if (B < 0 || (B > 0 && (!Z || !F))) return fail(c, SOCP_ERR_ARG, "residual_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nZ = (size_t)B * c->n;
    double *d_Z;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * nZ));
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, d_Z));
    int rc = socp_residual_batch_dev(c, B, d_Z, c->s_out.as<double>());
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, F, c->s_out.as<double>(), nZ));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

/* ---- batched trace ------------------------------------------------------------------------- */

int socp_trace_width(const socp_ctx *c) { return c ? 1 + c->S + c->nu + 1 + 2 : SOCP_ERR_ARG; }

namespace {
int trace_args(socp_ctx *c, const char *who, int B, int stride, int cap)
{
    if (const int rc = args_head(c, who, B >= 0 && stride >= 1 && cap >= 1, "B >= 0, stride >= 1 and cap >= 1 are required")) return rc;
    return args_tail(c, who, table_of(c)->trace && table_of(c)->trace_fill, "trace entry", nullptr);
}
}  // namespace

int socp_trace_batch_dev(socp_ctx *c, int B, const double *d_Z, int stride, int cap, double *d_rows, int *d_count)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc = trace_args(c, "trace_batch", B, stride, cap);
    if (rc != SOCP_OK) return rc;
    if (B > 0 && (!d_Z || !d_rows || !d_count)) return fail(c, SOCP_ERR_ARG, "trace_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_traj += (long long)B * c->M; c->n_launch += 2;
    HIP_TRY(c, table_of(c)->trace(c->stream, c->P, c->pb, B, d_Z, stride, cap, d_rows, d_count));
    HIP_TRY(c, table_of(c)->trace_fill(c->stream, c->P, c->pb, B, cap, d_rows, d_count));
    return SOCP_OK;
}

int socp_trace_batch(socp_ctx *c, int B, const double *Z, int stride, int cap, double *rows, int *count)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc0 = trace_args(c, "trace_batch", B, stride, cap);
    if (rc0 != SOCP_OK) return rc0;
    if (B > 0 && (!Z || !rows || !count)) return fail(c, SOCP_ERR_ARG, "trace_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t segs = (size_t)B * c->M, nR = segs * cap * socp_trace_width(c);
    double *d_Z, *d_rows;
    HIP_TRY(c, c->s_var.reserve(sizeof(int) * segs));
    HIP_TRY(c, stage_up(c, c->s_in, Z, (size_t)B * c->n, d_Z));
    // the caller's buffers travel both ways: what the kernels leave untouched (rows at or beyond min(count, cap)) comes back as it went
    HIP_TRY(c, stage_up(c, c->s_out, rows, nR, d_rows));
    const int rc = socp_trace_batch_dev(c, B, d_Z, stride, cap, d_rows, c->s_var.as<int>());
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, rows, d_rows, nR));
    HIP_TRY(c, copy_down(c, count, c->s_var.as<int>(), segs));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_trace_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                            const double *xnode, int stride, int cap, double *rows, int *count)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = args_head(c, "trace_batch_blocks", B >= 0, "B >= 0 is required")) return rc;
    if (const int rc = blocks_stride(c, "trace_batch_blocks: the parameter stride", params, pstride)) return rc;
    // what the host form refuses, under its name as before: nothing is staged for a call that is refused, or for an empty batch
    if (const int rc = trace_args(c, "trace_batch", B, stride, cap)) return rc;
    if (B > 0 && (!Z || !rows || !count)) return fail(c, SOCP_ERR_ARG, "trace_batch: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode, [&] { return socp_trace_batch(c, B, Z, stride, cap, rows, count); });
}

/* ---- batched cost -------------------------------------------------------------------------- */

int socp_ctx_has_cost(const socp_ctx *c) { return c ? (table_of(c)->cost ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
int cost_args(socp_ctx *c, const char *who, int B, const void *Z, const void *cost)
{
    if (const int rc = args_head(c, who, B >= 0, "B >= 0 is required")) return rc;
    if (B > 0 && (!Z || !cost)) return fail(c, SOCP_ERR_ARG, std::string(who) + ": null argument");
    return args_tail(c, who, table_of(c)->cost != nullptr, "cost entry", "the running cost is integrated with");
}
}  // namespace

int socp_cost_batch_dev(socp_ctx *c, int B, const double *d_Z, double *d_cost, double *d_total, double *d_Xend)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc = cost_args(c, "cost_batch", B, d_Z, d_cost);
    if (rc != SOCP_OK) return rc;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_traj += (long long)B * c->M; c->n_launch += d_total ? 2 : 1;
    HIP_TRY(c, table_of(c)->cost(c->stream, c->P, c->pb, B, d_Z, d_cost, d_Xend));
    if (d_total) HIP_TRY(c, cost_total(c->stream, B, c->M, d_cost, d_total));
    return SOCP_OK;
}

int socp_cost_batch(socp_ctx *c, int B, const double *Z, double *cost, double *total, double *Xend)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc0 = cost_args(c, "cost_batch", B, Z, cost);
    if (rc0 != SOCP_OK) return rc0;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t segs = (size_t)B * c->M, nT = total ? (size_t)B : 0, nX = Xend ? segs * c->S : 0;
    double *d_Z;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (segs + nT + nX)));
    double *dC = c->s_out.as<double>(), *dT = dC + segs, *dX = dT + nT;
    HIP_TRY(c, stage_up(c, c->s_in, Z, (size_t)B * c->n, d_Z));
    const int rc = socp_cost_batch_dev(c, B, d_Z, dC, total ? dT : nullptr, Xend ? dX : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, cost, dC, segs));
    if (total) HIP_TRY(c, copy_down(c, total, dT, nT));
    if (Xend) HIP_TRY(c, copy_down(c, Xend, dX, nX));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_cost_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                           const double *xnode, double *cost, double *total, double *Xend)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = cost_args(c, "cost_batch", B, Z, cost)) return rc;          // under the host form's name, as before
    if (const int rc = blocks_stride(c, "cost_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode, [&] { return socp_cost_batch(c, B, Z, cost, total, Xend); });
}

/* ---- batched extrema ----------------------------------------------------------------------- */

int socp_ctx_has_extrema(const socp_ctx *c) { return c ? (table_of(c)->extrema ? 1 : 0) : SOCP_ERR_ARG; }

int socp_extrema_width(const socp_ctx *c) { return c ? c->S + c->nu + 1 + socp_ctx_event_channels(c) : SOCP_ERR_ARG; }

namespace {
int extrema_args(socp_ctx *c, const char *who, int B, int what, const void *Z, const void *vmin, const void *vmax, const void *count)
{
    if (const int rc = args_head(c, who, B >= 0 && what >= 0 && what <= 7, "B >= 0 and 0 <= what <= 7 are required")) return rc;
    if (B > 0 && (!Z || !vmin || !vmax || !count)) return fail(c, SOCP_ERR_ARG, std::string(who) + ": null argument");
    return args_tail(c, who, table_of(c)->extrema != nullptr, "extrema entry", nullptr);
}
}  // namespace

int socp_extrema_batch_dev(socp_ctx *c, int B, const double *d_Z, int what, double *d_vmin, double *d_vmax, double *d_tmin,
                           double *d_tmax, int *d_count, int *d_nbad)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc = extrema_args(c, "extrema_batch", B, what, d_Z, d_vmin, d_vmax, d_count);
    if (rc != SOCP_OK) return rc;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_traj += (long long)B * c->M; c->n_launch += 1;
    HIP_TRY(c, table_of(c)->extrema(c->stream, c->P, c->pb, B, d_Z, what, d_vmin, d_vmax, d_tmin, d_tmax, d_count, d_nbad));
    return SOCP_OK;
}

int socp_extrema_batch(socp_ctx *c, int B, const double *Z, int what, double *vmin, double *vmax, double *tmin, double *tmax,
                       int *count, int *nbad)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc0 = extrema_args(c, "extrema_batch", B, what, Z, vmin, vmax, count);
    if (rc0 != SOCP_OK) return rc0;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t segs = (size_t)B * c->M, nV = segs * socp_extrema_width(c);
    double *d_Z;
    HIP_TRY(c, stage_up(c, c->s_in, Z, (size_t)B * c->n, d_Z));
    // the caller's arrays travel both ways: the columns of a group `what` does not select come back as they went
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * 4 * nV));
    HIP_TRY(c, c->s_var.reserve(sizeof(int) * 2 * segs));
    double *dLo = c->s_out.as<double>(), *dHi = dLo + nV, *dTa = dHi + nV, *dTb = dTa + nV;
    int *dC = c->s_var.as<int>(), *dN = dC + segs;
    HIP_TRY(c, copy_up(c, dLo, vmin, nV));
    HIP_TRY(c, copy_up(c, dHi, vmax, nV));
    if (tmin) HIP_TRY(c, copy_up(c, dTa, tmin, nV));
    if (tmax) HIP_TRY(c, copy_up(c, dTb, tmax, nV));
    const int rc = socp_extrema_batch_dev(c, B, d_Z, what, dLo, dHi, tmin ? dTa : nullptr, tmax ? dTb : nullptr, dC, nbad ? dN : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, vmin, dLo, nV));
    HIP_TRY(c, copy_down(c, vmax, dHi, nV));
    if (tmin) HIP_TRY(c, copy_down(c, tmin, dTa, nV));
    if (tmax) HIP_TRY(c, copy_down(c, tmax, dTb, nV));
    HIP_TRY(c, copy_down(c, count, dC, segs));
    if (nbad) HIP_TRY(c, copy_down(c, nbad, dN, segs));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_extrema_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                              const double *xnode, int what, double *vmin, double *vmax, double *tmin, double *tmax, int *count,
                              int *nbad)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = extrema_args(c, "extrema_batch_blocks", B, what, Z, vmin, vmax, count)) return rc;
    if (const int rc = blocks_stride(c, "extrema_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_extrema_batch(c, B, Z, what, vmin, vmax, tmin, tmax, count, nbad); });
}

/* ---- batched observables ------------------------------------------------------------------- */

int socp_ctx_has_observe(const socp_ctx *c) { return c ? (table_of(c)->observe ? 1 : 0) : SOCP_ERR_ARG; }

int socp_ctx_observables(const socp_ctx *c) { return c ? (table_of(c)->observe ? table_of(c)->observables : 0) : SOCP_ERR_ARG; }

const char *socp_ctx_observable_name(const socp_ctx *c, int k)
{
    if (!c || k < 0 || k >= socp_ctx_observables(c) || !table_of(c)->observable_names) return nullptr;
    return table_of(c)->observable_names[k];
}

namespace {
int observe_args(socp_ctx *c, const char *who, int B, const void *Z, const void *ymin, const void *ymax, const void *count)
{
    if (const int rc = args_head(c, who, B >= 0, "B >= 0 is required")) return rc;
    if (B > 0 && (!Z || !ymin || !ymax || !count)) return fail(c, SOCP_ERR_ARG, std::string(who) + ": null argument");
    return args_tail(c, who, table_of(c)->observe != nullptr && table_of(c)->observables > 0, "observe entry", nullptr);
}
}  // namespace

int socp_observe_batch_dev(socp_ctx *c, int B, const double *d_Z, double *d_ymin, double *d_ymax, double *d_tmin, double *d_tmax,
                           double *d_integral, int *d_count, int *d_nbad)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc = observe_args(c, "observe_batch", B, d_Z, d_ymin, d_ymax, d_count);
    if (rc != SOCP_OK) return rc;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_traj += (long long)B * c->M; c->n_launch += 1;
    HIP_TRY(c, table_of(c)->observe(c->stream, c->P, c->pb, B, d_Z, d_ymin, d_ymax, d_tmin, d_tmax, d_integral, d_count, d_nbad));
    return SOCP_OK;
}

int socp_observe_batch(socp_ctx *c, int B, const double *Z, double *ymin, double *ymax, double *tmin, double *tmax, double *integral,
                       int *count, int *nbad)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc0 = observe_args(c, "observe_batch", B, Z, ymin, ymax, count);
    if (rc0 != SOCP_OK) return rc0;
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t segs = (size_t)B * c->M, nV = segs * table_of(c)->observables;
    double *d_Z;
    HIP_TRY(c, stage_up(c, c->s_in, Z, (size_t)B * c->n, d_Z));
    // the launch writes every element of every array it is given: nothing travels up but Z
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * 5 * nV));
    HIP_TRY(c, c->s_var.reserve(sizeof(int) * 2 * segs));
    double *dLo = c->s_out.as<double>(), *dHi = dLo + nV, *dTa = dHi + nV, *dTb = dTa + nV, *dI = dTb + nV;
    int *dC = c->s_var.as<int>(), *dN = dC + segs;
    const int rc = socp_observe_batch_dev(c, B, d_Z, dLo, dHi, tmin ? dTa : nullptr, tmax ? dTb : nullptr, integral ? dI : nullptr, dC,
                                          nbad ? dN : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, ymin, dLo, nV));
    HIP_TRY(c, copy_down(c, ymax, dHi, nV));
    if (tmin) HIP_TRY(c, copy_down(c, tmin, dTa, nV));
    if (tmax) HIP_TRY(c, copy_down(c, tmax, dTb, nV));
    if (integral) HIP_TRY(c, copy_down(c, integral, dI, nV));
    HIP_TRY(c, copy_down(c, count, dC, segs));
    if (nbad) HIP_TRY(c, copy_down(c, nbad, dN, segs));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_observe_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                              const double *xnode, double *ymin, double *ymax, double *tmin, double *tmax, double *integral, int *count,
                              int *nbad)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = observe_args(c, "observe_batch_blocks", B, Z, ymin, ymax, count)) return rc;
    if (const int rc = blocks_stride(c, "observe_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_observe_batch(c, B, Z, ymin, ymax, tmin, tmax, integral, count, nbad); });
}

/* ---- batched Move(tf) / re-grid ------------------------------------------------------------- */

namespace {
int move_args(socp_ctx *c, const char *who, int B, int K)
{
    if (const int rc = args_head(c, who, B >= 0 && K >= 0, "B >= 0 and K >= 0 are required")) return rc;
    return args_tail(c, who, table_of(c)->move != nullptr, "move entry", nullptr);
}

hipError_t run_move(socp_ctx *c, int B, const double *d_Z, int K, const double *d_tq, double *d_Xq, double *d_tout)
{
    c->n_traj += (long long)B * K; c->n_launch += 1;
    return table_of(c)->move(c->stream, c->P, c->pb, B, d_Z, K, d_tq, d_Xq, d_tout);
}

// the target structure of a re-grid: n2 = S M2 + #FREE, the FREE-node bit words; SOCP_ERR_ARG for what the entry points refuse
int regrid_layout(const socp_ctx *c, int M2, const int *mode_t2, unsigned long long (&bits)[4])
{
    if (!c || !mode_t2 || M2 < 1 || M2 > 255) return SOCP_ERR_ARG;
    int n2 = c->S * M2;
    for (int k = 0; k < 4; k++) bits[k] = 0;
    for (int j = 0; j <= M2; j++) {
        if (mode_t2[j] < SOCP_FIXED || mode_t2[j] > SOCP_CONTINUOUS) return SOCP_ERR_ARG;
        if (mode_t2[j] == SOCP_FREE) { bits[j >> 6] |= 1ull << (j & 63); n2++; }
    }
    return n2;
}

int regrid_args(socp_ctx *c, int B, int M2, const int *mode_t2, unsigned long long (&bits)[4], int *n2)
{
    const int rc = move_args(c, "regrid_batch", B, 0);
    if (rc != SOCP_OK) return rc;
    if (M2 < 1 || M2 > 255) return fail(c, SOCP_ERR_ARG, "regrid_batch: 1 <= M2 <= 255 is required");
    if (!mode_t2) return fail(c, SOCP_ERR_ARG, "regrid_batch: null time-mode table");
    *n2 = regrid_layout(c, M2, mode_t2, bits);
    if (*n2 < 0) return fail(c, SOCP_ERR_ARG, "regrid_batch: bad time mode in the target structure");
    return SOCP_OK;
}
}  // namespace

int socp_move_batch_dev(socp_ctx *c, int B, const double *d_Z, int K, const double *d_tq, double *d_Xq, double *d_tout)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc = move_args(c, "move_batch", B, K);
    if (rc != SOCP_OK) return rc;
    if (B == 0 || K == 0) return SOCP_OK;
    if (!d_Z || !d_tq || !d_Xq) return fail(c, SOCP_ERR_ARG, "move_batch: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, run_move(c, B, d_Z, K, d_tq, d_Xq, d_tout));
    return SOCP_OK;
}

int socp_move_batch(socp_ctx *c, int B, const double *Z, int K, const double *tq, double *Xq, double *tout)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc0 = move_args(c, "move_batch", B, K);
    if (rc0 != SOCP_OK) return rc0;
    if (B == 0 || K == 0) return SOCP_OK;
    if (!Z || !tq || !Xq) return fail(c, SOCP_ERR_ARG, "move_batch: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t lanes = (size_t)B * K, nX = lanes * c->S;
    double *d_Z, *d_tq;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (nX + lanes)));
    double *dX = c->s_out.as<double>(), *dT = dX + nX;
    HIP_TRY(c, stage_up(c, c->s_in, Z, (size_t)B * c->n, d_Z));
    HIP_TRY(c, stage_up(c, c->s_t0, tq, lanes, d_tq));
    const int rc = socp_move_batch_dev(c, B, d_Z, K, d_tq, dX, tout ? dT : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, Xq, dX, nX));
    if (tout) HIP_TRY(c, copy_down(c, tout, dT, lanes));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_move_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                           const double *xnode, int K, const double *tq, double *Xq, double *tout)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc0 = move_args(c, "move_batch_blocks", B, K);
    if (rc0 != SOCP_OK) return rc0;
    if (const int rc = blocks_stride(c, "move_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B == 0 || K == 0) return SOCP_OK;
    if (!Z || !tq || !Xq) return fail(c, SOCP_ERR_ARG, "move_batch_blocks: null argument");
    return with_blocks(c, B, params, pstride, time, xnode, [&] { return socp_move_batch(c, B, Z, K, tq, Xq, tout); });
}

/* ---- batched events ------------------------------------------------------------------------ */

int socp_ctx_event_channels(const socp_ctx *c) { return c ? (table_of(c)->events ? table_of(c)->event_channels : 0) : SOCP_ERR_ARG; }

namespace {
// *chans: the watches' channels, four bits each (a kernel argument: the host array is read here)
int events_args(socp_ctx *c, const char *who, int B, int E, const int *chan, int refine, int cap, unsigned *chans)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (E < 1 || E > kMaxEventWatches) return fail(c, SOCP_ERR_ARG, w + ": 1 <= E <= 8 watches are required");
    if (refine < 0 || refine > kMaxEventRefine) return fail(c, SOCP_ERR_ARG, w + ": 0 <= refine <= 8 is required");
    if (cap < 1) return fail(c, SOCP_ERR_ARG, w + ": cap >= 1 is required");
    if (!chan) return fail(c, SOCP_ERR_ARG, w + ": null channel table");
    if (const int rc = args_tail(c, w, table_of(c)->events != nullptr, "events entry (the model has no event channels)", "events are located along"))
        return rc;
    *chans = 0;
    for (int e = 0; e < E; e++) {
        if (chan[e] < 0 || chan[e] >= table_of(c)->event_channels)
            return fail(c, SOCP_ERR_ARG, w + ": watch " + std::to_string(e) + " names channel " + std::to_string(chan[e]) +
                                             ", the model has " + std::to_string(table_of(c)->event_channels));
        *chans |= (unsigned)chan[e] << (4 * e);
    }
    return SOCP_OK;
}
}  // namespace

int socp_events_batch_dev(socp_ctx *c, int B, const double *d_Z, int E, const int *chan, const double *d_levels, int refine, int cap,
                          double *d_tev, int *d_id, int *d_count, double *d_Xev)
{
    if (!c) return SOCP_ERR_ARG;
    unsigned chans = 0;
    const int rc = events_args(c, "events_batch", B, E, chan, refine, cap, &chans);
    if (rc != SOCP_OK) return rc;
    if (B > 0 && (!d_Z || !d_levels || !d_tev || !d_id || !d_count)) return fail(c, SOCP_ERR_ARG, "events_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_traj += (long long)B * c->M; c->n_launch += 1;
    HIP_TRY(c, table_of(c)->events(c->stream, c->P, c->pb, B, d_Z, E, chans, d_levels, refine, cap, d_tev, d_id, d_count, d_Xev));
    return SOCP_OK;
}

int socp_events_batch(socp_ctx *c, int B, const double *Z, int E, const int *chan, const double *levels, int refine, int cap,
                      double *tev, int *id, int *count, double *Xev)
{
    if (!c) return SOCP_ERR_ARG;
    unsigned chans = 0;
    const int rc0 = events_args(c, "events_batch", B, E, chan, refine, cap, &chans);
    if (rc0 != SOCP_OK) return rc0;
    if (B > 0 && (!Z || !levels || !tev || !id || !count)) return fail(c, SOCP_ERR_ARG, "events_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t segs = (size_t)B * c->M, slots = segs * cap, nZ = (size_t)B * c->n, nL = (size_t)B * E, nX = Xev ? slots * c->S : 0;
    double *dZ, *dT;
    int *dI;
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, dZ, nZ + nL));
    double *dL = dZ + nZ;
    HIP_TRY(c, copy_up(c, dL, levels, nL));
    // the caller's buffers travel both ways: what the kernel leaves untouched (rows at or beyond min(count, cap)) comes back as it went
    HIP_TRY(c, stage_up(c, c->s_out, tev, slots, dT, slots + nX));
    HIP_TRY(c, stage_up(c, c->s_var, id, slots, dI, slots + segs));
    double *dX = dT + slots;
    int *dC = dI + slots;
    if (Xev) HIP_TRY(c, copy_up(c, dX, Xev, nX));
    const int rc = socp_events_batch_dev(c, B, dZ, E, chan, dL, refine, cap, dT, dI, dC, Xev ? dX : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, tev, dT, slots));
    HIP_TRY(c, copy_down(c, id, dI, slots));
    HIP_TRY(c, copy_down(c, count, dC, segs));
    if (Xev) HIP_TRY(c, copy_down(c, Xev, dX, nX));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_events_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                             const double *xnode, int E, const int *chan, const double *levels, int refine, int cap, double *tev,
                             int *id, int *count, double *Xev)
{
    if (!c) return SOCP_ERR_ARG;
    unsigned chans = 0;
    const int rc0 = events_args(c, "events_batch_blocks", B, E, chan, refine, cap, &chans);
    if (rc0 != SOCP_OK) return rc0;
    if (const int rc = blocks_stride(c, "events_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !levels || !tev || !id || !count)) return fail(c, SOCP_ERR_ARG, "events_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_events_batch(c, B, Z, E, chan, levels, refine, cap, tev, id, count, Xev); });
}

/* ---- batched Jacobi fields ----------------------------------------------------------------- */

int socp_ctx_has_jacobi(const socp_ctx *c) { return c ? (table_of(c)->jacobi ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
int jacobi_args(socp_ctx *c, const char *who, int B, int stride, int skip, int cap)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (stride < 1) return fail(c, SOCP_ERR_ARG, w + ": stride >= 1 is required");
    if (skip < 0) return fail(c, SOCP_ERR_ARG, w + ": skip >= 0 is required");
    if (cap < 1) return fail(c, SOCP_ERR_ARG, w + ": cap >= 1 is required");
    return args_tail(c, w, table_of(c)->jacobi != nullptr,
                     "jacobi entry (a model with its own ComputeTraj, or one the entry is not offered for)", "the Jacobi fields follow");
}
}  // namespace

int socp_jacobi_batch_dev(socp_ctx *c, int B, const double *d_Z, double epsfcn, int stride, int skip, int cap, double *d_tq, double *d_det,
                          int *d_count, int *d_nchange, double *d_tconj, double *d_Jend)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = jacobi_args(c, "jacobi_batch", B, stride, skip, cap)) return rc;
    if (B > 0 && (!d_Z || !d_tq || !d_det || !d_count || !d_nchange || !d_tconj)) return fail(c, SOCP_ERR_ARG, "jacobi_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_traj += (long long)B * c->M * (c->S / 2 + 1); c->n_launch += 1;
    HIP_TRY(c, table_of(c)->jacobi(c->stream, c->P, c->pb, B, d_Z, fd_eps(epsfcn), stride, skip, cap, d_tq, d_det, d_count, d_nchange, d_tconj,
                                   d_Jend));
    return SOCP_OK;
}

int socp_jacobi_batch(socp_ctx *c, int B, const double *Z, double epsfcn, int stride, int skip, int cap, double *tq, double *det, int *count,
                      int *nchange, double *tconj, double *Jend)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = jacobi_args(c, "jacobi_batch", B, stride, skip, cap)) return rc;
    if (B > 0 && (!Z || !tq || !det || !count || !nchange || !tconj)) return fail(c, SOCP_ERR_ARG, "jacobi_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t d = (size_t)c->S / 2, segs = (size_t)B * c->M, slots = segs * cap, nZ = (size_t)B * c->n, nJ = Jend ? segs * d * d : 0;
    double *dZ, *dT;
    int *dC;
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, dZ));
    // tq and det travel both ways: what the kernel leaves untouched (entries at or beyond min(count, cap)) comes back as it went
    HIP_TRY(c, stage_up(c, c->s_out, tq, slots, dT, 2 * slots + segs + nJ));
    double *dD = dT + slots, *dTc = dD + slots, *dJ = dTc + segs;
    HIP_TRY(c, copy_up(c, dD, det, slots));
    HIP_TRY(c, c->s_var.reserve(sizeof(int) * 2 * segs));
    dC = c->s_var.as<int>();
    int *dN = dC + segs;
    const int rc = socp_jacobi_batch_dev(c, B, dZ, epsfcn, stride, skip, cap, dT, dD, dC, dN, dTc, Jend ? dJ : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, tq, dT, slots));
    HIP_TRY(c, copy_down(c, det, dD, slots));
    HIP_TRY(c, copy_down(c, count, dC, segs));
    HIP_TRY(c, copy_down(c, nchange, dN, segs));
    HIP_TRY(c, copy_down(c, tconj, dTc, segs));
    if (Jend) HIP_TRY(c, copy_down(c, Jend, dJ, nJ));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_jacobi_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                             const double *xnode, double epsfcn, int stride, int skip, int cap, double *tq, double *det, int *count,
                             int *nchange, double *tconj, double *Jend)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = jacobi_args(c, "jacobi_batch_blocks", B, stride, skip, cap)) return rc;
    if (const int rc = blocks_stride(c, "jacobi_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !tq || !det || !count || !nchange || !tconj)) return fail(c, SOCP_ERR_ARG, "jacobi_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_jacobi_batch(c, B, Z, epsfcn, stride, skip, cap, tq, det, count, nchange, tconj, Jend); });
}

/* ---- batched exact fields ------------------------------------------------------------------ */

// an entry of the exact-derivative stack as this context offers it: vtolUAV's only after socp_ctx_set_exact_hooks(ctx, 1)
static bool exact_entry_on(const socp_ctx *c, bool has) { return has && (c->model_id != SOCP_MODEL_VTOLUAV || c->exact_hooks); }

int socp_ctx_has_fields(const socp_ctx *c) { return c ? (exact_entry_on(c, table_of(c)->fields != nullptr) ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
int fields_args(socp_ctx *c, const char *who, int B, int cols, int stride, int skip, int cap)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (cols != SOCP_FIELDS_COSTATE && cols != SOCP_FIELDS_ALL) return fail(c, SOCP_ERR_ARG, w + ": cols is SOCP_FIELDS_COSTATE or SOCP_FIELDS_ALL");
    if (stride < 1) return fail(c, SOCP_ERR_ARG, w + ": stride >= 1 is required");
    if (skip < 0) return fail(c, SOCP_ERR_ARG, w + ": skip >= 0 is required");
    if (cap < 1) return fail(c, SOCP_ERR_ARG, w + ": cap >= 1 is required");
    return args_tail(c, w, exact_entry_on(c, table_of(c)->fields != nullptr),
                     "fields entry (a model with its own ComputeTraj, one without the rhs_t trait, or vtolUAV before socp_ctx_set_exact_hooks)", "the exact fields follow");
}
}  // namespace

int socp_fields_batch_dev(socp_ctx *c, int B, const double *d_Z, int cols, int stride, int skip, int cap, double *d_tq, double *d_det,
                          int *d_count, int *d_nchange, double *d_tconj, double *d_Phi)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = fields_args(c, "fields_batch", B, cols, stride, skip, cap)) return rc;
    if (B > 0 && (!d_Z || !d_tq || !d_det || !d_count || !d_nchange || !d_tconj)) return fail(c, SOCP_ERR_ARG, "fields_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_traj += (long long)B * c->M * (cols == SOCP_FIELDS_ALL ? c->S : c->S / 2); c->n_launch += 1;
    HIP_TRY(c, table_of(c)->fields(c->stream, c->P, c->pb, B, d_Z, cols, stride, skip, cap, d_tq, d_det, d_count, d_nchange, d_tconj, d_Phi));
    return SOCP_OK;
}

int socp_fields_batch(socp_ctx *c, int B, const double *Z, int cols, int stride, int skip, int cap, double *tq, double *det, int *count,
                      int *nchange, double *tconj, double *Phi)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = fields_args(c, "fields_batch", B, cols, stride, skip, cap)) return rc;
    if (B > 0 && (!Z || !tq || !det || !count || !nchange || !tconj)) return fail(c, SOCP_ERR_ARG, "fields_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t s = (size_t)c->S, C = cols == SOCP_FIELDS_ALL ? s : s / 2, segs = (size_t)B * c->M, slots = segs * cap, nZ = (size_t)B * c->n,
                 nP = Phi ? segs * s * C : 0;
    double *dZ, *dT;
    int *dC;
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, dZ));
    // tq and det travel both ways: what the kernel leaves untouched (entries at or beyond min(count, cap)) comes back as it went
    HIP_TRY(c, stage_up(c, c->s_out, tq, slots, dT, 2 * slots + segs + nP));
    double *dD = dT + slots, *dTc = dD + slots, *dP = dTc + segs;
    HIP_TRY(c, copy_up(c, dD, det, slots));
    HIP_TRY(c, c->s_var.reserve(sizeof(int) * 2 * segs));
    dC = c->s_var.as<int>();
    int *dN = dC + segs;
    const int rc = socp_fields_batch_dev(c, B, dZ, cols, stride, skip, cap, dT, dD, dC, dN, dTc, Phi ? dP : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, tq, dT, slots));
    HIP_TRY(c, copy_down(c, det, dD, slots));
    HIP_TRY(c, copy_down(c, count, dC, segs));
    HIP_TRY(c, copy_down(c, nchange, dN, segs));
    HIP_TRY(c, copy_down(c, tconj, dTc, segs));
    if (Phi) HIP_TRY(c, copy_down(c, Phi, dP, nP));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_fields_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                             const double *xnode, int cols, int stride, int skip, int cap, double *tq, double *det, int *count,
                             int *nchange, double *tconj, double *Phi)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = fields_args(c, "fields_batch_blocks", B, cols, stride, skip, cap)) return rc;
    if (const int rc = blocks_stride(c, "fields_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !tq || !det || !count || !nchange || !tconj)) return fail(c, SOCP_ERR_ARG, "fields_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_fields_batch(c, B, Z, cols, stride, skip, cap, tq, det, count, nchange, tconj, Phi); });
}

/* ---- batched exact shooting Jacobian ------------------------------------------------------- */

int socp_ctx_has_exact_jacobian(const socp_ctx *c) { return c ? (exact_entry_on(c, table_of(c)->exact_jacobian != nullptr) ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
int exact_jacobian_args(socp_ctx *c, const char *who, int B)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (const int rc = args_tail(c, w, exact_entry_on(c, table_of(c)->exact_jacobian != nullptr),
                                 "exact_jacobian entry (a model without the rhs_t, hamiltonian_t and switching_fn_t traits, one with its own "
                                 "ComputeTraj, one with custom final rows and no final_row_t, or one with a switching_state hook and no "
                                 "switching_state_t with kSwitchingStateXpContinuous, or vtolUAV before socp_ctx_set_exact_hooks)",
                                 "the exact Jacobian follows"))
        return rc;
    // a FREE state component of an interior node: its rows are the model's SwitchingStateFunction.  vtolUAV's entry covers them
    // (switching_state_t, models_vtol.hpp); the launch table does not say whether another model's does, so those stay refused
    if (c->model_id == SOCP_MODEL_VTOLUAV) return SOCP_OK;
    for (int k = 1; k < c->M; k++)
        for (int j = 0; j < c->dim; j++)
            if (c->mode_x[(size_t)k * c->dim + j] == SOCP_FREE)
                return fail(c, SOCP_ERR_UNSUPPORTED, w + ": a FREE state component on an interior node (node " + std::to_string(k) +
                                                         ", component " + std::to_string(j) + ") is not covered");
    return SOCP_OK;
}
}  // namespace

namespace {
// the zero-fill and the launch of a batch that is checked and not empty
int exact_jacobian_launch(socp_ctx *c, int B, const double *d_Z, double *d_Fjac, double *d_F)
{
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_traj += (long long)B * c->M * (c->S + 1); c->n_launch += 1;
    HIP_TRY(c, table_of(c)->exact_jacobian(c->stream, c->P, c->pb, B, d_Z, d_Fjac, d_F));
    return SOCP_OK;
}
}  // namespace

int socp_exact_jacobian_batch_dev(socp_ctx *c, int B, const double *d_Z, double *d_Fjac, double *d_F)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = exact_jacobian_args(c, "exact_jacobian_batch", B)) return rc;
    if (B > 0 && (!d_Z || !d_Fjac)) return fail(c, SOCP_ERR_ARG, "exact_jacobian_batch: null argument");
    if (B == 0) return SOCP_OK;
    return exact_jacobian_launch(c, B, d_Z, d_Fjac, d_F);
}

int socp_exact_jacobian_batch(socp_ctx *c, int B, const double *Z, double *Fjac, double *F)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = exact_jacobian_args(c, "exact_jacobian_batch", B)) return rc;
    if (B > 0 && (!Z || !Fjac)) return fail(c, SOCP_ERR_ARG, "exact_jacobian_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nZ = (size_t)B * c->n, nJ = nZ * c->n;
    double *dZ, *dJ;
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, dZ));
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (nJ + nZ)));
    dJ = c->s_out.as<double>();
    double *dF = dJ + nJ;
    const int rc = exact_jacobian_launch(c, B, dZ, dJ, F ? dF : nullptr);      // the arguments are checked above, once
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, Fjac, dJ, nJ));
    if (F) HIP_TRY(c, copy_down(c, F, dF, nZ));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_exact_jacobian_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                                     const double *xnode, double *Fjac, double *F)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = exact_jacobian_args(c, "exact_jacobian_batch_blocks", B)) return rc;
    if (const int rc = blocks_stride(c, "exact_jacobian_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !Fjac)) return fail(c, SOCP_ERR_ARG, "exact_jacobian_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode, [&] { return socp_exact_jacobian_batch(c, B, Z, Fjac, F); });
}

int socp_regrid_num_param(const socp_ctx *c, int M2, const int *mode_t2)
{
    unsigned long long bits[4];
    return regrid_layout(c, M2, mode_t2, bits);
}

int socp_regrid_batch_dev(socp_ctx *c, int B, const double *d_Z, int M2, const int *mode_t2, const double *d_T2, double *d_Z2,
                          double *d_xnode2)
{
    if (!c) return SOCP_ERR_ARG;
    unsigned long long bits[4];
    int n2 = 0;
    const int rc = regrid_args(c, B, M2, mode_t2, bits, &n2);
    if (rc != SOCP_OK) return rc;
    if (B == 0) return SOCP_OK;
    if (!d_Z || !d_T2 || !d_Z2) return fail(c, SOCP_ERR_ARG, "regrid_batch: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    // launch 1: Move(T2[b][j]) for every node of the target, into the caller's xnode2 or a workspace buffer of the context
    // (grow-only: the first use and every growth is a hipMalloc, which synchronises the device -- the header says so)
    double *d_Xm = d_xnode2;
    if (!d_Xm) {
        HIP_TRY(c, c->s_var.reserve(sizeof(double) * (size_t)B * (M2 + 1) * c->S));
        d_Xm = c->s_var.as<double>();
    }
    HIP_TRY(c, run_move(c, B, d_Z, M2 + 1, d_T2, d_Xm, nullptr));
    // launch 2: the unknown vectors of the target structure
    c->n_launch += 1;
    HIP_TRY(c, regrid_pack(c->stream, B, c->S, M2, n2, bits, d_Xm, d_T2, d_Z2));
    return SOCP_OK;
}

int socp_regrid_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                             const double *xnode, int M2, const int *mode_t2, const double *T2, double *Z2, double *xnode2)
{
    if (!c) return SOCP_ERR_ARG;
    unsigned long long bits[4];
    int n2 = 0;
    const int rc0 = regrid_args(c, B, M2, mode_t2, bits, &n2);
    if (rc0 != SOCP_OK) return rc0;
    if (const int rc = blocks_stride(c, "regrid_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B == 0) return SOCP_OK;
    if (!Z || !T2 || !Z2) return fail(c, SOCP_ERR_ARG, "regrid_batch_blocks: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nT = (size_t)B * (M2 + 1), nZ2 = (size_t)B * n2, nX = nT * c->S;
    double *d_Z, *d_T2;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (nZ2 + nX)));
    double *dZ2 = c->s_out.as<double>(), *dX = dZ2 + nZ2;
    HIP_TRY(c, stage_up(c, c->s_in, Z, (size_t)B * c->n, d_Z));
    HIP_TRY(c, stage_up(c, c->s_t0, T2, nT, d_T2));
    // (the device form's workspace is s_var: the blocks in s_aux stay clear of it)
    const int rc = with_blocks(c, B, params, pstride, time, xnode,
                               [&] { return socp_regrid_batch_dev(c, B, d_Z, M2, mode_t2, d_T2, dZ2, xnode2 ? dX : nullptr); });
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, Z2, dZ2, nZ2));
    if (xnode2) HIP_TRY(c, copy_down(c, xnode2, dX, nX));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_fd_jacobian_multi_dev(socp_ctx *c, int np, const double *d_Z, const double *d_Fvec, double epsfcn,
                               double *d_Fjac, int dedup)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "fd_jacobian: no problem set");
    if (np < 0 || (np > 0 && (!d_Z || !d_Fvec || !d_Fjac))) return fail(c, SOCP_ERR_ARG, "fd_jacobian: null argument");
    if (np == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const double eps = fd_eps(epsfcn);
    if (dedup) {
        // rows a column cannot change reproduce fvec bit for bit => exact zeros
        HIP_TRY(c, hipMemsetAsync(d_Fjac, 0, sizeof(double) * (size_t)np * c->n * c->n, c->stream));
        HIP_TRY(c, run_fdjac(c, np, c->T_dedup, c->d_pairs_dedup.as<int2>(), d_Z, d_Fvec, eps, d_Fjac));
    } else {
        HIP_TRY(c, run_fdjac(c, np, c->T_full, c->d_pairs_full.as<int2>(), d_Z, d_Fvec, eps, d_Fjac));
    }
    return SOCP_OK;
}

int socp_fd_jacobian_dev(socp_ctx *c, const double *d_z, const double *d_fvec, double epsfcn, double *d_fjac, int dedup)
{
    return socp_fd_jacobian_multi_dev(c, 1, d_z, d_fvec, epsfcn, d_fjac, dedup);
}

int socp_fd_rows_dev(socp_ctx *c, int np, const double *d_Z, double epsfcn, double *d_Rows)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "fd_rows: no problem set");
    if (np < 0 || (np > 0 && (!d_Z || !d_Rows))) return fail(c, SOCP_ERR_ARG, "fd_rows: null argument");
    if (np == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, run_fdrows(c, np, d_Z, fd_eps(epsfcn), d_Rows));
    return SOCP_OK;
}

int socp_fd_diff_dev(socp_ctx *c, int np, const double *d_Z, double epsfcn, const double *d_Rows, double *d_Fjac)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "fd_diff: no problem set");
    if (np < 0 || (np > 0 && (!d_Z || !d_Rows || !d_Fjac))) return fail(c, SOCP_ERR_ARG, "fd_diff: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_launch += 1;
    HIP_TRY(c, fd_diff(c->stream, c->n, np, d_Z, fd_eps(epsfcn), d_Rows, d_Fjac));
    return SOCP_OK;
}

int socp_fd_rows(socp_ctx *c, int np, const double *Z, double epsfcn, double *Rows)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "fd_rows: no problem set");
    if (np < 0 || (np > 0 && (!Z || !Rows))) return fail(c, SOCP_ERR_ARG, "fd_rows: null argument");
    if (np == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = c->n, nR = n * (n + 1) * np;
    double *d_Z;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * nR));
    HIP_TRY(c, stage_up(c, c->s_in, Z, n * np, d_Z));
    int rc = socp_fd_rows_dev(c, np, d_Z, epsfcn, c->s_out.as<double>());
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, Rows, c->s_out.as<double>(), nR));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_fd_jacobian(socp_ctx *c, const double *z, const double *fvec, double epsfcn, double *fjac, int dedup)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "fd_jacobian: no problem set");
    if (!z || !fvec || !fjac) return fail(c, SOCP_ERR_ARG, "fd_jacobian: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = c->n;
    double *d_z, *d_fvec;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * n * n));
    HIP_TRY(c, stage_up(c, c->s_in, z, n, d_z));
    HIP_TRY(c, stage_up(c, c->s_aux, fvec, n, d_fvec));
    int rc = socp_fd_jacobian_dev(c, d_z, d_fvec, epsfcn, c->s_out.as<double>(), dedup);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, fjac, c->s_out.as<double>(), n * n));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_register_model(int model_id, const void *table, int table_bytes)
{
    if (model_id < SOCP_PLUGIN_ID_MIN) return fail(nullptr, SOCP_ERR_ARG, "register_model: ids below 100 are reserved for in-tree models");
    if (!table || table_bytes != (int)sizeof(ModelLaunchers)) return fail(nullptr, SOCP_ERR_ARG, "register_model: launch table size mismatch (plugin built against other headers)");
    const ModelLaunchers *t = static_cast<const ModelLaunchers *>(table);
    if (t->abi != kPluginAbi || t->dim < 1 || 2 * t->dim > 64 || t->nparams < 0 || t->nparams > kMaxParams || t->default_step_nbr < 1 ||
        !t->traj || !t->residual || !t->fdjac || !t->fdrows || !t->dense || !t->eval)
        return fail(nullptr, SOCP_ERR_ARG, "register_model: malformed launch table");
    std::lock_guard<std::mutex> guard(plugins_lock());
    plugins()[model_id] = *t;
    return SOCP_OK;
}

int socp_plugin_load(const char *path)
{
    if (!path) return fail(nullptr, SOCP_ERR_ARG, "plugin_load: null path");
    void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(nullptr, SOCP_ERR_ARG, std::string("plugin_load: ") + dlerror());
    typedef int (*reg_fn)(void);
    reg_fn reg = reinterpret_cast<reg_fn>(dlsym(h, "socp_plugin_register"));
    if (!reg) { dlclose(h); return fail(nullptr, SOCP_ERR_ARG, "plugin_load: socp_plugin_register not exported"); }
    return reg();        // the handle stays open: the kernels live in it
}

int socp_var_jacobian_multi_dev(socp_ctx *c, int np, const double *d_Z, double *d_Fjac)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "var_jacobian: no problem set");
    if (np < 0 || (np > 0 && (!d_Z || !d_Fjac))) return fail(c, SOCP_ERR_ARG, "var_jacobian: null argument");
    if (!has_var(c))
        return fail(c, SOCP_ERR_UNSUPPORTED, "var_jacobian: this model has no variational equations (modelOrder 0)");
    if (np == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->s_var.reserve(sizeof(double) * var_work_doubles(c, np)));
    HIP_TRY(c, run_var_jacobian(c, np, d_Z, c->s_var.as<double>(), d_Fjac));
    return SOCP_OK;
}

int socp_var_jacobian(socp_ctx *c, const double *z, double *fjac)
{
    if (!c) return SOCP_ERR_ARG;
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, "var_jacobian: no problem set");
    if (!z || !fjac) return fail(c, SOCP_ERR_ARG, "var_jacobian: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = c->n;
    double *d_z;
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * n * n));
    HIP_TRY(c, stage_up(c, c->s_in, z, n, d_z));
    if (int rc = socp_var_jacobian_multi_dev(c, 1, d_z, c->s_out.as<double>())) return rc;
    HIP_TRY(c, copy_down(c, fjac, c->s_out.as<double>(), n * n));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

/* ---- batched tangent ----------------------------------------------------------------------- */

namespace {
// the workspace of socp_tangent_batch_dev, in doubles from its start: block rows, replicated unknowns and residual rows of the
// R = B (K + 1) launched rows, the Jacobians, the steps; then what the variational Jacobian integrates in (models that have one)
struct TangentWork {
    size_t params, time, xnode, Z, F, J, h, var, total;
};

TangentWork tangent_layout(const socp_ctx *c, int B, int K)
{
    const size_t R = (size_t)B * (K + 1), nodes = (size_t)c->M + 1, n = c->n;
    TangentWork w{};
    size_t at = 0;
    auto take = [&](size_t count) { const size_t here = at; at += (count + 1) & ~(size_t)1; return here; };      // 16-byte aligned pieces
    w.params = take(R * (c->nparams + 2));
    w.time = take(R * nodes);
    w.xnode = take(R * nodes * c->S);
    w.Z = take(R * n);
    w.F = take(R * n);
    w.J = take((size_t)B * n * n);
    w.h = take((size_t)B * K);
    w.var = take(has_var(c) ? var_work_doubles(c, B) : 0);
    w.total = at;
    return w;
}

// the K directions checked against the problem's ranges and copied as they travel to the kernel (the host arrays are read here)
int direction_args(socp_ctx *c, const std::string &w, int K, const int *dir_kind, const int *dir_index, TangentDirs *dirs)
{
    for (int k = 0; k < K; k++) {
        const int kind = dir_kind[k], index = dir_index[k];
        int range = -1;
        if (kind == SOCP_DIR_PARAM) range = c->nparams + 2;
        else if (kind == SOCP_DIR_TIME) range = c->M + 1;
        else if (kind == SOCP_DIR_XNODE) range = (c->M + 1) * c->S;
        if (range < 0) return fail(c, SOCP_ERR_ARG, w + ": direction " + std::to_string(k) + " has kind " + std::to_string(kind) + " (0 .. 2)");
        // only the first d entries of a node's row are boundary values the residual reads
        if (index < 0 || index >= range || (kind == SOCP_DIR_XNODE && index % c->S >= c->dim))
            return fail(c, SOCP_ERR_ARG, w + ": direction " + std::to_string(k) + " has index " + std::to_string(index) + " outside its range");
        dirs->kind[k] = kind; dirs->index[k] = index;
    }
    for (int k = K; k < kMaxTangentDirs; k++) dirs->kind[k] = dirs->index[k] = -1;
    return SOCP_OK;
}

int tangent_args(socp_ctx *c, const char *who, int B, int K, const int *dir_kind, const int *dir_index, int jac, TangentDirs *dirs)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (K < 1 || K > kMaxTangentDirs) return fail(c, SOCP_ERR_ARG, w + ": 1 <= K <= 16 directions are required");
    if (!dir_kind || !dir_index) return fail(c, SOCP_ERR_ARG, w + ": null direction table");
    if (jac != 0 && jac != 1) return fail(c, SOCP_ERR_ARG, w + ": jac must be 0 (forward differences) or 1 (variational)");
    if (const int rc = direction_args(c, w, K, dir_kind, dir_index, dirs)) return rc;
    if (jac == 1 && !has_var(c))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": this model has no variational equations (modelOrder 0): jac = 1 needs them");
    return SOCP_OK;
}
}  // namespace

size_t socp_tangent_work_bytes(const socp_ctx *c, int B, int K)
{
    if (!c || !c->has_problem || B < 0 || K < 1 || K > kMaxTangentDirs) return 0;
    return sizeof(double) * tangent_layout(c, B, K).total;
}

int socp_linsolve_batch_dev(socp_ctx *c, int B, int n, int K, double *d_A, double *d_Y, int *d_info)
{
    if (!c) return SOCP_ERR_ARG;
    if (B < 0 || n < 1 || K < 1) return fail(c, SOCP_ERR_ARG, "linsolve_batch: B >= 0, n >= 1 and K >= 1 are required");
    if (!linsolve_fits(n, K))
        return fail(c, SOCP_ERR_ARG, "linsolve_batch: a pivot row and a multiplier column (2 n + K doubles; n <= 16: of four problems) must fit 64 KiB of LDS");
    if (B > 0 && (!d_A || !d_Y || !d_info)) return fail(c, SOCP_ERR_ARG, "linsolve_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_launch += 1;
    HIP_TRY(c, (c->variant == SOCP_VARIANT_LANE_FAST ? linsolve_fast : linsolve)(c->stream, B, n, K, d_A, d_Y, d_info));
    return SOCP_OK;
}

int socp_tangent_batch_dev(socp_ctx *c, int B, const double *d_Z, int K, const int *dir_kind, const int *dir_index, double epsfcn, int jac,
                           void *d_work, size_t work_bytes, double *d_dZ, int *d_info, double *d_Fp)
{
    if (!c) return SOCP_ERR_ARG;
    TangentDirs dirs;
    const int rc = tangent_args(c, "tangent_batch", B, K, dir_kind, dir_index, jac, &dirs);
    if (rc != SOCP_OK) return rc;
    if (B > 0 && (!d_Z || !d_work || !d_dZ || !d_info)) return fail(c, SOCP_ERR_ARG, "tangent_batch: null argument");
    if (B == 0) return SOCP_OK;
    const TangentWork w = tangent_layout(c, B, K);
    if (work_bytes < sizeof(double) * w.total) return fail(c, SOCP_ERR_ARG, "tangent_batch: the workspace is smaller than socp_tangent_work_bytes");
    // the elimination stages a pivot row and a multiplier column in LDS when the matrix does not fit there
    if (!linsolve_fits(c->n, K))
        return fail(c, SOCP_ERR_UNSUPPORTED, "tangent_batch: too many unknowns for the batched linear solve (2 n + K doubles must fit 64 KiB of LDS)");
    HIP_TRY(c, hipSetDevice(c->device));
    const bool fast = c->variant == SOCP_VARIANT_LANE_FAST;
    double *wk = static_cast<double *>(d_work);
    double *wP = wk + w.params, *wT = wk + w.time, *wX = wk + w.xnode, *wZ = wk + w.Z, *wF = wk + w.F, *wJ = wk + w.J, *wH = wk + w.h;
    const int R = B * (K + 1);
    // launch 1: the block rows (row kk B + b: direction kk - 1 of row b; kk = 0 its own block), the replicated unknowns, the steps
    c->n_launch += 1;
    HIP_TRY(c, (fast ? tangent_expand_fast : tangent_expand)(c->stream, c->P, c->pb, c->nparams, B, K, dirs, fd_eps(epsfcn), d_Z, wP, wT, wX, wZ, wH));
    // launch 2: F0 and every Fk, each row with its own block.  A smooth-law promise (or, with shared parameters, the context's own
    // mu2 > 0) covers the moved blocks: a moved mu2 is mu2 + e |mu2|
    {
        BlocksGuard guard(c);
        const int smooth = c->pb.pp_params ? c->pb.pp_smooth : (c->model_id == SOCP_MODEL_GODDARD && c->P.p[6] > 0 ? 1 : 0);
        c->pb.pp_params = wP; c->pb.pp_stride = c->nparams + 2; c->pb.pp_time = wT; c->pb.pp_xnode = wX; c->pb.pp_smooth = smooth;
        HIP_TRY(c, run_residual(c, R, wZ, wF));
    }
    // launch 3: the Jacobian at (z, F0) with the row's own blocks (rows 0 .. B-1 of F are the base rows)
    if (jac == 0) {
        const int r = socp_fd_jacobian_multi_dev(c, B, d_Z, wF, epsfcn, wJ, 1);
        if (r != SOCP_OK) return r;
    } else {
        HIP_TRY(c, run_var_jacobian(c, B, d_Z, wk + w.var, wJ));
    }
    // launches 4, 5: -G into dZ, G into Fp; J x = -G in place
    c->n_launch += 2;
    HIP_TRY(c, (fast ? tangent_diff_fast : tangent_diff)(c->stream, B, K, c->n, wF, wH, d_dZ, d_Fp));
    HIP_TRY(c, (fast ? linsolve_fast : linsolve)(c->stream, B, c->n, K, wJ, d_dZ, d_info));
    return SOCP_OK;
}

int socp_tangent_batch(socp_ctx *c, int B, const double *Z, int K, const int *dir_kind, const int *dir_index, double epsfcn, int jac,
                       double *dZ, int *info, double *Fp)
{
    if (!c) return SOCP_ERR_ARG;
    TangentDirs dirs;
    const int rc0 = tangent_args(c, "tangent_batch", B, K, dir_kind, dir_index, jac, &dirs);
    if (rc0 != SOCP_OK) return rc0;
    if (B > 0 && (!Z || !dZ || !info)) return fail(c, SOCP_ERR_ARG, "tangent_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nZ = (size_t)B * c->n, nD = (size_t)B * K * c->n, nF = Fp ? nD : 0, bytes = socp_tangent_work_bytes(c, B, K);
    double *d_Z;
    HIP_TRY(c, c->s_var.reserve(bytes));
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (nD + nF) + sizeof(int) * (size_t)B));
    double *dD = c->s_out.as<double>(), *dF = dD + nD;
    int *dI = reinterpret_cast<int *>(dF + nF);
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, d_Z));
    const int rc = socp_tangent_batch_dev(c, B, d_Z, K, dir_kind, dir_index, epsfcn, jac, c->s_var.p, bytes, dD, dI, Fp ? dF : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, dZ, dD, nD));
    if (Fp) HIP_TRY(c, copy_down(c, Fp, dF, nF));
    HIP_TRY(c, copy_down(c, info, dI, (size_t)B));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_tangent_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                              const double *xnode, int K, const int *dir_kind, const int *dir_index, double epsfcn, int jac, double *dZ,
                              int *info, double *Fp)
{
    if (!c) return SOCP_ERR_ARG;
    TangentDirs dirs;
    const int rc0 = tangent_args(c, "tangent_batch_blocks", B, K, dir_kind, dir_index, jac, &dirs);
    if (rc0 != SOCP_OK) return rc0;
    if (const int rc = blocks_stride(c, "tangent_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !dZ || !info)) return fail(c, SOCP_ERR_ARG, "tangent_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_tangent_batch(c, B, Z, K, dir_kind, dir_index, epsfcn, jac, dZ, info, Fp); });
}

/* ---- batched singular values ----------------------------------------------------------------- */

namespace {
// the workspace of socp_singular_batch_dev, in doubles from its start: the residual rows, the Jacobians (scaled in place), then what
// the variational Jacobian integrates in (models that have one)
struct SingularWork {
    size_t F, J, var, total;
};

SingularWork singular_layout(const socp_ctx *c, int B)
{
    const size_t n = c->n;
    SingularWork w{};
    size_t at = 0;
    auto take = [&](size_t count) { const size_t here = at; at += (count + 1) & ~(size_t)1; return here; };      // 16-byte aligned pieces
    w.F = take((size_t)B * n);
    w.J = take((size_t)B * n * n);
    w.var = take(has_var(c) ? var_work_doubles(c, B) : 0);
    w.total = at;
    return w;
}

bool svd_sweeps_ok(int max_sweeps) { return max_sweeps >= 1 && max_sweeps <= 1000; }

int singular_args(socp_ctx *c, const char *who, int B, int jac, int scale, int max_sweeps)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (jac != 0 && jac != 1) return fail(c, SOCP_ERR_ARG, w + ": jac must be 0 (forward differences) or 1 (variational)");
    if (scale != 0 && scale != 1) return fail(c, SOCP_ERR_ARG, w + ": scale must be 0 (J as it is) or 1 (columns of unit norm)");
    if (!svd_sweeps_ok(max_sweeps)) return fail(c, SOCP_ERR_ARG, w + ": 1 <= max_sweeps <= 1000 is required");
    if (jac == 1 && !has_var(c))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": this model has no variational equations (modelOrder 0): jac = 1 needs them");
    if (!svd_fits(c->n))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": too many unknowns for the batched singular values (n <= " + std::to_string(kSvdMaxN) + ": the matrix must fit 160 KiB of LDS)");
    return SOCP_OK;
}
}  // namespace

int socp_svd_batch_dev(socp_ctx *c, int B, int n, const double *d_A, int max_sweeps, double *d_sigma, double *d_Vt, int *d_sweeps,
                       int *d_info)
{
    if (!c) return SOCP_ERR_ARG;
    if (B < 0 || n < 1 || !svd_sweeps_ok(max_sweeps))
        return fail(c, SOCP_ERR_ARG, "svd_batch: B >= 0, n >= 1 and 1 <= max_sweeps <= 1000 are required");
    if (B > 0 && (!d_A || !d_sigma || !d_sweeps || !d_info)) return fail(c, SOCP_ERR_ARG, "svd_batch: null argument");
    if (!svd_fits(n))
        return fail(c, SOCP_ERR_UNSUPPORTED, "svd_batch: n <= " + std::to_string(kSvdMaxN) + " is required (the matrix must fit 160 KiB of LDS)");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->n_launch += 1;
    HIP_TRY(c, (c->variant == SOCP_VARIANT_LANE_FAST ? svd_fast : svd)(c->stream, B, n, d_A, max_sweeps, d_Vt ? 1 : 0, d_sigma, d_Vt, d_sweeps,
                                                                       d_info));
    return SOCP_OK;
}

size_t socp_singular_work_bytes(const socp_ctx *c, int B)
{
    if (!c || !c->has_problem || B < 0) return 0;
    return sizeof(double) * singular_layout(c, B).total;
}

int socp_singular_batch_dev(socp_ctx *c, int B, const double *d_Z, double epsfcn, int jac, int scale, int max_sweeps, void *d_work,
                            size_t work_bytes, double *d_sigma, double *d_vmin, double *d_colnorm, int *d_sweeps, int *d_info)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc = singular_args(c, "singular_batch", B, jac, scale, max_sweeps);
    if (rc != SOCP_OK) return rc;
    if (B > 0 && (!d_Z || !d_work || !d_sigma || !d_vmin || !d_sweeps || !d_info)) return fail(c, SOCP_ERR_ARG, "singular_batch: null argument");
    if (B == 0) return SOCP_OK;
    const SingularWork w = singular_layout(c, B);
    if (work_bytes < sizeof(double) * w.total) return fail(c, SOCP_ERR_ARG, "singular_batch: the workspace is smaller than socp_singular_work_bytes");
    HIP_TRY(c, hipSetDevice(c->device));
    const bool fast = c->variant == SOCP_VARIANT_LANE_FAST;
    double *wk = static_cast<double *>(d_work), *wF = wk + w.F, *wJ = wk + w.J;
    // launch 1: F0; then the Jacobian at (z, F0) (1 launch, variational: 3), each row with its own blocks
    HIP_TRY(c, run_residual(c, B, d_Z, wF));
    if (jac == 0) {
        const int r = socp_fd_jacobian_multi_dev(c, B, d_Z, wF, epsfcn, wJ, 1);
        if (r != SOCP_OK) return r;
    } else {
        HIP_TRY(c, run_var_jacobian(c, B, d_Z, wk + w.var, wJ));
    }
    // the column norms (only when something is to be scaled or reported), then the decomposition
    if (scale || d_colnorm) {
        c->n_launch += 1;
        HIP_TRY(c, (fast ? svd_colscale_fast : svd_colscale)(c->stream, B, c->n, scale, wJ, d_colnorm));
    }
    c->n_launch += 1;
    HIP_TRY(c, (fast ? svd_fast : svd)(c->stream, B, c->n, wJ, max_sweeps, 2, d_sigma, d_vmin, d_sweeps, d_info));
    return SOCP_OK;
}

int socp_singular_batch(socp_ctx *c, int B, const double *Z, double epsfcn, int jac, int scale, int max_sweeps, double *sigma, double *vmin,
                        double *colnorm, int *sweeps, int *info)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc0 = singular_args(c, "singular_batch", B, jac, scale, max_sweeps);
    if (rc0 != SOCP_OK) return rc0;
    if (B > 0 && (!Z || !sigma || !vmin || !sweeps || !info)) return fail(c, SOCP_ERR_ARG, "singular_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nZ = (size_t)B * c->n, nC = colnorm ? nZ : 0, bytes = socp_singular_work_bytes(c, B);
    double *d_Z;
    HIP_TRY(c, c->s_var.reserve(bytes));
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (2 * nZ + nC) + sizeof(int) * 2 * (size_t)B));
    double *dS = c->s_out.as<double>(), *dV = dS + nZ, *dC = dV + nZ;
    int *dW = reinterpret_cast<int *>(dC + nC), *dI = dW + B;
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, d_Z));
    const int rc = socp_singular_batch_dev(c, B, d_Z, epsfcn, jac, scale, max_sweeps, c->s_var.p, bytes, dS, dV, colnorm ? dC : nullptr, dW, dI);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, sigma, dS, nZ));
    HIP_TRY(c, copy_down(c, vmin, dV, nZ));
    if (colnorm) HIP_TRY(c, copy_down(c, colnorm, dC, nC));
    HIP_TRY(c, copy_down(c, sweeps, dW, (size_t)B));
    HIP_TRY(c, copy_down(c, info, dI, (size_t)B));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_singular_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                               const double *xnode, double epsfcn, int jac, int scale, int max_sweeps, double *sigma, double *vmin,
                               double *colnorm, int *sweeps, int *info)
{
    if (!c) return SOCP_ERR_ARG;
    const int rc0 = singular_args(c, "singular_batch_blocks", B, jac, scale, max_sweeps);
    if (rc0 != SOCP_OK) return rc0;
    if (const int rc = blocks_stride(c, "singular_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !sigma || !vmin || !sweeps || !info)) return fail(c, SOCP_ERR_ARG, "singular_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_singular_batch(c, B, Z, epsfcn, jac, scale, max_sweeps, sigma, vmin, colnorm, sweeps, info); });
}

/* ---- batched branch following ---------------------------------------------------------------- */

namespace {
constexpr int kBranchChunk = 8;       // rounds the host forms enqueue between two read-backs of the "unfinished rows" word

// the workspace of socp_branch_batch_dev, in doubles from its start: block rows, unknowns and residual rows of the 2B launched rows,
// the Jacobians, the bordered matrices, the right-hand sides, the row state (BranchState; the int pieces take whole doubles), then
// what the variational Jacobian integrates in (models that have one)
struct BranchWork {
    size_t params, time, xnode, Z, F, J, Mx, rhs, v, y, t, h, hth, rn, k, kase, info, live, var, total;
};

BranchWork branch_layout(const socp_ctx *c, int B)
{
    const size_t R = 2 * (size_t)B, nodes = (size_t)c->M + 1, n = c->n, n1 = n + 1, ints = ((size_t)B + 1) / 2;
    BranchWork w{};
    size_t at = 0;
    auto take = [&](size_t count) { const size_t here = at; at += (count + 1) & ~(size_t)1; return here; };      // 16-byte aligned pieces
    w.params = take(R * (c->nparams + 2));
    w.time = take(R * nodes);
    w.xnode = take(R * nodes * c->S);
    w.Z = take(R * n);
    w.F = take(R * n);
    w.J = take((size_t)B * n * n);
    w.Mx = take((size_t)B * n1 * n1);
    w.rhs = take((size_t)B * n1);
    w.v = take((size_t)B * n1);
    w.y = take((size_t)B * n1);
    w.t = take((size_t)B * n1);
    w.h = take(B);
    w.hth = take(B);
    w.rn = take(B);
    w.k = take(ints);
    w.kase = take(ints);
    w.info = take(ints);
    w.live = take(2);
    w.var = take(has_var(c) ? var_work_doubles(c, B) : 0);
    w.total = at;
    return w;
}

// the refusals all three forms share; *A: the direction and the options as they travel to the kernels
int branch_args(socp_ctx *c, const char *who, int B, int kind, int index, const socp_branch_options *o, BranchArgs *A)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (!o) return fail(c, SOCP_ERR_ARG, w + ": null options");
    TangentDirs dirs;
    if (const int rc = direction_args(c, w, 1, &kind, &index, &dirs)) return rc;
    if (o->jac != 0 && o->jac != 1) return fail(c, SOCP_ERR_ARG, w + ": jac must be 0 (forward differences) or 1 (variational)");
    if (!(o->wtheta > 0.0) || !std::isfinite(o->wtheta)) return fail(c, SOCP_ERR_ARG, w + ": wtheta must be positive and finite");
    if (o->dir != 1 && o->dir != -1) return fail(c, SOCP_ERR_ARG, w + ": dir must be +1 or -1");
    if (!(0.0 < o->hmin && o->hmin <= o->h0 && o->h0 <= o->hmax) || !std::isfinite(o->hmax))
        return fail(c, SOCP_ERR_ARG, w + ": 0 < hmin <= h0 <= hmax (finite) is required");
    if (!(o->grow >= 1.0) || !std::isfinite(o->grow)) return fail(c, SOCP_ERR_ARG, w + ": grow >= 1 (finite) is required");
    if (o->max_corr < 1 || o->kfast < 0) return fail(c, SOCP_ERR_ARG, w + ": max_corr >= 1 and kfast >= 0 are required");
    if (!(o->ftol > 0.0)) return fail(c, SOCP_ERR_ARG, w + ": ftol > 0 is required");
    if (o->cap < 2 || o->rounds < 1) return fail(c, SOCP_ERR_ARG, w + ": cap >= 2 and rounds >= 1 are required");
    if (o->jac == 1 && !has_var(c))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": this model has no variational equations (modelOrder 0): jac = 1 needs them");
    if (!linsolve_fits(c->n + 1, 1))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": too many unknowns for the batched linear solve (2 (n + 1) + 1 doubles must fit 64 KiB of LDS)");
    A->kind = kind; A->index = index; A->dir = o->dir; A->kfast = o->kfast; A->max_corr = o->max_corr; A->have_goal = o->have_goal ? 1 : 0;
    A->cap = o->cap; A->e = fd_eps(o->epsfcn); A->wtheta = o->wtheta; A->h0 = o->h0; A->hmin = o->hmin; A->hmax = o->hmax; A->grow = o->grow;
    A->ftol = o->ftol; A->goal = o->goal;
    return SOCP_OK;
}

// rounds [from, to) of a checked call, enqueued on the context's stream; d_live: where the update leaves the number of unfinished rows
int branch_rounds(socp_ctx *c, int B, const double *d_Z, const BranchArgs &A, double epsfcn, int jac, void *d_work, const BranchOut &O,
                  int from, int to, const int **d_live)
{
    const BranchWork w = branch_layout(c, B);
    double *wk = static_cast<double *>(d_work);
    double *wP = wk + w.params, *wT = wk + w.time, *wX = wk + w.xnode, *wZ = wk + w.Z, *wF = wk + w.F, *wJ = wk + w.J, *wM = wk + w.Mx, *wR = wk + w.rhs;
    BranchState S;
    S.v = wk + w.v; S.y = wk + w.y; S.t = wk + w.t; S.h = wk + w.h; S.hth = wk + w.hth; S.rn = wk + w.rn;
    S.k = reinterpret_cast<int *>(wk + w.k); S.kase = reinterpret_cast<int *>(wk + w.kase); S.info = reinterpret_cast<int *>(wk + w.info);
    S.live = reinterpret_cast<int *>(wk + w.live);
    if (d_live) *d_live = S.live;
    const int n = c->n;
    for (int round = from; round < to; round++) {
        const int first = round == 0;
        // launch 1: the block rows of the evaluation points (theta, theta + h_theta) and their unknowns; the first round sets the state
        c->n_launch += 1;
        HIP_TRY(c, branch_expand(c->stream, c->P, c->pb, c->nparams, B, A, first, d_Z, S, O, wP, wT, wX, wZ));
        {
            // F0, F1 and the Jacobian at (v_z, F0) under the SAME expanded blocks.  A smooth-law promise covers them unless mu2 itself moves
            BlocksGuard guard(c);
            int smooth = c->pb.pp_params ? c->pb.pp_smooth : (c->model_id == SOCP_MODEL_GODDARD && c->P.p[6] > 0 ? 1 : 0);
            if (c->model_id == SOCP_MODEL_GODDARD && A.kind == SOCP_DIR_PARAM && A.index == 6) smooth = 0;
            c->pb.pp_params = wP; c->pb.pp_stride = c->nparams + 2; c->pb.pp_time = wT; c->pb.pp_xnode = wX; c->pb.pp_smooth = smooth;
            HIP_TRY(c, run_residual(c, 2 * B, wZ, wF));
            if (jac == 0) {
                const int r = socp_fd_jacobian_multi_dev(c, B, wZ, wF, epsfcn, wJ, 1);
                if (r != SOCP_OK) return r;
            } else {
                HIP_TRY(c, run_var_jacobian(c, B, wZ, wk + w.var, wJ));
            }
        }
        // the row's case, the bordered matrix and its right-hand side; the elimination; the transitions
        c->n_launch += 3;
        HIP_TRY(c, branch_assemble(c->stream, B, n, A, first, wF, wJ, S, O.status, wM, wR));
        HIP_TRY(c, linsolve(c->stream, B, n + 1, 1, wM, wR, S.info));      // reference order in both flavours
        HIP_TRY(c, branch_update(c->stream, B, n, A, S, O, wR));
    }
    return SOCP_OK;
}
}  // namespace

size_t socp_branch_work_bytes(const socp_ctx *c, int B)
{
    if (!c || !c->has_problem || B < 0) return 0;
    return sizeof(double) * branch_layout(c, B).total;
}

int socp_branch_batch_dev(socp_ctx *c, int B, const double *d_Z, int dir_kind, int dir_index, const socp_branch_options *opt, void *d_work,
                          size_t work_bytes, double *d_Y, double *d_ttheta, double *d_rnorm, int *d_count, int *d_nfold, int *d_ifold,
                          int *d_status, int *d_nreject, double *d_hlast, double *d_zgoal)
{
    if (!c) return SOCP_ERR_ARG;
    BranchArgs A;
    const int rc = branch_args(c, "branch_batch", B, dir_kind, dir_index, opt, &A);
    if (rc != SOCP_OK) return rc;
    if (B > 0 && (!d_Z || !d_work || !d_Y || !d_ttheta || !d_rnorm || !d_count || !d_nfold || !d_ifold || !d_status || !d_nreject || !d_hlast))
        return fail(c, SOCP_ERR_ARG, "branch_batch: null argument");
    if (B == 0) return SOCP_OK;
    if (work_bytes < socp_branch_work_bytes(c, B)) return fail(c, SOCP_ERR_ARG, "branch_batch: the workspace is smaller than socp_branch_work_bytes");
    HIP_TRY(c, hipSetDevice(c->device));
    const BranchOut O{d_Y, d_ttheta, d_rnorm, d_count, d_nfold, d_ifold, d_status, d_nreject, d_hlast, d_zgoal};
    return branch_rounds(c, B, d_Z, A, opt->epsfcn, opt->jac, d_work, O, 0, opt->rounds, nullptr);
}

int socp_branch_batch(socp_ctx *c, int B, const double *Z, int dir_kind, int dir_index, const socp_branch_options *opt, double *Y,
                      double *ttheta, double *rnorm, int *count, int *nfold, int *ifold, int *status, int *nreject, double *hlast, double *zgoal)
{
    if (!c) return SOCP_ERR_ARG;
    BranchArgs A;
    const int rc0 = branch_args(c, "branch_batch", B, dir_kind, dir_index, opt, &A);
    if (rc0 != SOCP_OK) return rc0;
    if (B > 0 && (!Z || !Y || !ttheta || !rnorm || !count || !nfold || !ifold || !status || !nreject || !hlast))
        return fail(c, SOCP_ERR_ARG, "branch_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = c->n, nZ = (size_t)B * n, nC = (size_t)B * opt->cap, nY = nC * (n + 1), nG = zgoal ? nZ : 0;
    const size_t bytes = socp_branch_work_bytes(c, B);
    double *d_Z;
    HIP_TRY(c, c->s_var.reserve(bytes));
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (nY + 2 * nC + (size_t)B + nG) + sizeof(int) * 5 * (size_t)B));
    double *dY = c->s_out.as<double>(), *dT = dY + nY, *dR = dT + nC, *dH = dR + nC, *dG = dH + B;
    int *dI = reinterpret_cast<int *>(dG + nG);                   // count, nfold, ifold, status, nreject: B each
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, d_Z));
    const BranchOut O{dY, dT, dR, dI, dI + B, dI + 2 * (size_t)B, dI + 3 * (size_t)B, dI + 4 * (size_t)B, dH, zgoal ? dG : nullptr};
    // chunks of rounds; between two chunks the number of unfinished rows comes back: 0 ends the call (a finished row changes nothing)
    for (int from = 0; from < opt->rounds; from += kBranchChunk) {
        const int to = from + kBranchChunk < opt->rounds ? from + kBranchChunk : opt->rounds;
        const int *d_live = nullptr;
        const int rc = branch_rounds(c, B, d_Z, A, opt->epsfcn, opt->jac, c->s_var.p, O, from, to, &d_live);
        if (rc != SOCP_OK) return rc;
        if (to == opt->rounds) break;
        int live = 0;
        HIP_TRY(c, copy_down(c, &live, d_live, 1));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (live == 0) break;
    }
    HIP_TRY(c, copy_down(c, Y, dY, nY));
    HIP_TRY(c, copy_down(c, ttheta, dT, nC));
    HIP_TRY(c, copy_down(c, rnorm, dR, nC));
    HIP_TRY(c, copy_down(c, hlast, dH, (size_t)B));
    if (zgoal) HIP_TRY(c, copy_down(c, zgoal, dG, nG));
    HIP_TRY(c, copy_down(c, count, O.count, (size_t)B));
    HIP_TRY(c, copy_down(c, nfold, O.nfold, (size_t)B));
    HIP_TRY(c, copy_down(c, ifold, O.ifold, (size_t)B));
    HIP_TRY(c, copy_down(c, status, O.status, (size_t)B));
    HIP_TRY(c, copy_down(c, nreject, O.nreject, (size_t)B));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_branch_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time, const double *xnode,
                             int dir_kind, int dir_index, const socp_branch_options *opt, double *Y, double *ttheta, double *rnorm,
                             int *count, int *nfold, int *ifold, int *status, int *nreject, double *hlast, double *zgoal)
{
    if (!c) return SOCP_ERR_ARG;
    BranchArgs A;
    const int rc0 = branch_args(c, "branch_batch_blocks", B, dir_kind, dir_index, opt, &A);
    if (rc0 != SOCP_OK) return rc0;
    if (const int rc = blocks_stride(c, "branch_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !Y || !ttheta || !rnorm || !count || !nfold || !ifold || !status || !nreject || !hlast))
        return fail(c, SOCP_ERR_ARG, "branch_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode, [&] {
        return socp_branch_batch(c, B, Z, dir_kind, dir_index, opt, Y, ttheta, rnorm, count, nfold, ifold, status, nreject, hlast, zgoal);
    });
}

/* ---- batched Newton polish ------------------------------------------------------------------- */

namespace {
// the workspace of socp_newton_batch_dev, in doubles from its start: F0 by row; the compact slots' points, residuals, right-hand
// sides, block rows and Jacobians; the trial rows' points, residuals and block rows; the int pieces (whole doubles); then what the
// variational Jacobian integrates in (models that have one)
struct NewtonLayout {
    size_t F0, cZ, cF, cR, cP, cT, cX, J, tZ, tF, tP, tT, tX, list, info, bcount, live, var, total;
};

NewtonLayout newton_layout(const socp_ctx *c, int B, int trials)
{
    const size_t b = (size_t)B, R = b * trials, nodes = (size_t)c->M + 1, n = c->n, stride = (size_t)c->nparams + 2, ints = (b + 1) / 2;
    NewtonLayout w{};
    size_t at = 0;
    auto take = [&](size_t count) { const size_t here = at; at += (count + 1) & ~(size_t)1; return here; };      // 16-byte aligned pieces
    w.F0 = take(b * n);
    w.cZ = take(b * n);
    w.cF = take(b * n);
    w.cR = take(b * n);
    w.cP = take(b * stride);
    w.cT = take(b * nodes);
    w.cX = take(b * nodes * c->S);
    w.J = take(b * n * n);
    w.tZ = take(R * n);
    w.tF = take(R * n);
    w.tP = take(R * stride);
    w.tT = take(R * nodes);
    w.tX = take(R * nodes * c->S);
    w.list = take(ints);
    w.info = take(ints);
    w.bcount = take(((size_t)newton_scan_blocks(B) + 1) / 2);
    w.live = take(2);
    w.var = take(has_var(c) ? var_work_doubles(c, B) : 0);
    w.total = at;
    return w;
}

// the refusals all three forms share; *A: the options as they travel to the kernels
int newton_args(socp_ctx *c, const char *who, int B, const socp_newton_options *o, NewtonArgs *A)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (!o) return fail(c, SOCP_ERR_ARG, w + ": null options");
    if (o->jac < 0 || o->jac > 2) return fail(c, SOCP_ERR_ARG, w + ": jac must be 0 (forward differences), 1 (variational) or 2 (exact)");
    if (o->trials < 1 || o->trials > 8) return fail(c, SOCP_ERR_ARG, w + ": 1 <= trials <= 8 is required");
    if (o->rounds < 1) return fail(c, SOCP_ERR_ARG, w + ": rounds >= 1 is required");
    if (!(o->ftol > 0.0)) return fail(c, SOCP_ERR_ARG, w + ": ftol > 0 is required");
    if (!(o->xtol >= 0.0)) return fail(c, SOCP_ERR_ARG, w + ": xtol >= 0 is required");
    if (o->jac == 1 && !has_var(c))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": this model has no variational equations (modelOrder 0): jac = 1 needs them");
    if (o->jac == 2)
        if (const int rc = exact_jacobian_args(c, who, B)) return rc;
    if (!linsolve_fits(c->n, 1))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": too many unknowns for the batched linear solve (2 n + 1 doubles must fit 64 KiB of LDS)");
    A->trials = o->trials; A->rounds = o->rounds; A->ftol = o->ftol; A->xtol = o->xtol;
    return SOCP_OK;
}

NewtonWork newton_work(const socp_ctx *c, int B, int trials, void *d_work, double **J, double **var)
{
    const NewtonLayout w = newton_layout(c, B, trials);
    double *wk = static_cast<double *>(d_work);
    NewtonWork W;
    W.F0 = wk + w.F0; W.cZ = wk + w.cZ; W.cF = wk + w.cF; W.cR = wk + w.cR; W.cP = wk + w.cP; W.cT = wk + w.cT; W.cX = wk + w.cX;
    W.tZ = wk + w.tZ; W.tF = wk + w.tF; W.tP = wk + w.tP; W.tT = wk + w.tT; W.tX = wk + w.tX;
    W.list = reinterpret_cast<int *>(wk + w.list); W.info = reinterpret_cast<int *>(wk + w.info);
    W.bcount = reinterpret_cast<int *>(wk + w.bcount); W.live = reinterpret_cast<int *>(wk + w.live);
    *J = wk + w.J; *var = wk + w.var;
    return W;
}

// the start of a checked call: F0 = F(Z) with the rows' blocks, then every row's state and outputs
int newton_begin(socp_ctx *c, int B, const double *d_Z, const NewtonArgs &A, const NewtonWork &W, const NewtonOut &O)
{
    HIP_TRY(c, run_residual(c, B, d_Z, W.F0));
    c->n_launch += 1;
    HIP_TRY(c, newton_start(c->stream, c->pb, B, c->n, A, d_Z, W, O));
    return SOCP_OK;
}

// the compaction that begins a round: list and live
int newton_begin_round(socp_ctx *c, int B, const NewtonWork &W, const NewtonOut &O)
{
    c->n_launch += 3;
    HIP_TRY(c, newton_compact(c->stream, B, O.status, W));
    return SOCP_OK;
}

// the rest of a round on `slots` compact slots (the _dev form: B; the host forms: the live count they read back)
int newton_round(socp_ctx *c, int slots, const socp_newton_options *o, const NewtonArgs &A, const NewtonWork &W, const NewtonOut &O,
                 double *wJ, double *wVar)
{
    const int n = c->n;
    const ProblemDev own = c->pb;                                  // the rows' blocks: read by row, through the list
    c->n_launch += 1;
    HIP_TRY(c, newton_gather(c->stream, own, slots, n, W, O));
    {
        // the Jacobian at (y, F0) of the slots, each under its own block rows
        BlocksGuard guard(c);
        if (own.pp_params) c->pb.pp_params = W.cP;
        if (own.pp_time) c->pb.pp_time = W.cT;
        if (own.pp_xnode) c->pb.pp_xnode = W.cX;
        if (o->jac == 0) {
            const int r = socp_fd_jacobian_multi_dev(c, slots, W.cZ, W.cF, o->epsfcn, wJ, 1);
            if (r != SOCP_OK) return r;
        } else if (o->jac == 1) {
            HIP_TRY(c, run_var_jacobian(c, slots, W.cZ, wVar, wJ));
        } else {
            const int r = exact_jacobian_launch(c, slots, W.cZ, wJ, nullptr);
            if (r != SOCP_OK) return r;
        }
    }
    // J delta = -F0 in place (reference order in both flavours); the trial points
    c->n_launch += 2;
    HIP_TRY(c, linsolve(c->stream, slots, n, 1, wJ, W.cR, W.info));
    HIP_TRY(c, newton_trials(c->stream, own, slots, n, A.trials, W));
    {
        // ONE residual launch of slots x trials rows under the expanded block rows
        BlocksGuard guard(c);
        if (own.pp_params) c->pb.pp_params = W.tP;
        if (own.pp_time) c->pb.pp_time = W.tT;
        if (own.pp_xnode) c->pb.pp_xnode = W.tX;
        HIP_TRY(c, run_residual(c, slots * A.trials, W.tZ, W.tF));
    }
    c->n_launch += 1;
    HIP_TRY(c, newton_update(c->stream, slots, n, A, W, O));
    return SOCP_OK;
}
}  // namespace

size_t socp_newton_work_bytes(const socp_ctx *c, int B, const socp_newton_options *opt)
{
    if (!c || !c->has_problem || B < 0 || !opt || opt->trials < 1 || opt->trials > 8) return 0;
    return sizeof(double) * newton_layout(c, B, opt->trials).total;
}

int socp_newton_batch_dev(socp_ctx *c, int B, const double *d_Z, const socp_newton_options *opt, void *d_work, size_t work_bytes,
                          double *d_Zout, double *d_Fout, double *d_rnorm, double *d_dnorm, int *d_iters, int *d_nhalf, int *d_status,
                          double *d_rhist)
{
    if (!c) return SOCP_ERR_ARG;
    NewtonArgs A;
    const int rc = newton_args(c, "newton_batch", B, opt, &A);
    if (rc != SOCP_OK) return rc;
    if (B > 0 && (!d_Z || !d_work || !d_Zout || !d_rnorm || !d_dnorm || !d_iters || !d_nhalf || !d_status))
        return fail(c, SOCP_ERR_ARG, "newton_batch: null argument");
    if (B == 0) return SOCP_OK;
    if (work_bytes < socp_newton_work_bytes(c, B, opt)) return fail(c, SOCP_ERR_ARG, "newton_batch: the workspace is smaller than socp_newton_work_bytes");
    HIP_TRY(c, hipSetDevice(c->device));
    const NewtonOut O{d_Zout, d_Fout, d_rnorm, d_dnorm, d_iters, d_nhalf, d_status, d_rhist};
    double *wJ, *wVar;
    const NewtonWork W = newton_work(c, B, A.trials, d_work, &wJ, &wVar);
    if (const int r = newton_begin(c, B, d_Z, A, W, O)) return r;
    for (int round = 0; round < A.rounds; round++) {
        if (const int r = newton_begin_round(c, B, W, O)) return r;
        if (const int r = newton_round(c, B, opt, A, W, O, wJ, wVar)) return r;
    }
    return SOCP_OK;
}

int socp_newton_batch(socp_ctx *c, int B, const double *Z, const socp_newton_options *opt, double *Zout, double *Fout, double *rnorm,
                      double *dnorm, int *iters, int *nhalf, int *status, double *rhist)
{
    if (!c) return SOCP_ERR_ARG;
    NewtonArgs A;
    const int rc0 = newton_args(c, "newton_batch", B, opt, &A);
    if (rc0 != SOCP_OK) return rc0;
    if (B > 0 && (!Z || !Zout || !rnorm || !dnorm || !iters || !nhalf || !status)) return fail(c, SOCP_ERR_ARG, "newton_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nZ = (size_t)B * c->n, nF = Fout ? nZ : 0, nH = rhist ? (size_t)B * ((size_t)A.rounds + 1) : 0;
    const size_t bytes = socp_newton_work_bytes(c, B, opt);
    double *d_Z;
    HIP_TRY(c, c->s_var.reserve(bytes));
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (nZ + nF + 2 * (size_t)B + nH) + sizeof(int) * 3 * (size_t)B));
    double *dY = c->s_out.as<double>(), *dF = dY + nZ, *dR = dF + nF, *dD = dR + B, *dH = dD + B;
    int *dI = reinterpret_cast<int *>(dH + nH);                   // iters, nhalf, status: B each
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, d_Z));
    const NewtonOut O{dY, Fout ? dF : nullptr, dR, dD, dI, dI + B, dI + 2 * (size_t)B, rhist ? dH : nullptr};
    double *wJ, *wVar;
    const NewtonWork W = newton_work(c, B, A.trials, c->s_var.p, &wJ, &wVar);
    if (const int r = newton_begin(c, B, d_Z, A, W, O)) return r;
    // after every compaction the number of unfinished rows comes back: the round runs on that many slots, 0 ends the call
    for (int round = 0; round < A.rounds; round++) {
        if (const int r = newton_begin_round(c, B, W, O)) return r;
        int live = 0;
        HIP_TRY(c, copy_down(c, &live, W.live, 1));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (live <= 0) break;
        if (const int r = newton_round(c, live < B ? live : B, opt, A, W, O, wJ, wVar)) return r;
    }
    HIP_TRY(c, copy_down(c, Zout, dY, nZ));
    if (Fout) HIP_TRY(c, copy_down(c, Fout, dF, nF));
    HIP_TRY(c, copy_down(c, rnorm, dR, (size_t)B));
    HIP_TRY(c, copy_down(c, dnorm, dD, (size_t)B));
    if (rhist) HIP_TRY(c, copy_down(c, rhist, dH, nH));
    HIP_TRY(c, copy_down(c, iters, O.iters, (size_t)B));
    HIP_TRY(c, copy_down(c, nhalf, O.nhalf, (size_t)B));
    HIP_TRY(c, copy_down(c, status, O.status, (size_t)B));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_newton_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time, const double *xnode,
                             const socp_newton_options *opt, double *Zout, double *Fout, double *rnorm, double *dnorm, int *iters, int *nhalf,
                             int *status, double *rhist)
{
    if (!c) return SOCP_ERR_ARG;
    NewtonArgs A;
    const int rc0 = newton_args(c, "newton_batch_blocks", B, opt, &A);
    if (rc0 != SOCP_OK) return rc0;
    if (const int rc = blocks_stride(c, "newton_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !Zout || !rnorm || !dnorm || !iters || !nhalf || !status)) return fail(c, SOCP_ERR_ARG, "newton_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_newton_batch(c, B, Z, opt, Zout, Fout, rnorm, dnorm, iters, nhalf, status, rhist); });
}

/* ---- batched exact sensitivities ------------------------------------------------------------- */

int socp_ctx_has_sensitivity(const socp_ctx *c) { return c ? (table_of(c)->sensitivity ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
// the workspace of socp_sensitivity_batch_dev, in doubles from its start
struct SensitivityWork {
    size_t J, G, total;
};

SensitivityWork sensitivity_layout(const socp_ctx *c, int B, int K)
{
    const size_t n = c->n;
    SensitivityWork w{};
    w.J = 0;
    w.G = ((size_t)B * n * n + 1) & ~(size_t)1;
    w.total = w.G + (((size_t)B * K * n + 1) & ~(size_t)1);
    return w;
}

// the directions of a checked call as they travel to the kernels: the PARAM directions, the TIME directions on a FIXED node (the
// others read nothing), and the XNODE directions' mask and packed (node, component)
struct SensitivityPlan {
    SensDirs param, time;
    unsigned xnode_mask;
    unsigned long long xnode_index[4];
};

// the refusals all three forms share
int sensitivity_args(socp_ctx *c, const char *who, int B, int K, const int *dir_kind, const int *dir_index, SensitivityPlan *plan)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (K < 1 || K > kMaxTangentDirs) return fail(c, SOCP_ERR_ARG, w + ": 1 <= K <= 16 directions are required");
    if (!dir_kind || !dir_index) return fail(c, SOCP_ERR_ARG, w + ": null direction table");
    TangentDirs dirs;
    if (const int rc = direction_args(c, w, K, dir_kind, dir_index, &dirs)) return rc;
    for (int k = 0; k < K; k++)
        if (dirs.kind[k] == SOCP_DIR_PARAM && dirs.index[k] >= c->nparams)
            return fail(c, SOCP_ERR_ARG, w + ": direction " + std::to_string(k) + " addresses a switching time (slot " +
                                             std::to_string(dirs.index[k]) + " of the block): the discrete flow is piecewise constant in it");
    if (!table_of(c)->sensitivity)
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": this model's launch table has no sensitivity entry (a model whose rhs_t, hamiltonian_t and "
                                                 "switching_fn_t are not generic in the parameter view, or one with a switching_state hook, custom "
                                                 "final rows or its own ComputeTraj; rebuild a plugin written for an older launch table)");
    if (const int rc = exact_jacobian_args(c, who, B)) return rc;
    if (!linsolve_fits(c->n, K))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": too many unknowns for the batched linear solve (2 n + K doubles must fit 64 KiB of LDS)");
    SensitivityPlan p{};
    p.param.kind = kSensParam; p.time.kind = kSensTime;
    auto put = [](SensDirs &d, int k, int index) {
        d.slot |= (unsigned long long)k << (4 * d.n);
        d.index[d.n >> 2] |= (unsigned long long)index << (16 * (d.n & 3));
        d.n += 1;
    };
    for (int k = 0; k < K; k++) {
        const int index = dirs.index[k];
        if (dirs.kind[k] == SOCP_DIR_PARAM) put(p.param, k, index);
        else if (dirs.kind[k] == SOCP_DIR_TIME) {
            if (c->mode_t[index] == SOCP_FIXED) put(p.time, k, index);
        } else {
            p.xnode_mask |= 1u << k;
            p.xnode_index[k >> 2] |= (unsigned long long)(((index / c->S) << 5) | (index % c->S)) << (16 * (k & 3));
        }
    }
    *plan = p;
    return SOCP_OK;
}
}  // namespace

size_t socp_sensitivity_work_bytes(const socp_ctx *c, int B, int K)
{
    if (!c || !c->has_problem || B < 0 || K < 1 || K > kMaxTangentDirs) return 0;
    return sizeof(double) * sensitivity_layout(c, B, K).total;
}

int socp_sensitivity_batch_dev(socp_ctx *c, int B, const double *d_Z, int K, const int *dir_kind, const int *dir_index, void *d_work,
                               size_t work_bytes, double *d_dZ, int *d_info, double *d_Gp)
{
    if (!c) return SOCP_ERR_ARG;
    SensitivityPlan plan;
    const int rc = sensitivity_args(c, "sensitivity_batch", B, K, dir_kind, dir_index, &plan);
    if (rc != SOCP_OK) return rc;
    if (B > 0 && (!d_Z || !d_work || !d_dZ || !d_info)) return fail(c, SOCP_ERR_ARG, "sensitivity_batch: null argument");
    if (B == 0) return SOCP_OK;
    const SensitivityWork w = sensitivity_layout(c, B, K);
    if (work_bytes < sizeof(double) * w.total)
        return fail(c, SOCP_ERR_ARG, "sensitivity_batch: the workspace is smaller than socp_sensitivity_work_bytes");
    double *wk = static_cast<double *>(d_work);
    double *wJ = wk + w.J, *G = d_Gp ? d_Gp : wk + w.G;
    // J: the exact Jacobian's own launch
    if (const int r = exact_jacobian_launch(c, B, d_Z, wJ, nullptr)) return r;
    // G: zero-filled, then the integrating directions kind by kind
    HIP_TRY(c, hipMemsetAsync(G, 0, sizeof(double) * (size_t)B * K * c->n, c->stream));
    for (const SensDirs *d : {&plan.param, &plan.time}) {
        if (d->n == 0) continue;
        c->n_traj += (long long)B * c->M * d->n; c->n_launch += 1;
        HIP_TRY(c, table_of(c)->sensitivity(c->stream, c->P, c->pb, B, d_Z, *d, K, G));
    }
    // the XNODE directions' entries and rhs = -G into dZ; J x = rhs in place, in reference order in both flavours
    c->n_launch += 2;
    HIP_TRY(c, sensitivity_finish(c->stream, c->pb, B, K, plan.xnode_mask, plan.xnode_index, G, d_dZ));
    HIP_TRY(c, linsolve(c->stream, B, c->n, K, wJ, d_dZ, d_info));
    return SOCP_OK;
}

int socp_sensitivity_batch(socp_ctx *c, int B, const double *Z, int K, const int *dir_kind, const int *dir_index, double *dZ, int *info,
                           double *Gp)
{
    if (!c) return SOCP_ERR_ARG;
    SensitivityPlan plan;
    const int rc0 = sensitivity_args(c, "sensitivity_batch", B, K, dir_kind, dir_index, &plan);
    if (rc0 != SOCP_OK) return rc0;
    if (B > 0 && (!Z || !dZ || !info)) return fail(c, SOCP_ERR_ARG, "sensitivity_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nZ = (size_t)B * c->n, nD = (size_t)B * K * c->n, nG = Gp ? nD : 0, bytes = socp_sensitivity_work_bytes(c, B, K);
    double *d_Z;
    HIP_TRY(c, c->s_var.reserve(bytes));
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (nD + nG) + sizeof(int) * (size_t)B));
    double *dD = c->s_out.as<double>(), *dG = dD + nD;
    int *dI = reinterpret_cast<int *>(dG + nG);
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, d_Z));
    const int rc = socp_sensitivity_batch_dev(c, B, d_Z, K, dir_kind, dir_index, c->s_var.p, bytes, dD, dI, Gp ? dG : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, dZ, dD, nD));
    if (Gp) HIP_TRY(c, copy_down(c, Gp, dG, nG));
    HIP_TRY(c, copy_down(c, info, dI, (size_t)B));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_sensitivity_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                                  const double *xnode, int K, const int *dir_kind, const int *dir_index, double *dZ, int *info, double *Gp)
{
    if (!c) return SOCP_ERR_ARG;
    SensitivityPlan plan;
    const int rc0 = sensitivity_args(c, "sensitivity_batch_blocks", B, K, dir_kind, dir_index, &plan);
    if (rc0 != SOCP_OK) return rc0;
    if (const int rc = blocks_stride(c, "sensitivity_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !dZ || !info)) return fail(c, SOCP_ERR_ARG, "sensitivity_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_sensitivity_batch(c, B, Z, K, dir_kind, dir_index, dZ, info, Gp); });
}

/* ---- batched neighbouring-extremal gains ---------------------------------------------------- */

int socp_ctx_has_gain(const socp_ctx *c) { return c ? (table_of(c)->gain ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
// the refusals all three forms share
int gain_args(socp_ctx *c, const char *who, int B, int stride, int cap)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (stride < 1) return fail(c, SOCP_ERR_ARG, w + ": stride >= 1 is required");
    if (cap < (c->P.step_nbr + stride - 1) / stride)
        return fail(c, SOCP_ERR_ARG, w + ": cap >= ceil(step_nbr / stride) is required (every block of a segment must be stored)");
    if (const int rc = args_tail(c, w, table_of(c)->gain != nullptr,
                                 "gain entry (a model without the rhs_t trait, or one with a switching_state hook, custom final rows or its own "
                                 "ComputeTraj; rebuild a plugin written for an older launch table)",
                                 "the gains follow"))
        return rc;
    // the structures that need a bordered sweep
    for (int k = 0; k <= c->M; k++)
        if (c->mode_t[k] == SOCP_FREE)
            return fail(c, SOCP_ERR_UNSUPPORTED, w + ": a free time (node " + std::to_string(k) + ") is not covered");
    for (int k = 1; k < c->M; k++)
        for (int j = 0; j < c->dim; j++)
            if (c->mode_x[(size_t)k * c->dim + j] != SOCP_CONTINUOUS)
                return fail(c, SOCP_ERR_UNSUPPORTED, w + ": a FIXED or FREE state component on an interior node (node " + std::to_string(k) +
                                                         ", component " + std::to_string(j) + ") is not covered");
    if (!linsolve_fits(c->dim, c->dim))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": too many states for the batched linear solve (3 d doubles must fit 64 KiB of LDS)");
    return SOCP_OK;
}
}  // namespace

int socp_gain_batch_dev(socp_ctx *c, int B, const double *d_Z, int stride, int cap, double *d_tq, double *d_Kp, int *d_info, int *d_count,
                        double *d_Xq, double *d_Wq, double *d_Psi)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = gain_args(c, "gain_batch", B, stride, cap)) return rc;
    if (B > 0 && (!d_Z || !d_tq || !d_Kp || !d_info || !d_count)) return fail(c, SOCP_ERR_ARG, "gain_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // the workspace: the elimination's matrices and, unless the caller takes them, the blocks (grow-only: the first use and every
    // growth is a hipMalloc, which synchronises the device -- the header says so)
    const size_t d = (size_t)c->dim, s = (size_t)c->S, slots = (size_t)B * c->M * cap;
    HIP_TRY(c, c->s_gain.reserve(sizeof(double) * slots * (d * d + (d_Psi ? 0 : s * s))));
    double *wA = c->s_gain.as<double>(), *psi = d_Psi ? d_Psi : wA + slots * d * d;
    // launches 1 and 2: the blocks, then the backward sweep, which leaves -A_x in Kp and A_p in the workspace
    c->n_traj += (long long)B * c->M * c->S; c->n_launch += 2;
    HIP_TRY(c, table_of(c)->gain(c->stream, c->P, c->pb, B, d_Z, stride, cap, d_tq, d_Xq, d_count, psi, d_Wq, wA, d_Kp));
    // launch 3: A_p K = -A_x in place, in reference order in both flavours; the slots at or beyond count are not touched
    c->n_launch += 1;
    HIP_TRY(c, linsolve_slots(c->stream, B * c->M, cap, d_count, c->dim, c->dim, wA, d_Kp, d_info));
    return SOCP_OK;
}

int socp_gain_batch(socp_ctx *c, int B, const double *Z, int stride, int cap, double *tq, double *Kp, int *info, int *count, double *Xq,
                    double *Wq, double *Psi)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = gain_args(c, "gain_batch", B, stride, cap)) return rc;
    if (B > 0 && (!Z || !tq || !Kp || !info || !count)) return fail(c, SOCP_ERR_ARG, "gain_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t d = (size_t)c->dim, s = (size_t)c->S, segs = (size_t)B * c->M, slots = segs * cap, nZ = (size_t)B * c->n;
    const size_t nK = slots * d * d, nX = Xq ? slots * s : 0, nW = Wq ? slots * d * s : 0, nP = Psi ? slots * s * s : 0;
    double *dZ, *dT;
    int *dI;
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, dZ));
    // every slab travels both ways: what the kernels leave untouched (slots at or beyond count) comes back as it went
    HIP_TRY(c, stage_up(c, c->s_out, tq, slots, dT, slots + nK + nX + nW + nP));
    double *dK = dT + slots, *dX = dK + nK, *dW = dX + nX, *dP = dW + nW;
    HIP_TRY(c, copy_up(c, dK, Kp, nK));
    if (Xq) HIP_TRY(c, copy_up(c, dX, Xq, nX));
    if (Wq) HIP_TRY(c, copy_up(c, dW, Wq, nW));
    if (Psi) HIP_TRY(c, copy_up(c, dP, Psi, nP));
    HIP_TRY(c, stage_up(c, c->s_var, info, slots, dI, slots + segs));
    int *dC = dI + slots;
    const int rc = socp_gain_batch_dev(c, B, dZ, stride, cap, dT, dK, dI, dC, Xq ? dX : nullptr, Wq ? dW : nullptr, Psi ? dP : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, tq, dT, slots));
    HIP_TRY(c, copy_down(c, Kp, dK, nK));
    HIP_TRY(c, copy_down(c, info, dI, slots));
    HIP_TRY(c, copy_down(c, count, dC, segs));
    if (Xq) HIP_TRY(c, copy_down(c, Xq, dX, nX));
    if (Wq) HIP_TRY(c, copy_down(c, Wq, dW, nW));
    if (Psi) HIP_TRY(c, copy_down(c, Psi, dP, nP));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_gain_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time, const double *xnode,
                           int stride, int cap, double *tq, double *Kp, int *info, int *count, double *Xq, double *Wq, double *Psi)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = gain_args(c, "gain_batch_blocks", B, stride, cap)) return rc;
    if (const int rc = blocks_stride(c, "gain_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !tq || !Kp || !info || !count)) return fail(c, SOCP_ERR_ARG, "gain_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_gain_batch(c, B, Z, stride, cap, tq, Kp, info, count, Xq, Wq, Psi); });
}

/* ---- batched neighbouring-extremal gains with a free final time ------------------------------ */

int socp_ctx_has_gain_free(const socp_ctx *c) { return c ? (table_of(c)->gain_free ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
// the refusals all three forms share
int gain_free_args(socp_ctx *c, const char *who, int B, int stride, int cap)
{
    const std::string w(who);
    if (const int rc = args_head(c, w, B >= 0, "B >= 0 is required")) return rc;
    if (stride < 1) return fail(c, SOCP_ERR_ARG, w + ": stride >= 1 is required");
    if (cap < (c->P.step_nbr + stride - 1) / stride)
        return fail(c, SOCP_ERR_ARG, w + ": cap >= ceil(step_nbr / stride) is required (every block of a segment must be stored)");
    if (const int rc = args_tail(c, w, table_of(c)->gain_free != nullptr,
                                 "gain_free entry (a model without the rhs_t or the hamiltonian_t trait, or one with a switching_state hook, "
                                 "custom final rows or its own ComputeTraj; rebuild a plugin written for an older launch table)",
                                 "the gains follow"))
        return rc;
    // the structure the bordered sweep covers: t_f free, every other time fixed or interpolated, interior nodes CONTINUOUS
    if (c->mode_t[c->M] != SOCP_FREE)
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": the final time (node " + std::to_string(c->M) + ") is not FREE: use socp_gain_batch");
    for (int k = 0; k < c->M; k++)
        if (c->mode_t[k] == SOCP_FREE)
            return fail(c, SOCP_ERR_UNSUPPORTED, w + ": a free time before the final node (node " + std::to_string(k) + ") is not covered");
    for (int k = 1; k < c->M; k++)
        for (int j = 0; j < c->dim; j++)
            if (c->mode_x[(size_t)k * c->dim + j] != SOCP_CONTINUOUS)
                return fail(c, SOCP_ERR_UNSUPPORTED, w + ": a FIXED or FREE state component on an interior node (node " + std::to_string(k) +
                                                         ", component " + std::to_string(j) + ") is not covered");
    if (!linsolve_fits(c->dim + 1, c->dim))
        return fail(c, SOCP_ERR_UNSUPPORTED, w + ": too many states for the batched linear solve (3 d + 2 doubles must fit 64 KiB of LDS)");
    return SOCP_OK;
}
}  // namespace

int socp_gain_free_batch_dev(socp_ctx *c, int B, const double *d_Z, int stride, int cap, double *d_tq, double *d_Ke, int *d_info, int *d_count,
                             double *d_Xq, double *d_Wq, double *d_Psi, double *d_Len)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = gain_free_args(c, "gain_free_batch", B, stride, cap)) return rc;
    if (B > 0 && (!d_Z || !d_tq || !d_Ke || !d_info || !d_count)) return fail(c, SOCP_ERR_ARG, "gain_free_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // the workspace: the elimination's bordered matrices, grad H of every row and, unless the caller takes them, the blocks and their
    // length columns (grow-only: the first use and every growth is a hipMalloc, which synchronises the device -- the header says so)
    const size_t d1 = (size_t)c->dim + 1, s = (size_t)c->S, slots = (size_t)B * c->M * cap;
    HIP_TRY(c, c->s_gain.reserve(sizeof(double) * (slots * (d1 * d1 + (d_Psi ? 0 : s * s) + (d_Len ? 0 : s)) + (size_t)B * s)));
    double *wA = c->s_gain.as<double>(), *gh = wA + slots * d1 * d1, *next = gh + (size_t)B * s;
    double *psi = d_Psi ? d_Psi : next;
    double *len = d_Len ? d_Len : next + (d_Psi ? 0 : slots * s * s);
    // launches 1 and 2: the blocks, then the bordered backward sweep, which leaves -A_x in Ke and [A_p | wtau] in the workspace
    c->n_traj += (long long)B * c->M * (c->S + 1); c->n_launch += 2;
    HIP_TRY(c, table_of(c)->gain_free(c->stream, c->P, c->pb, B, d_Z, stride, cap, d_tq, d_Xq, d_count, psi, len, gh, d_Wq, wA, d_Ke));
    // launch 3: [A_p | wtau] [K_p; k_t] = -A_x in place, in reference order in both flavours; the slots at or beyond count are not touched
    c->n_launch += 1;
    HIP_TRY(c, linsolve_slots(c->stream, B * c->M, cap, d_count, c->dim + 1, c->dim, wA, d_Ke, d_info));
    return SOCP_OK;
}

int socp_gain_free_batch(socp_ctx *c, int B, const double *Z, int stride, int cap, double *tq, double *Ke, int *info, int *count, double *Xq,
                         double *Wq, double *Psi, double *Len)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = gain_free_args(c, "gain_free_batch", B, stride, cap)) return rc;
    if (B > 0 && (!Z || !tq || !Ke || !info || !count)) return fail(c, SOCP_ERR_ARG, "gain_free_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t d = (size_t)c->dim, s = (size_t)c->S, segs = (size_t)B * c->M, slots = segs * cap, nZ = (size_t)B * c->n;
    const size_t nK = slots * (d + 1) * d, nX = Xq ? slots * s : 0, nW = Wq ? slots * (d + 1) * (s + 1) : 0, nP = Psi ? slots * s * s : 0,
                 nL = Len ? slots * s : 0;
    double *dZ, *dT;
    int *dI;
    HIP_TRY(c, stage_up(c, c->s_in, Z, nZ, dZ));
    // every slab travels both ways: what the kernels leave untouched (slots at or beyond count) comes back as it went
    HIP_TRY(c, stage_up(c, c->s_out, tq, slots, dT, slots + nK + nX + nW + nP + nL));
    double *dK = dT + slots, *dX = dK + nK, *dW = dX + nX, *dP = dW + nW, *dL = dP + nP;
    HIP_TRY(c, copy_up(c, dK, Ke, nK));
    if (Xq) HIP_TRY(c, copy_up(c, dX, Xq, nX));
    if (Wq) HIP_TRY(c, copy_up(c, dW, Wq, nW));
    if (Psi) HIP_TRY(c, copy_up(c, dP, Psi, nP));
    if (Len) HIP_TRY(c, copy_up(c, dL, Len, nL));
    HIP_TRY(c, stage_up(c, c->s_var, info, slots, dI, slots + segs));
    int *dC = dI + slots;
    const int rc = socp_gain_free_batch_dev(c, B, dZ, stride, cap, dT, dK, dI, dC, Xq ? dX : nullptr, Wq ? dW : nullptr, Psi ? dP : nullptr,
                                            Len ? dL : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, tq, dT, slots));
    HIP_TRY(c, copy_down(c, Ke, dK, nK));
    HIP_TRY(c, copy_down(c, info, dI, slots));
    HIP_TRY(c, copy_down(c, count, dC, segs));
    if (Xq) HIP_TRY(c, copy_down(c, Xq, dX, nX));
    if (Wq) HIP_TRY(c, copy_down(c, Wq, dW, nW));
    if (Psi) HIP_TRY(c, copy_down(c, Psi, dP, nP));
    if (Len) HIP_TRY(c, copy_down(c, Len, dL, nL));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_gain_free_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time,
                                const double *xnode, int stride, int cap, double *tq, double *Ke, int *info, int *count, double *Xq,
                                double *Wq, double *Psi, double *Len)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = gain_free_args(c, "gain_free_batch_blocks", B, stride, cap)) return rc;
    if (const int rc = blocks_stride(c, "gain_free_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !tq || !Ke || !info || !count)) return fail(c, SOCP_ERR_ARG, "gain_free_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode,
                       [&] { return socp_gain_free_batch(c, B, Z, stride, cap, tq, Ke, info, count, Xq, Wq, Psi, Len); });
}

/* ---- closed-loop flight under the sampled neighbouring-extremal law ------------------------------ */

int socp_ctx_has_guide(const socp_ctx *c) { return c ? (table_of(c)->guide ? 1 : 0) : SOCP_ERR_ARG; }

namespace {
// the refusals all three forms share: those of the gain call whose tables the problem's structure expects, then the entry itself
int guide_args(socp_ctx *c, const char *who, int B, int stride, int cap, int K, int every, bool *free_tf)
{
    const std::string w(who);
    if (!c->has_problem) return fail(c, SOCP_ERR_ARG, w + ": no problem set");
    if (K < 1 || every < 0) return fail(c, SOCP_ERR_ARG, w + ": K >= 1 and every >= 0 are required");
    *free_tf = c->mode_t[c->M] == SOCP_FREE;
    if (const int rc = *free_tf ? gain_free_args(c, who, B, stride, cap) : gain_args(c, who, B, stride, cap)) return rc;
    return args_tail(c, w, table_of(c)->guide != nullptr,
                     "guide entry (a model with a switching_state hook, custom final rows or its own ComputeTraj; rebuild a plugin written "
                     "for an older launch table)",
                     "the flight follows");
}

struct GuideSizes {
    size_t nZ, slots, segs, nXq, nKg, nD0, cases, nXf, nMiss, nXs;
};
GuideSizes guide_sizes(const socp_ctx *c, int B, int cap, int K, bool free_tf, bool xs)
{
    GuideSizes g;
    const size_t d = (size_t)c->dim, s = (size_t)c->S;
    g.nZ = (size_t)B * c->n;
    g.segs = (size_t)B * c->M;
    g.slots = g.segs * cap;
    g.nXq = g.slots * s;
    g.nKg = g.slots * (free_tf ? d + 1 : d) * d;
    g.cases = (size_t)B * K;
    g.nD0 = g.cases * d;
    g.nXf = g.cases * s;
    g.nMiss = g.cases * (free_tf ? d + 1 : d);
    g.nXs = xs ? g.cases * c->M * cap * s : 0;
    return g;
}
}  // namespace

int socp_guide_batch_dev(socp_ctx *c, int B, const double *d_Z, int stride, int cap, const double *d_Xq, const double *d_Kg, const int *d_info,
                         const int *d_count, int K, const double *d_dX0, int every, double *d_Xf, double *d_miss, int *d_nupd, int *d_nskip,
                         double *d_tf, double *d_dxmax, double *d_Xs)
{
    if (!c) return SOCP_ERR_ARG;
    bool free_tf = false;
    if (const int rc = guide_args(c, "guide_batch", B, stride, cap, K, every, &free_tf)) return rc;
    if (B > 0 && (!d_Z || !d_Xq || !d_Kg || !d_info || !d_count || !d_dX0 || !d_Xf || !d_miss || !d_nupd || !d_nskip))
        return fail(c, SOCP_ERR_ARG, "guide_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    GuideArgs A;
    A.K = K; A.stride = stride; A.cap = cap; A.every = every;
    A.Xq = d_Xq; A.Kg = d_Kg; A.dX0 = d_dX0; A.info = d_info; A.count = d_count;
    A.Xf = d_Xf; A.miss = d_miss; A.tf = d_tf; A.dxmax = d_dxmax; A.Xs = d_Xs; A.nupd = d_nupd; A.nskip = d_nskip;
    // ONE launch: every case flies its M segments
    c->n_traj += (long long)B * K * c->M; c->n_launch += 1;
    HIP_TRY(c, table_of(c)->guide(c->stream, c->P, c->pb, B, d_Z, free_tf ? 1 : 0, A));
    return SOCP_OK;
}

int socp_guide_batch(socp_ctx *c, int B, const double *Z, int stride, int cap, const double *Xq, const double *Kg, const int *info,
                     const int *count, int K, const double *dX0, int every, double *Xf, double *miss, int *nupd, int *nskip, double *tf,
                     double *dxmax, double *Xs)
{
    if (!c) return SOCP_ERR_ARG;
    bool free_tf = false;
    if (const int rc = guide_args(c, "guide_batch", B, stride, cap, K, every, &free_tf)) return rc;
    if (B > 0 && (!Z || !Xq || !Kg || !info || !count || !dX0 || !Xf || !miss || !nupd || !nskip))
        return fail(c, SOCP_ERR_ARG, "guide_batch: null argument");
    if (B == 0) return SOCP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const GuideSizes g = guide_sizes(c, B, cap, K, free_tf, Xs != nullptr);
    // the inputs: Z, the tables and the deviations; the integer tables behind the doubles
    double *dZ;
    int *dI;
    HIP_TRY(c, stage_up(c, c->s_in, Z, g.nZ, dZ, g.nZ + g.nXq + g.nKg + g.nD0));
    double *dQ = dZ + g.nZ, *dK = dQ + g.nXq, *dD = dK + g.nKg;
    HIP_TRY(c, copy_up(c, dQ, Xq, g.nXq));
    HIP_TRY(c, copy_up(c, dK, Kg, g.nKg));
    HIP_TRY(c, copy_up(c, dD, dX0, g.nD0));
    HIP_TRY(c, stage_up(c, c->s_var, info, g.slots, dI, g.slots + g.segs + 2 * g.cases));
    int *dC = dI + g.slots, *dU = dC + g.segs, *dS = dU + g.cases;
    HIP_TRY(c, copy_up(c, dC, count, g.segs));
    // the outputs; Xs travels both ways: the slots at or beyond count come back as they went
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * (g.nXf + g.nMiss + 2 * g.cases + g.nXs)));
    double *dF = c->s_out.as<double>(), *dM = dF + g.nXf, *dT = dM + g.nMiss, *dX = dT + g.cases, *dXs = dX + g.cases;
    if (Xs) HIP_TRY(c, copy_up(c, dXs, Xs, g.nXs));
    const int rc = socp_guide_batch_dev(c, B, dZ, stride, cap, dQ, dK, dI, dC, K, dD, every, dF, dM, dU, dS, tf ? dT : nullptr,
                                        dxmax ? dX : nullptr, Xs ? dXs : nullptr);
    if (rc != SOCP_OK) return rc;
    HIP_TRY(c, copy_down(c, Xf, dF, g.nXf));
    HIP_TRY(c, copy_down(c, miss, dM, g.nMiss));
    HIP_TRY(c, copy_down(c, nupd, dU, g.cases));
    HIP_TRY(c, copy_down(c, nskip, dS, g.cases));
    if (tf) HIP_TRY(c, copy_down(c, tf, dT, g.cases));
    if (dxmax) HIP_TRY(c, copy_down(c, dxmax, dX, g.cases));
    if (Xs) HIP_TRY(c, copy_down(c, Xs, dXs, g.nXs));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

int socp_guide_batch_blocks(socp_ctx *c, int B, const double *Z, const double *params, int pstride, const double *time, const double *xnode,
                            int stride, int cap, const double *Xq, const double *Kg, const int *info, const int *count, int K,
                            const double *dX0, int every, double *Xf, double *miss, int *nupd, int *nskip, double *tf, double *dxmax,
                            double *Xs)
{
    if (!c) return SOCP_ERR_ARG;
    bool free_tf = false;
    if (const int rc = guide_args(c, "guide_batch_blocks", B, stride, cap, K, every, &free_tf)) return rc;
    if (const int rc = blocks_stride(c, "guide_batch_blocks: the parameter stride", params, pstride)) return rc;
    if (B > 0 && (!Z || !Xq || !Kg || !info || !count || !dX0 || !Xf || !miss || !nupd || !nskip))
        return fail(c, SOCP_ERR_ARG, "guide_batch_blocks: null argument");
    if (B == 0) return SOCP_OK;
    return with_blocks(c, B, params, pstride, time, xnode, [&] {
        return socp_guide_batch(c, B, Z, stride, cap, Xq, Kg, info, count, K, dX0, every, Xf, miss, nupd, nskip, tf, dxmax, Xs);
    });
}

/* ---- row grouping --------------------------------------------------------------------------- */

namespace {
constexpr int kGroupChunk = 16;       // rounds enqueued between two read-backs of the "next leader" word, once the first few came singly

int group_args(socp_ctx *c, int B, int n, int ld, const double *V, double atol, double rtol, int max_groups, const int *label,
               const int *leader, const int *count, const double *radius, const int *summary)
{
    if (B < 0 || n < 1 || ld < n || max_groups < 1)
        return fail(c, SOCP_ERR_ARG, "group_batch: B >= 0, n >= 1, ld >= n and max_groups >= 1 are required");
    if (!(atol >= 0.0) || !(rtol >= 0.0) || !std::isfinite(atol) || !std::isfinite(rtol))
        return fail(c, SOCP_ERR_ARG, "group_batch: atol and rtol must be finite and not negative");
    if (!leader || !count || !radius || !summary || (B > 0 && !label)) return fail(c, SOCP_ERR_ARG, "group_batch: null output pointer");
    if (B > 0 && !V) return fail(c, SOCP_ERR_ARG, "group_batch: null table");
    return SOCP_OK;
}
}  // namespace

int socp_group_batch_dev(socp_ctx *c, int B, int n, int ld, const double *d_V, const int *d_mask, double atol, double rtol, int max_groups,
                         int *d_label, int *d_leader, int *d_count, double *d_radius, int *d_summary)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = group_args(c, B, n, ld, d_V, atol, rtol, max_groups, d_label, d_leader, d_count, d_radius, d_summary)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->s_var.reserve(sizeof(int) * ((size_t)max_groups + 1)));
    int *next = c->s_var.as<int>();
    c->n_launch += B > 0 ? 2 : 1;
    HIP_TRY(c, group_begin(c->stream, B, n, ld, d_V, d_mask, max_groups, d_label, d_leader, d_count, d_radius, d_summary, next));
    if (B == 0) return SOCP_OK;
    // rounds g .. g + chunk - 1, then the leader of round g + chunk back: none, and the rows ran out (rounds enqueued behind the last
    // group found no leader and returned at once)
    for (int g = 0, chunk = 1; g < max_groups; chunk = chunk < kGroupChunk ? 2 * chunk : kGroupChunk) {
        const int end = max_groups - g < chunk ? max_groups : g + chunk;
        for (; g < end; g++) {
            c->n_launch += 1;
            HIP_TRY(c, group_round(c->stream, B, n, ld, d_V, atol, rtol, g, d_label, d_leader, d_count, d_radius, d_summary, next));
        }
        if (g == max_groups) break;
        int lead = 0;
        HIP_TRY(c, copy_down(c, &lead, next + g, 1));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (lead < 0 || lead >= B) break;
    }
    c->n_launch += 1;
    HIP_TRY(c, group_end(c->stream, B, d_label, d_summary));
    return SOCP_OK;
}

int socp_group_batch(socp_ctx *c, int B, int n, int ld, const double *V, const int *mask, double atol, double rtol, int max_groups,
                     int *label, int *leader, int *count, double *radius, int *summary)
{
    if (!c) return SOCP_ERR_ARG;
    if (const int rc = group_args(c, B, n, ld, V, atol, rtol, max_groups, label, leader, count, radius, summary)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nV = (size_t)B * ld, nB = (size_t)B, nG = (size_t)max_groups;
    double *d_V = nullptr;
    int *d_mask = nullptr;
    // radius[G] first (8-byte aligned), then label[B], leader[G], count[G], summary[4]
    HIP_TRY(c, c->s_out.reserve(sizeof(double) * nG + sizeof(int) * (nB + 2 * nG + 4)));
    double *dR = c->s_out.as<double>();
    int *dL = reinterpret_cast<int *>(dR + nG), *dLead = dL + nB, *dCount = dLead + nG, *dSum = dCount + nG;
    if (B > 0) HIP_TRY(c, stage_up(c, c->s_in, V, nV, d_V));
    if (B > 0 && mask) HIP_TRY(c, stage_up(c, c->s_aux, mask, nB, d_mask));
    const int rc = socp_group_batch_dev(c, B, n, ld, d_V, d_mask, atol, rtol, max_groups, dL, dLead, dCount, dR, dSum);
    if (rc != SOCP_OK) return rc;
    if (B > 0) HIP_TRY(c, copy_down(c, label, dL, nB));
    HIP_TRY(c, copy_down(c, leader, dLead, nG));
    HIP_TRY(c, copy_down(c, count, dCount, nG));
    HIP_TRY(c, copy_down(c, radius, dR, nG));
    HIP_TRY(c, copy_down(c, summary, dSum, (size_t)4));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SOCP_OK;
}

}  // extern "C"
