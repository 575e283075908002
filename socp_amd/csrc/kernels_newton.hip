// kernels_newton.hip -- the kernels of socp_newton_batch (include/socp_hip.h): damped Newton polish of a whole batch with the exact
// (or differenced, or variational) shooting Jacobian, one round per (compaction, gather, Jacobian, elimination, trial build, residual,
// update) with the per-row state machine on the device.
// Built ONCE with -ffp-contract=off, for both flavours (like kernels_branch.hip): every operation is one IEEE rounding, in the order
// socp_hip.h writes down; all norms are maxima, so no reduction order enters a result.  A throughput-flavour context differs from a
// reference-order one through the model's own launches only (residual, Jacobian).
// Model-independent: the trajectories run through the model's own launch table (residual, fdjac, var_jacobian, exact_jacobian), the
// elimination is kernels_tangent.hip's.  No workgroup waits on another: the compaction is a count -> scan -> scatter chain of three
// launches.  Every per-row scalar is written by an ordinary store from plain C++.
#include "launch.hpp"
#include "wave_reduce.hpp"

namespace socp {
namespace {

constexpr int kRunning = 0, kConverged = 1, kSmallStep = 2, kStalled = 3, kSingular = 4, kBadStart = 5;
constexpr int kScanBlock = 256;                       // rows per workgroup of the compaction: four wavefronts

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7FF8000000000000LL); }

// the larger of two magnitudes, a NaN when either is one
__device__ __forceinline__ double nanmax(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// one wave-wide maximum, the result in every lane (the stages of wave_reduce.hpp's wave_sum)
__device__ __forceinline__ double wave_max(double x)
{
    using devsolver::dpp_move;
    x = nanmax(x, dpp_move<0xB1>(x));                                        // quad_perm [1, 0, 3, 2]
    x = nanmax(x, dpp_move<0x4E>(x));                                        // quad_perm [2, 3, 0, 1]
    x = nanmax(x, dpp_move<0x141>(x));                                       // row_half_mirror: l ^ 7
    x = nanmax(x, dpp_move<0x140>(x));                                       // row_mirror: l ^ 15
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(x), 16 * k), hi = __builtin_amdgcn_readlane(__double2hiint(x), 16 * k);
        r[k] = __hiloint2double(hi, lo);
    }
    return nanmax(nanmax(r[0], r[1]), nanmax(r[2], r[3]));
}

// max_i |v_i| of a row of n entries held by one wavefront; +0.0 for n == 0
__device__ __forceinline__ double row_maxabs(const double *__restrict__ v, int n, int lane)
{
    double m = 0.0;
    for (int i = lane; i < n; i += 64) m = nanmax(m, fabs(v[i]));
    return wave_max(m);
}

// ---- K_newton_start: one wavefront per row: the state and the outputs from Z and F(Z); compact slot b is set to row b --------------
__global__ __launch_bounds__(64) void newton_start_kernel(ProblemDev pb, int B, int n, NewtonArgs A, const double *__restrict__ Z,
                                                          NewtonWork W, NewtonOut O)
{
    const long b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= B) return;
    const double *F0 = W.F0 + b * n, *z = Z + b * n;
    const double rn = row_maxabs(F0, n, lane);
    for (int i = lane; i < n; i += 64) {
        const double zi = z[i], fi = F0[i];
        O.Zout[b * n + i] = zi;
        if (O.Fout) O.Fout[b * n + i] = fi;
        W.cZ[b * n + i] = zi; W.cF[b * n + i] = fi; W.cR[b * n + i] = -fi;
    }
    const int stride = pb.pp_stride, nodes = pb.M + 1, nx = nodes * 2 * pb.dim;
    if (pb.pp_params)
        for (int k = lane; k < stride; k += 64) W.cP[b * stride + k] = pb.pp_params[b * stride + k];
    if (pb.pp_time)
        for (int k = lane; k < nodes; k += 64) W.cT[b * nodes + k] = pb.pp_time[b * nodes + k];
    if (pb.pp_xnode)
        for (int k = lane; k < nx; k += 64) W.cX[b * (long)nx + k] = pb.pp_xnode[b * (long)nx + k];
    if (O.rhist) {
        const long len = (long)A.rounds + 1;
        for (long k = lane; k < len; k += 64) O.rhist[b * len + k] = k == 0 ? rn : qnan();
    }
    if (lane == 0) {
        const bool finite = fabs(rn) < INFINITY;
        O.rnorm[b] = rn; O.dnorm[b] = qnan(); O.iters[b] = 0; O.nhalf[b] = 0;
        O.status[b] = !finite ? kBadStart : (rn <= A.ftol ? kConverged : kRunning);
        W.list[b] = (int)b; W.info[b] = 0;
    }
}

// ---- the compaction: the unfinished rows in ascending order into list[0 .. live) -- count, scan, scatter ----------------------------
// the number of unfinished rows before this one inside its workgroup, and the workgroup's total in every thread
__device__ __forceinline__ int block_rank(bool flag, int &total)
{
    __shared__ int wtot[kScanBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    const int before = __popcll(mask & ((1ULL << lane) - 1ULL));
    if (lane == 0) wtot[w] = __popcll(mask);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < kScanBlock / 64; k++) {
        if (k < w) off += wtot[k];
        total += wtot[k];
    }
    return off + before;
}

__global__ __launch_bounds__(kScanBlock) void newton_count_kernel(int B, const int *__restrict__ status, int *__restrict__ bcount)
{
    const long b = (long)blockIdx.x * kScanBlock + threadIdx.x;
    int total;
    block_rank(b < B && status[b] == kRunning, total);
    if (threadIdx.x == 0) bcount[blockIdx.x] = total;
}

// ONE workgroup: bcount[nb] -> its exclusive prefix sums in place, the total into *live
__global__ __launch_bounds__(kScanBlock) void newton_scan_kernel(int nb, int *__restrict__ bcount, int *__restrict__ live)
{
    __shared__ int wtot[kScanBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int carry = 0;                                                 // the same in every thread
    for (int base = 0; base < nb; base += kScanBlock) {
        const int i = base + tid, v = i < nb ? bcount[i] : 0;
        int x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wtot[w] = x;
        __syncthreads();
        int off = carry, total = 0;
#pragma unroll
        for (int k = 0; k < kScanBlock / 64; k++) {
            if (k < w) off += wtot[k];
            total += wtot[k];
        }
        if (i < nb) bcount[i] = off + x - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) *live = carry;
}

__global__ __launch_bounds__(kScanBlock) void newton_scatter_kernel(int B, const int *__restrict__ status, const int *__restrict__ bcount,
                                                                    int *__restrict__ list)
{
    const long b = (long)blockIdx.x * kScanBlock + threadIdx.x;
    const bool flag = b < B && status[b] == kRunning;
    int total;
    const int rank = block_rank(flag, total);
    if (flag) list[bcount[blockIdx.x] + rank] = (int)b;            // below live <= B
}

// ---- K_newton_gather: one wavefront per live slot: y, F0, the right-hand side -F0 and the row's block rows into the compact buffers --
__global__ __launch_bounds__(64) void newton_gather_kernel(ProblemDev pb, int n, NewtonWork W, NewtonOut O)
{
    const long s = blockIdx.x;
    const int lane = threadIdx.x;
    if (s >= *W.live) return;                                      // a slot without a row keeps what an earlier round left there
    const long b = W.list[s];
    for (int i = lane; i < n; i += 64) {
        const double fi = W.F0[b * n + i];
        W.cZ[s * n + i] = O.Zout[b * n + i];
        W.cF[s * n + i] = fi;
        W.cR[s * n + i] = -fi;
    }
    const int stride = pb.pp_stride, nodes = pb.M + 1, nx = nodes * 2 * pb.dim;
    if (pb.pp_params)
        for (int k = lane; k < stride; k += 64) W.cP[s * stride + k] = pb.pp_params[b * stride + k];
    if (pb.pp_time)
        for (int k = lane; k < nodes; k += 64) W.cT[s * nodes + k] = pb.pp_time[b * nodes + k];
    if (pb.pp_xnode)
        for (int k = lane; k < nx; k += 64) W.cX[s * (long)nx + k] = pb.pp_xnode[b * (long)nx + k];
}

// ---- K_newton_trials: one lane per element: trial row r = s trials + k of slot s is y + fl(2^-k delta), under the slot's block rows ---
__global__ __launch_bounds__(256) void newton_trials_kernel(ProblemDev pb, long rows, int n, int trials, NewtonWork W)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const int stride = pb.pp_stride, nodes = pb.M + 1, nx = nodes * 2 * pb.dim;
    if (e < rows * n) {
        const long r = e / n, s = r / trials;
        const int i = (int)(e - r * n), k = (int)(r - s * trials);
        const double sk = 1.0 / (double)(1 << k), step = sk * W.cR[s * n + i];
        W.tZ[e] = W.cZ[s * n + i] + step;
    }
    if (pb.pp_params && e < rows * stride) {
        const long r = e / stride;
        W.tP[e] = W.cP[(r / trials) * stride + (e - r * stride)];
    }
    if (pb.pp_time && e < rows * nodes) {
        const long r = e / nodes;
        W.tT[e] = W.cT[(r / trials) * nodes + (e - r * nodes)];
    }
    if (pb.pp_xnode && e < rows * nx) {
        const long r = e / nx;
        W.tX[e] = W.cX[(r / trials) * nx + (e - r * nx)];
    }
}

// ---- K_newton_update: one wavefront per live slot: the norms, the selection, the copy of the winning trial row, the end tests -------
__global__ __launch_bounds__(64) void newton_update_kernel(int n, NewtonArgs A, NewtonWork W, NewtonOut O)
{
    const long s = blockIdx.x;
    const int lane = threadIdx.x;
    if (s >= *W.live) return;
    const long b = W.list[s];
    const int info = W.info[s];
    const double dn = row_maxabs(W.cR + s * n, n, lane);
    if (info != 0) {                                               // y stays
        if (lane == 0) { O.status[b] = kSingular; O.dnorm[b] = qnan(); }
        return;
    }
    const double rn = O.rnorm[b];
    int won = -1;
    double rk = 0.0, sk = 1.0;
    for (int k = 0; k < A.trials; k++) {
        sk = 1.0 / (double)(1 << k);
        const double ck = 1.0 - sk / 4, bar = ck * rn;
        rk = row_maxabs(W.tF + (s * A.trials + k) * n, n, lane);
        if (rk < bar) { won = k; break; }                          // a NaN never passes
    }
    if (won < 0) {
        if (lane == 0) { O.status[b] = kStalled; O.dnorm[b] = dn; }
        return;
    }
    const double *tz = W.tZ + (s * A.trials + won) * n, *tf = W.tF + (s * A.trials + won) * n;
    for (int i = lane; i < n; i += 64) {
        const double zi = tz[i], fi = tf[i];
        O.Zout[b * n + i] = zi;
        W.F0[b * n + i] = fi;
        if (O.Fout) O.Fout[b * n + i] = fi;
    }
    const double yn = row_maxabs(tz, n, lane);
    if (lane == 0) {
        const int it = O.iters[b] + 1;
        int status = kRunning;
        if (rk <= A.ftol) {
            status = kConverged;
        } else if (A.xtol > 0.0) {
            const double taken = sk * dn, small = A.xtol * yn;
            if (taken <= small) status = kSmallStep;
        }
        O.rnorm[b] = rk; O.dnorm[b] = dn; O.iters[b] = it; O.nhalf[b] = O.nhalf[b] + won; O.status[b] = status;
        if (O.rhist) O.rhist[b * ((long)A.rounds + 1) + it] = rk;
    }
}

}  // namespace

hipError_t newton_start(hipStream_t st, const ProblemDev &pb, int B, int n, const NewtonArgs &A, const double *Z, const NewtonWork &W,
                        const NewtonOut &O)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(newton_start_kernel, dim3((unsigned)B), dim3(64), 0, st, pb, B, n, A, Z, W, O);
    return hipGetLastError();
}

hipError_t newton_compact(hipStream_t st, int B, const int *status, const NewtonWork &W)
{
    if (B <= 0) return hipSuccess;
    const int nb = newton_scan_blocks(B);
    hipLaunchKernelGGL(newton_count_kernel, dim3((unsigned)nb), dim3(kScanBlock), 0, st, B, status, W.bcount);
    hipLaunchKernelGGL(newton_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, nb, W.bcount, W.live);
    hipLaunchKernelGGL(newton_scatter_kernel, dim3((unsigned)nb), dim3(kScanBlock), 0, st, B, status, W.bcount, W.list);
    return hipGetLastError();
}

hipError_t newton_gather(hipStream_t st, const ProblemDev &pb, int slots, int n, const NewtonWork &W, const NewtonOut &O)
{
    if (slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(newton_gather_kernel, dim3((unsigned)slots), dim3(64), 0, st, pb, n, W, O);
    return hipGetLastError();
}

hipError_t newton_trials(hipStream_t st, const ProblemDev &pb, int slots, int n, int trials, const NewtonWork &W)
{
    if (slots <= 0) return hipSuccess;
    const long rows = (long)slots * trials;
    long widest = n;
    if (pb.pp_params && pb.pp_stride > widest) widest = pb.pp_stride;
    if (pb.pp_time && pb.M + 1 > widest) widest = pb.M + 1;
    if (pb.pp_xnode && (long)(pb.M + 1) * 2 * pb.dim > widest) widest = (long)(pb.M + 1) * 2 * pb.dim;
    hipLaunchKernelGGL(newton_trials_kernel, dim3((unsigned)((rows * widest + 255) / 256)), dim3(256), 0, st, pb, rows, n, trials, W);
    return hipGetLastError();
}

hipError_t newton_update(hipStream_t st, int slots, int n, const NewtonArgs &A, const NewtonWork &W, const NewtonOut &O)
{
    if (slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(newton_update_kernel, dim3((unsigned)slots), dim3(64), 0, st, n, A, W, O);
    return hipGetLastError();
}

}  // namespace socp
