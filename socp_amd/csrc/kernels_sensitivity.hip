// kernels_sensitivity.hip -- socp_sensitivity_batch of the in-tree Goddard, double-integrator and covid19 models (sensitivity.hpp,
// dual.hpp) and the call's model-independent finish.  MUST be compiled with -ffp-contract=off (see socp_amd/csrc/Makefile): every
// dual-number rule is a fixed sequence of IEEE roundings and tests/sensitivity_reference.py restates them bit for bit.  ONE object for
// both flavours: the tables of kernels_exact.hip and of kernels_fast.hip point to the launchers below, so a throughput-flavour context
// returns the same bits.  The value trajectories are the reference-order ones, not the fast residual's.
#include "models_exact.hpp"
#include "builtin_tables.hpp"

namespace socp {

hipError_t sensitivity_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, const SensDirs &dirs, int K,
                               double *G)
{
    return (goddard_smooth(P, pb) ? &plugin::sensitivity<GoddardExactSmooth> : &plugin::sensitivity<GoddardExact>)(st, P, pb, B, Z, dirs, K, G);
}

hipError_t sensitivity_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, const SensDirs &dirs, int K,
                            double *G)
{
    return plugin::sensitivity<DIntExact>(st, P, pb, B, Z, dirs, K, G);
}

hipError_t sensitivity_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, const SensDirs &dirs, int K,
                             double *G)
{
    return plugin::sensitivity<CovidExact>(st, P, pb, B, Z, dirs, K, G);
}

// one lane per entry of G[B][K][n].  An XNODE direction (node j, component c) stores -1.0 at every row that reads xd[j][c]: row c of
// a non-FREE component of node 0, row d + c of one of node M, rows S j + c and S j + d + c of a FIXED interior component; no other
// lane writes an XNODE direction's rows.  Then rhs = -G, entry by entry
__global__ __launch_bounds__(256) void sensitivity_finish_kernel(ProblemDev pb, long total, int K, unsigned xnode_mask, unsigned long long i0,
                                                                 unsigned long long i1, unsigned long long i2, unsigned long long i3,
                                                                 double *__restrict__ G, double *__restrict__ rhs)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int n = pb.n, D = pb.dim, S = 2 * D, M = pb.M;
    const int row = (int)(e % n);
    const int k = (int)((e / n) % K);
    double g = G[e];
    if ((xnode_mask >> k) & 1u) {
        const unsigned long long word = k < 4 ? i0 : (k < 8 ? i1 : (k < 12 ? i2 : i3));
        const int packed = (int)((word >> (16 * (k & 3))) & 0xffffull);
        const int j = packed >> 5, c = packed & 31;
        const int mode = pb.mode_x[j * D + c];
        bool reads;
        if (j == 0) reads = mode != 1 && row == c;
        else if (j == M) reads = mode != 1 && row == D + c;
        else reads = mode == 0 && (row == S * j + c || row == S * j + D + c);
        if (reads) {
            g = -1.0;
            G[e] = g;
        }
    }
    rhs[e] = -g;
}

hipError_t sensitivity_finish(hipStream_t st, const ProblemDev &pb, int B, int K, unsigned xnode_mask, const unsigned long long (&index)[4],
                              double *G, double *rhs)
{
    const long total = (long)B * K * pb.n;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(sensitivity_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pb, total, K, xnode_mask, index[0],
                       index[1], index[2], index[3], G, rhs);
    return hipGetLastError();
}

}  // namespace socp
