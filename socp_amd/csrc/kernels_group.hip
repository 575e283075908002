// kernels_group.hip -- the kernels of socp_group_batch (include/socp_hip.h): greedy leader grouping of the rows of a table, in row
// order.  Built ONCE, without contraction (socp_amd/csrc/Makefile): labels, leaders, counts and the summary are integers and a radius
// is a maximum of exactly rounded differences, so nothing depends on a summation order and one object serves both arithmetic
// flavours bit for bit (like cost_total and regrid_pack).  Model-independent: no launch table is involved.
//
// Geometry shared by the three row kernels.  A wavefront takes TILES of 64 consecutive rows, tile = wave, wave + W, ... (W the
// waves of the grid).  For a tile it first reads the 64 labels, one lane per ROW (one coalesced 256-byte load); rows that already
// hold a label are never looked at again, and a tile without an unassigned row costs those 256 bytes and nothing of V.  The rows
// still unassigned are then loaded with one lane per ELEMENT: a row owns LPR = 2^lgL consecutive lanes (the power of two >= n,
// 64 when n > 32, each lane then striding over the columns by 64), so one load instruction of the wave covers 64 / LPR
// consecutive rows -- a contiguous piece of the table.  The per-row verdicts come from two ballots (some element not finite,
// some element not near); lane r picks the bits of the lanes that own row r out of them, so no LDS and no shuffle is needed.
#include <climits>

#include "launch.hpp"

namespace socp {
namespace {

constexpr int kGroupUnassigned = -1;                 // == SOCP_GROUP_OVERFLOW: what is still unassigned after the last round IS overflow
constexpr int kGroupNotFinite = -2, kGroupMasked = -3;
constexpr int kGroupNone = INT_MAX;                  // a "next leader" word without a candidate
constexpr int kGroupLdsCols = 2048;                  // leader columns (value and bound) a workgroup keeps in LDS at most (32 KiB); the rest from HBM

__device__ __forceinline__ unsigned long long low_bits(int k) { return k >= 64 ? ~0ull : (1ull << k) - 1ull; }
__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }
__device__ __forceinline__ int relaxed_load(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

struct WaveId {
    int lane;
    long wave, waves;
};
__device__ __forceinline__ WaveId wave_id()
{
    WaveId w;
    w.lane = threadIdx.x & 63;
    w.wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    w.waves = (long)gridDim.x * (blockDim.x >> 6);
    return w;
}

// ---- K_group_fill: the slots of the outputs and the scratch words; the only kernel of an empty table ------------------------------
__global__ __launch_bounds__(256) void group_fill_kernel(int max_groups, int *__restrict__ leader, int *__restrict__ count,
                                                         double *__restrict__ radius, int *__restrict__ summary, int *__restrict__ next)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < max_groups) { leader[i] = -1; count[i] = 0; radius[i] = 0.0; }
    if (i <= max_groups) next[i] = kGroupNone;
    if (i < 4) summary[i] = 0;
}

// ---- K_group_init: label = MASKED or unassigned for every row, and the first leader into next[0] ----------------------------------
// The first leader is the lowest unmasked row whose n entries are all finite.  A wave walks the unmasked rows of a tile upwards, one
// whole row per step (a lane per element), marks the ones that are not finite and stops at the first finite one; tiles above the
// best candidate so far are not scanned at all, so with a finite row 0 the scan reads a few rows.  Rows it does not reach keep
// "unassigned": round 0 loads every such row anyway and marks the ones that are not finite (group_round_kernel).
__global__ __launch_bounds__(256) void group_init_kernel(int B, int n, int ld, const double *__restrict__ V, const int *__restrict__ mask,
                                                         int *__restrict__ label, int *__restrict__ next)
{
    const WaveId w = wave_id();
    const long tiles = ((long)B + 63) / 64;
    bool found = false;
    for (long tile = w.wave; tile < tiles; tile += w.waves) {
        const long r0 = tile * 64, myrow = r0 + w.lane;
        const bool in = myrow < B;
        int lab = (in && mask && mask[myrow] == 0) ? kGroupMasked : kGroupUnassigned;
        unsigned long long todo = __ballot(in && lab == kGroupUnassigned);
        if (!found && r0 < (long)relaxed_load(next)) {
            while (todo) {
                const int r = __ffsll((long long)todo) - 1;
                const double *row = V + (r0 + r) * (long)ld;
                bool bad = false;
                for (int col = w.lane; col < n; col += 64) bad |= !finite(row[col]);
                if (!__ballot(bad)) {
                    found = true;
                    if (w.lane == 0) atomicMin(next, (int)(r0 + r));
                    break;
                }
                if (w.lane == r) lab = kGroupNotFinite;
                todo &= todo - 1;
            }
        }
        if (in) label[myrow] = lab;
    }
}

// ---- K_group_round: round g -- every unassigned row near the leader next[g] takes label g ------------------------------------------
// Equivalence with the sequential definition, by induction on g: suppose that after rounds 0 .. g-1 the rows labelled 0 .. g-1 are
// exactly the sequential members of groups 0 .. g-1.  The lowest row still unassigned is near none of the leaders 0 .. g-1 (it would
// carry their label), and every row below it is assigned or excluded, so the sequential loop opens group g exactly there: it is
// leader[g].  A row b joins group g sequentially iff it is near no leader 0 .. g-1 -- all of which have a lower index than
// leader[g] <= b, so they were all known when b was visited: iff b is unassigned now -- and near leader[g]: what this round tests.
//
// Per wave and round: one atomic add into count[g], one 64-bit unsigned atomic max into radius[g] (bit patterns of doubles >= 0
// order like the doubles) and at most one atomic min into next[g + 1], the lowest row the wave leaves unassigned -- skipped when the
// word already holds a lower row.  A round whose next[g] holds no row returns at once.
__global__ __launch_bounds__(256) void group_round_kernel(int B, int n, int ld, int lgL, const double *__restrict__ V, double atol, double rtol,
                                                          int g, int *__restrict__ label, int *__restrict__ leader, int *__restrict__ count,
                                                          double *__restrict__ radius, int *__restrict__ summary, int *__restrict__ next)
{
    extern __shared__ double group_lds[];                              // min(n, kGroupLdsCols) leader values, then as many bounds
    double *sL = group_lds, *sBound = group_lds + (n < kGroupLdsCols ? n : kGroupLdsCols);
    const int lead = next[g];
    if (lead < 0 || lead >= B) return;
    const double *__restrict__ L = V + (long)lead * ld;
    for (int col = threadIdx.x; col < n && col < kGroupLdsCols; col += 256) {
        const double l = L[col];
        sL[col] = l;
        sBound[col] = atol + rtol * fabs(l);
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) { leader[g] = lead; summary[0] = g + 1; }

    const WaveId w = wave_id();
    const int LPR = 1 << lgL, lgR = 6 - lgL, RPI = 1 << lgR;         // lanes per row; rows per load instruction
    const int sub = w.lane >> lgL, col0 = w.lane & (LPR - 1);          // as an element lane: the row within the instruction, the first column
    const unsigned long long sub_lanes = low_bits(LPR) << (sub << lgL);
    const int my_it = w.lane >> lgR;                                   // as a row lane: the instruction that loads row `lane`, and its lanes
    const unsigned long long my_lanes = low_bits(LPR) << ((w.lane & (RPI - 1)) << lgL);
    const bool one_column = n <= 64;                                   // a lane meets one column only: leader value and bound in registers
    const double l0 = col0 < n ? sL[col0] : 0.0, bound0 = col0 < n ? sBound[col0] : 0.0;
    const long tiles = ((long)B + 63) / 64;
    int joined_total = 0;
    long remains = -1;                                                 // the lowest row this wave leaves unassigned
    double wr = 0.0;                                                   // max |v - l| over the elements of joined rows this lane loaded
    for (long tile = w.wave; tile < tiles; tile += w.waves) {
        const long r0 = tile * 64, myrow = r0 + w.lane;
        const bool mine = myrow < B && label[myrow] == kGroupUnassigned;
        const unsigned long long todo = __ballot(mine);
        if (!todo) continue;
        bool my_nf = false, my_nn = false;
        // the verdicts of the rows of load instruction `it` from its lanes' findings
        auto verdicts = [&](int it, bool act, bool nf, bool nn, double dmax) {
            const unsigned long long bnf = __ballot(nf), bnn = __ballot(nn);
            if (act && !((bnf | bnn) & sub_lanes)) wr = fmax(wr, dmax);
            if (my_it == it) { my_nf = (bnf & my_lanes) != 0; my_nn = (bnn & my_lanes) != 0; }
        };
        if (one_column) {
            // four load instructions in flight before the first verdict
            for (int it0 = 0; it0 < LPR; it0 += 4) {
                if (!((todo >> (it0 << lgR)) & low_bits(4 << lgR))) continue;
                double v[4];
                bool act[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int r = ((it0 + u) << lgR) + sub;
                    act[u] = it0 + u < LPR && col0 < n && ((todo >> (r & 63)) & 1ull);
                    v[u] = act[u] ? V[(r0 + r) * (long)ld + col0] : l0;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const double d = fabs(v[u] - l0);
                    verdicts(it0 + u, act[u], act[u] && !finite(v[u]), act[u] && !(d <= bound0), d);
                }
            }
        } else {
            for (int it = 0; it < LPR; it++) {
                if (!((todo >> it) & 1ull)) continue;               // LPR = 64: one row per instruction, every lane on it
                bool nf = false, nn = false;
                double dmax = 0.0;
                const double *__restrict__ row = V + (r0 + it) * (long)ld;
#pragma unroll 4
                for (int col = col0; col < n; col += 64) {
                    const double v = row[col];
                    double l, bound;
                    if (col < kGroupLdsCols) { l = sL[col]; bound = sBound[col]; }
                    else { l = L[col]; bound = atol + rtol * fabs(l); }
                    const double d = fabs(v - l);
                    nf |= !finite(v);
                    nn |= !(d <= bound);
                    dmax = fmax(dmax, d);
                }
                verdicts(it, true, nf, nn, dmax);
            }
        }
        const bool joined = mine && !my_nf && !my_nn, left = mine && !my_nf && my_nn;
        if (mine && my_nf) label[myrow] = kGroupNotFinite;
        else if (joined) label[myrow] = g;
        joined_total += __popcll(__ballot(joined));
        const unsigned long long rem = __ballot(left);
        if (rem && remains < 0) remains = r0 + __ffsll((long long)rem) - 1;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) wr = fmax(wr, __shfl_xor(wr, m));
    if (w.lane == 0) {
        if (joined_total > 0) {
            atomicAdd(&count[g], joined_total);
            atomicMax(reinterpret_cast<unsigned long long *>(&radius[g]), (unsigned long long)__double_as_longlong(wr));
        }
        if (remains >= 0 && remains < (long)relaxed_load(&next[g + 1])) atomicMin(&next[g + 1], (int)remains);
    }
}

// ---- K_group_final: the numbers of overflow (still unassigned), not-finite and masked rows into summary[1 .. 3] ---------------------
__global__ __launch_bounds__(256) void group_final_kernel(int B, const int *__restrict__ label, int *__restrict__ summary)
{
    const WaveId w = wave_id();
    const long tiles = ((long)B + 63) / 64;
    int over = 0, notfinite = 0, masked = 0;
    for (long tile = w.wave; tile < tiles; tile += w.waves) {
        const long myrow = tile * 64 + w.lane;
        const int lab = myrow < B ? label[myrow] : 0;
        over += __popcll(__ballot(lab == kGroupUnassigned));
        notfinite += __popcll(__ballot(lab == kGroupNotFinite));
        masked += __popcll(__ballot(lab == kGroupMasked));
    }
    if (w.lane == 0) {
        if (over) atomicAdd(&summary[1], over);
        if (notfinite) atomicAdd(&summary[2], notfinite);
        if (masked) atomicAdd(&summary[3], masked);
    }
}

// workgroups of four waves, at most four waves per SIMD over the chip (all resident at once at the round kernel's registers, four
// loads in flight each): a wave then walks several tiles and pays its atomics once
unsigned group_grid(int B)
{
    const long tiles = ((long)B + 63) / 64, waves = tiles < 4L * kNumSIMD ? tiles : 4L * kNumSIMD;
    return (unsigned)((waves + 3) / 4);
}

}  // namespace

hipError_t group_begin(hipStream_t st, int B, int n, int ld, const double *V, const int *mask, int max_groups, int *label, int *leader,
                       int *count, double *radius, int *summary, int *next)
{
    hipLaunchKernelGGL(group_fill_kernel, dim3((unsigned)(((long)max_groups + 1 + 255) / 256)), dim3(256), 0, st, max_groups, leader, count, radius,
                       summary, next);
    if (B > 0) hipLaunchKernelGGL(group_init_kernel, dim3(group_grid(B)), dim3(256), 0, st, B, n, ld, V, mask, label, next);
    return hipGetLastError();
}

hipError_t group_round(hipStream_t st, int B, int n, int ld, const double *V, double atol, double rtol, int g, int *label, int *leader,
                       int *count, double *radius, int *summary, int *next)
{
    if (B <= 0) return hipSuccess;
    int lgL = 0;
    while (lgL < 6 && (1 << lgL) < n) lgL++;
    const size_t lds = 2 * sizeof(double) * (size_t)(n < kGroupLdsCols ? n : kGroupLdsCols);
    hipLaunchKernelGGL(group_round_kernel, dim3(group_grid(B)), dim3(256), lds, st, B, n, ld, lgL, V, atol, rtol, g, label, leader, count, radius,
                       summary, next);
    return hipGetLastError();
}

hipError_t group_end(hipStream_t st, int B, const int *label, int *summary)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(group_final_kernel, dim3(group_grid(B)), dim3(256), 0, st, B, label, summary);
    return hipGetLastError();
}

}  // namespace socp
