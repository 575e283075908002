// hamiltonian_model.hpp -- the costate equations of a model from its Hamiltonian text alone (socp_hamiltonian_gradient_batch, and
// plugin::FromHamiltonian: a model that brings control_only and hamiltonian_t and nothing else), their Jacobian
// (socp_hamiltonian_jacobian_batch) and plugin::FromHamiltonianExact, which gives such a model the exact-derivative entries.
//
// symplectic_gradient is G = (dH/dp, -dH/dx) of the function the model's hamiltonian_t computes, X -> H(X, u(X)), the control law
// INSIDE: the TOTAL derivative, taken by forward-mode numbers (dualn.hpp) through the text as it stands.  What that is worth:
//   * it EQUALS Pontryagin's equations x' = dH/dp, p' = -dH/dx (partials at fixed u) wherever the law u(X) minimises H(X, .) over a
//     set that does not depend on X: the extra term dH/du du/dX vanishes at an interior minimiser, and on the boundary of the set it
//     is a multiplier times the derivative of a constraint X does not move (envelope theorem).  Goddard's smooth law, its bang and
//     off arcs, the double integrator's saturated control and the osc1d examples are such laws;
//   * at a kink (a clamp that opens, a penalty that starts, a switching time) it differentiates the BRANCH TAKEN at X, the one the
//     value parts select, like every dual-number kernel here;
//   * a law that is NOT such a minimiser -- a prescribed feedback, an approximation, a set that moves with X -- gives a G that is not
//     the costate equation: that model needs a hand-written rhs.  Goddard's closed-form singular control is one off the singular
//     surface: G - rhs = Switch (d alpha/dp, -d alpha/dx) there (tests/test_hamiltonian_model_cpu.py).  Where a hand-written rhs and G disagree, one of the two texts does
//     not belong to the other: socp_hamiltonian_gradient_batch against SOCP_EVAL_RHS is the check.
// The definition down to the operation order is in include/socp_hip.h ("HAMILTONIAN GRADIENT"); tests/hamiltonian_model_reference.py
// restates it bit for bit.  MUST be compiled with -ffp-contract=off.
#pragma once
#include <type_traits>
#include <utility>

#include "dualn.hpp"

namespace socp {

// optional model hint kGradientWidth: the derivative parts a pass of symplectic_gradient carries (1 .. S); the gradient takes
// ceil(S / W) passes through hamiltonian_t.  Without the hint: S, one pass.  The width changes registers and time, never a bit
// (dualn.hpp)
template <class M, class = void> struct gradient_width : std::integral_constant<int, M::S> {};
template <class M> struct gradient_width<M, std::void_t<decltype(M::kGradientWidth)>> : std::integral_constant<int, M::kGradientWidth> {};

// optional model hint kNestedGradientWidth: the same for the gradient on the carrier Dual (FromHamiltonianExact's rhs_t<Dual> and the
// Jacobian call), whose numbers are 2 (1 + W) doubles.  Without the hint: gradient_width.  A hint of its own because every pass
// recomputes the value part: a width chosen for the nested kernels' registers would slow the plain right-hand side down (measured on
// dint_hx: one residual launch 4.5 x dint_h's with W = 2 for both)
template <class M, class = void> struct nested_gradient_width : gradient_width<M> {};
template <class M> struct nested_gradient_width<M, std::void_t<decltype(M::kNestedGradientWidth)>> : std::integral_constant<int, M::kNestedGradientWidth> {};
template <class M, class T> struct carrier_gradient_width : std::conditional_t<std::is_same<T, double>::value, gradient_width<M>, nested_gradient_width<M>> {};

// G[i] = dH/dX[i + D], G[i + D] = -(dH/dX[i]) for i < D, H = Mdl::hamiltonian_t at (P, sw0, sw1, t, X).  Pass q seeds
// X[i] = (X[i], e_i restricted to the directions q W .. q W + W - 1); a direction at or beyond S has an all-zero seed and is dropped.
// The passes are a LOOP, not unrolled copies: the compiler interleaves unrolled passes and their registers add up.
// The CARRIER T of X and G is double, or Dual for the gradient of the gradient (dualn.hpp; include/socp_hip.h, "NESTED DUAL
// NUMBERS"): the seeds are then T(1.0) = (1.0, +0.0) and T(0.0) = (0.0, +0.0), the minus of G[i + D] is Dual's, and the value parts
// of G are the bits of the T = double gradient.
template <class Mdl, int W = gradient_width<Mdl>::value, class T = double, class PV>
__device__ __forceinline__ void symplectic_gradient(const PV &P, double sw0, double sw1, double t, const T (&X)[Mdl::S], T (&G)[Mdl::S])
{
    constexpr int S = Mdl::S, D = Mdl::D;
    static_assert(W >= 1 && W <= S, "1 <= W <= S");
    constexpr int passes = (S + W - 1) / W;
    using N = DualN<W, T>;
    if constexpr (passes == 1) {
        N Y[S];
#pragma unroll
        for (int i = 0; i < S; i++) {
            Y[i].v = X[i];
#pragma unroll
            for (int k = 0; k < W; k++) Y[i].d[k] = (i == k) ? T(1.0) : T(0.0);
        }
        const N H = Mdl::template hamiltonian_t<N>(P, sw0, sw1, t, Y);
#pragma unroll
        for (int i = 0; i < D; i++) {
            G[i] = H.d[i + D];
            G[i + D] = -H.d[i];
        }
    } else {
#pragma unroll 1
        for (int q = 0; q < passes; q++) {
            N Y[S];
#pragma unroll
            for (int i = 0; i < S; i++) {
                Y[i].v = X[i];
#pragma unroll
                for (int k = 0; k < W; k++) Y[i].d[k] = (i == q * W + k) ? T(1.0) : T(0.0);
            }
            const N H = Mdl::template hamiltonian_t<N>(P, sw0, sw1, t, Y);
#pragma unroll
            for (int k = 0; k < W; k++) {
                const int j = q * W + k;                 // the direction: dH/dX[j]
#pragma unroll
                for (int i = 0; i < D; i++) {
                    if (j == i + D) G[i] = H.d[k];
                    if (j == i) G[i + D] = -H.d[k];
                }
            }
        }
    }
}

// K_hgrad: symplectic_gradient for a batch of (t, X) points, the arguments of eval_lane_kernel: one lane per point, G[B][S]
template <class Mdl>
__global__ __launch_bounds__(64) void hamiltonian_gradient_kernel(ModelParams P, int B, const double *__restrict__ t,
                                                                  const double *__restrict__ sw, const double *__restrict__ Xin,
                                                                  double *__restrict__ out)
{
    constexpr int S = Mdl::S;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double X[S], G[S];
#pragma unroll
    for (int k = 0; k < S; k++) X[k] = Xin[(long)b * S + k];
    const double s0 = sw ? sw[2 * b] : P.sw0;
    const double s1 = sw ? sw[2 * b + 1] : P.sw1;
    symplectic_gradient<Mdl>(P, s0, s1, t[b], X, G);
#pragma unroll
    for (int k = 0; k < S; k++) out[(long)b * S + k] = G[k];
}

// K_hjac: A = dG/dX of symplectic_gradient for a batch of (t, X) points (socp_hamiltonian_jacobian_batch; include/socp_hip.h,
// "NESTED DUAL NUMBERS"): one lane per point, A[B][S * S] column-major, A[S j + i] = dG_i/dX_j, and the value parts into G[B][S]
// unless null.  Column j is the derivative part of symplectic_gradient<Mdl, W, Dual> at X seeded with (X, e_j); the S outer
// directions are a LOOP like the passes inside, so the registers are those of one nested gradient.  No LDS.  W: the derivative parts
// of an inner pass, chosen for registers: the width changes no bit.
template <class Mdl, int W>
__global__ __launch_bounds__(64) void hamiltonian_jacobian_kernel(ModelParams P, int B, const double *__restrict__ t,
                                                                  const double *__restrict__ sw, const double *__restrict__ Xin,
                                                                  double *__restrict__ A, double *__restrict__ Gout)
{
    constexpr int S = Mdl::S;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double X[S];
#pragma unroll
    for (int k = 0; k < S; k++) X[k] = Xin[(long)b * S + k];
    const double s0 = sw ? sw[2 * b] : P.sw0;
    const double s1 = sw ? sw[2 * b + 1] : P.sw1;
    const double tb = t[b];
    double *const Ab = A + (long)b * S * S;
#pragma unroll 1
    for (int j = 0; j < S; j++) {
        Dual Y[S], G[S];
#pragma unroll
        for (int k = 0; k < S; k++) Y[k] = Dual(X[k], k == j ? 1.0 : 0.0);
        symplectic_gradient<Mdl, W, Dual>(P, s0, s1, tb, Y, G);
#pragma unroll
        for (int k = 0; k < S; k++) Ab[S * j + k] = G[k].d;
        if (Gout && j == 0) {
#pragma unroll
            for (int k = 0; k < S; k++) Gout[(long)b * S + k] = G[k].v;
        }
    }
}

namespace plugin {

template <class M, class = void> struct has_switching_fn : std::false_type {};
template <class M>
struct has_switching_fn<M, std::void_t<decltype(M::switching_fn(std::declval<const ModelParams &>(), 0.0, 0.0, 0.0,
                                                                 std::declval<const double (&)[M::S]>(),
                                                                 std::declval<const double (&)[M::S]>()))>> : std::true_type {};

// Mdl's own free-interior-time row, or the reference's default H(t, X-) - H(t, X+) (model.hpp:299-304) when it has none
template <class Mdl, bool OWN = has_switching_fn<Mdl>::value> struct HamiltonianSwitching : Mdl {};
template <class Mdl> struct HamiltonianSwitching<Mdl, false> : Mdl {
    __device__ static double switching_fn(const ModelParams &P, double sw0, double sw1, double t, const double (&X)[Mdl::S],
                                          const double (&Xp)[Mdl::S])
    {
        return Mdl::template hamiltonian_t<double>(P, sw0, sw1, t, X) - Mdl::template hamiltonian_t<double>(P, sw0, sw1, t, Xp);
    }
};

// A model written from its Hamiltonian alone.  Mdl brings D, S, NU, kRefOrder, control_only and hamiltonian_t (and, if it likes,
// event channels, observables, a switching_fn of its own: they pass through); the adaptor adds
//   rhs          = symplectic_gradient (see the head of this file for what that equals)
//   hamiltonian  = hamiltonian_t<double>
//   switching_fn = H(t, X-) - H(t, X+) unless Mdl has one.
// Every launch-table kernel that reads rhs, hamiltonian or switching_fn then runs unchanged.  The model has NO rhs_t (the gradient of
// a gradient needs nested dual numbers), so the fields, exact_jacobian and sensitivity entries stay empty.  FromHamiltonianExact below
// is the opt-in adaptor that takes the gradient on nested numbers and has them.
template <class Mdl>
struct FromHamiltonian : HamiltonianSwitching<Mdl> {
    static constexpr int S = Mdl::S;
    __device__ static __forceinline__ void rhs(const ModelParams &P, double sw0, double sw1, double t, const double (&X)[S], double (&dX)[S])
    {
        symplectic_gradient<Mdl>(P, sw0, sw1, t, X, dX);
    }
    __device__ static __forceinline__ double hamiltonian(const ModelParams &P, double sw0, double sw1, double t, const double (&X)[S])
    {
        return Mdl::template hamiltonian_t<double>(P, sw0, sw1, t, X);
    }
    static void rhs_t() = delete;                      // hides an rhs_t of Mdl: it would not be the text of this rhs
};

// The free-interior-time row over a number type for the default H(t, X-) - H(t, X+); a model that brings a switching_fn of its own
// brings its switching_fn_t (and kSwitchingReadsXp) too, or has no exact-Jacobian entry
template <class Mdl, bool OWN = has_switching_fn<Mdl>::value> struct HamiltonianSwitchingT {};
template <class Mdl> struct HamiltonianSwitchingT<Mdl, false> {
    static constexpr bool kSwitchingReadsXp = true;
    template <class T, class PV>
    __device__ static __forceinline__ auto switching_fn_t(const PV &P, double sw0, double sw1, double t, const T (&X)[Mdl::S],
                                                          const T (&Xp)[Mdl::S]) -> decltype(Mdl::template hamiltonian_t<T>(P, sw0, sw1, t, X))
    {
        return Mdl::template hamiltonian_t<T>(P, sw0, sw1, t, X) - Mdl::template hamiltonian_t<T>(P, sw0, sw1, t, Xp);
    }
};

// FromHamiltonian plus the three texts over a number type, so that the model has exact fields, the exact shooting Jacobian and -- when
// its hamiltonian_t is generic in the parameter view -- exact sensitivities (plugin_impl.hpp: has_fields, has_exact_jacobian,
// has_sensitivity; the kernels are the unchanged ones):
//   rhs_t<T, PV>          = symplectic_gradient on the carrier T, the parameter view passed through.  T = double: rhs itself.
//                           T = Dual: the gradient taken on NESTED numbers DualN<W, Dual>; its value parts are rhs's bits
//   hamiltonian_t<T, PV>  = Mdl's own text
//   switching_fn_t<T, PV> = H(t, X-) - H(t, X+) with kSwitchingReadsXp = true, unless Mdl has a switching_fn of its own.
// Opt-in (SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT): Mdl's hamiltonian_t must instantiate on DualN<W, Dual>, and the nested kernels take
// more registers than FromHamiltonian's -- choose kNestedGradientWidth for them.
template <class Mdl>
struct FromHamiltonianExact : FromHamiltonian<Mdl>, HamiltonianSwitchingT<Mdl> {
    static constexpr int S = Mdl::S;
    template <class T, class PV>
    __device__ static __forceinline__ void rhs_t(const PV &P, double sw0, double sw1, double t, const T (&X)[S], T (&dX)[S])
    {
        symplectic_gradient<Mdl, carrier_gradient_width<Mdl, T>::value>(P, sw0, sw1, t, X, dX);
    }
};

}  // namespace plugin
}  // namespace socp
