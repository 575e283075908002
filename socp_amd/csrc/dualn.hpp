// dualn.hpp -- forward-mode numbers with W derivative parts (v, d[0 .. W)) in ONE lane, for symplectic_gradient
// (hamiltonian_model.hpp).  Component k of every rule is Dual's rule (dual.hpp; include/socp_hip.h, "DUAL NUMBERS") on (v, d[k]), one
// IEEE rounding per listed step; the translation unit that uses them is built with -ffp-contract=off, so nothing is fused.  The value
// part is computed ONCE, and so is every intermediate that reads value parts only (a quotient's q, a root's s + s).  The components
// never meet: what component k holds does not depend on W, nor on which other directions travel beside it -- a gradient may be cut
// into passes of any width and gives the same bits (tests/hamiltonian_model_reference.py restates the rules and checks just that).
// A plain double takes part through the mixed overloads, which DROP its zero derivative terms, as in dual.hpp.  There is no implicit
// conversion from double.
//
// The CARRIER T of the parts is double (DualN<W>, the gradient) or Dual (DualN<W, Dual>, the NESTED number: the gradient of a
// gradient; include/socp_hip.h, "NESTED DUAL NUMBERS").  The rules are written once: every listed operation is carried out in T, so
// with T = Dual it is dual.hpp's operation with its own listed roundings, and the value part of a DualN<W, Dual> operation is the
// DualN<W> operation, step for step.  A plain T -- a parameter read through SeededParams -- is plain at the OUTER level (its outer
// zero terms are dropped) and a full Dual at the inner one.  Seeds and the zero of d_sqrt are explicit T(1.0) / T(0.0): for Dual
// (1.0, +0.0) and (0.0, +0.0), computed with like any other number.  tests/hamiltonian_exact_reference.py restates the nested rules.
#pragma once
#include <type_traits>

#include "dual.hpp"

namespace socp {

template <int W, class T = double>
struct DualN {
    static_assert(W >= 1, "at least one derivative part");
    static_assert(std::is_same<T, double>::value || std::is_same<T, Dual>::value, "the carrier is double or Dual");
    T v, d[W];
    __device__ __forceinline__ DualN() {}
    __device__ __forceinline__ explicit DualN(double c) : v(c)
    {
#pragma unroll
        for (int k = 0; k < W; k++) d[k] = T(0.0);
    }
};

// a plain number of type C beside a DualN<W, T>: an arithmetic type (it takes part as a double), or the carrier itself when that is Dual
template <class C, class T>
using if_plain = std::enable_if_t<std::is_arithmetic<C>::value || (std::is_same<C, Dual>::value && std::is_same<T, Dual>::value), int>;

// a +- b, -a
template <int W, class T> __device__ __forceinline__ DualN<W, T> operator+(const DualN<W, T> &a, const DualN<W, T> &b)
{
    DualN<W, T> r;
    r.v = a.v + b.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k] + b.d[k];
    return r;
}
template <int W, class T> __device__ __forceinline__ DualN<W, T> operator-(const DualN<W, T> &a, const DualN<W, T> &b)
{
    DualN<W, T> r;
    r.v = a.v - b.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k] - b.d[k];
    return r;
}
template <int W, class T> __device__ __forceinline__ DualN<W, T> operator-(const DualN<W, T> &a)
{
    DualN<W, T> r;
    r.v = -a.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = -a.d[k];
    return r;
}
// a b = (a.v b.v, (a.d b.v) + (a.v b.d))
template <int W, class T> __device__ __forceinline__ DualN<W, T> operator*(const DualN<W, T> &a, const DualN<W, T> &b)
{
    DualN<W, T> r;
    r.v = a.v * b.v;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const T l = a.d[k] * b.v;
        const T m = a.v * b.d[k];
        r.d[k] = l + m;
    }
    return r;
}
// a / b: q = a.v / b.v; (q, (a.d - q b.d) / b.v)
template <int W, class T> __device__ __forceinline__ DualN<W, T> operator/(const DualN<W, T> &a, const DualN<W, T> &b)
{
    DualN<W, T> r;
    const T q = a.v / b.v;
    r.v = q;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const T m = q * b.d[k];
        r.d[k] = (a.d[k] - m) / b.v;
    }
    return r;
}

// a plain number c (a double, or a plain T when T = Dual): its zero derivative terms are dropped, not computed
template <int W, class T, class C, if_plain<C, T> = 0> __device__ __forceinline__ DualN<W, T> operator+(C c, const DualN<W, T> &a)
{
    DualN<W, T> r;
    r.v = c + a.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k];
    return r;
}
template <int W, class T, class C, if_plain<C, T> = 0> __device__ __forceinline__ DualN<W, T> operator+(const DualN<W, T> &a, C c)
{
    DualN<W, T> r;
    r.v = a.v + c;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k];
    return r;
}
template <int W, class T, class C, if_plain<C, T> = 0> __device__ __forceinline__ DualN<W, T> operator-(C c, const DualN<W, T> &a)
{
    DualN<W, T> r;
    r.v = c - a.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = -a.d[k];
    return r;
}
template <int W, class T, class C, if_plain<C, T> = 0> __device__ __forceinline__ DualN<W, T> operator-(const DualN<W, T> &a, C c)
{
    DualN<W, T> r;
    r.v = a.v - c;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k];
    return r;
}
template <int W, class T, class C, if_plain<C, T> = 0> __device__ __forceinline__ DualN<W, T> operator*(C c, const DualN<W, T> &a)
{
    DualN<W, T> r;
    r.v = c * a.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = c * a.d[k];
    return r;
}
template <int W, class T, class C, if_plain<C, T> = 0> __device__ __forceinline__ DualN<W, T> operator*(const DualN<W, T> &a, C c)
{
    DualN<W, T> r;
    r.v = a.v * c;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k] * c;
    return r;
}
template <int W, class T, class C, if_plain<C, T> = 0> __device__ __forceinline__ DualN<W, T> operator/(const DualN<W, T> &a, C c)
{
    DualN<W, T> r;
    r.v = a.v / c;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k] / c;
    return r;
}
// c / a: q = c / a.v; (q, (-(q a.d)) / a.v)
template <int W, class T, class C, if_plain<C, T> = 0> __device__ __forceinline__ DualN<W, T> operator/(C c, const DualN<W, T> &a)
{
    DualN<W, T> r;
    const T q = c / a.v;
    r.v = q;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const T m = q * a.d[k];
        r.d[k] = (-m) / a.v;
    }
    return r;
}

// the value a comparison reads: the innermost one
template <int W, class T> __device__ __forceinline__ double d_val(const DualN<W, T> &a) { return d_val(a.v); }
// |a| acts on all parts: every d flips when the value is < 0
template <int W, class T> __device__ __forceinline__ DualN<W, T> d_abs(const DualN<W, T> &a)
{
    DualN<W, T> r;
    r.v = d_abs(a.v);
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = d_val(a.v) < 0.0 ? -a.d[k] : a.d[k];
    return r;
}
// sqrt a: s = sqrt(a.v); (s, a.d / (s + s)), the derivatives T(0.0) when the value of s is 0
template <int W, class T> __device__ __forceinline__ DualN<W, T> d_sqrt(const DualN<W, T> &a)
{
    DualN<W, T> r;
    const T s = d_sqrt(a.v);
    const T s2 = s + s;
    r.v = s;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const T q = a.d[k] / s2;
        r.d[k] = d_val(s) == 0.0 ? T(0.0) : q;
    }
    return r;
}
// exp a: e = exp(a.v) (exp_glibc on the innermost value); (e, e a.d)
template <int W, class T> __device__ __forceinline__ DualN<W, T> d_exp(const DualN<W, T> &a)
{
    DualN<W, T> r;
    const T e = d_exp(a.v);
    r.v = e;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = e * a.d[k];
    return r;
}

}  // namespace socp
