/*
 * ref_interceptor_driver.cpp -- C-ABI shim over the REFERENCE's own interceptor object (test infrastructure).
 *
 * oracle/Makefile compiles this file with the reference's models/interceptor/interceptor.cpp, which it names by
 * path on the compiler's command line (-include: that file is read first, as it lies, into this translation unit)
 * against oracle/eigen_shim, the stand-in for the three things it uses of Eigen.  One translation unit because the
 * stage and chart flags, the step count, the Earth radius, the gravity constant and the chart limit live in
 * interceptor::data_struct, which only interceptor.cpp defines; -fno-access-control lets the entry points below
 * reach it and the private ConversionState12/21 and ComputeMass.  Neither changes the arithmetic the compiler
 * emits for the reference's functions.  No reference source is copied into this repository.
 *
 * The result, oracle/_ref/libsocp_ref_interceptor.so, pins oracle/interceptor_oracle.c through
 * tests/golden/make_interceptor_pin_golden.py (which records its doubles) and tests/test_interceptor_pin_cpu.py
 * (which compares the C oracle with the record, bit for bit).
 */
#include <cstring>
#include <string>
#include <vector>

namespace {
model::mstate vec12(const double *X) { return model::mstate(X, X + 12); }
interceptor *obj(void *h) { return static_cast<interceptor *>(h); }
}  // namespace

extern "C" {

void *ref_icpt_new() { return new interceptor(std::string("")); }
void ref_icpt_free(void *h) { delete obj(h); }

/* p in the order of oracle/socp_oracle.h's IP_* slots: the 15 read members of parameters_struct, then R_Earth,
 * mu0, chartLimit */
void ref_icpt_set_params(void *h, const double *p, int step_nbr)
{
    interceptor *m = obj(h);
    interceptor::parameters_struct &q = m->GetParameterData();
    q.c0 = p[0]; q.hr = p[1]; q.d0 = p[2]; q.eta = p[3]; q.propellant_mass = p[4]; q.empty_mass = p[5];
    q.q = p[6]; q.ve = p[7]; q.alpha_max = p[8]; q.u_max = p[9]; q.a_max = p[10]; q.mu_gft = p[11];
    q.muT = p[12]; q.muV = p[13]; q.muC = p[14];
    m->data->R_Earth = p[15];
    m->data->mu0 = p[16];
    m->data->chartLimit = p[17];
    m->data->stepNbr = step_nbr;
}

void ref_icpt_get_params(void *h, double *p, int *step_nbr)
{
    interceptor *m = obj(h);
    const interceptor::parameters_struct &q = m->GetParameterData();
    const double v[18] = { q.c0, q.hr, q.d0, q.eta, q.propellant_mass, q.empty_mass, q.q, q.ve, q.alpha_max, q.u_max,
                           q.a_max, q.mu_gft, q.muT, q.muV, q.muC, m->data->R_Earth, m->data->mu0, m->data->chartLimit };
    std::memcpy(p, v, sizeof(v));
    *step_nbr = m->data->stepNbr;
}

void ref_icpt_set_flags(void *h, int chart, int stage)
{
    obj(h)->data->currentChart = chart;
    obj(h)->data->stageMode = stage;
}

void ref_icpt_get_flags(void *h, int *chart, int *stage)
{
    *chart = obj(h)->data->currentChart;
    *stage = obj(h)->data->stageMode;
}

/* Model, Control, Hamiltonian at the flags in force, through the virtual interface */
void ref_icpt_rhs(void *h, double t, const double *X, double *out)
{
    model *m = obj(h);
    model::mstate d = m->Model(t, vec12(X), 0);
    std::memcpy(out, d.data(), sizeof(double) * 12);
}

void ref_icpt_control(void *h, double t, const double *X, double *out)
{
    model *m = obj(h);
    model::mcontrol u = m->Control(t, vec12(X));
    std::memcpy(out, u.data(), sizeof(double) * 2);
}

double ref_icpt_hamiltonian(void *h, double t, const double *X)
{
    model *m = obj(h);
    return m->Hamiltonian(t, vec12(X), 0)[0];
}

double ref_icpt_mass(void *h, double t, const double *X) { return obj(h)->ComputeMass(t, vec12(X)); }

void ref_icpt_chart12(void *h, const double *X1, double *X2)
{
    model::mstate v = obj(h)->ConversionState12(vec12(X1));
    std::memcpy(X2, v.data(), sizeof(double) * 12);
}

void ref_icpt_chart21(void *h, const double *X2, double *X1)
{
    model::mstate v = obj(h)->ConversionState21(vec12(X2));
    std::memcpy(X1, v.data(), sizeof(double) * 12);
}

void ref_icpt_traj(void *h, double t0, const double *X0, double tf, double *Xf)
{
    model *m = obj(h);
    model::mstate v = m->ComputeTraj(t0, vec12(X0), tf, 0, 0);
    std::memcpy(Xf, v.data(), sizeof(double) * 12);
}

/* FinalFunction (6 rows) or FinalHFunction (7 rows: + H + muT at the flags in force) */
void ref_icpt_final(void *h, int with_h, double tf, const double *Xtf, const double *Xf, const int *mode_x, double *out)
{
    model *m = obj(h);
    std::vector<int> md(mode_x, mode_x + 6);
    std::vector<real> f(with_h ? 7 : 6, 0.0);
    if (with_h) m->FinalHFunction(tf, vec12(Xtf), vec12(Xf), md, f, 0);
    else m->FinalFunction(tf, vec12(Xtf), vec12(Xf), md, f, 0);
    std::memcpy(out, f.data(), sizeof(double) * f.size());
}

/* Xi[0..6) in, Xi[6..12) out */
void ref_icpt_init_analytical(void *h, double ti, double *Xi, double tf, const double *Xf)
{
    model::mstate a = vec12(Xi), b = vec12(Xf);
    obj(h)->InitAnalytical(ti, a, tf, b);
    std::memcpy(Xi, a.data(), sizeof(double) * 12);
}

}  // extern "C"
