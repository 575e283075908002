// vtol_flow.cpp -- the workload of the reference's tests/testVtolUAV.cpp as a checkable program: the same set-up and
// API calls (path continuation that adds one waypoint and one shooting segment per solve, then three parameter
// continuations), one JSON line per SolveOCP.
//   vtol_flow <xtol> <modeMPP> <sigma> <mu> [max_waypoints]
// The data directory (files `obstacles` and `waypoints`) comes from SOCP_VTOL_DATA.  max_waypoints cuts the path to its
// first max_waypoints + 1 points (nWP_tot follows, as it would with a shorter file).  SOCP_FLOW_THREADS = numThread handed to Resize (default 4, the reference program's value).
// With SOCP_FLOW_PRE set, every solve is preceded by a line {"pre": ...} that describes the problem about to be solved:
// modes, desired node times and states, packed parameters, the initial unknowns z0 and the residual F(z0).
// SOCP_FLOW_Z0_DIR: see pre().
//
// The program only uses the reference's public API, so it also compiles against the REFERENCE's own headers and
// sources (-DSOCP_REFERENCE_BUILD; tests/golden/make_vtol_golden.py does that in a temporary directory).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#ifdef SOCP_REFERENCE_BUILD
#define private public      // F(z0) of the reference: its residual callback is a private static member
#include "socp/shooting.hpp"
#undef private
#else
#include "socp/shooting.hpp"
#endif
#include "maps/obstacle/obstacle.hpp"
#include "models/vtolUAV/vtolUAV.hpp"

namespace {

bool g_pre = false;
int g_threads = 4;

void print_vec(const char *name, const std::vector<real> &v)
{
    std::printf("\"%s\": [", name);
    for (size_t k = 0; k < v.size(); k++) std::printf("%s%.17g", k ? ", " : "", v[k]);
    std::printf("]");
}

std::vector<real> packed_params(vtolUAV &m, obstacle &o)
{
    const vtolUAV::parameters_struct &p = m.GetParameterData();
    const obstacle::parameters_struct &q = o.GetParameterData();
    return {p.u_max, p.a_max, p.alphaT, p.alphaV, p.invSigmaXwp, p.Vd, p.ca, (real)p.nWP_tot, (real)p.nWP, q.phiObs, q.psiWP, q.muObs, q.sigmaWP};
}

// the problem a SolveOCP call is about to solve; vt / vX: the desired node times and states in force
void pre(const char *stage, vtolUAV &m, obstacle &o, const shooting &s, const std::vector<int> &mode_t, const std::vector<std::vector<int>> &mode_X,
         const std::vector<real> &vt, const std::vector<model::mstate> &vXd)
{
    if (!g_pre) return;
    std::vector<real> z0;
    s.GetParameters(z0);
    const int n = (int)z0.size();
    // SOCP_FLOW_Z0_DIR: exchange the points of evaluation between two builds of this program, so that both report F at the
    // SAME z0 -- "<dir>/<stage>.z0" is written when absent and read (replacing this run's own z0 in the report) when present
    if (const char *zdir = std::getenv("SOCP_FLOW_Z0_DIR")) {
        const std::string file = std::string(zdir) + "/" + stage + ".z0";
        std::ifstream in(file.c_str());
        if (in) {
            for (int k = 0; k < n; k++) in >> z0[k];
        } else {
            std::ofstream outf(file.c_str());
            outf.precision(17);
            for (int k = 0; k < n; k++) outf << z0[k] << "\n";
        }
    }
    std::vector<real> F(n, 0.0);
#ifdef SOCP_REFERENCE_BUILD
    // a second object with the same modes whose boundary tables ARE the desired ones (InitShooting sets both), evaluated at z0
    shooting probe(m, (int)vt.size() - 1, 1);
    probe.SetMode(mode_t, mode_X);
    probe.InitShooting(vt, vXd);
    shooting::StaticShootingFunction((void *)&probe, n, z0.data(), F.data(), 1);
#else
    F = s.ResidualAt(z0);
#endif
    std::printf("{\"pre\": \"%s\", \"nMulti\": %d, \"n\": %d, ", stage, (int)vt.size() - 1, n);
    std::printf("\"mode_t\": [");
    for (size_t k = 0; k < mode_t.size(); k++) std::printf("%s%d", k ? ", " : "", mode_t[k]);
    std::printf("], \"mode_X\": [");
    for (size_t i = 0; i < mode_X.size(); i++)
        for (size_t j = 0; j < mode_X[i].size(); j++) std::printf("%s%d", (i || j) ? ", " : "", mode_X[i][j]);
    std::printf("], ");
    print_vec("time", vt);
    std::vector<real> xd;
    for (size_t i = 0; i < vXd.size(); i++) xd.insert(xd.end(), vXd[i].begin(), vXd[i].begin() + 6);
    std::printf(", ");
    print_vec("xd", xd);
    std::printf(", ");
    print_vec("params", packed_params(m, o));
    std::printf(", ");
    print_vec("z0", z0);
    std::printf(", ");
    print_vec("F0", F);
    std::printf("}\n");
    std::fflush(stdout);
}

void report(const char *stage, int nMulti, int info, const shooting &s)
{
    std::vector<real> z;
    s.GetParameters(z);
    std::vector<int> calls = s.GetCallNumber();
    std::printf("{\"stage\": \"%s\", \"nMulti\": %d, \"info\": %d, \"nfev\": %d, \"n\": %d, ", stage, nMulti, info, calls[0], (int)z.size());
    print_vec("z", z);
    std::printf("}\n");
    std::fflush(stdout);
}

void waypoint_targets(std::vector<model::mstate> &vX, const std::vector<std::vector<real>> &path, int count)
{
    for (int i = 0; i < count; i++) {
        for (int k = 0; k < 3; k++) vX[i][k] = path[i][k];
        for (int k = 3; k < 6; k++) vX[i][k] = 0.001;      // a zero speed makes the right-hand side NaN (0/0 in the drag terms)
    }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: vtol_flow <xtol> <modeMPP> <sigma> <mu> [max_waypoints]\n");
        return 64;
    }
    const double xtol = std::atof(argv[1]);
    const int modeMPP = std::atoi(argv[2]);
    const real sigma = std::atof(argv[3]), mu = std::atof(argv[4]);
    const int max_wp = argc > 5 ? std::atoi(argv[5]) : 0;
    if (!(sigma > 0)) { std::fprintf(stderr, "sigma must be greater than 0\n"); return 64; }
    const char *dir = std::getenv("SOCP_VTOL_DATA");
    if (!dir) { std::fprintf(stderr, "SOCP_VTOL_DATA (directory of the obstacle and waypoint files) is not set\n"); return 64; }
    g_pre = std::getenv("SOCP_FLOW_PRE") != nullptr;
    if (const char *thr = std::getenv("SOCP_FLOW_THREADS")) g_threads = std::atoi(thr);

    obstacle my_obstacle(std::string(dir) + "/obstacles", std::string(dir) + "/waypoints");
    vtolUAV m(my_obstacle, "");
    std::vector<std::vector<real>> path = my_obstacle.GetPath();
    if (path.size() < 2) { std::fprintf(stderr, "no waypoint path in %s\n", dir); return 65; }
    if (max_wp > 0 && (int)path.size() > max_wp + 1) path.resize(max_wp + 1);
    if (modeMPP < 2) m.GetParameterData().nWP_tot = (int)path.size() - 1;
    shooting sh(m, 1, 1);
    sh.SetPrecision(xtol);
    m.SetODEIntPrecision(1e-5);
    const int d = m.GetDim();

    // ---- continuation along the path (testVtolUAV.cpp:162-335) ----
    int nMulti = 1;
    sh.Resize(nMulti, g_threads);
    m.GetParameterData().nWP = nMulti - 1;
    std::vector<int> mode_t(nMulti + 1);
    mode_t[0] = 0;
    mode_t[nMulti] = 1;
    std::vector<std::vector<int>> mode_X(nMulti + 1);
    mode_X[0] = std::vector<int>(d, 0);
    mode_X[nMulti] = std::vector<int>(d, modeMPP == 1 ? 0 : 1);
    for (int k = 3; k < 6; k++) mode_X[nMulti][k] = 1;
    sh.SetMode(mode_t, mode_X);
    std::vector<real> vt(nMulti + 1);
    vt[0] = 0;
    std::vector<model::mstate> vX(nMulti + 1, model::mstate(12, 0));
    waypoint_targets(vX, path, nMulti + 1);
    {
        // first guess: the minimum-energy transfer between the first two waypoints
        const real ex = vX[nMulti][0] - vX[0][0], ey = vX[nMulti][1] - vX[0][1], ez = vX[nMulti][2] - vX[0][2];
        const real dist = sqrt(ex * ex + ey * ey + ez * ez);
        const real T = pow(4.5 * dist * dist / m.GetParameterData().alphaT, 0.25);
        vt[nMulti] = T;
        vX[0][6] = -3 * ex / T / T / T;  vX[0][7] = -3 * ey / T / T / T;  vX[0][8] = -3 * ez / T / T / T;
        vX[0][9] = -3 * ex / T / T;      vX[0][10] = -3 * ey / T / T;     vX[0][11] = -3 * ez / T / T;
    }
    sh.InitShooting(vt, vX);
    std::vector<model::mstate> vXd = vX;        // desired states in force (InitShooting sets them from the guess)

    int info = 1, Nwp = nMulti;
    const int end = (int)path.size();
    char name[32];
    while (info == 1 && Nwp < end) {
        std::snprintf(name, sizeof name, "path_%d", nMulti);
        pre(name, m, my_obstacle, sh, mode_t, mode_X, vt, vXd);
        info = sh.SolveOCP(1.0);
        report(name, nMulti, info, sh);
        if (nMulti == 1 && info) {
            pre("ca", m, my_obstacle, sh, mode_t, mode_X, vt, vXd);
            info = sh.SolveOCP(0.1, m.GetParameterData().ca, 0.05);
            report("ca", nMulti, info, sh);
        }
        if (info != 1) break;
        sh.GetSolution(vt, vX);
        nMulti += 1;
        Nwp += 1;
        if (Nwp >= end) break;
        vt.resize(nMulti + 1);
        vX.resize(nMulti + 1);
        mode_t.resize(nMulti + 1);
        mode_X.resize(nMulti + 1);
        if (modeMPP < 2) m.GetParameterData().nWP += 1;
        if (modeMPP > 1) {
            const real tf = vt[nMulti - 1] + 0.4 * 10;
            for (int i = 0; i < nMulti + 1; i++) vt[i] = i * tf / nMulti;
            for (int i = 0; i < nMulti + 1; i++) vX[i] = sh.Move(vt[i]);
            mode_t[0] = 0;
            for (int i = 1; i < nMulti; i++) mode_t[i] = 2;
            mode_t[nMulti] = 1;
            mode_X[0] = std::vector<int>(d, 0);
            mode_X[nMulti] = std::vector<int>(d, 1);
            for (int i = 1; i < nMulti; i++) mode_X[i] = std::vector<int>(d, 2);
        } else {
            vt[nMulti] = vt[nMulti - 1] + 0.4 * 10;
            vX[nMulti] = sh.Move(vt[nMulti]);
            for (int i = 1; i < nMulti; i++) mode_t[i] = 1;
            mode_t[nMulti] = 1;
            mode_X[0] = std::vector<int>(d, 0);
            mode_X[nMulti] = std::vector<int>(d, modeMPP == 1 ? 0 : 1);
            if (nMulti < end - 1)
                for (int k = 3; k < 6; k++) mode_X[nMulti][k] = 1;
            for (int i = 1; i < nMulti; i++) {
                mode_X[i] = std::vector<int>(d, 1);
                for (int k = 3; k < 6; k++) mode_X[i][k] = 2;
                if (modeMPP == 1)
                    for (int k = 0; k < 3; k++) mode_X[i][k] = 0;
            }
        }
        sh.Resize(nMulti, g_threads);
        sh.SetMode(mode_t, mode_X);
        sh.InitShooting(vt, vX);
        waypoint_targets(vX, path, Nwp + 1);
        sh.SetDesiredState(vt, vX);
        vXd = vX;
    }
    const int M = nMulti - (info == 1 ? 1 : 0);

    // ---- continuation on model and map parameters (testVtolUAV.cpp:95-105) ----
    if (info == 1) {
        pre("invSigma", m, my_obstacle, sh, mode_t, mode_X, vt, vXd);
        info = sh.SolveOCP(1.0, m.GetParameterData().invSigmaXwp, 1 / sigma);
        report("invSigma", M, info, sh);
    }
    if (info == 1) {
        pre("muObs", m, my_obstacle, sh, mode_t, mode_X, vt, vXd);
        info = sh.SolveOCP(1.0, my_obstacle.GetParameterData().muObs, mu);
        report("muObs", M, info, sh);
    }
    if (info == 1) {
        pre("u_max", m, my_obstacle, sh, mode_t, mode_X, vt, vXd);
        info = sh.SolveOCP(1.0, m.GetParameterData().u_max, 1.0);
        report("u_max", M, info, sh);
    }
    return info == 1 ? 0 : 2;
}
