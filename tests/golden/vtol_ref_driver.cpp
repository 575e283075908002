// vtol_ref_driver.cpp -- authoring-container tool of make_vtol_golden.py: instantiates the REFERENCE's own obstacle and
// vtolUAV objects (its headers and sources are given to the compiler by path, in a temporary directory) and evaluates
// them at the points read from standard input.  One request per line, one line of %.17g numbers per answer:
//   P <13 packed parameters>                 set the model's and the map's parameters (SOCP_VTOL_NPARAMS order)
//   E <X[12]>                                Model(12) Control(3) Hamiltonian(1) map Function(1) map Gradient(3)
//   M <x y z>                                map Function(1) Gradient(3)
//   I <t0> <tf> <X[12]>                      ModelInt(t0, X, tf) (12)
//   F <mode[6]> <X[12]> <Xf[6]>              FinalFunction rows (6), FinalHFunction rows (7)
//   S <X[12]> <Xp[12]> <Xd[6]>               SwitchingStateFunction for stateID 0..5, fvec (12)
//   W                                        the waypoint path: count, then 6 numbers per waypoint
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#define private public
#include "models/vtolUAV/vtolUAV.hpp"
#undef private
#include "maps/obstacle/obstacle.hpp"

static void out(const std::vector<real> &v)
{
    for (size_t k = 0; k < v.size(); k++) std::printf("%s%.17g", k ? " " : "", v[k]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 3) return 64;
    obstacle o(argv[1], argv[2]);
    vtolUAV m(o, "");
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char c;
        in >> c;
        std::vector<real> a;
        real v;
        while (in >> v) a.push_back(v);
        std::vector<real> r;
        if (c == 'P') {
            vtolUAV::parameters_struct &p = m.GetParameterData();
            p.u_max = a[0]; p.a_max = a[1]; p.alphaT = a[2]; p.alphaV = a[3]; p.invSigmaXwp = a[4]; p.Vd = a[5]; p.ca = a[6];
            p.nWP_tot = (int)a[7]; p.nWP = (int)a[8];
            obstacle::parameters_struct &q = o.GetParameterData();
            q.phiObs = a[9]; q.psiWP = a[10]; q.muObs = a[11]; q.sigmaWP = a[12];
            continue;
        }
        if (c == 'E' || c == 'M') {
            std::vector<real> pos(a.begin(), a.begin() + 3), g(3, 0);
            real f = 0;
            if (c == 'E') {
                const model::mstate X(a.begin(), a.begin() + 12);
                r = m.Model(0.0, X, 0);
                const model::mcontrol u = m.Control(0.0, X);
                r.insert(r.end(), u.begin(), u.end());
                r.push_back(m.Hamiltonian(0.0, X, 0)[0]);
            }
            o.Function(pos, f);
            o.Gradient(pos, g);
            r.push_back(f);
            r.insert(r.end(), g.begin(), g.end());
        } else if (c == 'I') {
            const model::mstate X(a.begin() + 2, a.begin() + 14);
            r = m.ModelInt(a[0], X, a[1], 0, 0);
        } else if (c == 'F') {
            std::vector<int> mode(6);
            for (int j = 0; j < 6; j++) mode[j] = (int)a[j];
            const model::mstate X(a.begin() + 6, a.begin() + 18);
            model::mstate Xf(12, 0);
            for (int j = 0; j < 6; j++) Xf[j] = a[18 + j];
            std::vector<real> f(6, 0), fh(7, 0);
            m.FinalFunction(0.0, X, Xf, mode, f, 0);
            m.FinalHFunction(0.0, X, Xf, mode, fh, 0);
            r = f;
            r.insert(r.end(), fh.begin(), fh.end());
        } else if (c == 'S') {
            const model::mstate X(a.begin(), a.begin() + 12), Xp(a.begin() + 12, a.begin() + 24);
            model::mstate Xd(12, 0), f(12, 0);
            for (int j = 0; j < 6; j++) Xd[j] = a[24 + j];
            for (int j = 0; j < 6; j++) m.SwitchingStateFunction(0.0, j, X, Xp, Xd, f, 0);
            r = f;
        } else if (c == 'W') {
            const std::vector<std::vector<real>> &path = o.GetPath();
            r.push_back((real)path.size());
            for (size_t i = 0; i < path.size(); i++) r.insert(r.end(), path[i].begin(), path[i].end());
        }
        out(r);
    }
    return 0;
}
