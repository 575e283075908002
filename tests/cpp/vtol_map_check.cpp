// vtol_map_check.cpp -- the host side of the vtolUAV mirror without a device: the obstacle map's file readers and its
// Function / Gradient, and the model's boundary-row functions, evaluated at the points read from standard input
// (tests/test_vtol_host.py compares them with reference-generated fixtures).  No context is created, no GPU is needed.
//   vtol_map_check <obstacle file> <waypoint file>
// One request per line, one line of %.17g numbers per answer:
//   P <13 packed parameters>            set the model's and the map's parameters (SOCP_VTOL_NPARAMS order)
//   T                                   the device table: obstacle count, then 7 numbers per obstacle
//   W                                   the waypoint path: count, then 6 numbers per waypoint
//   M <x y z>                           map Function (1), Gradient (3)
//   F <mode[6]> <X[12]> <Xf[6]>         FinalFunction rows (6), FinalHFunction rows 0..5 (6; its H row is the device's: left out here)
//   S <X[12]> <Xp[12]> <Xd[6]>          SwitchingStateFunction for stateID 0..5: fvec (12)
//   X                                   a vtolUAV over a map class WITHOUT the device hook: 1 when packing its parameters is refused
//                                       with an error that names the hook, else 0
#include <cstdio>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "maps/obstacle/obstacle.hpp"
#include "models/vtolUAV/vtolUAV.hpp"

// a map written for the reference: Function / Gradient only
class plain_map : public map
{
public:
    void Function(std::vector<real> const &, real &func) const override { func = 0; }
    void Gradient(std::vector<real> const &, std::vector<real> &grad) const override { grad.assign(3, 0); }
};

// the model with its Hamiltonian taken off the device, so that FinalHFunction -- the class's own rows 0..5, then H -- runs here
class host_rows_vtol : public vtolUAV
{
public:
    host_rows_vtol(map &the_map) : vtolUAV(the_map, "") {}

private:
    mstate Hamiltonian(real const &, mstate const &, int) const override { return mstate(1, 0.0); }
};

static void out(const std::vector<real> &v)
{
    for (size_t k = 0; k < v.size(); k++) std::printf("%s%.17g", k ? " " : "", v[k]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: vtol_map_check <obstacle file> <waypoint file>\n"); return 64; }
    obstacle o(argv[1], argv[2]);
    host_rows_vtol m(o);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char c = 0;
        in >> c;
        std::vector<real> a, r;
        real v;
        while (in >> v) a.push_back(v);
        if (c == 'P' && a.size() == 13) {
            vtolUAV::parameters_struct &p = m.GetParameterData();
            p.u_max = a[0]; p.a_max = a[1]; p.alphaT = a[2]; p.alphaV = a[3]; p.invSigmaXwp = a[4]; p.Vd = a[5]; p.ca = a[6];
            p.nWP_tot = (int)a[7]; p.nWP = (int)a[8];
            obstacle::parameters_struct &q = o.GetParameterData();
            q.phiObs = a[9]; q.psiWP = a[10]; q.muObs = a[11]; q.sigmaWP = a[12];
            continue;
        } else if (c == 'T') {
            std::vector<double> table;
            if (!o.DeviceMapTable(table)) return 3;
            r.push_back((real)(table.size() / 7));
            r.insert(r.end(), table.begin(), table.end());
        } else if (c == 'W') {
            const std::vector<std::vector<real>> &path = o.GetPath();
            r.push_back((real)path.size());
            for (size_t i = 0; i < path.size(); i++) r.insert(r.end(), path[i].begin(), path[i].end());
        } else if (c == 'M' && a.size() == 3) {
            std::vector<real> g(3, 0);
            real f = 0;
            o.Function(a, f);
            o.Gradient(a, g);
            r.push_back(f);
            r.insert(r.end(), g.begin(), g.end());
        } else if (c == 'F' && a.size() == 24) {
            std::vector<int> mode(6);
            for (int j = 0; j < 6; j++) mode[j] = (int)a[j];
            const model::mstate X(a.begin() + 6, a.begin() + 18);
            model::mstate Xf(12, 0);
            for (int j = 0; j < 6; j++) Xf[j] = a[18 + j];
            std::vector<real> f(6, 0), fh(7, 0);
            m.FinalFunction(0.0, X, Xf, mode, f, 0);
            m.FinalHFunction(0.0, X, Xf, mode, fh, 0);
            r = f;
            r.insert(r.end(), fh.begin(), fh.begin() + 6);
        } else if (c == 'S' && a.size() == 30) {
            const model::mstate X(a.begin(), a.begin() + 12), Xp(a.begin() + 12, a.begin() + 24);
            model::mstate Xd(12, 0), f(12, 0);
            for (int j = 0; j < 6; j++) Xd[j] = a[24 + j];
            for (int j = 0; j < 6; j++) m.SwitchingStateFunction(0.0, j, X, Xp, Xd, f, 0);
            r = f;
        } else if (c == 'X') {
            plain_map bare;
            vtolUAV over_bare(bare, "");
            double p[24];
            real refused = 0;
            try {
                over_bare.DeviceParams(p, 24);
            } catch (const std::runtime_error &e) {
                refused = std::string(e.what()).find("DeviceMapParams") != std::string::npos ? 1 : 0;
            }
            r.push_back(refused);
        } else {
            std::fprintf(stderr, "vtol_map_check: malformed request: %s\n", line.c_str());
            return 2;
        }
        out(r);
    }
    return 0;
}
