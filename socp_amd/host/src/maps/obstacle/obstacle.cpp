// obstacle.cpp -- host side of the obstacle map mirror (reference: obstacle.cpp:20-390).  The file readers accept what
// the reference's accept (a caption line before every block, one record per line, silent stop at the first malformed
// record); the penalty is evaluated term by term in the reference's operation order.
#include "obstacle.hpp"

#include <cmath>
#include <fstream>
#include <sstream>

#include "socp_hip.h"

struct obstacle::data_struct {
    int obstacleNbr = 0;
    std::vector<real> type;                        // 0 ellipsoid, 1 box; anything else contributes nothing
    std::vector<std::vector<real>> centre, radius;
    int WPNbr = 0;
    std::vector<std::vector<real>> WPState;       // position (3) and unit direction to the next waypoint (3)
    parameters_struct parameters;
    real penalizationRange = 10;
    std::string fileObstacles, fileWP;
};

obstacle::obstacle(std::string the_fileObstacles, std::string the_fileWP) : data(new data_struct)
{
    const parameters_struct def = {1, 0.03, 1, 2.5};      // obstacle.cpp:49-52
    data->parameters = def;
    data->fileObstacles = the_fileObstacles;
    data->fileWP = the_fileWP;
    ReadObstacleInput();
    ReadWPInput();
}

// the reference's class is copied with its raw pointer (testVtolUAV.cpp:57 copy-initialises one); a deep copy here
obstacle::obstacle(obstacle const &other) : map(other), data(new data_struct(*other.data)) {}
obstacle &obstacle::operator=(obstacle const &other)
{
    if (this != &other) *data = *other.data;
    return *this;
}
obstacle::~obstacle() { delete data; }

obstacle::parameters_struct &obstacle::GetParameterData() { return data->parameters; }
const std::vector<std::vector<real>> &obstacle::GetPath() { return data->WPState; }

namespace {
bool next_line(std::ifstream &is, std::istringstream &rec)
{
    std::string line;
    std::getline(is, line);
    rec.clear();
    rec.str(line);
    return true;
}
}  // namespace

// obstacle.cpp:69-109: "n:" count, "type:" n lines, "position:" n lines of three, "radius:" n lines of three
void obstacle::ReadObstacleInput()
{
    std::ifstream is(data->fileObstacles);
    if (!is) return;
    std::istringstream rec;
    next_line(is, rec);                                    // caption
    next_line(is, rec);
    if (!(rec >> data->obstacleNbr)) return;
    const int n = data->obstacleNbr;
    data->type.assign(n, 0);
    next_line(is, rec);                                    // caption
    for (int i = 0; i < n; i++) {
        next_line(is, rec);
        if (!(rec >> data->type[i])) return;
    }
    data->centre.assign(n, std::vector<real>());
    next_line(is, rec);                                    // caption
    for (int i = 0; i < n; i++) {
        data->centre[i].assign(3, 0);
        next_line(is, rec);
        if (!(rec >> data->centre[i][0] >> data->centre[i][1] >> data->centre[i][2])) return;
    }
    data->radius.assign(n, std::vector<real>());
    next_line(is, rec);                                    // caption
    for (int i = 0; i < n; i++) {
        data->radius[i].assign(3, 0);
        next_line(is, rec);
        if (!(rec >> data->radius[i][0] >> data->radius[i][1] >> data->radius[i][2])) return;
    }
}

// obstacle.cpp:114-150: count, positions, then the unit direction from each waypoint to the next; the last one copies its predecessor's
void obstacle::ReadWPInput()
{
    std::ifstream is(data->fileWP);
    if (!is) return;
    std::istringstream rec;
    next_line(is, rec);                                    // caption
    next_line(is, rec);
    if (!(rec >> data->WPNbr)) return;
    const int n = data->WPNbr;
    data->WPState.assign(n, std::vector<real>());
    next_line(is, rec);                                    // caption
    for (int i = 0; i < n; i++) {
        data->WPState[i].assign(6, 0);
        next_line(is, rec);
        if (!(rec >> data->WPState[i][0] >> data->WPState[i][1] >> data->WPState[i][2])) return;
    }
    for (int i = 0; i < n - 1; i++) {
        const real ex = data->WPState[i + 1][0] - data->WPState[i][0];
        const real ey = data->WPState[i + 1][1] - data->WPState[i][1];
        const real ez = data->WPState[i + 1][2] - data->WPState[i][2];
        const real distance = sqrt(ex * ex + ey * ey + ez * ez);
        data->WPState[i][3] = ex / distance;
        data->WPState[i][4] = ey / distance;
        data->WPState[i][5] = ez / distance;
    }
    if (n >= 2)
        for (int k = 3; k < 6; k++) data->WPState[n - 1][k] = data->WPState[n - 2][k];
}

// obstacle.cpp:155-181: only the obstacle part is live upstream; the waypoint weight multiplies a zero
void obstacle::Function(std::vector<real> const &position, real &funcTot) const
{
    real funcObs = 0, funcWP = 0;
    ObstaclePenalizationFunction(position, funcObs);
    funcTot = data->parameters.phiObs * funcObs + data->parameters.psiWP * funcWP;
}

void obstacle::Gradient(std::vector<real> const &position, std::vector<real> &gradTot) const
{
    std::vector<real> gradObs(3, 0), gradWP(3, 0);
    ObstaclePenalizationGradient(position, gradObs);
    for (int k = 0; k < 3; k++) gradTot[k] = data->parameters.phiObs * gradObs[k] + data->parameters.psiWP * gradWP[k];
}

// obstacle.cpp:186-231
void obstacle::ObstaclePenalizationFunction(std::vector<real> const &position, real &funcObs) const
{
    const real mu = data->parameters.muObs;
    real f = 0;
    for (int i = 0; i < data->obstacleNbr; i++) {
        const real x = data->centre[i][0], y = data->centre[i][1], z = data->centre[i][2];
        const real radx = data->radius[i][0], rady = data->radius[i][1], radz = data->radius[i][2];
        if (data->type[i] == 0) {
            const real hx = position[0] - x, hy = position[1] - y, hz = position[2] - z;
            const real d = sqrt(hx*hx + hy*hy + hz*hz);
            const real rad = d / sqrt(hx*hx / radx / radx + hy*hy / rady / rady + hz*hz / radz / radz);
            const real h = (d - rad) / mu;
            f = f + (1 - tanh(h)) / 2;
        } else if (data->type[i] == 1) {
            const real hx = (fabs(position[0] - x) - radx) / mu;
            const real hy = (fabs(position[1] - y) - rady) / mu;
            const real hz = (fabs(position[2] - z) - radz) / mu;
            f = f + (1 - tanh(hx))*(1 - tanh(hy))*(1 - tanh(hz)) / 8;
        }
    }
    if (std::isnan(f)) f = 0.0;
    funcObs = f;
}

// obstacle.cpp:236-319.  Upstream quirks kept: the ellipsoid's `rad` has no z term here and its z component is zero; a
// position on a box's centre plane gives 0/0, and the reset below then clears the whole component.
void obstacle::ObstaclePenalizationGradient(std::vector<real> const &position, std::vector<real> &gradObs) const
{
    const real mu = data->parameters.muObs;
    real g0 = 0, g1 = 0, g2 = 0;
    for (int i = 0; i < data->obstacleNbr; i++) {
        const real x = data->centre[i][0], y = data->centre[i][1], z = data->centre[i][2];
        const real radx = data->radius[i][0], rady = data->radius[i][1], radz = data->radius[i][2];
        if (data->type[i] == 0) {
            const real hx = position[0] - x, hy = position[1] - y, hz = position[2] - z;
            const real d = sqrt(hx*hx + hy*hy + hz*hz);
            const real q = sqrt(hx*hx / radx / radx + hy*hy / rady / rady);
            const real rad = d / q;
            const real h = (d - rad) / mu;
            const real rho2 = (radx*radx - rady*rady) / (radx*radx*rady*rady) / q / q / q;
            const real th = tanh(h);
            g0 = g0 - hx / d*(1 - hy*hy*rho2) / mu*(1 - th*th) / 2;
            g1 = g1 - hy / d*(1 + hx*hx*rho2) / mu*(1 - th*th) / 2;
            g2 = g2 - 0;
        } else if (data->type[i] == 1) {
            const real dx = position[0] - x, dy = position[1] - y, dz = position[2] - z;
            const real thx = tanh((fabs(dx) - radx) / mu);
            const real thy = tanh((fabs(dy) - rady) / mu);
            const real thz = tanh((fabs(dz) - radz) / mu);
            g0 = g0 - dx / fabs(dx) / mu*(1 - thx*thx)*(1 - thy)*(1 - thz) / 8;
            g1 = g1 - dy / fabs(dy) / mu*(1 - thy*thy)*(1 - thx)*(1 - thz) / 8;
            g2 = g2 - dz / fabs(dz) / mu*(1 - thz*thz)*(1 - thx)*(1 - thy) / 8;
        }
    }
    gradObs[0] = std::isnan(g0) ? 0.0 : g0;
    gradObs[1] = std::isnan(g1) ? 0.0 : g1;
    gradObs[2] = std::isnan(g2) ? 0.0 : g2;
}

// obstacle.cpp:324-378: Gaussian wells around the waypoints within penalizationRange.  Not reached from Function /
// Gradient (switched off upstream); kept because they are public.
void obstacle::WPPenalizationFunction(std::vector<real> const &position, real &funcWP) const
{
    const real sigma = data->parameters.sigmaWP;
    real f = 0;
    for (int i = 0; i < data->WPNbr; i++) {
        const real hx = (position[0] - data->WPState[i][0]) / sigma;
        const real hy = (position[1] - data->WPState[i][1]) / sigma;
        const real hz = (position[2] - data->WPState[i][2]) / sigma;
        const real d = sqrt(hx*hx + hy*hy + hz*hz);
        if (d * sigma <= data->penalizationRange) f = f - exp(-d * d / 2.0);
    }
    funcWP = std::isnan(f) ? 0.0 : f;
}

void obstacle::WPPenalizationGradient(std::vector<real> const &position, std::vector<real> &gradWP) const
{
    const real sigma = data->parameters.sigmaWP;
    real g[3] = {0, 0, 0};
    for (int i = 0; i < data->WPNbr; i++) {
        const real hx = (position[0] - data->WPState[i][0]) / sigma;
        const real hy = (position[1] - data->WPState[i][1]) / sigma;
        const real hz = (position[2] - data->WPState[i][2]) / sigma;
        const real d = sqrt(hx*hx + hy*hy + hz*hz);
        if (d * sigma <= data->penalizationRange) {
            g[0] = g[0] + hx / sigma * exp(-d * d / 2.0);
            g[1] = g[1] + hy / sigma * exp(-d * d / 2.0);
            g[2] = g[2] + hz / sigma * exp(-d * d / 2.0);
        }
    }
    for (int k = 0; k < 3; k++) gradWP[k] = std::isnan(g[k]) ? 0.0 : g[k];
}

bool obstacle::DeviceMapTable(std::vector<double> &table) const
{
    const int n = data->obstacleNbr;
    table.assign((size_t)n * SOCP_MAP_STRIDE, 0.0);
    for (int i = 0; i < n; i++) {
        double *row = &table[(size_t)i * SOCP_MAP_STRIDE];
        // a file that ended early leaves later blocks empty: such an obstacle would be an out-of-range read upstream; here it contributes nothing
        const bool whole = i < (int)data->centre.size() && data->centre[i].size() == 3 && i < (int)data->radius.size() && data->radius[i].size() == 3;
        row[0] = whole ? data->type[i] : -1;
        for (int k = 0; k < 3 && whole; k++) { row[1 + k] = data->centre[i][k]; row[4 + k] = data->radius[i][k]; }
    }
    return true;
}

int obstacle::DeviceMapParams(double *out, int cap) const
{
    if (cap < 4) return 0;
    out[0] = data->parameters.phiObs; out[1] = data->parameters.psiWP; out[2] = data->parameters.muObs; out[3] = data->parameters.sigmaWP;
    return 4;
}
