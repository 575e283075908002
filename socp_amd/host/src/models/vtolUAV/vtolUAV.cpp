// vtolUAV.cpp -- host side of the VTOL waypoint model mirror (reference: vtolUAV.cpp:22-282).
#include "vtolUAV.hpp"

#include <stdexcept>

#include "socp_hip.h"

struct vtolUAV::data_struct {
    vtolUAV::parameters_struct parameters;
    std::vector<real> switchingTimes;
    int stepNbr;                       // the model integrates with its own step count (vtolUAV.cpp:38)
    std::string strFileTrace;
};

vtolUAV::vtolUAV(map &the_map, std::string the_fileTrace) : model(6), myMap(the_map), data(new data_struct)
{
    const parameters_struct def = {10, 0.3, 0.05, 0 * 0.05, 1. / 60, 1, 0 * 0.05, 0, 0};      // vtolUAV.cpp:27-35
    data->parameters = def;
    data->stepNbr = 100;
    data->strFileTrace = the_fileTrace;
    strFileTrace = the_fileTrace;      // the base constructor got the default "": keep both in step
    std::ofstream wipe(data->strFileTrace.c_str(), std::ios::trunc);
}

vtolUAV::~vtolUAV() { delete data; }
vtolUAV::parameters_struct &vtolUAV::GetParameterData() { return data->parameters; }
map &vtolUAV::GetMap() const { return myMap; }

int vtolUAV::DeviceModelId() const { return SOCP_MODEL_VTOLUAV; }
int vtolUAV::DeviceStepNumber() const { return data->stepNbr; }

// the model's nine, then the map's four (SOCP_VTOL_NPARAMS)
int vtolUAV::DeviceParams(double *out, int cap) const
{
    if (cap < SOCP_VTOL_NPARAMS) return 0;
    const parameters_struct &p = data->parameters;
    const double v[9] = {p.u_max, p.a_max, p.alphaT, p.alphaV, p.invSigmaXwp, p.Vd, p.ca, (double)p.nWP_tot, (double)p.nWP};
    for (int i = 0; i < 9; i++) out[i] = v[i];
    if (myMap.DeviceMapParams(out + 9, cap - 9) != SOCP_VTOL_NPARAMS - 9)
        throw std::runtime_error("vtolUAV: this map class has no device twin (map::DeviceMapParams / DeviceMapTable not implemented); "
                                 "the device dynamics cannot read its penalty");
    return SOCP_VTOL_NPARAMS;
}

// the obstacle table goes with the parameters: re-read on every use (socp_ctx_set_map copies only when it changed)
void vtolUAV::DeviceConfigure(socp_ctx *ctx) const
{
    std::vector<double> table;
    if (!myMap.DeviceMapTable(table))
        throw std::runtime_error("vtolUAV: this map class has no device twin (map::DeviceMapTable not implemented); "
                                 "refusing to integrate in free space");
    if (socp_ctx_set_map(ctx, (int)(table.size() / SOCP_MAP_STRIDE), table.data()) != SOCP_OK)
        throw std::runtime_error(std::string("vtolUAV: ") + socp_last_error(ctx));
}

vtolUAV::mstate vtolUAV::Model(real const &t, mstate const &X, int) const { return DeviceEval(SOCP_EVAL_RHS, t, X, 0); }
vtolUAV::mcontrol vtolUAV::Control(real const &t, mstate const &X) const { return DeviceEval(SOCP_EVAL_CONTROL, t, X, 0); }
vtolUAV::mstate vtolUAV::Hamiltonian(real const &t, mstate const &X, int) const { return DeviceEval(SOCP_EVAL_HAMILTONIAN, t, X, 0); }

// vtolUAV.cpp:193-214: the generic segment integration with dt = (tf - t0)/data->stepNbr
vtolUAV::mstate vtolUAV::ModelInt(real const &t0, mstate const &X, real const &tf, int isTrace, int isJac)
{
    const real dt = (tf - t0) / data->stepNbr;
    mstate Xs = X;
    if (isTrace) {
        std::stringstream ss;
        integrate(modelStruct(this, isJac), Xs, t0, tf, dt, observerStruct(this, ss));
        std::ofstream fileTrace(data->strFileTrace.c_str(), std::ios::app);
        fileTrace << ss.str();
    } else {
        integrate(modelStruct(this, isJac), Xs, t0, tf, dt);
    }
    return Xs;
}

namespace {
// vtolUAV.cpp:222-236: a FREE component's transversality row is pulled towards the target by the waypoints still ahead
void final_rows(const vtolUAV::parameters_struct &p, int d, model::mstate const &X_tf, model::mstate const &Xf, std::vector<int> const &mode_X,
                std::vector<real> &fvec)
{
    for (int j = 0; j < d; j++) {
        if (mode_X[j] == model::FREE)
            fvec[j] = X_tf[j + d] - p.invSigmaXwp*(p.nWP_tot - p.nWP)*(X_tf[j] - Xf[j]) - 0.02*(X_tf[j] - Xf[j]);
        else
            fvec[j] = X_tf[j] - Xf[j];
    }
}
}  // namespace

void vtolUAV::FinalFunction(real const &, mstate const &X_tf, mstate const &Xf, std::vector<int> const &mode_X, std::vector<real> &fvec, int) const
{
    final_rows(data->parameters, dim, X_tf, Xf, mode_X, fvec);
}

// vtolUAV.cpp:239-258: the same rows, then H(tf) = 0 for the free final time
void vtolUAV::FinalHFunction(real const &tf, mstate const &X_tf, mstate const &Xf, std::vector<int> const &mode_X, std::vector<real> &fvec, int isJac) const
{
    final_rows(data->parameters, dim, X_tf, Xf, mode_X, fvec);
    fvec[dim] = Hamiltonian(tf, X_tf, isJac)[0];
}

void vtolUAV::SwitchingTimesUpdate(std::vector<real> const &switchingTimes) { data->switchingTimes = switchingTimes; }

// vtolUAV.cpp:268-278: a FREE component of an interior node is continuous, its costate jumps by the waypoint pull
void vtolUAV::SwitchingStateFunction(real const &, int const &stateID, mstate const &X, mstate const &Xp, mstate const &Xd, mstate &fvec, int) const
{
    const int j = stateID, d = dim;
    fvec[j] = (X[j] - Xp[j]);
    fvec[j + d] = (X[j + d] - Xp[j + d]);
    if (j < 6) fvec[j + d] = (X[j + d] - Xp[j + d]) - data->parameters.invSigmaXwp*(X[j] - Xd[j]);
}
