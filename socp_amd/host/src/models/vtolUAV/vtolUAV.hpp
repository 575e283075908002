// vtolUAV.hpp -- host mirror of the reference's waypoint-following VTOL model class (vtolUAV.hpp:17-113); dynamics on
// the device (SOCP_MODEL_VTOLUAV), including the obstacle penalty of the map it is constructed with: the map's table is
// pushed to the device context and its scalars join the packed parameter block on every use, because continuation
// writes through GetParameterData() of both objects.
#ifndef SOCP_AMD_VTOLUAV_HPP_
#define SOCP_AMD_VTOLUAV_HPP_

#include <iostream>   // user programs written for the reference rely on these transitive includes

#include "../../socp/map.hpp"
#include "../../socp/model.hpp"

class vtolUAV : public model
{
public:
    // same members, order and types as the reference's structure (users assign them through GetParameterData())
    struct parameters_struct {
        real u_max;          // bound on the norm of the normalised control
        real a_max;          // acceleration per unit control
        real alphaT;         // weight of the flight time
        real alphaV;         // weight of the deviation from the desired speed Vd
        real invSigmaXwp;    // weight of the distance to a waypoint at the interior nodes
        real Vd;             // desired speed
        real ca;             // drag coefficient
        int nWP_tot;         // waypoints of the whole path (the final point included)
        int nWP;             // waypoints of the current problem
    };

    vtolUAV(map &the_map, std::string the_fileTrace = std::string(""));
    ~vtolUAV() override;

    parameters_struct &GetParameterData();
    map &GetMap() const;

    void FinalFunction(real const &tf, mstate const &X_tf, mstate const &Xf, std::vector<int> const &mode_X, std::vector<real> &fvec, int isJac) const override;
    void FinalHFunction(real const &tf, mstate const &X_tf, mstate const &Xf, std::vector<int> const &mode_X, std::vector<real> &fvec, int isJac) const override;
    void SwitchingTimesUpdate(std::vector<real> const &switchingTimes) override;
    void SwitchingStateFunction(real const &t, int const &stateID, mstate const &X, mstate const &Xp, mstate const &Xd, mstate &fvec, int isJac) const override;

    // device hook
    int DeviceModelId() const override;
    int DeviceParams(double *out, int cap) const override;
    int DeviceStepNumber() const override;
    void DeviceConfigure(socp_ctx *ctx) const override;

private:
    map &myMap;
    struct data_struct;
    data_struct *data;

    // the plugin virtuals: evaluated by the device twin
    mstate Model(real const &t, mstate const &X, int isJac = 0) const override;
    mcontrol Control(real const &t, mstate const &X) const override;
    mstate Hamiltonian(real const &t, mstate const &X, int isJac = 0) const override;
    mstate ModelInt(real const &t0, mstate const &X, real const &tf, int isTrace, int isJac = 0) override;
};

#endif
