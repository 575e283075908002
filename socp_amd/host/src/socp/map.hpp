// map.hpp -- abstract penalty-map interface of the reference (map.hpp:15-47): what a model such as vtolUAV reads its
// obstacle penalty from.  New here is the device hook, as in model.hpp: a map whose penalty has a device-resident twin
// reports its obstacle table and its scalar parameters, and the model that owns it pushes them to its device context
// (socp_ctx_set_map, packed parameter block).  A map subclass written for the reference -- Function / Gradient only --
// still compiles; a device model that needs a table refuses it with an error instead of running in free space.
#ifndef SOCP_AMD_MAP_HPP_
#define SOCP_AMD_MAP_HPP_

#include "commonType.hpp"

#include <vector>

class map
{
public:
    map() {}
    virtual ~map() {}
    virtual void Function(std::vector<real> const &state, real &func) const = 0;
    virtual void Gradient(std::vector<real> const &state, std::vector<real> &grad) const = 0;

    // ---- device hook (new) -------------------------------------------------------------------
    // rows of SOCP_MAP_STRIDE doubles (type, centre xyz, radii xyz), include/socp_hip.h; false: no device twin
    virtual bool DeviceMapTable(std::vector<double> &table) const { (void)table; return false; }
    // the map's scalars in the order the device model packs them after its own (phiObs, psiWP, muObs, sigmaWP); returns the count
    virtual int DeviceMapParams(double *out, int cap) const { (void)out; (void)cap; return 0; }
};

#endif
