// kernels_vtol_fast.hip -- throughput flavour of the vtolUAV model (VtolT<true>, models_vtol.hpp): compiled WITH
// FMA contraction.  capi.cpp uses this table when the context's variant is SOCP_VARIANT_LANE_FAST.
#include "models_vtol.hpp"
#include "plugin_impl.hpp"

namespace socp {

const ModelLaunchers *vtol_launchers_fast()
{
    static const ModelLaunchers t = plugin::table<VtolFast>(VP_COUNT, 100, SOCP_VTOL_DEFAULTS);
    return &t;
}

}  // namespace socp
