// kernels_vtol.hip -- the vtolUAV waypoint model's kernels (models_vtol.hpp), reference operation order:
// MUST be compiled with -ffp-contract=off.  Table-driven like the interceptor (plugin_impl.hpp); capi.cpp binds
// the table to SOCP_MODEL_VTOLUAV and fills ModelParams::map / n_map from the context's obstacle table.
#include "models_vtol.hpp"
#include "plugin_impl.hpp"

namespace socp {

const ModelLaunchers *vtol_launchers()
{
    static const ModelLaunchers t = [] {
        ModelLaunchers t = plugin::table<VtolExact, false>(VP_COUNT, 100, SOCP_VTOL_DEFAULTS);
        t.fields = &fields_vtol;                     // kernels_vtol_exact.hip: the same reference-order object in both flavours
        t.exact_jacobian = &exact_jacobian_vtol;     // likewise
        return t;
    }();
    return &t;
}

}  // namespace socp
