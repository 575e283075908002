// kernels_vtol_fast.hip -- throughput flavour of the vtolUAV model (VtolT<true>, models_vtol.hpp): compiled WITH
// FMA contraction.  capi.cpp uses this table when the context's variant is SOCP_VARIANT_LANE_FAST.
#include "models_vtol.hpp"
#include "plugin_impl.hpp"

namespace socp {

const ModelLaunchers *vtol_launchers_fast()
{
    static const ModelLaunchers t = [] {
        ModelLaunchers t = plugin::table<VtolFast, false>(VP_COUNT, 100, SOCP_VTOL_DEFAULTS);
        t.fields = &fields_vtol;                     // kernels_vtol_exact.hip: the reference-order object, the same bits
        t.exact_jacobian = &exact_jacobian_vtol;     // likewise
        return t;
    }();
    return &t;
}

}  // namespace socp
