// akmi_stage_march_x3.hip -- the marches along x3 (k_sweep_update<2, ..>, the u0 and face forms of the MHD PLM march
// included), instantiated from akmi_stage_march.hpp.
#include "akmi_stage_march.hpp"

namespace akmi {

AKMI_INST_MARCH(2, true, 0, true)      // consumes acc and finishes the update (MHD: also the u0 / face forms)
AKMI_INST_MARCH(2, false, 0, true)
AKMI_INST_MARCH(2, true, 2, false)     // task-granular path: stores the fluxes
AKMI_INST_MARCH(2, false, 2, false)

}  // namespace akmi
