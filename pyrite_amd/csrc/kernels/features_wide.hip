// features_wide.hip -- the feature pass (kernels/features.hip) once more with the wide interpreter build's register file
// (kernels.hip PYR_WIDE_VM), as kernels/wide.hip is to the render kernels.
#define PYR_WIDE_VM
#include "features.hip"
