// vrt_ray_gn_diag_ordered_kernel.hip -- the ORDERED instantiations of the Gauss-Newton diagonal bundle's two kernels
// (vrt_hip_set_grad_ordered) and launch_ray_gn_diag_bundle_ordered.  The text is vrt_ray_gn_diag_kernel.hip's, compiled here with the
// other half of its launch section, so that the two halves build beside each other.
#define VRT_GN_DIAG_ORDERED_UNIT 1
#include "vrt_ray_gn_diag_kernel.hip"
