// vrt_ray_grad_ordered_kernel.hip -- the ORDERED instantiations of the gradient bundle's two kernels (vrt_hip_set_grad_ordered) and
// launch_ray_grad_bundle_ordered.  The text is vrt_ray_grad_kernel.hip's, compiled here with the other half of its launch section, so
// that the sixteen new kernels build beside the old ones and not behind them.
#define VRT_GRAD_ORDERED_UNIT 1
#include "vrt_ray_grad_kernel.hip"
