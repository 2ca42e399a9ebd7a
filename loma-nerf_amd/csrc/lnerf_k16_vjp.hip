// lnerf_k16_vjp.hip -- the VJP instantiations of k16_fwd_bwd_kernel (lnerf_render_maps_vjp: the reverse
// pass seeded from the caller's adjoints of the render maps) and their launcher, k16_launch_vjp. The
// source is lnerf_k16.hip's; it is compiled once more here so that lnerf_k16.o and lnerf_k16_maps.o
// hold exactly the kernels they held before (see LNERF_VJP_TU there).
#define LNERF_VJP_TU 1
#include "lnerf_k16.hip"
