// lnerf_k16_maps.hip -- the MAPS instantiations of k16_fwd_bwd_kernel (lnerf_render_maps: depth,
// opacity, sample weights and rgba beside the colour) and their launcher, k16_launch_maps. The source
// is lnerf_k16.hip's; it is compiled a second time here so that the object training and lnerf_render
// run, lnerf_k16.o, holds exactly the kernels it held before (see LNERF_MAPS_TU there).
#define LNERF_MAPS_TU 1
#include "lnerf_k16.hip"
