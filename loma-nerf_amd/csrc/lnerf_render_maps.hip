// lnerf_render_maps.hip -- the MAPS instantiations of kr_fwd_kernel (lnerf_render_maps: depth,
// opacity, sample weights and rgba beside the colour) and their launcher, kr_launch_maps. The source
// is lnerf_render.hip's, compiled a second time here so that lnerf_render.o holds exactly the kernels
// it held before (see LNERF_MAPS_TU there).
#define LNERF_MAPS_TU 1
#include "lnerf_render.hip"
