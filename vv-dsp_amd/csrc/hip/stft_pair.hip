// stft_pair.hip -- k_stft_pair for magnitude, complex and power rows (modes
// 0..2) of every size whose last FFT pass is mirror-paired, and k_stft_r32's
// magnitude rows: the instantiations of run_stft_pair (stft_pair_launch.hpp),
// except <1024, 2> (stft_mel.hip).
#include "stft_pair_launch.hpp"

namespace vvh {

#define VVH_INST(NN, M) template hipError_t run_stft_pair<NN, M>(const StftJob&);
#define VVH_INST3(NN) VVH_INST(NN, 0) VVH_INST(NN, 1) VVH_INST(NN, 2)
VVH_INST3(2) VVH_INST3(4) VVH_INST3(8) VVH_INST3(16) VVH_INST3(32) VVH_INST3(64) VVH_INST3(128) VVH_INST3(512)
VVH_INST(1024, 0) VVH_INST(1024, 1) VVH_INST3(2048) VVH_INST3(8192)
#undef VVH_INST3
#undef VVH_INST

}  // namespace vvh
