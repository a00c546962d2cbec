// analytic_kernels.hip -- the unit of the single-pass Hilbert analytic signal
// (hilbert_fused.hpp: k_hilbert_pair, k_hilbert_small, launch_hilbert_fused)
// and DCT-II (dct2_fused.hpp: k_dct2_pair, k_dct2_small, launch_dct2_fused).
// The two families share nothing but fft_core.hpp; they stay one unit because
// k_hilbert_pair<512> and <1024> compile to other device code without the
// DCT-II kernels beside them.
#include "hilbert_fused.hpp"
#include "dct2_fused.hpp"
