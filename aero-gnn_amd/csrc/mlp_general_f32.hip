// The general fused-MLP kernels for float32 storage (mlp_general.hpp): 54 instantiations.
#include "mlp_general.hpp"

namespace agn {
int mlp_general_fwd_f32(const agn_mlp_fwd_args& a, int mode, void* stream) { return launch_fwd<float>(a, mode, stream); }
int mlp_general_bwd_f32(const agn_mlp_bwd_args& a, int mode, void* stream) { return launch_bwd<float>(a, mode, stream); }
}  // namespace agn
