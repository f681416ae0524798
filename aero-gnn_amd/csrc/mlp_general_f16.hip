// The general fused-MLP kernels for float16 storage (mlp_general.hpp): 54 instantiations.
#include "mlp_general.hpp"

namespace agn {
int mlp_general_fwd_f16(const agn_mlp_fwd_args& a, int mode, void* stream) { return launch_fwd<f16>(a, mode, stream); }
int mlp_general_bwd_f16(const agn_mlp_bwd_args& a, int mode, void* stream) { return launch_bwd<f16>(a, mode, stream); }
}  // namespace agn
