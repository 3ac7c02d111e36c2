// Resident workgroups per CU of both k_conv_wgrad_f32 instantiations, by the occupancy query
// (profiles/r15/conv_backward.txt).  Stand-alone; -DRTH_WGF_TREE probes r06's tree epilogue:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xclang -target-feature -Xclang -packed-fp32-ops \
//     -Iinclude -Ireth_amd/csrc -o wgf_occupancy scripts/probes/wgf_occupancy.hip
#include <cstdio>

#include "../../reth_amd/csrc/wgrad.hip"

namespace rth {
void set_error(const char *, ...) {}
}  // namespace rth

int main() {
  int c2 = 0, c3 = 0;
  const hipError_t e2 =
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&c2, rth::k_conv_wgrad_f32<4, 4, 2, 32, 20, 20, 2, 8, 8>, 512, 0);
  const hipError_t e3 =
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&c3, rth::k_conv_wgrad_f32<3, 3, 1, 64, 9, 9, 3, 4, 8>, 256, 0);
#ifdef RTH_WGF_TREE
  const char *v = "r06 tree epilogue";
#else
  const char *v = "r15 epilogue";
#endif
  printf("%s: workgroups per CU conv2 (8 waves) %d (rc %d), conv3 (4 waves) %d (rc %d)\n", v, c2, (int)e2, c3, (int)e3);
  return 0;
}
