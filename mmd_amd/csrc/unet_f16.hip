// The fused TemporalUnet forward in fp16 precision (mmd_unet_options.precision = MMD_UNET_PRECISION_F16): unet_kernel.h compiled a second
// time under MMD_UNET_F16 -- one fp16 piece per operand and ONE MFMA per K = 32 chunk with fp32 accumulation, everything else (stages,
// slabs, weight packs, scales, epilogues, the fused unguided step) as in unet.hip's f16x2 build -- in namespace mmd::f16, so that the
// kernels have symbols of their own (two translation units that both define mmd::unet_kernel<4> get their host stubs merged by the linker).
// unet.hip packs the weights, builds the argument block and decides the launch form; this file only launches.
#define MMD_UNET_F16 1
#include "unet_kernel.h"

namespace mmd {

// args: unet.hip's mmd::UnetArgs -- the same struct text as f16::UnetArgs, compiled here in the variant's namespace -- passed as bytes
int launch_unet_f16(int ns, int blocks, hipStream_t st, const void* args, size_t args_bytes) {
  MMD_REQUIRE(args && args_bytes == sizeof(f16::UnetArgs) && blocks >= 1, "launch_unet_f16: argument block");
  f16::UnetArgs a;
  memcpy(&a, args, sizeof(a));
  if (ns == 1) hipLaunchKernelGGL(f16::unet_kernel<1>, dim3(blocks), dim3(256), 0, st, a);
  else if (ns == 2) hipLaunchKernelGGL(f16::unet_kernel<2>, dim3(blocks), dim3(256), 0, st, a);
  else if (ns == 4) hipLaunchKernelGGL(f16::unet_kernel<4>, dim3(blocks), dim3(256), 0, st, a);
  else MMD_REQUIRE(false, "launch_unet_f16: %d trajectories per workgroup", ns);
  return 0;
}

// args_dev: the argument block in device memory (unet_persist_steps)
int launch_unet_persist_f16(int ns, int blocks, hipStream_t st, const void* args_dev, size_t args_bytes, const FusedStep* steps_dev,
                            int n_steps, int tb_total) {
  MMD_REQUIRE(args_dev && args_bytes == sizeof(f16::UnetArgs) && blocks >= 1, "launch_unet_persist_f16: argument block");
  const f16::UnetArgs* ap = reinterpret_cast<const f16::UnetArgs*>(args_dev);
  if (ns == 2) hipLaunchKernelGGL(f16::unet_persist_kernel<2>, dim3(blocks), dim3(256), 0, st, ap, steps_dev, n_steps, tb_total);
  else if (ns == 4) hipLaunchKernelGGL(f16::unet_persist_kernel<4>, dim3(blocks), dim3(256), 0, st, ap, steps_dev, n_steps, tb_total);
  else MMD_REQUIRE(false, "launch_unet_persist_f16: %d trajectories per workgroup", ns);
  return 0;
}

}  // namespace mmd
