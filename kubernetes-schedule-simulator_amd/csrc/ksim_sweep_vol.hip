// ksim_sweep_vol.hip — the VOL instantiations of ksim_sweep_general_kernel (ksim_sweep_volumes,
// include/ksim_volsweep.h) and their launcher, ksim_sweep_general_vol_launch.
//
// The kernel template, its accessor and its LDS words are ksim_sweep_kernels.h's, the header this unit
// shares with ksim_sweep.hip.  The instantiations are kept out of ksim_sweep.hip's unit because the
// compiler's output for a kernel there depends on which other kernels the unit instantiates: with the
// six VOL kernels beside them, all twelve other ksim_sweep_general_kernel instantiations came out with
// other branches and another register allocation (the volume-sweep section).  Apart, every
// kernel of ksim_sweep.hip compiles to the instruction text and metadata it had.
#include "ksim_sweep_kernels.h"

// The six VOL instantiations: <1, 1, PRE, SPR, IPA, 1> for (SPR, IPA) = (0, 0), (1, 0), (1, 1), chosen as
// ksim_sweep_general_launch chooses their parents; ABS and WHY are on in all of them.
extern "C" hipError_t ksim_sweep_general_vol_launch(const SwgLaunch* L, size_t lds) {
  const SwgArgsPre* args = L->args;
  const KsimCtx* ctx = args->ctx;
  const hipStream_t st = L->st;
  const dim3 grid((unsigned)L->n_scen), block(SB);
  auto launch = [&](auto pre) {
    constexpr bool PRE = decltype(pre)::value;
    if (L->ipa) {
      hipLaunchKernelGGL((ksim_sweep_general_kernel<true, true, PRE, true, true, true>), grid, block, lds, st, ctx,
                         swg_args<SwgArgsIpa>(*L));
    } else if (L->spr) {
      hipLaunchKernelGGL((ksim_sweep_general_kernel<true, true, PRE, true, false, true>), grid, block, lds, st, ctx,
                         swg_args<SwgArgsSpr>(*L));
    } else {
      hipLaunchKernelGGL((ksim_sweep_general_kernel<true, true, PRE, false, false, true>), grid, block, lds, st, ctx, *args);
    }
  };
  if (args->off != nullptr) launch(std::true_type{});
  else launch(std::false_type{});
  return hipGetLastError();
}
