// ksim_sweep_vol.hip — the VOL instantiations of ksim_sweep_general_kernel (ksim_sweep_volumes,
// include/ksim_volsweep.h) and their launcher, ksim_sweep_general_vol_launch.
//
// The kernel template, its accessor and its LDS words are ksim_sweep.hip's: this unit takes that file
// down to the end of the template and the launcher at its end, nothing between.  The instantiations
// are kept out of ksim_sweep.hip's own unit because the compiler's output for a kernel there depends on
// which other kernels the unit instantiates: with the six VOL kernels beside them, all twelve existing
// ksim_sweep_general_kernel instantiations came out with other branches and another register
// allocation (the volume-sweep section).  Apart, every kernel of ksim_sweep.hip compiles to
// the instruction text and metadata it had.
#define KSIM_SWEEP_VOL_TU
#include "ksim_sweep.hip"
