/* ksim_plan.h — which launch plan the general persistent kernels took (diagnostic): ksim_last_plan,
 * beside ksim_last_form of include/ksim.h.  Tests assert it so that a case built for one plan cannot
 * silently run another.
 *
 * The entry is exported from the same libksim.so and is plain C (cgo).  include/ksim.h, its function
 * list and KSIM_ABI_VERSION are unchanged. */
#ifndef KSIM_PLAN_H
#define KSIM_PLAN_H

#include "ksim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Launch plan of the last ksim_schedule call that ran a general persistent kernel (diagnostic, handle
 * state only): which kernel, its geometry and what of the tables it kept in LDS.  All zero
 * (KSIM_PLAN_NONE) after a call that took any other path — the fast kernel, tree mode, the launch
 * form from the start — and before any call.  A call cut into several launches reports the last. */
#define KSIM_PLAN_NONE 0
#define KSIM_PLAN_C2 1          /* selector / taint / port pods (ksim_persistent.hip) */
#define KSIM_PLAN_PGEN_SINGLE 2 /* affinity / spread / volume pods, single-hypothesis kernel */
#define KSIM_PLAN_PGEN_DUAL 3   /* ... dual-hypothesis kernel */
typedef struct ksim_plan_info {
  int32_t kernel;          /* KSIM_PLAN_* */
  int32_t grid;            /* workgroups */
  int32_t rows_per_wg;     /* node rows a workgroup holds (the last one may hold fewer) */
  int32_t rows_per_thread; /* 1, 2, 4 (C2: or 8) */
  int32_t finished;        /* 1: the kernel scheduled the whole range; 0: it stopped at a spin bound
                            * and the launch form finished the range */
  /* KSIM_PLAN_PGEN_*: */
  int32_t n_st;            /* pod classes whose static (class, row) words were staged (0: none) */
  int32_t hdense;          /* 1: the dense hypothesis deltas were staged */
  int32_t vslots, vcap;    /* volume slots per node held in LDS, and in the tables */
  int32_t rec_stride;      /* bytes of a pod-context record */
  /* KSIM_PLAN_C2: */
  int32_t ps;              /* host-port slots per row held in LDS (0: none, or they did not fit) */
  int32_t tables;          /* 1: the pod-class tables were held in LDS */
  int32_t static_table;    /* 1: ... and the static (class, row) words beside them */
  int32_t reserved;
  int64_t lds_bytes;       /* dynamic LDS of a workgroup */
} ksim_plan_info;
int ksim_last_plan(ksim_handle* h, ksim_plan_info* out);

#ifdef __cplusplus
}
#endif
#endif /* KSIM_PLAN_H */
