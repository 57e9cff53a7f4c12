// Run-time choice between the two builds of the split-operand kernels (csrc/split.h): namespace s1 = two fp16 planes / three MFMA
// products per fp32 product (weights pre-scaled by 2^8; operands must stay inside the fp16 range), s0 = three bf16 planes / six
// products (the whole fp32 exponent range, half the speed).  ctrlsim_set_option(OPT_SPLIT, 1 | 0) selects; the engine falls back
// from s1 to s0 when a rollout produced non-finite logits (engine.py).  Weight planes of both schemes travel in the packed buffer.
#include "launchers.h"

int split_npl() { return ctrlsim_option(OPT_SPLIT) ? 2 : 3; }

// The global name of every launcher of split_launchers.inc forwards to the selected scheme's build of it.  Two of them are not what they look like:
//   * launch_head_ce (loss.hip) exists as a kernel in the two-plane build only; s0's returns 1 — nothing launched — and the caller takes the
//     from-memory path;
//   * attn_mask_table_bytes (SPLIT_FIXED) always asks s1: the visibility-mask table does not depend on the split.
#define SPLIT_LAUNCHER(RET, NAME, PARAMS, ARGS) \
  RET NAME PARAMS { return ctrlsim_option(OPT_SPLIT) ? s1::NAME ARGS : s0::NAME ARGS; }
#define SPLIT_FIXED(RET, NAME, PARAMS, ARGS) \
  RET NAME PARAMS { return s1::NAME ARGS; }
#include "split_launchers.inc"
