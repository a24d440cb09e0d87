// kernels_m64_product_gad.hip -- the digit variants of the summed middle passes (pass.h: run_product_dot_pass / run_product_mv_pass with
// GAD = true: the balanced gadget decomposition in registers; ntt_polymul_gadget_pre), general odd 64-bit modulus: every unit size launch.h's
// product_gadget_unit names, the two-output variant where product_mv_unit names it too.  A translation unit of its own: the build's parallelism.
#define NTT_FIELD FieldM64
#define NTT_PRODUCT_GAD 1
#include "product_kernel.inc"
