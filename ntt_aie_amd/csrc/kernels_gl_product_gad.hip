// kernels_gl_product_gad.hip -- the digit variants of the summed middle passes (pass.h: run_product_dot_pass / run_product_mv_pass with
// GAD = true: the balanced gadget decomposition in registers; ntt_polymul_gadget_pre), Goldilocks: every unit size launch.h's
// product_gadget_unit names, the two-output variant where product_mv_unit names it too.  A translation unit of its own: the build's parallelism.
//  The product library uses none of them for this class (the A/B rule of DESIGN.md section 3.2); the experiment build has all six summed ones and the two-output ones.
#define NTT_FIELD FieldGL
#define NTT_PRODUCT_GAD 1
#include "product_kernel.inc"
