// kernels_gl_product_mv.hip -- the fused middle pass of two inner products of one operand with prepared operands (pass.h:
// run_product_mv_pass; ntt_polymul_matvec_pre), Goldilocks: every unit size launch.h's product_mv_unit names -- none in the product library, all six in the experiment build.  A translation unit of its own:
// the build's parallelism.
#define NTT_FIELD FieldGL
#define NTT_PRODUCT_MV 1
#include "product_kernel.inc"
