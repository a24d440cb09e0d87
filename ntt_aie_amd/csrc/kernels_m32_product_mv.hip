// kernels_m32_product_mv.hip -- the fused middle pass of two inner products of one operand with prepared operands (pass.h:
// run_product_mv_pass; ntt_polymul_matvec_pre), 4-byte words: every unit size launch.h's product_mv_unit names.  A translation unit of its own:
// the build's parallelism.
#define NTT_FIELD FieldM32
#define NTT_PRODUCT_MV 1
#include "product_kernel.inc"
