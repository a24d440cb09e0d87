// kernels_m64_product_pre.hip -- the fused middle pass of the negacyclic product with operand b prepared (pass.h: run_product_pass,
// PRE = true; ntt_polymul_negacyclic_pre), general odd 64-bit modulus: every unit size kernels_m64_product.hip has.  A translation unit of its own: the build's parallelism.
#define NTT_FIELD FieldM64
#define NTT_PRODUCT_PRE 1
#include "product_kernel.inc"
