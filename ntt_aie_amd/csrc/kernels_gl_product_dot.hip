// kernels_gl_product_dot.hip -- the fused middle pass of the negacyclic inner product with prepared operands (pass.h: run_product_dot_pass;
// ntt_polymul_dot_pre), Goldilocks: every unit size kernels_gl_product.hip has.  A translation unit of its own: the build's parallelism.
#define NTT_FIELD FieldGL
#define NTT_PRODUCT_DOT 1
#include "product_kernel.inc"
