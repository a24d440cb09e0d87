// kernels_gl_product.hip -- the fused middle pass of the Goldilocks negacyclic product (pass.h: run_product_pass):
// last inverse-network pass of both operands + pointwise product + first forward-network pass in one workgroup-resident
// sweep over each 2^LOG_M-word unit, unit sizes 2^7 .. 2^12 (no reference counterpart: the reference has no product).
#define NTT_FIELD ntt::FieldGL
#include "product_kernel.inc"
