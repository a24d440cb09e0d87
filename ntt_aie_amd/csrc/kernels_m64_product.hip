// kernels_m64_product.hip -- the fused middle pass of the negacyclic product (pass.h: run_product_pass) for the general odd 64-bit
// modulus (FieldM64): the same radix-8 schedule as kernels_gl_product.hip, unit sizes 2^7 .. 2^12.
#define NTT_FIELD ntt::FieldM64
#include "product_kernel.inc"
