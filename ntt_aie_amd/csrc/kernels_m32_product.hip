// kernels_m32_product.hip -- the same fused middle pass for 4-byte words (any odd p < 2^32): radix-16 rounds, unit sizes
// 2^5 .. 2^13 (launch.h: product_mid_used starts at 2^6); for N <= 2^13 the launch is the whole negacyclic product.
#define NTT_FIELD ntt::FieldM32
#include "product_kernel.inc"
