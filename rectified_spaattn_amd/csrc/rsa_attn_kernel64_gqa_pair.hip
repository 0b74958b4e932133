// K5, 64-rows-per-wave form: the grouped-query instantiations of bsfwd64_kernel in which two query heads of one K/V head share a
// workgroup's K/V ring (RSA_GQA_PAIR: four waves).  The kernel is rsa_attn_kernel64.hip's.
#define RSA_K64_GQA_UNIT 2
#include "rsa_attn_kernel64.hip"
