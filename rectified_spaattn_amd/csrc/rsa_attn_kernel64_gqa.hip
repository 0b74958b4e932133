// K5, 64-rows-per-wave form: the grouped-query (GQA / MQA) instantiations of bsfwd64_kernel in which each query head is a walk of
// its own (RSA_GQA_HEAD), and the launch hook of both grouped forms, rsa_launch_bsfwd64_gqa.  The kernel is rsa_attn_kernel64.hip's.
#define RSA_K64_GQA_UNIT 1
#include "rsa_attn_kernel64.hip"
