// The pooled-key cache from an MXFP4 K (rsa_pool_keys_kv4): rsa_block_select.hip again, as a translation unit
// of its own that holds pool_keys_kernel<mxfp4_tag> and its entry and nothing else -- sel_pool_block, sel_pool_mean and the element
// loader are that file's one definition -- built without packed fp32 arithmetic, while rsa_block_select.o keeps its flags.
#define RSA_POOL_KV4_UNIT 1
#include "rsa_block_select.hip"
