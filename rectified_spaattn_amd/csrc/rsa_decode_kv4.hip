// The MXFP4 instantiations of the decode kernels (rsa_block_sparse_decode_kv4): rsa_decode.hip again, as a
// translation unit of its own that holds the kv4_tag kernels and their entry and nothing else, so the 2-byte and e4m3 kernels of
// rsa_decode.o are built from the same statements under the same flags as before.
#define RSA_DECODE_KV4_UNIT 1
#include "rsa_decode.hip"
