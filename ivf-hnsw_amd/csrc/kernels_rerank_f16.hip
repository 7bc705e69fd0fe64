// The re-rank against the float16 base store: the HALF instantiations of kernels_rerank.hip's kernel and
// launch_rerank_f16, in a translation unit of their own so that the uint8 unit is compiled exactly as before while this
// one, new code, is compiled without packed float32 operations (the Makefile says why).
#define IVFHNSW_RERANK_F16_UNIT
#include "kernels_rerank.hip"
