// The SIDE instantiation of gt_chain2_kernel (a block tail that carries a side job) and its entry point anemoi_gt_chain2_side_fwd: the same source
// as gt_chain2.hip, compiled as a translation unit of its own so that the instantiations of gt_chain2.hip keep the code they were tuned with.
#define ANEMOI_CHAIN2_SIDE_TU 1
#include "gt_chain2.hip"
