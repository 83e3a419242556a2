// Host side shared by the chain family's translation units: the switches of chain_plan.h read from the environment, the refusal text of a
// plan, the operand-alignment test and the one launch of a planned kernel.
#pragma once
#include "chain_plan.h"
#include "common.h"

namespace anemoi {

// Read once per process.  The switches of the experiments build keep their defaults in the product (ANEMOI_EXPERIMENT_ENV).
inline const ChainSwitches& chain_switches() {
  static const ChainSwitches sw = [] {
    ChainSwitches s;
    s.chain_rows = env_int(getenv("ANEMOI_CHAIN_ROWS"), 0, 0, kGnnEdgeRows);
    s.gnn_node_rows = ANEMOI_EXPERIMENT_ENV("ANEMOI_GNN_NODE_ROWS", 0, 0, kPanel);
    s.even_grid = ANEMOI_EXPERIMENT_ENV("ANEMOI_CHAIN2_EVEN_GRID", 1, 0, 1) != 0;
    s.max_grid = ANEMOI_EXPERIMENT_ENV("ANEMOI_CHAIN2_MAX_GRID", kChipCus, 8, kChipCus);
    s.timeline_built = kExperiments;
    return s;
  }();
  return sw;
}

// The entry point's answer to a shape its plan refuses (nothing to say for ANEMOI_OK)
inline int chain_refused(const char* who, const ChainProblem& q, const ChainPlan& p) {
  if (p.status != ANEMOI_OK)
    set_error("%s: %s (n_rows=%d in_features=%d hidden=%d q_out_features=%d rows_per_tile=%d dtype=%d)", who, p.why, q.n_rows, q.in_features, q.hidden,
              q.q_out_features, q.rows_per_tile, (int)q.dtype);
  return p.status;
}

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// The plan's launch of `kernel` (in parentheses where its template arguments have commas), its dynamic-LDS limit raised to max_lds once per
// device.  A macro so that every call names its kernel: the compiler emits the kernels of a code object in the order the host code names
// them, and the host-only checks under tools/ record that name.
#define ANEMOI_CHAIN_LAUNCH(kernel, max_lds, plan, stream, args)                                                                                     \
  do {                                                                                                                                               \
    static PerDeviceOnce once_;                                                                                                                      \
    once_.run([&] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (max_lds)); });  \
    hipLaunchKernelGGL(kernel, dim3((plan).grid), dim3((plan).threads), (plan).lds_bytes, stream, args);                                           \
  } while (0)

}  // namespace anemoi
