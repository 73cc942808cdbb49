// hakai_elem_history.hpp -- element-set history (hakai_elem_history_*, include/hakai_hip.h): the hooks
// hakai_step and the state calls use. Kernels, device state and the C entry points are in
// hakai_elem_history.hip, the arithmetic in hakai_elem_history_gp.hpp; DESIGN.md "Element-set
// history" has the definition and the reduction tree.
#pragma once
#include <hip/hip_runtime.h>

struct hakai_ctx;

namespace hkc {
struct ElemHistory;  // device state: the enabled history's and the probe's scratch (hakai_elem_history.hip)

void elem_history_destroy(hakai_ctx* c);  // frees everything (destroy, a new model)
int elem_history_restart(hakai_ctx* c);   // reset / uploaded state: the count returns to 0
// step_once, after the nodal update, the BCs and the interface fix, before the buffers flip and
// before the element kernel: d_u[cur] is u_k and the Gauss-point state and flags are state k's,
// k = t - 1. Stream mode (t_rd null) launches only when k % stride == 0; captured steps launch
// always and the kernels take k from the device slot t_rd.
int elem_history_step(hakai_ctx* c, double t, const double* t_rd, hipStream_t s);
}  // namespace hkc
