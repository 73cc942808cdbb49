// hakai_history.hpp -- per-step history output (hakai_history_*, include/hakai_hip.h): the hooks
// hakai_step and the state calls use. Kernels, device state and the C entry points are in
// hakai_history.hip; DESIGN.md "History output" has the identity and the reduction tree.
#pragma once
#include <hip/hip_runtime.h>

struct hakai_ctx;
namespace hk {
struct NodalArgs;
}

namespace hkc {
struct History;  // device state of an enabled history (hakai_history.hip)
struct CommFix;  // what the interface fix of the step read (hakai_internal.hpp)

void history_destroy(hakai_ctx* c);             // frees everything (disable, destroy, a new model)
int history_restart(hakai_ctx* c);              // reset / uploaded state: count 0, seed at the next step
int history_bc_changed(hakai_ctx* c);           // hakai_set_bc: the per-node mask of prescribed dofs
bool history_needs_seed(const hakai_ctx* c);    // the next step seeds: it cannot come from a graph
// step_once, with the NodalArgs its launch_nodal takes (na.u = u_k; na.u_pre_out = u_{k-1} before
// the nodal update, u_{k+1} after it): the seed before the nodal update of the first step after a
// (re)start; the step's sums after the nodal update and the BCs, before the buffers flip.
// On a rank (a context with a communicator) the sums run over the nodes the rank owns, and `fix` is
// what comm_post_nodal's interface fix read in this step: the Q of an owned interface node.
int history_seed(hakai_ctx* c, const hk::NodalArgs& na, hipStream_t s);
int history_step(hakai_ctx* c, const hk::NodalArgs& na, const CommFix& fix, double t, const double* t_rd,
                 hipStream_t s);
}  // namespace hkc
