// hakai_loads.hpp -- external loads and rigid walls (hakai_set_loads, hakai_set_walls,
// include/hakai_hip.h): the hooks hakai_step and the model calls use. Kernel, device state and the C
// entry points are in hakai_loads.hip.
#pragma once

struct hakai_ctx;

namespace hkc {
struct Loads;  // device copy of the planned loads and walls (hakai_loads.hip)

void loads_destroy(hakai_ctx* c);  // frees everything (clear, destroy, a new model)
// step_once, after the contact phases: contact force fc (or null) + loads + walls -> c->d_ftot, one
// launch on the context's stream (graph mode: the time comes from the device step counter). No-op
// without loads and walls.
int loads_step(hakai_ctx* c, double t, double d_time, const double* fc);
}  // namespace hkc
