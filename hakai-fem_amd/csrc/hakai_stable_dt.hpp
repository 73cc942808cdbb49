// hakai_stable_dt.hpp -- the stable-time-step diagnostic (hakai_stable_dt, include/hakai_hip.h): what
// the context's owner calls. The kernels, the scratch and the C entry point are in
// hakai_stable_dt.hip, the element's arithmetic in hakai_stable_dt_elem.hpp; DESIGN.md section 2,
// "Stable time step", has the definitions and the bound.
#pragma once

struct hakai_ctx;

namespace hkc {
struct StableDt;  // scratch of the diagnostic (hakai_stable_dt.hip), allocated at the first call
void stable_dt_destroy(hakai_ctx* c);  // frees it (destroy, a new model)
}  // namespace hkc
