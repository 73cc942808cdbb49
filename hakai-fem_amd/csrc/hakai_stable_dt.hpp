// hakai_stable_dt.hpp -- the stable-time-step diagnostic (hakai_stable_dt, include/hakai_hip.h): what
// the context's owner calls. The kernels, the scratch and the C entry point are in
// hakai_stable_dt.hip, the element's arithmetic in hakai_stable_dt_elem.hpp; DESIGN.md section 2,
// "Stable time step", has the definitions and the bound.
#pragma once

#include "hakai_stable_dt_elem.hpp"

struct hakai_ctx;

namespace hkc {
struct StableDt;  // scratch of the diagnostic (hakai_stable_dt.hip), allocated at the first call
void stable_dt_destroy(hakai_ctx* c);  // frees it (destroy, a new model)
// For hakai_mass_scale, which evaluates the same elements with the same material table and V0:
// allocate the scratch if this is the first call and send the table for mass_scaling (ordered on the
// context's stream); the table, the elements' V0 with whether a call has formed it yet, and the
// note that one now has (after the caller's kernel has completed).
int stable_dt_prepare(hakai_ctx* c, double mass_scaling);
const hk::StableMat* stable_dt_mats(const hakai_ctx* c);
double* stable_dt_v0(const hakai_ctx* c, bool* have);
void stable_dt_v0_formed(hakai_ctx* c);
}  // namespace hkc
