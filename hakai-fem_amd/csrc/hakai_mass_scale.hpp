// hakai_mass_scale.hpp -- selective mass scaling (hakai_mass_scale, include/hakai_hip.h): what the
// context's owner and the stable-step diagnostic call. The kernels, the scratch and the C entry
// points are in hakai_mass_scale.hip, the element's rule in hakai_mass_scale_elem.hpp; DESIGN.md
// section 2, "Selective mass scaling", has the definition and the guarantee.
#pragma once

struct hakai_ctx;

namespace hkc {
struct MassScale;  // per-element added mass, the uploaded nodal mass, partials (hakai_mass_scale.hip)
void mass_scale_destroy(hakai_ctx* c);  // frees it without touching d_mass (destroy, a new model)
// The elements' added mass [nE] while a scaling is in force (some element has added > 0), else null:
// hakai_stable_dt then evaluates m0 + added.
const double* mass_scale_added(const hakai_ctx* c);
}  // namespace hkc
