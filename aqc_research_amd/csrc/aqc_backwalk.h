// The backward walk of the sweep's first stage (objective by projection): where its partial R goes.
//
// The walk runs the LAST stage of the mirrored plan (aqc_ws.h: mirror_plan) from (w, z) = (psi, C).  Mirrored sub-stage m of that plan
// (index over all of the plan's sub-stages) is U_s^H of forward sub-stage s = nsubs_total - 1 - m and has the same register bits, so the
// 16 x 16 matrix it forms on those bits is the R of forward sub-stage s and goes to s's slot of the SWEEP plan's partial-R buffer: the
// gradient walk, lane_parts and the summation order stay the forward sweep's.  This is the one statement of that map -- the kernel
// (sweep_mfma_body<..., BACK>), the launch (sweep_mfma, aqc_ws_sweep.cpp) and tests/native/backwalk_selftest.cpp use it.
//
// What the slot holds: for every mirrored sub-stage but the stage's first, Z W^H of the sub-stage's INPUTS = R_s as it stands; for the
// stage's first (whose operands arrive in registers, in the layout the U products consume) Z' W'^H of its OUTPUTS, which is the
// "inputs" form of R_s the R-only sub-stage of the forward sweep leaves there as well: rgrad_kernel conjugates it by U_s (conj_sub).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AQC_BW_HD __host__ __device__
#else
#define AQC_BW_HD
#endif

namespace aqc {

// forward sub-stage (= partial-R slot row of the sweep plan) of mirrored sub-stage `mirrored_sub`; both index all sub-stages of their plan
AQC_BW_HD constexpr int backwalk_r_slot(int nsubs_total, int mirrored_sub) { return nsubs_total - 1 - mirrored_sub; }

// the forward sub-stage whose R arrives in the "inputs" form (see above): the one the mirrored stage starting at `mirrored_sub_begin` walks first
AQC_BW_HD constexpr int backwalk_conj_sub(int nsubs_total, int mirrored_sub_begin) { return backwalk_r_slot(nsubs_total, mirrored_sub_begin); }

// Tile sizes that have the backward form.  Not 2^11: its two waves per SIMD have 256 registers each, and holding both operand layouts of
// a group (R from the inputs, then the U^H products) next to the pipeline's next group needs scratch memory there; the route keeps the
// forward launches on such a plan (projected_backwalk, aqc_ws_project.cpp).
AQC_BW_HD constexpr bool backwalk_tile(int k) { return k >= 8 && k <= 12 && k != 11; }

}  // namespace aqc
