// The table-walk MSM for G2: the Fq2 instantiations of msm_table.hpp.  Default scheduler (why this is a unit of its own:
// msm_table.hpp).
#include "msm_table.hpp"

namespace spp {

template void launch_build_table<Fq2>(hipStream_t, const Affine<Fq2>*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, Affine<Fq2>*,
                                     XYZZ<Fq2>*, Fq2*, const MsmBlock*, uint32_t);
template void launch_msm_accumulate<Fq2>(hipStream_t, const Affine<Fq2>*, const MsmBlock*, const int16_t*, XYZZ<Fq2>*, uint32_t, uint32_t, uint32_t,
                                        const MsmPlan&, hipEvent_t, hipEvent_t, uint32_t*);
template void launch_msm_reduce_multi<Fq2>(hipStream_t, MsmFoldSets<Fq2>, uint32_t, uint32_t);
template void launch_msm_reduce<Fq2>(hipStream_t, XYZZ<Fq2>*, XYZZ<Fq2>*, uint32_t, const MsmPlan&, uint32_t, bool);
template void launch_fixed_base_mul<Fq2>(hipStream_t, const Affine<Fq2>*, uint32_t, const Fr*, uint32_t, Affine<Fq2>*);

}  // namespace spp
