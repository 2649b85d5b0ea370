// kw_fused_xinv_density_plain_tail.hip — density epilogues storing their terms, masked forms
#include "kw_fused.hip"

kw_status kwfused::xinv_density_plain_tail(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_density<false, true, X_ALL>(terms, ctx, ncomp, a, tile0, ntiles);
}
