// kw_fused_xinv_density_stokes_tail.hip — density epilogues with the Stokes pressure (terms == 4), plain and chained: masked forms
#include "kw_fused.hip"

kw_status kwfused::xinv_density_stokes_tail(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_density_stokes<true, X_ALL>(chain, ctx, ncomp, a, tile0, ntiles);
}
