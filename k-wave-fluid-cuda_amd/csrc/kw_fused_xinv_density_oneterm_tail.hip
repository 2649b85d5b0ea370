// kw_fused_xinv_density_oneterm_tail.hip — density epilogues of the one-term power law (terms == 5), plain and chained: masked forms
#include "kw_fused.hip"

kw_status kwfused::xinv_density_oneterm_tail(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_density_oneterm<true, X_ALL>(chain, ctx, ncomp, a, tile0, ntiles);
}
