// kw_fused_xinv_density_chain_long.hip — chained density epilogues of lines >= KW_LONG_LINES
#include "kw_fused.hip"

kw_status kwfused::xinv_density_chain_long(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_density<true, false, X_LONG>(terms, ctx, ncomp, a, tile0, ntiles);
}
