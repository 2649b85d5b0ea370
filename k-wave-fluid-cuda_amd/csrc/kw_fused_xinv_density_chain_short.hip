// kw_fused_xinv_density_chain_short.hip — chained density epilogues of lines < KW_LONG_LINES, whole planes too
#include "kw_fused.hip"

kw_status kwfused::xinv_density_chain_short(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_density<true, false, X_SHORT>(terms, ctx, ncomp, a, tile0, ntiles);
}

kw_status kwfused::xinv_density_plane(int chain, int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes)
{
  return chain ? launch_xinv_density<true, false, X_ALL, true>(terms, ctx, ncomp, a, plane0, nplanes)
               : launch_xinv_density<false, false, X_ALL, true>(terms, ctx, ncomp, a, plane0, nplanes);
}
