// kw_fused_xinv_density_oneterm_short.hip — density epilogues of the one-term power law (terms == 5), plain and chained: lines < KW_LONG_LINES, whole planes too
#include "kw_fused.hip"

kw_status kwfused::xinv_density_oneterm_short(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_density_oneterm<false, X_SHORT>(chain, ctx, ncomp, a, tile0, ntiles);
}

kw_status kwfused::xinv_density_oneterm_plane(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes)
{
  return launch_xinv_density_oneterm<false, X_ALL, true>(chain, ctx, ncomp, a, plane0, nplanes);
}
