// kw_fused_xinv_other.hip — store / velocity / initial-velocity / pressure-sum epilogues, whole planes too
#include "kw_fused.hip"

kw_status kwfused::xinv_other(int epi, int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_other<false>(epi, chain, ctx, ncomp, a, tile0, ntiles);
}

kw_status kwfused::xinv_other_plane(int epi, int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes)
{
  return launch_xinv_other<false, true>(epi, chain, ctx, ncomp, a, plane0, nplanes);
}
