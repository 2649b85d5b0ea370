// kw_fused_xinv_psum_one.hip — the one-term pressure sum (EPI_PSUM1), plain and chained: full tiles of every length, whole planes
#include "kw_fused.hip"

kw_status kwfused::xinv_psum_one(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_psum_one<false>(chain, ctx, ncomp, a, tile0, ntiles);
}

kw_status kwfused::xinv_psum_one_plane(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes)
{
  return launch_xinv_psum_one<false, true>(chain, ctx, ncomp, a, plane0, nplanes);
}
