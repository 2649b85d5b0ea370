// kw_fused_xinv_psum_one_tail.hip — the one-term pressure sum (EPI_PSUM1), plain and chained: masked forms
#include "kw_fused.hip"

kw_status kwfused::xinv_psum_one_tail(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_psum_one<true>(chain, ctx, ncomp, a, tile0, ntiles);
}
