// kw_fused_xinv_other_tail.hip — store / velocity / initial-velocity / pressure-sum epilogues, masked forms
#include "kw_fused.hip"

kw_status kwfused::xinv_other_tail(int epi, int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return launch_xinv_other<true>(epi, chain, ctx, ncomp, a, tile0, ntiles);
}
