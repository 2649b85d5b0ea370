// SecondOrder.cpp — the 3-D form of the exact k-space propagator: the device library's kw_second_order_mix and
// kw_fused_second_order_* entry points under SecondOrderCore.
#include "SecondOrder.h"

namespace
{
const SecondOrderEntries kEntries = { false,
                                      kw_fused_second_order_elems,
                                      kw_fused_second_order_forward,
                                      kw_fused_second_order_time,
                                      kw_second_order_mix,
                                      kw_fused_second_order_time_pair,
                                      kw_second_order_mix_pair,
                                      kw_fft_r2c_3d,
                                      kw_fft_c2r_3d };

SecondOrderForm form(const SecondOrderParameters& p)
{
  kw_second_order_op op{};
  op.dx = p.dx; op.dy = p.dy; op.dz = p.dz; op.c0 = p.c0;
  op.a  = p.a;
  op.alpha_power = p.alphaPower;
  op.absorbing   = p.a > 0.0 ? 1 : 0;
  return { p.ex, p.ey, p.ez, p.nx, p.ny, p.nz, 1.0f / static_cast<float>(p.nExpanded()), op, &kEntries };
}
} // namespace

SecondOrder::SecondOrder(const SecondOrderParameters& parameters)
  : mPar(parameters), mCore(mPar, form(mPar), mPar.expandedSensorIndex())
{
}
