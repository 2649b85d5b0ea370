// kw_second_order_op.h — what the code objects of the exact k-space propagator share (kw_second_order.hip: the passes and
// their rocFFT twins; kw_second_order_pair.hip: the same with dp0/dt; kw_second_order_line.hip: the line-sensor record): the constants that H needs besides the bin, how
// |k|^(y-1) is formed, their float64 derivation from a kw_second_order_op on the host, and the validation of that struct.
#ifndef KW_SECOND_ORDER_OP_H
#define KW_SECOND_ORDER_OP_H
#include <cmath>
#include <cstdint>

#include "kw_elementwise.h"

namespace {

// what H needs besides the bin: the constants of one output time, float64 on the host
struct SecondH
{
  double   dkx, dky, dkz;   // 2 pi / (E? d?)
  double   ct;              // c0 t
  double   c0, t;           // for Hs (kw_second_order_pair.hip): w = c0 k, and Hs = t at |k| = 0
  double   ac, twoT, ym1;   // a c0^y, 2 tan(pi y / 2) (0 for y = 2), y - 1
  float    divider;
  uint32_t ex, ey, ez;
  uint32_t absorbing, power;  // power: how |k|^(y-1) is formed — kPowGeneral pow(), kPowStokes y = 2: |k|, kPowHalf y = 1.5: sqrt
};

enum : uint32_t { kPowGeneral = 0, kPowStokes = 1, kPowHalf = 2 };

// the constants of one output time on the grid (Ex, Ey, Ez) = (c.nx, c.ny, c.nz), float64 on the host; frames: on the planes
// (Ex, Ey) of a frames context — the bin along y stands where the z bin does (dkz, ez := dky, Ey) and op->dz is not read
[[maybe_unused]] SecondH time_constants(const kw_constants& c, const kw_second_order_op* op, float divider, bool frames = false)
{
  SecondH g{};
  g.dkx = kTwoPi / (static_cast<double>(c.nx) * op->dx);
  g.dky = kTwoPi / (static_cast<double>(c.ny) * op->dy);
  g.dkz = frames ? g.dky : kTwoPi / (static_cast<double>(c.nz) * op->dz);
  g.ct  = op->c0 * op->t;
  g.c0  = op->c0;
  g.t   = op->t;
  g.divider = divider;
  g.ex = c.nx; g.ey = c.ny; g.ez = frames ? c.ny : c.nz;
  g.absorbing = (op->absorbing != 0 && op->a > 0.0) ? 1u : 0u;
  if (g.absorbing)
  {
    const double y = op->alpha_power;
    g.power = y == 2.0 ? kPowStokes : (y == 1.5 ? kPowHalf : kPowGeneral);
    g.ac   = op->a * pow(op->c0, y);
    g.twoT = y == 2.0 ? 0.0 : 2.0 * tan(0.5 * kTwoPi * 0.5 * y);
    g.ym1  = y - 1.0;
  }
  return g;
}

// frames: op->dz is not looked at
[[maybe_unused]] bool valid_op(const kw_second_order_op* op, bool frames = false)
{
  if (!(op->dx > 0.0 && op->dy > 0.0 && (frames || op->dz > 0.0) && op->c0 > 0.0 && op->t >= 0.0)) return false;
  return op->absorbing == 0 || (op->a >= 0.0 && op->alpha_power >= 0.0 && op->alpha_power != 1.0);
}

#ifdef __HIPCC__
// (kx*kx) of column i (0 ... Ex/2), float64: what a frame's pass hands second_h where the z-pass hands kx^2 + ky^2
__device__ __forceinline__ double frame_kr2(double dkx, uint32_t ex, uint32_t i)
{
#pragma clang fp contract(off)
  const double kx = dkx * static_cast<double>(kw_folded(i, ex));
  return kx * kx;
}
#endif

} // namespace
#endif
