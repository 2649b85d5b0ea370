// kw_second_order_op.h — what the code objects of the exact k-space propagator share (kw_second_order.hip: the passes and
// their rocFFT twins; kw_second_order_pair.hip: the same with dp0/dt; kw_second_order_line.hip: the line-sensor record; kw_second_order_plane.hip: the plane-sensor record): the constants that H needs besides the bin, how
// |k|^(y-1) is formed, their float64 derivation from a kw_second_order_op on the host, the validation of that struct, and
// for the two records the time-independent factors of a bin, H from them, and the phase of the recorded position.
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

// ---- what the two records share (kw_second_order_line.hip: a row of every frame; kw_second_order_plane.hip: a plane of the
// volume): both sum H Q over the folded bins of the axis they do not invert, with H formed by the same expressions ----

// the factors of H that do not depend on time (second_h's float64 expressions in its order, up to the products with ct)
struct LineBin
{
  double   kr;   // |k| r   (lossless: |k|)
  double   kg;   // |k| g
  float    q;    // g / r
  uint32_t zero; // |k| = 0: H = 1
};

// bin m (folded: m <= E/2) along the summed axis, whose 2 pi / (E d) is g.dkz (a frames pass: 2 pi / (Ey dy)); kr2: the rest
// of |k|^2 as the pass that feeds second_h forms it — (kx*kx) of a frame's column, kx^2 + ky^2 of the volume's
__device__ __forceinline__ LineBin line_bin(const SecondH& g, double kr2, uint32_t m)
{
#pragma clang fp contract(off)
  const double ky = g.dkz * static_cast<double>(m);
  const double k2 = kr2 + (ky * ky);
  LineBin b{ 0.0, 0.0, 0.f, 0u };
  if (k2 == 0.0) { b.zero = 1u; return b; }
  const double k = sqrt(k2);
  if (g.absorbing == 0) { b.kr = k; return b; }
  const uint32_t pw = g.power;
  const double   s  = pw == kPowStokes ? k : (pw == kPowHalf ? sqrt(k) : pow(k, g.ym1));
  const double   gg = g.ac * s;
  const double   B  = (1.0 - (g.twoT * gg)) - (gg * gg);
  const double   r  = sqrt(B);
  b.kr = k * r;
  b.kg = k * gg;
  b.q  = static_cast<float>(gg / r);
  return b;
}

// H of one bin at ct = c0 t: second_h from the phase word on, without the divider (Q carries it)
__device__ __forceinline__ float line_h(double kr, double kg, float q, uint32_t zero, double ct, bool absorbing)
{
#pragma clang fp contract(off)
  const uint32_t word = kw_phase_word((kr * ct) / kTwoPi);
  const float    ang  = static_cast<float>(static_cast<int32_t>(word)) * 1.4629180792671596e-9f;
  float h;
  if (!absorbing) h = cosf(ang);
  else
  {
    float sn, cs;
    sincosf(ang, &sn, &cs);
    const float E = exp2f(-static_cast<float>((kg * ct) * kLog2e));
    h = E * (cs + (q * sn));
  }
  return zero != 0u ? 1.0f : h;
}

// exp(+2 pi i m r / E) of bin m, for the record at position r (`row`) of an axis of E (`ey`) points: the exact integer
// m r mod E, the angle and its cosine and sine in float64, rounded once
__device__ __forceinline__ float2 row_phase(uint32_t m, uint32_t row, uint32_t ey)
{
  const uint32_t e   = static_cast<uint32_t>((static_cast<uint64_t>(m) * row) % ey);
  const double   ang = kTwoPi * (static_cast<double>(e) / static_cast<double>(ey));
  return make_float2(static_cast<float>(cos(ang)), static_cast<float>(sin(ang)));
}
#endif

} // namespace
#endif
