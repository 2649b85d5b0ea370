// cw_host_check.cpp — the host side of the CW field propagator as a stand-alone CPU program: CwParameters::init through
// its valid inputs (T and the expanded grid by the no-wrap-around rule) and every refusal.  Built with
// -fsanitize=address,undefined by tests/test_cw_host.py together with host/CwParameters.cpp and host/GridRules.cpp.
// Every case prints "<name>: ok ..." or "<name>: <message>".
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>

#include "CwParameters.h"

namespace {

CwParameters base()
{
  CwParameters p;
  p.nx = 32; p.ny = 32; p.nz = 32;
  p.dx = p.dy = p.dz = 1e-3;
  p.c0 = 1500.0;
  p.f0 = 250e3;
  return p;
}

void run(const char* name, const std::function<void(CwParameters&)>& change, bool fused = true)
{
  CwParameters p = base();
  change(p);
  DeviceOptions o;
  o.fusedKernels = fused;
  try
  {
    p.init(o);
    std::printf("%s: ok T=%.9e E=%zux%zux%zu fast=%d scale=%g,%g\n", name, p.t, p.ex, p.ey, p.ez, p.fastPath ? 1 : 0, p.scaleRe,
                p.scaleIm);
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}
} // namespace

int main()
{
  // ---- valid ----------------------------------------------------------------------------------------------------------
  run("cube32", [](CwParameters&) {});
  run("cube32_rocfft", [](CwParameters&) {}, false);
  run("three_sides", [](CwParameters& p) { p.nx = 8; p.ny = 12; p.nz = 10; p.dy = 0.7e-3; p.dz = 0.9e-3; });
  run("given_t", [](CwParameters& p) { p.t = 2e-5; });
  run("given_e", [](CwParameters& p) { p.nx = 6; p.ny = 8; p.nz = 8; p.ex = 22; p.ey = 24; p.ez = 26; });
  run("given_e_fast", [](CwParameters& p) { p.ex = p.ey = p.ez = 128; });
  run("beyond_1024", [](CwParameters& p) { p.nx = 600; p.ny = 16; p.nz = 16; });
  run("kwave_scale", [](CwParameters& p) { p.kwaveScale(); });
  run("lengths", [](CwParameters&) {
    if (!GridRule::isFastLength(16) || !GridRule::isFastLength(1024) || GridRule::isFastLength(22) || GridRule::nextFastLength(17) != 32 ||
        GridRule::nextFastLength(1025) != 0 || GridRule::nextFastLength(0) != 16 || CwRule::leastSide(32, 1e-3, 1500.0, 3.7e-5) != 88)
      throw std::invalid_argument("length table is wrong");
  });
  // ---- refused --------------------------------------------------------------------------------------------------------
  run("nx_zero", [](CwParameters& p) { p.nx = 0; });
  run("ny_zero", [](CwParameters& p) { p.ny = 0; });
  run("two_d", [](CwParameters& p) { p.nz = 1; });
  run("dx_zero", [](CwParameters& p) { p.dx = 0.0; });
  run("dy_negative", [](CwParameters& p) { p.dy = -1e-3; });
  run("dz_nan", [](CwParameters& p) { p.dz = std::stod("nan"); });
  run("c0_zero", [](CwParameters& p) { p.c0 = 0.0; });
  run("f0_zero", [](CwParameters& p) { p.f0 = 0.0; });
  run("f0_nyquist", [](CwParameters& p) { p.f0 = 800e3; p.dz = 1.25e-3; });
  run("t_negative", [](CwParameters& p) { p.t = -1e-6; });
  run("t_huge", [](CwParameters& p) { p.t = 1e9; });
  run("e_partial", [](CwParameters& p) { p.ex = 96; p.ez = 96; });
  run("e_odd", [](CwParameters& p) { p.ex = 96; p.ey = 97; p.ez = 96; });
  run("e_small", [](CwParameters& p) { p.ex = 96; p.ey = 96; p.ez = 86; });
  run("e_total", [](CwParameters& p) { p.ex = p.ey = p.ez = 2048; });
  run("scale_nan", [](CwParameters& p) { p.scaleIm = std::stod("inf"); });
  return 0;
}
