// second_order_host_check.cpp — the host side of the exact k-space propagator as a stand-alone CPU program:
// SecondOrderParameters::init through valid inputs (the expanded sides by their rule, the wrap-free time, the damping rule,
// the sensor points translated into the expanded volume) and refusals.  Built with -fsanitize=address,undefined by
// tests/test_second_order_host.py together with host/SecondOrderParameters.cpp and host/GridRules.cpp (the shared rules
// and the fast-path length table).  Host code only.  Every case prints "<name>: ok ..." or "<name>: <message>".
#include <cmath>
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>

#include "SecondOrderParameters.h"

namespace {

SecondOrderParameters base()
{
  SecondOrderParameters p;
  p.nx = 24; p.ny = 20; p.nz = 18;
  p.dx = 1.0e-4; p.dy = 1.2e-4; p.dz = 0.9e-4;
  p.c0 = 1500.0;
  p.tMax = 1.03e-6;
  p.sensorIndex = { 0, 23, 24 * 20 * 18 - 1 };
  return p;
}

void run(const char* name, const std::function<void(SecondOrderParameters&)>& change, bool fused = true)
{
  SecondOrderParameters p = base();
  change(p);
  DeviceOptions o;
  o.fusedKernels = fused;
  try
  {
    p.init(o);
    const std::vector<uint64_t> s = p.expandedSensorIndex();
    std::printf("%s: ok E=%zux%zux%zu fast=%d t_free=%.6e B=%.6f/%.6f last=%llu\n", name, p.ex, p.ey, p.ez, p.fastPath ? 1 : 0,
                p.tFree, p.bSmallest, p.bLargest, s.empty() ? 0ull : static_cast<unsigned long long>(s.back()));
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}

void time(const char* name, double t)
{
  try
  {
    SecondOrderParameters::checkTime(t);
    std::printf("%s: ok\n", name);
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}

} // namespace

int main()
{
  run("default", [](SecondOrderParameters&) {});
  run("rocfft", [](SecondOrderParameters&) {}, false);
  run("beyond_1024", [](SecondOrderParameters& p) { p.nx = 1020; p.sensorIndex.clear(); });
  run("box", [](SecondOrderParameters& p) { p.ex = 24; p.ey = 20; p.ez = 18; p.tMax = 0.0; });
  run("given_odd", [](SecondOrderParameters& p) { p.ex = 27; p.ey = 20; p.ez = 33; });
  run("absorbing", [](SecondOrderParameters& p) { p.alphaCoeff = 0.75; });
  run("stokes", [](SecondOrderParameters& p) { p.alphaCoeff = 0.01; p.alphaPower = 2.0; });
  run("no_sensors", [](SecondOrderParameters& p) { p.sensorIndex.clear(); });
  run("overdamped", [](SecondOrderParameters& p) { p.alphaCoeff = 500.0; });
  run("overdamped_low_k", [](SecondOrderParameters& p) { p.alphaCoeff = 100.0; p.alphaPower = 0.5; });
  run("nz_zero", [](SecondOrderParameters& p) { p.nz = 0; });
  run("dz_zero", [](SecondOrderParameters& p) { p.dz = 0.0; });
  run("c0_negative", [](SecondOrderParameters& p) { p.c0 = -1.0; });
  run("t_max_missing", [](SecondOrderParameters& p) { p.tMax = 0.0; });
  run("alpha_negative", [](SecondOrderParameters& p) { p.alphaCoeff = -1.0; });
  run("power_one", [](SecondOrderParameters& p) { p.alphaPower = 1.0; });
  run("power_three", [](SecondOrderParameters& p) { p.alphaPower = 3.0; });
  run("e_missing", [](SecondOrderParameters& p) { p.ex = 48; p.ey = 48; });
  run("e_small", [](SecondOrderParameters& p) { p.ex = 48; p.ey = 48; p.ez = 17; });
  run("too_large", [](SecondOrderParameters& p) { p.ex = 2048; p.ey = 2048; p.ez = 1024; });
  run("sensor_outside", [](SecondOrderParameters& p) { p.sensorIndex.push_back(24 * 20 * 18); });
  time("t_zero", 0.0);
  time("t_negative", -1.0e-6);
  time("t_nan", std::nan(""));
  return 0;
}
