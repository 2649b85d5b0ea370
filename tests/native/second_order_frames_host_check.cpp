// second_order_frames_host_check.cpp — the host side of the batched 2-D exact k-space propagator as a stand-alone CPU
// program: SecondOrderFramesParameters::init through valid inputs (the expanded sides by their rule, the wrap-free time over
// the two axes, the damping rule on the 2-D grid, the sensor points of one plane translated into every frame of the expanded
// batch) and refusals.  Built with -fsanitize=address,undefined by tests/test_second_order_frames_host.py together with
// host/SecondOrderFramesParameters.cpp and host/GridRules.cpp.  Host code only.  Every case prints "<name>: ok ..." or
// "<name>: <message>".
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>

#include "SecondOrderFramesParameters.h"

namespace {

SecondOrderFramesParameters base()
{
  SecondOrderFramesParameters p;
  p.nx = 24; p.ny = 20; p.frames = 5;
  p.dx = 1.0e-4; p.dy = 1.2e-4;
  p.c0 = 1500.0;
  p.tMax = 1.03e-6;
  p.sensorIndex = { 0, 23, 24 * 20 - 1 };
  return p;
}

void run(const char* name, const std::function<void(SecondOrderFramesParameters&)>& change, bool fused = true)
{
  SecondOrderFramesParameters p = base();
  change(p);
  DeviceOptions o;
  o.fusedKernels = fused;
  try
  {
    p.init(o);
    const std::vector<uint64_t> s = p.expandedSensorIndex();
    std::printf("%s: ok E=%zux%zu F=%zu fast=%d t_free=%.6e B=%.6f/%.6f n=%zu first=%llu last=%llu\n", name, p.ex, p.ey, p.frames,
                p.fastPath ? 1 : 0, p.tFree, p.bSmallest, p.bLargest, s.size(),
                s.empty() ? 0ull : static_cast<unsigned long long>(s[p.sensorIndex.size() - 1]),
                s.empty() ? 0ull : static_cast<unsigned long long>(s.back()));
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}

} // namespace

int main()
{
  using P = SecondOrderFramesParameters;
  run("default", [](P&) {});
  run("rocfft", [](P&) {}, false);
  run("beyond_1024", [](P& p) { p.nx = 1020; p.sensorIndex.clear(); });
  run("plane", [](P& p) { p.ex = 24; p.ey = 20; p.tMax = 0.0; });
  run("given_odd", [](P& p) { p.ex = 27; p.ey = 33; });
  run("one_frame", [](P& p) { p.frames = 1; });
  run("most_frames", [](P& p) { p.frames = 65535; p.sensorIndex = { 24 * 20 - 1 }; });
  run("absorbing", [](P& p) { p.alphaCoeff = 0.75; });
  run("stokes", [](P& p) { p.alphaCoeff = 0.01; p.alphaPower = 2.0; });
  run("no_sensors", [](P& p) { p.sensorIndex.clear(); });
  run("overdamped", [](P& p) { p.alphaCoeff = 500.0; });
  run("overdamped_low_k", [](P& p) { p.alphaCoeff = 100.0; p.alphaPower = 0.5; });
  run("nx_zero", [](P& p) { p.nx = 0; });
  run("frames_zero", [](P& p) { p.frames = 0; });
  run("frames_65536", [](P& p) { p.frames = 65536; });
  run("dy_zero", [](P& p) { p.dy = 0.0; });
  run("c0_negative", [](P& p) { p.c0 = -1.0; });
  run("t_max_missing", [](P& p) { p.tMax = 0.0; });
  run("alpha_negative", [](P& p) { p.alphaCoeff = -1.0; });
  run("power_one", [](P& p) { p.alphaPower = 1.0; });
  run("e_missing", [](P& p) { p.ex = 48; });
  run("e_small", [](P& p) { p.ex = 48; p.ey = 19; });
  run("too_large", [](P& p) { p.ex = 2048; p.ey = 2048; p.frames = 1024; });
  run("sensor_outside", [](P& p) { p.sensorIndex.push_back(24 * 20); });
  return 0;
}
