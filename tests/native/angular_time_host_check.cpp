// angular_time_host_check.cpp — the host side of the time-domain angular-spectrum projector as a stand-alone CPU program:
// AngularTimeParameters::init through valid inputs (the expanded sides and the record length by their rules) and refusals,
// and the absorption table.  Built with -fsanitize=address,undefined by tests/test_angular_time_host.py together with
// host/AngularTimeParameters.cpp and host/GridRules.cpp (the shared rules and the fast-path length table).  Host code only.
// Every case prints "<name>: ok ..." or "<name>: <message>".
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>

#include "AngularTimeParameters.h"

namespace {

AngularTimeParameters base()
{
  AngularTimeParameters p;
  p.nx = 24; p.ny = 20; p.nt = 40;
  p.dx = p.dy = 1e-3;
  p.dt = 2e-7;
  p.c0 = 1500.0;
  p.z = { 0.5e-3, 1.6e-3, 2.0e-3 };
  return p;
}

void run(const char* name, const std::function<void(AngularTimeParameters&)>& change, bool fused = true)
{
  AngularTimeParameters p = base();
  change(p);
  DeviceOptions o;
  o.fusedKernels = fused;
  try
  {
    p.init(o);
    const std::vector<double> ak = p.akTable();
    std::printf("%s: ok E=%zux%zu Lt=%zu fast=%d ak=%zu last=%.6e\n", name, p.ex, p.ey, p.lt, p.fastPath ? 1 : 0, ak.size(),
                ak.back());
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}

} // namespace

int main()
{
  run("default", [](AngularTimeParameters&) {});
  run("rocfft", [](AngularTimeParameters&) {}, false);
  run("odd_nt_rocfft", [](AngularTimeParameters& p) { p.nt = 41; }, false);
  run("beyond_1024", [](AngularTimeParameters& p) { p.nt = 1025; });
  run("given", [](AngularTimeParameters& p) { p.ex = 32; p.ey = 48; p.lt = 64; });
  run("given_slow", [](AngularTimeParameters& p) { p.lt = 42; });
  run("absorbing", [](AngularTimeParameters& p) { p.alphaCoeff = 0.75; p.alphaPower = 1.5; });
  run("planes_4096", [](AngularTimeParameters& p) { p.z.assign(4096, 1e-3); });
  run("planes_4097", [](AngularTimeParameters& p) { p.z.assign(4097, 1e-3); });
  run("planes_0", [](AngularTimeParameters& p) { p.z.clear(); });
  run("z_negative", [](AngularTimeParameters& p) { p.z[1] = -1e-3; });
  run("nt_zero", [](AngularTimeParameters& p) { p.nt = 0; });
  run("dt_zero", [](AngularTimeParameters& p) { p.dt = 0.0; });
  run("lt_odd", [](AngularTimeParameters& p) { p.lt = 41; });
  run("lt_small", [](AngularTimeParameters& p) { p.lt = 38; });
  run("e_odd", [](AngularTimeParameters& p) { p.ex = 49; p.ey = 48; });
  run("e_small", [](AngularTimeParameters& p) { p.ex = 48; p.ey = 18; });
  run("alpha_negative", [](AngularTimeParameters& p) { p.alphaCoeff = -1.0; });
  run("power_negative", [](AngularTimeParameters& p) { p.alphaPower = -1.0; });
  run("too_large", [](AngularTimeParameters& p) { p.ex = 2048; p.ey = 2048; p.lt = 1024; });
  return 0;
}
