// second_order_plane_record_host_check.cpp — the host side of the plane-sensor record of the 3-D exact k-space propagator
// as a stand-alone CPU program: the plane rule, the output times of one pass (the default from the byte budget, a given
// number and its refusals), the order of the passes, and the indexing that carries a pass [count][Ny][Nx] into the record
// [n_times][Ny][Nx] — run on host arrays exactly as SecondOrder::planeRecord runs it on its copies, every value checked to
// arrive once and in its place.  Built with -fsanitize=address,undefined by tests/test_second_order_plane_record_host.py
// together with host/SecondOrderParameters.cpp and host/GridRules.cpp.  Host code only.  Every case prints
// "<name>: ok ..." or "<name>: <message>".
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "SecondOrderParameters.h"

namespace {

using P = SecondOrderParameters;

P base()
{
  P p;
  p.nx = 24; p.ny = 20; p.nz = 18;
  p.dx = 1.0e-4; p.dy = 1.2e-4; p.dz = 0.9e-4;
  p.c0 = 1500.0;
  p.tMax = 1.03e-6;
  return p;
}

// the record of nTimes output times in passes of `given` (0: the default): value (t, y, x) = its own flat index + 1
void run(const char* name, const std::function<void(P&)>& change, int64_t plane, uint64_t given, size_t nTimes)
{
  P p = base();
  change(p);
  try
  {
    p.init(DeviceOptions());
    p.checkPlane(plane);
    const size_t chunk = p.planeChunkTimes(given);
    const std::vector<P::TimeChunk> chunks = P::planeChunks(nTimes, chunk);
    const size_t points = p.nx * p.ny;
    std::vector<float> dst(nTimes * points, 0.f);
    size_t next = 0, largest = 0;
    for (const P::TimeChunk& c : chunks)
    {
      if (c.first != next || c.count == 0 || c.count > chunk) throw std::logic_error("passes out of order");
      next = c.first + c.count;
      largest = c.count > largest ? c.count : largest;
      std::vector<float> pass(c.count * points); // [count][Ny][Nx], as the crop leaves it
      for (size_t i = 0; i < pass.size(); i++) pass[i] = static_cast<float>(c.first * points + i + 1);
      float* to = dst.data() + p.planeOffset(c.first);
      for (size_t i = 0; i < p.planeOffset(c.count); i++)
      {
        if (to[i] != 0.f) throw std::logic_error("a value of the record is written twice");
        to[i] = pass[i];
      }
    }
    if (next != nTimes) throw std::logic_error("the passes do not cover the times");
    for (size_t i = 0; i < dst.size(); i++)
      if (dst[i] != static_cast<float>(i + 1)) throw std::logic_error("a value of the record is out of place");
    std::printf("%s: ok plane=%lld chunk=%zu passes=%zu largest=%zu q=%zu g=%zu\n", name, static_cast<long long>(plane), chunk,
                chunks.size(), largest, p.planeElems(), p.planeSpectrumElems(largest));
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}

} // namespace

int main()
{
  const auto same = [](P&) {};
  run("default", same, 0, 0, 12);
  run("last_plane", same, 17, 0, 1);
  run("off", same, -1, 0, 3);
  run("one_pass_exact", same, 7, 12, 12);
  run("two_passes", same, 7, 7, 12);
  run("single_times", same, 7, 1, 5);
  run("odd_box", [](P& p) { p.ex = 27; p.ey = 33; p.ez = 21; }, 3, 4, 9);
  run("budget", [](P& p) { p.nx = 128; p.ny = 128; p.nz = 128; p.ex = 256; p.ey = 256; p.ez = 256; }, 0, 0, 3);
  run("budget_one_time", [](P& p) { p.nx = 16; p.ny = 16; p.nz = 1; p.ex = 16384; p.ey = 16384; p.ez = 1; }, 0, 0, 2);
  run("plane_below", same, -2, 0, 12);
  run("plane_at_nz", same, 18, 0, 12);
  run("plane_in_expansion", same, 47, 0, 12);
  run("no_times", same, 0, 0, 0);
  run("chunk_too_many_points", same, 0, (1ull << 32) / (48 * 48) + 1, 12);
  run("chunk_too_many_times", [](P& p) { p.nx = 1; p.ny = 1; p.nz = 1; p.ex = 1; p.ey = 1; p.ez = 1; }, 0, 65535ull * 256 + 1, 12);
  run("chunk_overflow", same, 0, ~0ull, 12);
  run("bad_grid", [](P& p) { p.nx = 0; }, 0, 0, 12);
  return 0;
}
