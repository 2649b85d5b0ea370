// second_order_line_record_host_check.cpp — the host side of the line-sensor record of the batched 2-D exact k-space
// propagator as a stand-alone CPU program: the row rule, the output times of one pass (the default from the byte budget, a
// given number and its refusals), the order of the passes, and the indexing that carries a pass [F][count][Nx] into the
// record [F][n_times][Nx] — run on host arrays exactly as SecondOrderFrames::lineRecord runs it on its copies, every value
// checked to arrive once and in its place.  Built with -fsanitize=address,undefined by
// tests/test_second_order_line_record_host.py together with host/SecondOrderFramesParameters.cpp and host/GridRules.cpp.
// Host code only.  Every case prints "<name>: ok ..." or "<name>: <message>".
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "SecondOrderFramesParameters.h"

namespace {

using P = SecondOrderFramesParameters;

P base()
{
  P p;
  p.nx = 24; p.ny = 20; p.frames = 5;
  p.dx = 1.0e-4; p.dy = 1.2e-4;
  p.c0 = 1500.0;
  p.tMax = 1.03e-6;
  return p;
}

// the record of nTimes output times in passes of `given` (0: the default): value (f, t, x) = its own flat index + 1
void run(const char* name, const std::function<void(P&)>& change, int64_t row, uint64_t given, size_t nTimes)
{
  P p = base();
  change(p);
  try
  {
    p.init(DeviceOptions());
    p.checkLineRow(row);
    const size_t chunk = p.lineChunkTimes(given);
    const std::vector<P::LineChunk> chunks = P::lineChunks(nTimes, chunk);
    const size_t F = p.frames, nx = p.nx;
    std::vector<float> dst(F * nTimes * nx, 0.f);
    size_t next = 0, largest = 0;
    for (const P::LineChunk& c : chunks)
    {
      if (c.first != next || c.count == 0 || c.count > chunk) throw std::logic_error("passes out of order");
      next = c.first + c.count;
      largest = c.count > largest ? c.count : largest;
      std::vector<float> pass(F * c.count * nx); // [F][count][Nx], as the crop leaves it
      for (size_t f = 0; f < F; f++)
        for (size_t t = 0; t < c.count; t++)
          for (size_t x = 0; x < nx; x++) pass[(f * c.count + t) * nx + x] = static_cast<float>((f * nTimes + c.first + t) * nx + x + 1);
      for (size_t f = 0; f < F; f++)
      {
        const float* src = pass.data() + f * c.count * nx;
        float*       to  = dst.data() + p.lineOffset(f, c.first, nTimes);
        for (size_t i = 0; i < c.count * nx; i++)
        {
          if (to[i] != 0.f) throw std::logic_error("a value of the record is written twice");
          to[i] = src[i];
        }
      }
    }
    if (next != nTimes) throw std::logic_error("the passes do not cover the times");
    for (size_t i = 0; i < dst.size(); i++)
      if (dst[i] != static_cast<float>(i + 1)) throw std::logic_error("a value of the record is out of place");
    std::printf("%s: ok row=%lld chunk=%zu passes=%zu largest=%zu q=%zu g=%zu\n", name, static_cast<long long>(row), chunk,
                chunks.size(), largest, p.lineElems(), p.lineSpectrumElems(largest));
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
  run("last_row", same, 19, 0, 1);
  run("off", same, -1, 0, 3);
  run("one_pass_exact", same, 7, 12, 12);
  run("two_passes", same, 7, 7, 12);
  run("single_times", same, 7, 1, 5);
  run("odd_plane", [](P& p) { p.ex = 27; p.ey = 33; }, 3, 4, 9);
  run("one_frame", [](P& p) { p.frames = 1; }, 3, 5, 11);
  run("budget", [](P& p) { p.nx = 256; p.ny = 256; p.ex = 512; p.ey = 512; p.frames = 64; }, 0, 0, 3);
  run("budget_one_time", [](P& p) { p.nx = 16; p.ny = 16; p.ex = 1024; p.ey = 16; p.frames = 65535; }, 0, 0, 2);
  run("row_below", same, -2, 0, 12);
  run("row_at_ny", same, 20, 0, 12);
  run("row_in_expansion", same, 47, 0, 12);
  run("no_times", same, 0, 0, 0);
  run("chunk_too_many_points", same, 0, (1ull << 32) / (48 * 5) + 1, 12);
  run("chunk_too_many_times", [](P& p) { p.nx = 1; p.ny = 1; p.ex = 1; p.ey = 1; p.frames = 1; }, 0, 65535ull * 256 + 1, 12);
  run("chunk_overflow", same, 0, ~0ull, 12);
  run("bad_grid", [](P& p) { p.nx = 0; }, 0, 0, 12);
  return 0;
}
