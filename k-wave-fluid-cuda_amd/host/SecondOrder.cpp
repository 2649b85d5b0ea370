// SecondOrder.cpp — the 3-D form of the exact k-space propagator: the device library's kw_second_order_mix and
// kw_fused_second_order_* entry points under SecondOrderCore, and the plane-sensor record around kw_second_order_plane_*.
#include "SecondOrder.h"

#include <algorithm>
#include <vector>

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

void SecondOrder::setP0(const float* p0)
{
  mCore.setP0(p0);
  if (mPlaneWanted >= 0) preparePlane(); // (after the fused forward has read the volume)
}

// ---- the plane-sensor record --------------------------------------------------------------------------------------------
void SecondOrder::freePlane()
{
  mPlanePass.reset(); // its context, plans and arrays (after a sync of its own)
  for (void* p : { static_cast<void*>(mPlane.q), static_cast<void*>(mPlane.times) })
    if (p != nullptr) mCore.grid().release(p);
  mPlane = Plane();
}

void SecondOrder::setPlane(int64_t plane)
{
  mPar.checkPlane(plane);
  mPlaneWanted = plane;
  mPlane.ready = false; // the next setP0 prepares the plane
  if (plane < 0)
  {
    mCore.grid().check(kw_sync(context()));
    freePlane();
  }
}

void SecondOrder::setPlaneChunkTimes(uint64_t times)
{
  mPar.planeChunkTimes(times); // refuses what one pass cannot take
  mPlaneChunkGiven = times;
}

void SecondOrder::preparePlane()
{
  DeviceGrid& grid = mCore.grid();
  mPlane.ready = false;
  if (mPlane.q == nullptr) mPlane.q = grid.array(2 * mPar.planeElems());
  const uint32_t plane = static_cast<uint32_t>(mPlaneWanted);
  if (!grid.fused())
  {
    // the kept spectrum is the natural (kx, ky, kz) one
    grid.check(kw_second_order_plane_prepare(context(), mPlane.q, mCore.kept(), plane));
    mPlane.ready = true;
    return;
  }
  // the pipeline keeps (kx, ky, z) in its own layout: one 3-D transform of the embedded volume, which the fused forward has
  // left as it was.  Only the prepare reads the natural spectrum (8 R bytes: 1 GB at 512^3): it goes again at once.
  if (!mPlanePlans) grid.check(kw_fft_create_plans_3d(context()));
  mPlanePlans = true;
  float* spec = grid.array(2 * mPar.nReduced());
  grid.check(kw_fft_r2c_3d(context(), mCore.vol(), spec));
  grid.check(kw_second_order_plane_prepare(context(), mPlane.q, spec, plane));
  grid.check(kw_sync(context()));
  grid.release(spec);
  mPlane.ready = true;
}

SecondOrder::PlanePass::PlanePass(const SecondOrderParameters& par, size_t passTimes)
  : grid(par.options.deviceIdx), times(passTimes)
{
  grid.setConstants(gridConstants(par.ex, par.ey, times));
  grid.check(kw_fft_create_plans_frames(grid.ctx())); // `times` independent 2-D transforms of (Ex, Ey)
  g      = grid.array(2 * par.planeSpectrumElems(times));
  planes = grid.array(par.ex * par.ey * times);
  out    = grid.array(par.nx * par.ny * times);
  // a last pass of fewer times transforms the whole batch: the planes past its own hold what an earlier pass left there
  grid.check(kw_memset(grid.ctx(), g, 0, 2 * par.planeSpectrumElems(times) * sizeof(float)));
  grid.check(kw_sync(grid.ctx()));
}

void SecondOrder::makePlanePass(size_t times)
{
  if (mPlanePass && mPlanePass->times == times) return;
  mPlanePass.reset(); // the old one goes first
  mPlanePass.reset(new PlanePass(mPar, times));
}

void SecondOrder::planeRecord(const double* times, size_t nTimes, float* dst)
{
  if (mPlaneWanted < 0) throw std::invalid_argument("plane_record: no plane set");
  if (!mPlane.ready) throw std::invalid_argument("plane_record: no p0 since the plane was set");
  if (mCore.hasDp0dt())
    throw std::invalid_argument("plane_record: a dp0dt is set and the plane record takes p0 alone (not built: dp0dt in "
                                "plane_record); clear it with set_dp0dt(NULL), or sample the plane with run(times)");
  const size_t chunkTimes = std::min(planeChunkTimes(), std::max<size_t>(nTimes, 1));
  const std::vector<SecondOrderRules::TimeChunk> chunks = SecondOrderParameters::planeChunks(nTimes, chunkTimes);
  for (size_t i = 0; i < nTimes; i++) SecondOrderRules::checkTime(times[i]);

  DeviceGrid& grid = mCore.grid();
  if (nTimes > mPlane.timesCapacity)
  {
    if (mPlane.times != nullptr) grid.release(mPlane.times);
    mPlane.times = nullptr;
    mPlane.timesCapacity = 0;
    mPlane.times = static_cast<double*>(grid.bytes(nTimes * sizeof(double)));
    mPlane.timesCapacity = nTimes;
  }
  grid.check(kw_memcpy_h2d(context(), mPlane.times, times, nTimes * sizeof(double)));
  makePlanePass(chunkTimes);

  const kw_second_order_op op = mCore.op(0.0);
  PlanePass& pass = *mPlanePass;
  kw_ctx* second = pass.grid.ctx();
  for (const auto& c : chunks)
  {
    const uint32_t count = static_cast<uint32_t>(c.count);
    grid.check(kw_second_order_plane_record(context(), pass.g, mPlane.q, &op, mPlane.times + c.first, count));
    grid.check(kw_sync(context())); // the second context has a stream of its own
    pass.grid.check(kw_fft_c2r_frames(second, pass.g, pass.planes));
    pass.grid.check(kw_plane_recon_crop(second, pass.out, pass.planes, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
                                        count, static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny), count, 0));
    // the pass holds [count][Ny][Nx], the record [n_times][Ny][Nx]: one piece
    if (dst == nullptr) pass.grid.check(kw_sync(second));
    else pass.grid.check(kw_memcpy_d2h(second, dst + mPar.planeOffset(c.first), pass.out, mPar.planeOffset(c.count) * sizeof(float)));
  }
}
