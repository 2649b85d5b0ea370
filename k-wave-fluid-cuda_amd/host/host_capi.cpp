// host_capi.cpp — extern "C" entry points of libkwave_host.so (include/kwave_host.h).
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <string>

#include "HipError.h"
#include "CompressHelper.h"
#include "HostSolverHandle.h"
#include "MatrixNames.h"
#include "KSpaceFirstOrderSolver.h"
#include "ThermalSolver.h"
#include "AngularSpectrum.h"
#include "AngularSpectrumTime.h"
#include "CwPropagator.h"
#include "LineRecon.h"
#include "PlaneRecon.h"
#include "SecondOrder.h"
#include "SecondOrderFrames.h"
#include "kwave_host.h"

static thread_local std::string g_err;
void kwh_set_error(const std::string& e) { g_err = e; }

Parameters::Options kwh_convert_options(const kwh_options* o)
{
  Parameters::Options opt;
  opt.deviceIdx              = o->device_idx;
  opt.fusedKernels           = o->fused_kernels != 0;
  opt.samplingStartTimeIndex = o->sampling_start_time_index;
  opt.benchmarkTimeStepCount = o->benchmark_time_steps;
  opt.storePressureRaw = o->p_raw; opt.storePressureRms = o->p_rms; opt.storePressureMax = o->p_max;
  opt.storePressureMin = o->p_min; opt.storePressureMaxAll = o->p_max_all; opt.storePressureMinAll = o->p_min_all;
  opt.storePressureFinalAll = o->p_final;
  opt.storeVelocityRaw = o->u_raw; opt.storeVelocityRms = o->u_rms; opt.storeVelocityMax = o->u_max;
  opt.storeVelocityMin = o->u_min; opt.storeVelocityMaxAll = o->u_max_all; opt.storeVelocityMinAll = o->u_min_all;
  opt.storeVelocityFinalAll = o->u_final; opt.storeVelocityNonStaggeredRaw = o->u_non_staggered_raw;
  opt.storePressureC = o->p_c; opt.storeVelocityNonStaggeredC = o->u_non_staggered_c;
  opt.storeIntensityAvgC = o->i_avg_c; opt.noCompressionOverlap = o->no_overlap;
  opt.storeIntensityAvg = o->i_avg; opt.storeQTerm = o->q_term; opt.storeQTermC = o->q_term_c;
  opt.storeVelocityC = o->u_c; opt.frequency = o->frequency;
  opt.onlyPostProcessing = o->only_post_processing != 0;
  opt.complex40bit = o->complex_40bit != 0;
  opt.period = o->period; opt.mos = o->mos ? o->mos : 1; opt.harmonics = o->harmonics ? o->harmonics : 1;
  opt.slabRanks = o->slab_ranks ? o->slab_ranks : 1;
  opt.slabRank  = o->slab_rank;
  opt.nzGlobal  = o->nz_global;
  opt.commUniqueId = o->comm_unique_id;
  opt.exchangeFn   = reinterpret_cast<kw_exchange_fn>(o->exchange_fn);
  opt.exchangeUser = o->exchange_user;
  opt.exchangeStartFn = reinterpret_cast<kw_exchange_start_fn>(o->exchange_start_fn);
  opt.exchangeWaitFn  = reinterpret_cast<kw_exchange_wait_fn>(o->exchange_wait_fn);
  opt.exchangePieceFn = reinterpret_cast<kw_exchange_piece_fn>(o->exchange_piece_fn);
  for (int i = 0; i < 6; i++) opt.scratch[i] = o->scratch[i];
  if (o->tuning != nullptr) { opt.hasTuning = true; opt.tuning = *static_cast<const kw_tuning*>(o->tuning); }
  opt.stepGraph     = o->step_graph != 0;
  opt.commP2P       = o->comm_p2p != 0;
  opt.allgatherFn   = reinterpret_cast<int (*)(void*, const void*, void*, size_t)>(o->comm_allgather_fn);
  opt.allgatherUser = o->comm_allgather_user;
  if (o->rccl_library != nullptr) opt.rcclLibrary = o->rccl_library;
  opt.p2pEmulateLinkGbs   = o->p2p_emulate_link_gbs;
  opt.p2pEmulateLatencyUs = o->p2p_emulate_latency_us;
  opt.storePressureElements = o->p_elements != 0;
  opt.storeVelocityElements = o->u_elements != 0;
  opt.storeVelocityNonStaggeredElements = o->u_non_staggered_elements != 0;
  return opt;
}

/// Parameters::init + selectDevice + allocateMemory + loadInputData (main.cpp:857-917) on any InputProvider
void kwh_build_solver(kwh_solver& s, const InputProvider& fileInput, const Parameters::Options& opt)
{
  // Nz == 1 selects the 2-D simulation (Parameters.h:175-181 of the reference): complete the z datasets (see adapter)
  size_t nz = 0;
  fileInput.readScalarValue(kNzName, nz);
  const Input2DAdapter adapter(fileInput);
  const InputProvider& input = (nz == 1) ? static_cast<const InputProvider&>(adapter) : fileInput;
  KWH_BIND(&s)
  Parameters& params = Parameters::getInstance();
  params.init(input, opt);
  params.selectDevice();
  params.getHipParameters().setUpDeviceConstants();
  s.solver.reset(new KSpaceFirstOrderSolver());
  s.solver->allocateMemory();
  s.solver->loadInputData(input);
}


#define KWH_TRY try {
#define KWH_CATCH                                                                                                      \
  }                                                                                                                    \
  catch (const std::bad_alloc&) { g_err = "out of memory"; return 4; }                                                 \
  catch (const std::exception& e) { g_err = e.what(); return 1; }                                                      \
  catch (...) { g_err = "unknown exception"; return 1; }                                                               \
  return 0;

static DeviceOptions kwh_device_options(const kwh_options* o)
{
  DeviceOptions opt;
  opt.deviceIdx    = o->device_idx;
  opt.fusedKernels = o->fused_kernels != 0;
  return opt;
}

/// the body of kwh_cw_create and its kin: a handle, `build` (the parameters, then the operator) on it, and a failing
/// device call handed through as its kw_status (KW_ERR_NO_DEVICE among them)
template <class Handle, class Build>
static int kwh_create_handle(const char* who, const void* config, const kwh_options* o, Handle** out, Build build)
{
  KWH_TRY
  if (!config || !o || !out) throw std::invalid_argument(std::string(who) + ": NULL argument");
  *out = nullptr;
  std::unique_ptr<Handle> s(new Handle());
  try { build(*s); }
  catch (const DeviceError& e) { g_err = e.what(); return static_cast<int>(e.status); }
  *out = s.release();
  KWH_CATCH
}

/// a thermal solver with the input it was created from
struct kwh_thermal
{
  MemoryInput                    input;
  ThermalParameters              params;
  std::unique_ptr<ThermalSolver> solver;
};

/// a CW propagator with its completed parameters
struct kwh_cw
{
  CwParameters                  params;
  std::unique_ptr<CwPropagator> propagator;
};

static CwParameters kwh_cw_parameters(const kwh_cw_config* c, const kwh_options* o)
{
  if (c->source_scale_kwave != 0 && (c->source_scale_re != 0.0 || c->source_scale_im != 0.0))
    throw std::invalid_argument("source_scale: give source_scale_kwave or a factor, not both");
  CwParameters p;
  p.nx = c->nx; p.ny = c->ny; p.nz = c->nz;
  p.dx = c->dx; p.dy = c->dy; p.dz = c->dz;
  p.c0 = c->c0; p.f0 = c->f0; p.t = c->t;
  p.ex = c->ex; p.ey = c->ey; p.ez = c->ez;
  if (c->source_scale_kwave != 0) p.kwaveScale();
  else if (c->source_scale_re != 0.0 || c->source_scale_im != 0.0) { p.scaleRe = c->source_scale_re; p.scaleIm = c->source_scale_im; }
  p.init(kwh_device_options(o));
  return p;
}

/// an angular-spectrum projector with its completed parameters
struct kwh_angular
{
  AngularParameters                params;
  std::unique_ptr<AngularSpectrum> projector;
};

static AngularParameters kwh_angular_parameters(const kwh_angular_config* c, const kwh_options* o)
{
  AngularParameters p;
  p.nx = c->nx; p.ny = c->ny;
  p.dx = c->dx; p.dy = c->dy;
  p.c0 = c->c0; p.f0 = c->f0;
  p.z0 = c->z0; p.dz = c->dz;
  p.planes = c->planes;
  p.alphaNp = c->alpha_np;
  p.restriction = c->angular_restriction != 0;
  p.ex = c->ex; p.ey = c->ey;
  p.chunkPlanes = c->chunk_planes;
  p.init(kwh_device_options(o));
  return p;
}

/// a time-domain angular-spectrum projector with its completed parameters
struct kwh_angular_time
{
  AngularTimeParameters                params;
  std::unique_ptr<AngularSpectrumTime> projector;
};

static AngularTimeParameters kwh_angular_time_parameters(const kwh_angular_time_config* c, const kwh_options* o)
{
  AngularTimeParameters p;
  p.nx = c->nx; p.ny = c->ny; p.nt = c->nt;
  p.dx = c->dx; p.dy = c->dy; p.dt = c->dt;
  p.c0 = c->c0;
  p.alphaCoeff = c->alpha_coeff;
  p.alphaPower = c->alpha_power;
  p.restriction = c->angular_restriction != 0;
  p.retarded    = c->retarded_time != 0;
  p.ex = c->ex; p.ey = c->ey; p.lt = c->lt;
  if (c->n_planes > AngularRule::kMaxPlanes)
    throw std::invalid_argument("n_planes: " + std::to_string(c->n_planes) + " is above " + std::to_string(AngularRule::kMaxPlanes));
  if (c->n_planes != 0 && c->z == nullptr) throw std::invalid_argument("z: NULL with n_planes > 0");
  p.z.assign(c->z, c->z + c->n_planes);
  p.init(kwh_device_options(o));
  return p;
}

/// a k-space plane reconstruction with its completed parameters
struct kwh_plane_recon
{
  PlaneReconParameters        params;
  std::unique_ptr<PlaneRecon> recon;
};

static PlaneReconParameters kwh_plane_recon_parameters(const kwh_plane_recon_config* c, const kwh_options* o)
{
  PlaneReconParameters p;
  p.nx = c->nx; p.ny = c->ny; p.nt = c->nt;
  p.dx = c->dx; p.dy = c->dy; p.dt = c->dt;
  p.c0 = c->c0;
  p.ex = c->ex; p.ey = c->ey; p.lt = c->lt;
  p.planes = c->planes;
  p.interp = c->interp;
  p.positivity = c->positivity != 0;
  p.init(kwh_device_options(o));
  return p;
}

/// a batched k-space line reconstruction with its completed parameters
struct kwh_line_recon
{
  LineReconParameters        params;
  std::unique_ptr<LineRecon> recon;
};

static LineReconParameters kwh_line_recon_parameters(const kwh_line_recon_config* c, const kwh_options* o)
{
  LineReconParameters p;
  p.ny = c->ny; p.nt = c->nt; p.frames = c->frames;
  p.dy = c->dy; p.dt = c->dt;
  p.c0 = c->c0;
  p.ey = c->ey; p.lt = c->lt;
  p.depth = c->depth;
  p.chunkFrames = c->chunk_frames;
  p.interp = c->interp;
  p.positivity = c->positivity != 0;
  p.init(kwh_device_options(o));
  return p;
}

/// an exact k-space propagator with its completed parameters
struct kwh_second_order
{
  SecondOrderParameters        params;
  std::unique_ptr<SecondOrder> propagator;
};

/// a batched 2-D exact k-space propagator with its completed parameters
struct kwh_second_order_frames
{
  SecondOrderFramesParameters        params;
  std::unique_ptr<SecondOrderFrames> propagator;
};

/// what the two configs of the exact propagators share: the medium, t_max, the sensor points and the flags
template <class Config>
static void kwh_second_order_rules(SecondOrderRules& p, const Config* c)
{
  p.c0 = c->c0;
  p.alphaCoeff = c->alpha_coeff;
  p.alphaPower = c->alpha_power;
  p.tMax = c->t_max;
  if (c->n_sensor != 0 && c->sensor_index == nullptr) throw std::invalid_argument("sensor_index: NULL with n_sensor > 0");
  if (c->n_sensor != 0) p.sensorIndex.assign(c->sensor_index, c->sensor_index + c->n_sensor);
  p.pMax   = (c->flags & KWH_SECOND_ORDER_P_MAX) != 0;
  p.pMin   = (c->flags & KWH_SECOND_ORDER_P_MIN) != 0;
  p.pRms   = (c->flags & KWH_SECOND_ORDER_P_RMS) != 0;
  p.pFinal = (c->flags & KWH_SECOND_ORDER_P_FINAL) != 0;
}

static SecondOrderParameters kwh_second_order_parameters(const kwh_second_order_config* c, const kwh_options* o)
{
  SecondOrderParameters p;
  p.nx = c->nx; p.ny = c->ny; p.nz = c->nz;
  p.dx = c->dx; p.dy = c->dy; p.dz = c->dz;
  p.ex = c->ex; p.ey = c->ey; p.ez = c->ez;
  kwh_second_order_rules(p, c);
  p.init(kwh_device_options(o));
  return p;
}

static SecondOrderFramesParameters kwh_second_order_frames_parameters(const kwh_second_order_frames_config* c, const kwh_options* o)
{
  SecondOrderFramesParameters p;
  p.nx = c->nx; p.ny = c->ny; p.frames = c->frames;
  p.dx = c->dx; p.dy = c->dy;
  p.ex = c->ex; p.ey = c->ey;
  kwh_second_order_rules(p, c);
  p.init(kwh_device_options(o));
  return p;
}

// the entries that kwh_second_order_* and kwh_second_order_frames_* have alike; `who`: the entry's own name
template <class Handle>
static int kwh_propagator_destroy(Handle* s)
{
  KWH_TRY
  delete s;
  KWH_CATCH
}

template <class Handle>
static int kwh_propagator_set_p0(const char* who, Handle* s, const float* p0)
{
  KWH_TRY
  if (!s || !p0) throw std::invalid_argument(std::string(who) + ": NULL argument");
  s->propagator->setP0(p0);
  KWH_CATCH
}

template <class Handle>
static int kwh_propagator_set_dp0dt(const char* who, Handle* s, const float* dp0dt)
{
  KWH_TRY
  if (!s) throw std::invalid_argument(std::string(who) + ": NULL propagator");
  s->propagator->setDp0dt(dp0dt); // (NULL clears)
  KWH_CATCH
}

template <class Handle>
static int kwh_propagator_field(const char* who, Handle* s, double t, float* dst)
{
  KWH_TRY
  if (!s) throw std::invalid_argument(std::string(who) + ": NULL propagator");
  s->propagator->field(t, dst);
  KWH_CATCH
}

template <class Handle>
static int kwh_propagator_run(const char* who, Handle* s, const double* times, uint64_t n_times)
{
  KWH_TRY
  if (!s || (!times && n_times != 0)) throw std::invalid_argument(std::string(who) + ": NULL argument");
  s->propagator->run(times, n_times);
  KWH_CATCH
}

template <class Handle>
static int kwh_propagator_get(const char* who, Handle* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !name || (!dst && n != 0)) throw std::invalid_argument(std::string(who) + ": NULL argument");
  s->propagator->get(name, dst, n);
  KWH_CATCH
}

template <class Handle>
static void* kwh_propagator_context(Handle* s) { return s ? s->propagator->context() : nullptr; }

extern "C" {

const char* kwh_last_error(void) { return g_err.c_str(); }

int kwh_create(const kwh_dataset* datasets, size_t n, const kwh_options* o, kwh_solver** out)
{
  KWH_TRY
  if (!datasets || !o || !out) throw std::invalid_argument("kwh_create: NULL argument");
  *out = nullptr;
  std::unique_ptr<kwh_solver> s(new kwh_solver());
  for (size_t i = 0; i < n; i++)
  {
    const kwh_dataset& d = datasets[i];
    DimensionSizes dims(d.nx, d.ny, d.nz);
    // complex datasets come with their float count in nx*ny*nz already doubled by the caller's shape
    s->input.add(d.name, d.data, d.dtype == 0 ? InputProvider::DataType::kFloat : InputProvider::DataType::kLong, dims);
  }
  kwh_build_solver(*s, s->input, kwh_convert_options(o));
  *out = s.release();
  KWH_CATCH
}

int kwh_destroy(kwh_solver* s)
{
  KWH_TRY
  if (s)
  {
    {
      KWH_BIND(s)
      if (s->solver) kw_sync(Parameters::getInstance().getHipParameters().getContext());
      s->series_writer.reset(); // drains and closes the streamed output datasets while the streams still exist
      s->solver.reset();
    }
    delete s; // releases the device context with the parameter set
  }
  KWH_CATCH
}

int kwh_run(kwh_solver* s, uint64_t n_steps)
{
  KWH_TRY
  KWH_BIND(s)
  if (!s) throw std::invalid_argument("kwh_run: NULL solver");
  s->solver->runTimeSteps(n_steps);
  KWH_CATCH
}

int kwh_finish(kwh_solver* s)
{
  KWH_TRY
  KWH_BIND(s)
  if (!s) throw std::invalid_argument("kwh_finish: NULL solver");
  s->solver->finish();
  KWH_CATCH
}

int kwh_sync(kwh_solver* s)
{
  KWH_TRY
  KWH_BIND(s)
  (void)s;
  kwCheck(kw_sync(Parameters::getInstance().getHipParameters().getContext()));
  KWH_CATCH
}

uint64_t kwh_time_index(const kwh_solver* s) { return s ? s->params->getTimeIndex() : 0; }
void*    kwh_context(kwh_solver* s) { return s ? s->params->getHipParameters().getContext() : nullptr; }

static BaseMatrix* findMatrix(kwh_solver* s, const char* name, MatrixRecord::MatrixType* type)
{
  for (auto& rec : s->solver->getMatrixContainer().records())
    if (rec.second.matrixName == name)
    {
      *type = rec.second.matrixType;
      return rec.second.matrixPtr;
    }
  throw std::invalid_argument(std::string("no matrix named ") + name + " in this simulation");
}

int kwh_matrix_size(kwh_solver* s, const char* name, uint64_t* n)
{
  KWH_TRY
  KWH_BIND(s)
  MatrixRecord::MatrixType t;
  BaseMatrix* m = findMatrix(s, name, &t);
  if (t == MatrixRecord::MatrixType::kIndex) throw std::invalid_argument("index matrices are not float matrices");
  *n = static_cast<BaseFloatMatrix*>(m)->capacity();
  KWH_CATCH
}

int kwh_get_matrix(kwh_solver* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  KWH_BIND(s)
  MatrixRecord::MatrixType t;
  BaseMatrix* m = findMatrix(s, name, &t);
  if (t == MatrixRecord::MatrixType::kIndex) throw std::invalid_argument("index matrices are not float matrices");
  BaseFloatMatrix* f = static_cast<BaseFloatMatrix*>(m);
  if (f->capacity() != n) throw std::invalid_argument(std::string("size mismatch for matrix ") + name);
  kwCheck(kw_memcpy_d2h(Parameters::getInstance().getHipParameters().getContext(), dst, f->getDeviceData(), n * sizeof(float)));
  KWH_CATCH
}

int kwh_get_scalar(kwh_solver* s, const char* name, float* out)
{
  KWH_TRY
  KWH_BIND(s)
  const Parameters& p = Parameters::getInstance();
  const std::string n(name);
  if (n == "fused_pipeline")
  {
    if (!s) throw std::invalid_argument("kwh_get_scalar: NULL solver");
    *out = s->solver->usesFusedPipeline() ? 1.f : 0.f;
  }
  else if (n == "absorb_tau") *out = p.getAbsorbTauScalar();
  else if (n == "absorb_eta") *out = p.getAbsorbEtaScalar();
  else if (n == "c2") *out = p.getC2Scalar();
  else if (n == "dt_rho0_sgx") *out = p.getDtRho0SgxScalar();
  else if (n == "dt_rho0_sgy") *out = p.getDtRho0SgyScalar();
  else if (n == "dt_rho0_sgz") *out = p.getDtRho0SgzScalar();
  else if (n == "dt") *out = p.getDt();
  else throw std::invalid_argument("unknown scalar " + n);
  KWH_CATCH
}

int kwh_stream_info(kwh_solver* s, const char* name, uint64_t* size, uint64_t* steps)
{
  KWH_TRY
  KWH_BIND(s)
  BaseOutputStream* st = s->solver->getOutputStreamContainer().find(name);
  if (!st) throw std::invalid_argument(std::string("no output stream named ") + name);
  *size  = st->size();
  const bool series = st->reduceOp() == BaseOutputStream::ReduceOperator::kNone ||
                      st->reduceOp() == BaseOutputStream::ReduceOperator::kC;
  *steps = series ? st->sampledSteps() : 1; // raw: sampled steps; compressed: emitted frames
  KWH_CATCH
}

int kwh_stream_read(kwh_solver* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  KWH_BIND(s)
  BaseOutputStream* st = s->solver->getOutputStreamContainer().find(name);
  if (!st) throw std::invalid_argument(std::string("no output stream named ") + name);
  st->loadSeries(); // a series streamed to the output file is read back from there
  if (st->dataset().size() != n) throw std::invalid_argument(std::string("size mismatch for stream ") + name);
  std::memcpy(dst, st->dataset().data(), n * sizeof(float));
  st->releaseSeries();
  KWH_CATCH
}

int kwh_set_matrix(kwh_solver* s, const char* name, const float* src, uint64_t n)
{
  KWH_TRY
  KWH_BIND(s)
  if (!s || !name || !src) throw std::invalid_argument("kwh_set_matrix: NULL argument");
  s->solver->prepare();
  MatrixRecord::MatrixType t;
  BaseMatrix* m = findMatrix(s, name, &t);
  if (t == MatrixRecord::MatrixType::kIndex) throw std::invalid_argument("index matrices are not float matrices");
  BaseFloatMatrix* f = static_cast<BaseFloatMatrix*>(m);
  if (f->capacity() != n) throw std::invalid_argument(std::string("size mismatch for matrix ") + name);
  kwCheck(kw_memcpy_h2d(Parameters::getInstance().getHipParameters().getContext(), f->getDeviceData(), src, n * sizeof(float)));
  KWH_CATCH
}

int kwh_set_time_index(kwh_solver* s, uint64_t t)
{
  KWH_TRY
  KWH_BIND(s)
  if (!s) throw std::invalid_argument("kwh_set_time_index: NULL solver");
  if (t > Parameters::getInstance().getNt()) throw std::invalid_argument("kwh_set_time_index: beyond Nt");
  Parameters::getInstance().setTimeIndex(t);
  KWH_CATCH
}

int kwh_stream_count(kwh_solver* s, uint64_t* n)
{
  KWH_TRY
  KWH_BIND(s)
  *n = s->solver->getOutputStreamContainer().names().size();
  KWH_CATCH
}

int kwh_stream_name(kwh_solver* s, uint64_t i, char* out, uint64_t cap)
{
  KWH_TRY
  KWH_BIND(s)
  const std::vector<std::string> names = s->solver->getOutputStreamContainer().names();
  if (i >= names.size() || names[i].size() + 1 > cap) throw std::invalid_argument("kwh_stream_name: bad index or buffer");
  std::memcpy(out, names[i].c_str(), names[i].size() + 1);
  KWH_CATCH
}

int kwh_stream_count_all(kwh_solver* s, uint64_t* n)
{
  KWH_TRY
  KWH_BIND(s)
  *n = s->solver->getOutputStreamContainer().names(true).size();
  KWH_CATCH
}

int kwh_stream_name_all(kwh_solver* s, uint64_t i, char* out, uint64_t cap)
{
  KWH_TRY
  KWH_BIND(s)
  const std::vector<std::string> names = s->solver->getOutputStreamContainer().names(true);
  if (i >= names.size() || names[i].size() + 1 > cap) throw std::invalid_argument("kwh_stream_name_all: bad index or buffer");
  std::memcpy(out, names[i].c_str(), names[i].size() + 1);
  KWH_CATCH
}

int kwh_stream_checkpoint(kwh_solver* s, const char* name, float* dst, uint64_t cap, uint64_t* n_floats, uint64_t* steps)
{
  KWH_TRY
  KWH_BIND(s)
  BaseOutputStream* st = s->solver->getOutputStreamContainer().find(name);
  if (!st) throw std::invalid_argument(std::string("no output stream named ") + name);
  std::vector<float> state;
  size_t sampled = 0;
  st->checkpointState(state, sampled);
  *n_floats = state.size();
  *steps    = sampled;
  if (dst != nullptr)
  {
    if (cap < state.size()) throw std::invalid_argument("kwh_stream_checkpoint: buffer too small");
    std::memcpy(dst, state.data(), state.size() * sizeof(float));
  }
  KWH_CATCH
}

int kwh_stream_restore(kwh_solver* s, const char* name, const float* src, uint64_t n, uint64_t steps)
{
  KWH_TRY
  KWH_BIND(s)
  s->solver->prepare();
  BaseOutputStream* st = s->solver->getOutputStreamContainer().find(name);
  if (!st) throw std::invalid_argument(std::string("no output stream named ") + name);
  st->restoreState(src, n, steps);
  KWH_CATCH
}

int kwh_find_period(const float* signal, uint64_t length, float* period)
{
  KWH_TRY
  if (!signal || !period) throw std::invalid_argument("kwh_find_period: NULL argument");
  *period = CompressHelper::findPeriod(signal, length);
  KWH_CATCH
}

int kwh_pack_complex_40b(const float* v, uint64_t n, uint8_t* packed, int32_t e)
{
  KWH_TRY
  if (!v || !packed) throw std::invalid_argument("kwh_pack_complex_40b: NULL argument");
  for (uint64_t i = 0; i < n; i++) CompressHelper::convertFloatCTo40b(FloatComplex(v[2 * i], v[2 * i + 1]), packed + 5 * i, e);
  KWH_CATCH
}

int kwh_unpack_complex_40b(const uint8_t* packed, uint64_t n, float* v, int32_t e)
{
  KWH_TRY
  if (!v || !packed) throw std::invalid_argument("kwh_unpack_complex_40b: NULL argument");
  for (uint64_t i = 0; i < n; i++)
  {
    FloatComplex c;
    CompressHelper::convert40bToFloatC(packed + 5 * i, c, e);
    v[2 * i]     = c.real();
    v[2 * i + 1] = c.imag();
  }
  KWH_CATCH
}

// ---- bioheat solver --------------------------------------------------------------------------------------------------
int kwh_thermal_create(const kwh_dataset* datasets, size_t n, const kwh_options* o, kwh_thermal** out)
{
  KWH_TRY
  if (!datasets || !o || !out) throw std::invalid_argument("kwh_thermal_create: NULL argument");
  *out = nullptr;
  std::unique_ptr<kwh_thermal> s(new kwh_thermal());
  for (size_t i = 0; i < n; i++)
  {
    const kwh_dataset& d = datasets[i];
    s->input.add(d.name, d.data, d.dtype == 0 ? InputProvider::DataType::kFloat : InputProvider::DataType::kLong,
                 DimensionSizes(d.nx, d.ny, d.nz));
  }
  ThermalOptions opt;
  static_cast<DeviceOptions&>(opt) = kwh_device_options(o);
  opt.slabRanks = o->slab_ranks ? o->slab_ranks : 1;
  s->params.init(s->input, opt);
  s->solver.reset(new ThermalSolver(s->params));
  *out = s.release();
  KWH_CATCH
}

int kwh_thermal_destroy(kwh_thermal* s)
{
  KWH_TRY
  delete s;
  KWH_CATCH
}

int kwh_thermal_run(kwh_thermal* s, uint64_t n_steps, int heat_on)
{
  KWH_TRY
  if (!s) throw std::invalid_argument("kwh_thermal_run: NULL solver");
  s->solver->run(n_steps, heat_on != 0);
  KWH_CATCH
}

uint64_t kwh_thermal_time_index(const kwh_thermal* s) { return s ? s->solver->timeIndex() : 0; }
void*    kwh_thermal_context(kwh_thermal* s) { return s ? s->solver->context() : nullptr; }

int kwh_thermal_get_matrix(kwh_thermal* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !name || !dst) throw std::invalid_argument("kwh_thermal_get_matrix: NULL argument");
  s->solver->getMatrix(name, dst, n);
  KWH_CATCH
}

int kwh_thermal_set_matrix(kwh_thermal* s, const char* name, const float* src, uint64_t n)
{
  KWH_TRY
  if (!s || !name || !src) throw std::invalid_argument("kwh_thermal_set_matrix: NULL argument");
  s->solver->setMatrix(name, src, n);
  KWH_CATCH
}

int kwh_thermal_lesion_volume(kwh_thermal* s, float threshold_minutes, double* out_m3)
{
  KWH_TRY
  if (!s || !out_m3) throw std::invalid_argument("kwh_thermal_lesion_volume: NULL argument");
  *out_m3 = s->solver->lesionVolume(threshold_minutes);
  KWH_CATCH
}

int kwh_thermal_stream_read(kwh_thermal* s, const char* name, float* dst, uint64_t cap, uint64_t* size, uint64_t* steps)
{
  KWH_TRY
  if (!s || !name) throw std::invalid_argument("kwh_thermal_stream_read: NULL argument");
  const std::vector<float>& series = s->solver->series(name);
  const size_t ns = s->solver->sensorSize();
  if (size) *size = ns;
  if (steps) *steps = series.size() / ns;
  if (dst != nullptr)
  {
    if (cap < series.size()) throw std::invalid_argument(std::string("kwh_thermal_stream_read: buffer too small for ") + name);
    std::memcpy(dst, series.data(), series.size() * sizeof(float));
  }
  KWH_CATCH
}

int kwh_thermal_get_scalar(kwh_thermal* s, const char* name, float* out)
{
  KWH_TRY
  if (!s || !name || !out) throw std::invalid_argument("kwh_thermal_get_scalar: NULL argument");
  if (std::string(name) == "fused_pipeline") *out = s->solver->usesFusedPipeline() ? 1.f : 0.f;
  else throw std::invalid_argument(std::string("unknown scalar ") + name);
  KWH_CATCH
}

// ---- CW field propagator ---------------------------------------------------------------------------------------------
int kwh_cw_plan(const kwh_cw_config* config, const kwh_options* o, double* out_t, uint64_t out_expanded[3], int32_t* out_fast_path)
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_cw_plan: NULL argument");
  const CwParameters p = kwh_cw_parameters(config, o);
  if (out_t) *out_t = p.t;
  if (out_expanded) { out_expanded[0] = p.ex; out_expanded[1] = p.ey; out_expanded[2] = p.ez; }
  if (out_fast_path) *out_fast_path = p.fastPath ? 1 : 0;
  KWH_CATCH
}

int kwh_cw_create(const kwh_cw_config* config, const kwh_options* o, kwh_cw** out)
{
  return kwh_create_handle("kwh_cw_create", config, o, out, [&](kwh_cw& s) {
    s.params = kwh_cw_parameters(config, o);
    s.propagator.reset(new CwPropagator(s.params));
  });
}

int kwh_cw_destroy(kwh_cw* s)
{
  KWH_TRY
  delete s;
  KWH_CATCH
}

int kwh_cw_run(kwh_cw* s, const float* a, const float* b, int parts)
{
  KWH_TRY
  if (!s || !a || !b) throw std::invalid_argument("kwh_cw_run: NULL argument");
  s->propagator->run(a, b, parts != 0);
  KWH_CATCH
}

int kwh_cw_get(kwh_cw* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !name || !dst) throw std::invalid_argument("kwh_cw_get: NULL argument");
  s->propagator->get(name, dst, n);
  KWH_CATCH
}

int kwh_cw_heat(kwh_cw* s, const float* q, float q_scalar, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !dst) throw std::invalid_argument("kwh_cw_heat: NULL argument");
  s->propagator->heat(q, q_scalar, dst, n);
  KWH_CATCH
}

int kwh_cw_propagate(kwh_cw* s)
{
  KWH_TRY
  if (!s) throw std::invalid_argument("kwh_cw_propagate: NULL propagator");
  s->propagator->propagate();
  KWH_CATCH
}

int kwh_cw_get_scalar(kwh_cw* s, const char* name, double* out)
{
  KWH_TRY
  if (!s || !name || !out) throw std::invalid_argument("kwh_cw_get_scalar: NULL argument");
  const std::string n(name);
  const CwParameters& p = s->propagator->parameters();
  if (n == "fused_pipeline") *out = s->propagator->usesFusedPipeline() ? 1.0 : 0.0;
  else if (n == "t") *out = p.t;
  else if (n == "Ex") *out = static_cast<double>(p.ex);
  else if (n == "Ey") *out = static_cast<double>(p.ey);
  else if (n == "Ez") *out = static_cast<double>(p.ez);
  else if (n == "runs") *out = static_cast<double>(s->propagator->runs());
  else if (n == "source_scale_re") *out = p.scaleRe;
  else if (n == "source_scale_im") *out = p.scaleIm;
  else throw std::invalid_argument(std::string("unknown scalar ") + name);
  KWH_CATCH
}

void* kwh_cw_context(kwh_cw* s) { return s ? s->propagator->context() : nullptr; }

// ---- angular-spectrum projector --------------------------------------------------------------------------------------
int kwh_angular_plan(const kwh_angular_config* config, const kwh_options* o, uint64_t out_expanded[2], uint64_t* out_chunk_planes,
                     int32_t* out_fast_path)
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_angular_plan: NULL argument");
  const AngularParameters p = kwh_angular_parameters(config, o);
  if (out_expanded) { out_expanded[0] = p.ex; out_expanded[1] = p.ey; }
  if (out_chunk_planes) *out_chunk_planes = p.chunkPlanes;
  if (out_fast_path) *out_fast_path = p.fastPath ? 1 : 0;
  KWH_CATCH
}

int kwh_angular_create(const kwh_angular_config* config, const kwh_options* o, kwh_angular** out)
{
  return kwh_create_handle("kwh_angular_create", config, o, out, [&](kwh_angular& s) {
    s.params = kwh_angular_parameters(config, o);
    s.projector.reset(new AngularSpectrum(s.params));
  });
}

int kwh_angular_destroy(kwh_angular* s)
{
  KWH_TRY
  delete s;
  KWH_CATCH
}

int kwh_angular_run(kwh_angular* s, const float* a, const float* b, int parts)
{
  KWH_TRY
  if (!s || !a || !b) throw std::invalid_argument("kwh_angular_run: NULL argument");
  s->projector->run(a, b, parts != 0);
  KWH_CATCH
}

int kwh_angular_get(kwh_angular* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !name || !dst) throw std::invalid_argument("kwh_angular_get: NULL argument");
  s->projector->get(name, dst, n);
  KWH_CATCH
}

int kwh_angular_heat(kwh_angular* s, const float* q, float q_scalar, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !dst) throw std::invalid_argument("kwh_angular_heat: NULL argument");
  s->projector->heat(q, q_scalar, dst, n);
  KWH_CATCH
}

int kwh_angular_project(kwh_angular* s)
{
  KWH_TRY
  if (!s) throw std::invalid_argument("kwh_angular_project: NULL projector");
  s->projector->project();
  KWH_CATCH
}

int kwh_angular_get_scalar(kwh_angular* s, const char* name, double* out)
{
  KWH_TRY
  if (!s || !name || !out) throw std::invalid_argument("kwh_angular_get_scalar: NULL argument");
  const std::string n(name);
  const AngularParameters& p = s->projector->parameters();
  if (n == "fused_pipeline") *out = s->projector->usesFusedPipeline() ? 1.0 : 0.0;
  else if (n == "Ex") *out = static_cast<double>(p.ex);
  else if (n == "Ey") *out = static_cast<double>(p.ey);
  else if (n == "chunk_planes") *out = static_cast<double>(p.chunkPlanes);
  else if (n == "planes") *out = static_cast<double>(p.planes);
  else if (n == "runs") *out = static_cast<double>(s->projector->runs());
  else throw std::invalid_argument(std::string("unknown scalar ") + name);
  KWH_CATCH
}

void* kwh_angular_context(kwh_angular* s) { return s ? s->projector->context() : nullptr; }

// ---- time-domain angular-spectrum projector --------------------------------------------------------------------------
int kwh_angular_time_plan(const kwh_angular_time_config* config, const kwh_options* o, uint64_t out_expanded[3], int32_t* out_fast_path)
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_angular_time_plan: NULL argument");
  const AngularTimeParameters p = kwh_angular_time_parameters(config, o);
  if (out_expanded) { out_expanded[0] = p.ex; out_expanded[1] = p.ey; out_expanded[2] = p.lt; }
  if (out_fast_path) *out_fast_path = p.fastPath ? 1 : 0;
  KWH_CATCH
}

int kwh_angular_time_create(const kwh_angular_time_config* config, const kwh_options* o, kwh_angular_time** out)
{
  return kwh_create_handle("kwh_angular_time_create", config, o, out, [&](kwh_angular_time& s) {
    s.params = kwh_angular_time_parameters(config, o);
    s.projector.reset(new AngularSpectrumTime(s.params));
  });
}

int kwh_angular_time_destroy(kwh_angular_time* s)
{
  KWH_TRY
  delete s;
  KWH_CATCH
}

int kwh_angular_time_set_input(kwh_angular_time* s, const float* p0)
{
  KWH_TRY
  if (!s || !p0) throw std::invalid_argument("kwh_angular_time_set_input: NULL argument");
  s->projector->setInput(p0);
  KWH_CATCH
}

int kwh_angular_time_run(kwh_angular_time* s, const float* p0)
{
  KWH_TRY
  if (!s || !p0) throw std::invalid_argument("kwh_angular_time_run: NULL argument");
  s->projector->run(p0);
  KWH_CATCH
}

int kwh_angular_time_get(kwh_angular_time* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !name || !dst) throw std::invalid_argument("kwh_angular_time_get: NULL argument");
  s->projector->get(name, dst, n);
  KWH_CATCH
}

int kwh_angular_time_series(kwh_angular_time* s, uint64_t j, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !dst) throw std::invalid_argument("kwh_angular_time_series: NULL argument");
  s->projector->series(j, dst, n);
  KWH_CATCH
}

int kwh_angular_time_project(kwh_angular_time* s)
{
  KWH_TRY
  if (!s) throw std::invalid_argument("kwh_angular_time_project: NULL projector");
  s->projector->project();
  KWH_CATCH
}

int kwh_angular_time_get_scalar(kwh_angular_time* s, const char* name, double* out)
{
  KWH_TRY
  if (!s || !name || !out) throw std::invalid_argument("kwh_angular_time_get_scalar: NULL argument");
  const std::string n(name);
  const AngularTimeParameters& p = s->projector->parameters();
  if (n == "fused_pipeline") *out = s->projector->usesFusedPipeline() ? 1.0 : 0.0;
  else if (n == "Ex") *out = static_cast<double>(p.ex);
  else if (n == "Ey") *out = static_cast<double>(p.ey);
  else if (n == "Lt") *out = static_cast<double>(p.lt);
  else if (n == "planes") *out = static_cast<double>(p.z.size());
  else if (n == "runs") *out = static_cast<double>(s->projector->runs());
  else throw std::invalid_argument(std::string("unknown scalar ") + name);
  KWH_CATCH
}

void* kwh_angular_time_context(kwh_angular_time* s) { return s ? s->projector->context() : nullptr; }

// ---- k-space plane reconstruction ------------------------------------------------------------------------------------
int kwh_plane_recon_plan(const kwh_plane_recon_config* config, const kwh_options* o, uint64_t out_expanded[3], int32_t* out_fast_path)
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_plane_recon_plan: NULL argument");
  const PlaneReconParameters p = kwh_plane_recon_parameters(config, o);
  if (out_expanded) { out_expanded[0] = p.ex; out_expanded[1] = p.ey; out_expanded[2] = p.lt; }
  if (out_fast_path) *out_fast_path = p.fastPath ? 1 : 0;
  KWH_CATCH
}

int kwh_plane_recon_create(const kwh_plane_recon_config* config, const kwh_options* o, kwh_plane_recon** out)
{
  return kwh_create_handle("kwh_plane_recon_create", config, o, out, [&](kwh_plane_recon& s) {
    s.params = kwh_plane_recon_parameters(config, o);
    s.recon.reset(new PlaneRecon(s.params));
  });
}

int kwh_plane_recon_destroy(kwh_plane_recon* s)
{
  KWH_TRY
  delete s;
  KWH_CATCH
}

int kwh_plane_recon_run(kwh_plane_recon* s, const float* p)
{
  KWH_TRY
  if (!s || !p) throw std::invalid_argument("kwh_plane_recon_run: NULL argument");
  s->recon->run(p);
  KWH_CATCH
}

int kwh_plane_recon_get(kwh_plane_recon* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !name || !dst) throw std::invalid_argument("kwh_plane_recon_get: NULL argument");
  s->recon->get(name, dst, n);
  KWH_CATCH
}

int kwh_plane_recon_get_scalar(kwh_plane_recon* s, const char* name, double* out)
{
  KWH_TRY
  if (!s || !name || !out) throw std::invalid_argument("kwh_plane_recon_get_scalar: NULL argument");
  const std::string n(name);
  const PlaneReconParameters& p = s->recon->parameters();
  if (n == "fused_pipeline") *out = s->recon->usesFusedPipeline() ? 1.0 : 0.0;
  else if (n == "Ex") *out = static_cast<double>(p.ex);
  else if (n == "Ey") *out = static_cast<double>(p.ey);
  else if (n == "Lt") *out = static_cast<double>(p.lt);
  else if (n == "planes") *out = static_cast<double>(p.planes);
  else if (n == "dz") *out = p.dz();
  else if (n == "runs") *out = static_cast<double>(s->recon->runs());
  else throw std::invalid_argument(std::string("unknown scalar ") + name);
  KWH_CATCH
}

void* kwh_plane_recon_context(kwh_plane_recon* s) { return s ? s->recon->context() : nullptr; }

// ---- batched k-space line reconstruction -----------------------------------------------------------------------------
int kwh_line_recon_plan(const kwh_line_recon_config* config, const kwh_options* o, uint64_t out_sizes[4], int32_t* out_fast_path)
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_line_recon_plan: NULL argument");
  const LineReconParameters p = kwh_line_recon_parameters(config, o);
  if (out_sizes) { out_sizes[0] = p.ey; out_sizes[1] = p.lt; out_sizes[2] = p.depth; out_sizes[3] = p.chunkFrames; }
  if (out_fast_path) *out_fast_path = p.fastPath ? 1 : 0;
  KWH_CATCH
}

int kwh_line_recon_create(const kwh_line_recon_config* config, const kwh_options* o, kwh_line_recon** out)
{
  return kwh_create_handle("kwh_line_recon_create", config, o, out, [&](kwh_line_recon& s) {
    s.params = kwh_line_recon_parameters(config, o);
    s.recon.reset(new LineRecon(s.params));
  });
}

int kwh_line_recon_destroy(kwh_line_recon* s)
{
  KWH_TRY
  delete s;
  KWH_CATCH
}

int kwh_line_recon_run(kwh_line_recon* s, const float* p)
{
  KWH_TRY
  if (!s || !p) throw std::invalid_argument("kwh_line_recon_run: NULL argument");
  s->recon->run(p);
  KWH_CATCH
}

int kwh_line_recon_get(kwh_line_recon* s, const char* name, float* dst, uint64_t n)
{
  KWH_TRY
  if (!s || !name || !dst) throw std::invalid_argument("kwh_line_recon_get: NULL argument");
  s->recon->get(name, dst, n);
  KWH_CATCH
}

int kwh_line_recon_get_scalar(kwh_line_recon* s, const char* name, double* out)
{
  KWH_TRY
  if (!s || !name || !out) throw std::invalid_argument("kwh_line_recon_get_scalar: NULL argument");
  const std::string n(name);
  const LineReconParameters& p = s->recon->parameters();
  if (n == "fused_pipeline") *out = s->recon->usesFusedPipeline() ? 1.0 : 0.0;
  else if (n == "Ey") *out = static_cast<double>(p.ey);
  else if (n == "Lt") *out = static_cast<double>(p.lt);
  else if (n == "depth") *out = static_cast<double>(p.depth);
  else if (n == "frames") *out = static_cast<double>(p.frames);
  else if (n == "chunk_frames") *out = static_cast<double>(p.chunkFrames);
  else if (n == "dx") *out = p.dx();
  else if (n == "runs") *out = static_cast<double>(s->recon->runs());
  else throw std::invalid_argument(std::string("unknown scalar ") + name);
  KWH_CATCH
}

void* kwh_line_recon_context(kwh_line_recon* s) { return s ? s->recon->context() : nullptr; }

// ---- exact k-space propagator ------------------------------------------------------------------------------------------
int kwh_second_order_plan(const kwh_second_order_config* config, const kwh_options* o, uint64_t out_expanded[3], int32_t* out_fast_path)
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_second_order_plan: NULL argument");
  const SecondOrderParameters p = kwh_second_order_parameters(config, o);
  if (out_expanded) { out_expanded[0] = p.ex; out_expanded[1] = p.ey; out_expanded[2] = p.ez; }
  if (out_fast_path) *out_fast_path = p.fastPath ? 1 : 0;
  KWH_CATCH
}

int kwh_second_order_create(const kwh_second_order_config* config, const kwh_options* o, kwh_second_order** out)
{
  return kwh_create_handle("kwh_second_order_create", config, o, out, [&](kwh_second_order& s) {
    s.params = kwh_second_order_parameters(config, o);
    s.propagator.reset(new SecondOrder(s.params));
  });
}

int kwh_second_order_destroy(kwh_second_order* s) { return kwh_propagator_destroy(s); }

int kwh_second_order_set_p0(kwh_second_order* s, const float* p0)
{
  return kwh_propagator_set_p0("kwh_second_order_set_p0", s, p0);
}

int kwh_second_order_set_dp0dt(kwh_second_order* s, const float* dp0dt)
{
  return kwh_propagator_set_dp0dt("kwh_second_order_set_dp0dt", s, dp0dt);
}

int kwh_second_order_field(kwh_second_order* s, double t, float* dst)
{
  return kwh_propagator_field("kwh_second_order_field", s, t, dst);
}

int kwh_second_order_run(kwh_second_order* s, const double* times, uint64_t n_times)
{
  return kwh_propagator_run("kwh_second_order_run", s, times, n_times);
}

int kwh_second_order_get(kwh_second_order* s, const char* name, float* dst, uint64_t n)
{
  return kwh_propagator_get("kwh_second_order_get", s, name, dst, n);
}

int kwh_second_order_get_scalar(kwh_second_order* s, const char* name, double* out)
{
  KWH_TRY
  if (!s || !name || !out) throw std::invalid_argument("kwh_second_order_get_scalar: NULL argument");
  const std::string n(name);
  const SecondOrderParameters& p = s->propagator->parameters();
  if (n == "fused_pipeline") *out = s->propagator->usesFusedPipeline() ? 1.0 : 0.0;
  else if (n == "Ex") *out = static_cast<double>(p.ex);
  else if (n == "Ey") *out = static_cast<double>(p.ey);
  else if (n == "Ez") *out = static_cast<double>(p.ez);
  else if (n == "t_free") *out = p.tFree;
  else if (n == "runs") *out = static_cast<double>(s->propagator->runs());
  else if (n == "has_dp0dt") *out = s->propagator->hasDp0dt() ? 1.0 : 0.0;
  else if (n == "plane") *out = static_cast<double>(s->propagator->plane());
  else if (n == "plane_chunk_times") *out = static_cast<double>(s->propagator->planeChunkTimes());
  else throw std::invalid_argument(std::string("unknown scalar ") + name);
  KWH_CATCH
}

void* kwh_second_order_context(kwh_second_order* s) { return kwh_propagator_context(s); }

int kwh_second_order_plane_plan(const kwh_second_order_config* config, const kwh_options* o, int64_t plane, uint64_t chunk_times,
                                uint64_t n_times, uint64_t out[3])
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_second_order_plane_plan: NULL argument");
  const SecondOrderParameters p = kwh_second_order_parameters(config, o);
  p.checkPlane(plane);
  const size_t chunk = p.planeChunkTimes(chunk_times);
  const size_t passes = SecondOrderParameters::planeChunks(n_times, chunk).size();
  if (out) { out[0] = chunk; out[1] = passes; out[2] = p.planeElems(); }
  KWH_CATCH
}

int kwh_second_order_set_plane(kwh_second_order* s, int64_t plane)
{
  KWH_TRY
  if (!s) throw std::invalid_argument("kwh_second_order_set_plane: NULL propagator");
  s->propagator->setPlane(plane);
  KWH_CATCH
}

int kwh_second_order_set_plane_chunk_times(kwh_second_order* s, uint64_t times)
{
  KWH_TRY
  if (!s) throw std::invalid_argument("kwh_second_order_set_plane_chunk_times: NULL propagator");
  s->propagator->setPlaneChunkTimes(times);
  KWH_CATCH
}

int kwh_second_order_plane_record(kwh_second_order* s, const double* times, uint64_t n_times, float* dst)
{
  KWH_TRY
  if (!s || (!times && n_times != 0)) throw std::invalid_argument("kwh_second_order_plane_record: NULL argument");
  s->propagator->planeRecord(times, n_times, dst);
  KWH_CATCH
}

// ---- batched 2-D exact k-space propagator -----------------------------------------------------------------------------
int kwh_second_order_frames_plan(const kwh_second_order_frames_config* config, const kwh_options* o, uint64_t out_expanded[2],
                                 int32_t* out_fast_path)
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_second_order_frames_plan: NULL argument");
  const SecondOrderFramesParameters p = kwh_second_order_frames_parameters(config, o);
  if (out_expanded) { out_expanded[0] = p.ex; out_expanded[1] = p.ey; }
  if (out_fast_path) *out_fast_path = p.fastPath ? 1 : 0;
  KWH_CATCH
}

int kwh_second_order_frames_create(const kwh_second_order_frames_config* config, const kwh_options* o, kwh_second_order_frames** out)
{
  return kwh_create_handle("kwh_second_order_frames_create", config, o, out, [&](kwh_second_order_frames& s) {
    s.params = kwh_second_order_frames_parameters(config, o);
    s.propagator.reset(new SecondOrderFrames(s.params));
  });
}

int kwh_second_order_frames_destroy(kwh_second_order_frames* s) { return kwh_propagator_destroy(s); }

int kwh_second_order_frames_set_p0(kwh_second_order_frames* s, const float* p0)
{
  return kwh_propagator_set_p0("kwh_second_order_frames_set_p0", s, p0);
}

int kwh_second_order_frames_set_dp0dt(kwh_second_order_frames* s, const float* dp0dt)
{
  return kwh_propagator_set_dp0dt("kwh_second_order_frames_set_dp0dt", s, dp0dt);
}

int kwh_second_order_frames_field(kwh_second_order_frames* s, double t, float* dst)
{
  return kwh_propagator_field("kwh_second_order_frames_field", s, t, dst);
}

int kwh_second_order_frames_run(kwh_second_order_frames* s, const double* times, uint64_t n_times)
{
  return kwh_propagator_run("kwh_second_order_frames_run", s, times, n_times);
}

int kwh_second_order_frames_get(kwh_second_order_frames* s, const char* name, float* dst, uint64_t n)
{
  return kwh_propagator_get("kwh_second_order_frames_get", s, name, dst, n);
}

int kwh_second_order_frames_get_scalar(kwh_second_order_frames* s, const char* name, double* out)
{
  KWH_TRY
  if (!s || !name || !out) throw std::invalid_argument("kwh_second_order_frames_get_scalar: NULL argument");
  const std::string n(name);
  const SecondOrderFramesParameters& p = s->propagator->parameters();
  if (n == "fused_pipeline") *out = s->propagator->usesFusedPipeline() ? 1.0 : 0.0;
  else if (n == "Ex") *out = static_cast<double>(p.ex);
  else if (n == "Ey") *out = static_cast<double>(p.ey);
  else if (n == "frames") *out = static_cast<double>(p.frames);
  else if (n == "t_free") *out = p.tFree;
  else if (n == "runs") *out = static_cast<double>(s->propagator->runs());
  else if (n == "has_dp0dt") *out = s->propagator->hasDp0dt() ? 1.0 : 0.0;
  else if (n == "line_row") *out = static_cast<double>(s->propagator->lineRow());
  else if (n == "line_chunk_times") *out = static_cast<double>(s->propagator->lineChunkTimes());
  else throw std::invalid_argument(std::string("unknown scalar ") + name);
  KWH_CATCH
}

void* kwh_second_order_frames_context(kwh_second_order_frames* s) { return kwh_propagator_context(s); }

int kwh_second_order_frames_line_plan(const kwh_second_order_frames_config* config, const kwh_options* o, int64_t row,
                                      uint64_t chunk_times, uint64_t n_times, uint64_t out[3])
{
  KWH_TRY
  if (!config || !o) throw std::invalid_argument("kwh_second_order_frames_line_plan: NULL argument");
  const SecondOrderFramesParameters p = kwh_second_order_frames_parameters(config, o);
  p.checkLineRow(row);
  const size_t chunk = p.lineChunkTimes(chunk_times);
  const size_t passes = SecondOrderFramesParameters::lineChunks(n_times, chunk).size();
  if (out) { out[0] = chunk; out[1] = passes; out[2] = p.lineElems(); }
  KWH_CATCH
}

int kwh_second_order_frames_set_line_row(kwh_second_order_frames* s, int64_t row)
{
  KWH_TRY
  if (!s) throw std::invalid_argument("kwh_second_order_frames_set_line_row: NULL propagator");
  s->propagator->setLineRow(row);
  KWH_CATCH
}

int kwh_second_order_frames_set_line_chunk_times(kwh_second_order_frames* s, uint64_t times)
{
  KWH_TRY
  if (!s) throw std::invalid_argument("kwh_second_order_frames_set_line_chunk_times: NULL propagator");
  s->propagator->setLineChunkTimes(times);
  KWH_CATCH
}

int kwh_second_order_frames_line_record(kwh_second_order_frames* s, const double* times, uint64_t n_times, float* dst)
{
  KWH_TRY
  if (!s || (!times && n_times != 0)) throw std::invalid_argument("kwh_second_order_frames_line_record: NULL argument");
  s->propagator->lineRecord(times, n_times, dst);
  KWH_CATCH
}
}
