/*
 * kwave_hip.h — C-ABI of the MI355X (gfx950) device layer for the k-space first-order acoustic step.
 *
 * This is the drop-in boundary for the per-time-step hot path of klepo/k-Wave-Fluid-CUDA.  The reference
 * has no FFI layer; its device-operator boundary is four C++ surfaces:
 *   (1) namespace SolverCudaKernels            KSpaceSolver/SolverCudaKernels.cuh:52-500
 *   (2) class CufftComplexMatrix (plans+exec)   MatrixClasses/CufftComplexMatrix.h:73-238
 *   (3) namespace OutputStreamsCudaKernels     OutputStreams/OutputStreamsCudaKernels.cuh:47-106
 *   (4) CudaParameters / CudaDeviceConstants   Parameters/CudaParameters.h:140-146, CudaDeviceConstants.cuh:44-116
 * plus the memory verbs of the matrix classes   MatrixClasses/BaseFloatMatrix.h:85-131.
 * Every entry point below names the reference interface (file:line, relative to the reference root) it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; device pointers are raw HIP device addresses.
 *   - every function returns kw_status (0 = OK).  The reference's convention (void + C++ exception,
 *     Logger/Logger.h:194-216) is restored by the C++ host shims in k-wave-fluid-cuda_amd/host/, which turn
 *     a non-zero status into std::runtime_error(kw_last_error()).
 *   - all launches are asynchronous on the context's stream (reference: default stream, in order).
 *   - data layout: fp32, row-major with x fastest; complex = interleaved (re,im); indices = uint64, 0-based
 *     (KSpaceFirstOrderSolver.cpp:2916-2920, ComplexMatrix.cpp:124-135, IndexMatrix.cpp:161-168).
 *   - a NULL pointer for an optional per-voxel medium array selects the scalar from kw_constants, exactly
 *     like the reference's boolean template flags (e.g. SolverCudaKernels.cu:1401-1440).
 */
#ifndef KWAVE_HIP_H
#define KWAVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KW_API __attribute__((visibility("default")))

typedef struct kw_ctx kw_ctx;

typedef enum kw_status
{
  KW_OK            = 0,
  KW_ERR_INVALID   = 1, /* bad argument (NULL pointer, zero size, unsupported flag) */
  KW_ERR_HIP       = 2, /* HIP runtime error ("GPU error: ..." of Logger/ErrorMessages.h:331) */
  KW_ERR_FFT       = 3, /* rocFFT error (CufftComplexMatrix.cpp:63-72,706-720) */
  KW_ERR_ALLOC     = 4, /* out of memory (std::bad_alloc of BaseFloatMatrix.cpp:140-143) */
  KW_ERR_STATE     = 5, /* call order violated (constants / plans not set) */
  KW_ERR_NO_DEVICE = 6, /* no usable gfx950 device (CudaParameters.cpp:81-177) */
  KW_ERR_COMM      = 7  /* multi-GPU exchange failed: RCCL error, or a caller-supplied exchange callback returned non-zero */
} kw_status;

/* Parameters/Parameters.h:60-94 */
typedef enum kw_source_mode
{
  KW_SRC_DIRICHLET              = 0,
  KW_SRC_ADDITIVE_NO_CORRECTION = 1,
  KW_SRC_ADDITIVE               = 2
} kw_source_mode;

/* OutputStreams/BaseOutputStream.h ReduceOperator (device-side subset used by the samplers) */
typedef enum kw_reduce_op
{
  KW_OP_NONE = 0, /* buf[i]  = src      */
  KW_OP_RMS  = 1, /* buf[i] += src*src  */
  KW_OP_MAX  = 2, /* buf[i]  = max(buf[i], src) */
  KW_OP_MIN  = 3  /* buf[i]  = min(buf[i], src) */
} kw_reduce_op;

/* Mirror of struct CudaDeviceConstants (Parameters/CudaDeviceConstants.cuh:44-116), filled the way
 * CudaParameters::setUpDeviceConstants does (Parameters/CudaParameters.cpp:238-288).  Passed to kernels as a
 * by-value argument (SGPR-resident) instead of a __constant__ symbol. */
typedef struct kw_constants
{
  uint32_t nx, ny, nz, n_elements;
  uint32_t nx_complex, ny_complex, nz_complex, n_elements_complex;
  float    fft_divider, fft_divider_x, fft_divider_y, fft_divider_z;
  float    dt, dt_by_2, c2;
  float    rho0, dt_rho0, dt_rho0_sgx, dt_rho0_sgy, dt_rho0_sgz;
  float    b_on_a, absorb_tau, absorb_eta;
  uint32_t velocity_source_size, velocity_source_mode, velocity_source_many;
  uint32_t pressure_source_size, pressure_source_mode, pressure_source_many;
} kw_constants;

typedef struct kw_device_info
{
  char     name[128];
  char     arch[64];
  int32_t  device_id;
  int32_t  compute_units;
  int32_t  wavefront_size;
  int32_t  clock_mhz;
  uint64_t total_mem;
  uint64_t free_mem;
  uint64_t lds_per_cu;
  uint64_t l2_bytes;
} kw_device_info;

/* ------------------------------------------------------------------------------------------------------------------
 * Context / device  — replaces CudaParameters::selectDevice (CudaParameters.cpp:81-177)
 * ---------------------------------------------------------------------------------------------------------------- */
/* device_id < 0: first free device (reference: -g not given).  Creates the context's stream. */
KW_API kw_status   kw_init(int device_id, kw_ctx** out_ctx);
KW_API kw_status   kw_destroy(kw_ctx* ctx);
/* message of the last failing call on this thread (ctx may be NULL) */
KW_API const char* kw_last_error(void);
KW_API kw_status   kw_device_info_get(kw_ctx* ctx, kw_device_info* out);
/* use an externally owned hipStream_t (e.g. torch's current stream); NULL restores the context's own stream */
KW_API kw_status   kw_set_stream(kw_ctx* ctx, void* hip_stream);
KW_API void*       kw_get_stream(kw_ctx* ctx);
KW_API kw_status   kw_sync(kw_ctx* ctx);
/* Schedule parameters of the fused pipeline and of the multi-GPU exchange — every switch the library has, in one
 * documented place (the library reads no environment variable).  kw_get_tuning returns the current values (the defaults
 * after kw_init); kw_set_tuning takes effect at the next kw_fused_create.  struct_bytes = sizeof(kw_tuning) of the
 * caller, so that the struct can grow: fields beyond it keep their defaults. */
typedef struct kw_tuning
{
  uint32_t struct_bytes;
  int32_t  side_array;          /* 1: x-Nyquist bins of an even-Nx grid live in a compact side array behind rows of
                                   exactly Nx/2 bins; 0: in the rows, padded to whole 16-bin tiles */
  int32_t  tail_chunks;         /* single GPU: the plane-local tail of a stage (y-inverse, x-inverse + epilogue, chained
                                   x / y forward) runs per chunk of planes (a chunk's spectra stay in the Infinity
                                   Cache between those kernels); 0 or 1 = whole grid (the default: measured within
                                   +-2 % at 320^3 ... 512^3, profiles/r03_tail_chunks.txt), n = that many chunks */
  int32_t  split512;            /* 1: 512-point y / z lines as 2 x 256-point transforms; 0: 16 x 32-point kernels */
  int32_t  slab_pipeline;       /* 1: pipelined slab schedule (third buffer set, forward transposes started by the
                                   producing stage); 0: whole-array schedule */
  int32_t  slab_chunks;         /* plane chunks per array of the pipelined slab tail (1..4) */
  int32_t  slab_batch;          /* all arrays of a stage in ONE exchange per direction: -1 automatic (below 4 MB per
                                   peer and array), 0 never, 1 always */
  int32_t  p2p_blocks_per_peer; /* P2P transport: workgroups that store to one peer (1..8) */
  float    p2p_timeout_s;       /* P2P transport: a rank that waits longer than this for a peer gives up (KW_ERR_COMM) */
  int32_t  plane_kernels;       /* 1: grids with square planes of 32 / 64 points run each stage's tail (y-inverse,
                                   x-inverse + epilogue, chained x / y forward) as ONE launch whose blocks take whole
                                   z-planes; 0: the three-launch form of the larger grids */
  uint64_t offgrid_scratch_bytes; /* kw_offgrid_build: device bytes the element boxes of one round may take when the call
                                   itself names none (20 bytes per box cell; default, and what 0 selects: 256 MiB) */
} kw_tuning;
KW_API kw_status   kw_get_tuning(kw_ctx* ctx, kw_tuning* out);
KW_API kw_status   kw_set_tuning(kw_ctx* ctx, const kw_tuning* tuning);
/* Launch-bound loops (small grids): record the launches of a fixed sequence of kw_* calls once, replay it per step.
 * kw_graph_begin puts the context's stream into capture mode (nothing executes until the graph is launched);
 * every kw_* call in between must be a pure kernel-launch call (no allocation, copy or synchronisation). */
typedef struct kw_graph kw_graph;
KW_API kw_status   kw_graph_begin(kw_ctx* ctx);
KW_API kw_status   kw_graph_end(kw_ctx* ctx, kw_graph** out);
KW_API kw_status   kw_graph_launch(kw_ctx* ctx, kw_graph* g);
KW_API kw_status   kw_graph_destroy(kw_ctx* ctx, kw_graph* g);
/* Measured device-copy bandwidth: a float4 copy kernel over two freshly allocated buffers of `bytes` each (choose
 * them well above the 256 MB Infinity Cache), reps timed passes after one untimed; GB/s counts read + write.  bench.py
 * reports it beside the spec peak. */
KW_API kw_status   kw_measure_copy_bandwidth(kw_ctx* ctx, size_t bytes, int reps, double* out_gbs);
/* HIP events on the context's stream (bench.py times kernels with these) */
KW_API kw_status   kw_event_create(kw_ctx* ctx, void** out_event);
KW_API kw_status   kw_event_record(kw_ctx* ctx, void* event);
KW_API kw_status   kw_event_synchronize(kw_ctx* ctx, void* event);
KW_API kw_status   kw_event_elapsed_ms(kw_ctx* ctx, void* start, void* stop, float* out_ms);
KW_API kw_status   kw_event_destroy(kw_ctx* ctx, void* event);

/* Per-entry-point device timing (HIP events around every kw_* compute call while enabled); used by bench.py to
 * report kernel durations live.  The reference has only host wall-clock timers (Utils/TimeMeasure.h:90-123). */
typedef struct kw_profile_entry
{
  char     name[64];
  uint64_t calls;
  double   total_ms;
} kw_profile_entry;
KW_API kw_status kw_profile_enable(kw_ctx* ctx, int on);
KW_API int       kw_profile_enabled(kw_ctx* ctx); /* 1 while per-call timing is on (recorded graphs would bypass it) */
/* synchronises, aggregates by entry-point name, clears the recorded events; *n_out = number of entries written */
KW_API kw_status kw_profile_collect(kw_ctx* ctx, kw_profile_entry* out, size_t capacity, size_t* n_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Memory verbs — replace BaseFloatMatrix/BaseIndexMatrix allocate/copyToDevice/copyFromDevice/zeroDeviceMatrix
 * (MatrixClasses/BaseFloatMatrix.cpp:77-80,124-168; BaseIndexMatrix.cpp)
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_malloc(kw_ctx* ctx, size_t bytes, void** out_dptr);
KW_API kw_status kw_free(kw_ctx* ctx, void* dptr);
KW_API kw_status kw_memcpy_h2d(kw_ctx* ctx, void* dst, const void* src, size_t bytes);
KW_API kw_status kw_memcpy_d2h(kw_ctx* ctx, void* dst, const void* src, size_t bytes);
KW_API kw_status kw_memcpy_d2d(kw_ctx* ctx, void* dst, const void* src, size_t bytes);
KW_API kw_status kw_memcpy_d2h_async(kw_ctx* ctx, void* dst, const void* src, size_t bytes);
KW_API kw_status kw_memset(kw_ctx* ctx, void* dptr, int value, size_t bytes);
/* device -> pinned host on the context's COPY stream, ordered after everything enqueued so far on the compute stream;
 * `event` (kw_event_create) is recorded when the copy has landed.  The compute stream is not blocked: this is how raw
 * sensor series leave the device while the next step computes (reference: zero-copy mapped buffer + cudaEvent,
 * BaseOutputStream.cpp:369-388, IndexOutputStream.cpp:263,354). */
KW_API kw_status kw_memcpy_d2h_overlapped(kw_ctx* ctx, void* dst, const void* src, size_t bytes, void* event);
/* pinned host memory (reference: cudaHostRegister / mapped buffers, BaseOutputStream.cpp:369-388) */
KW_API kw_status kw_host_alloc(kw_ctx* ctx, size_t bytes, void** out_hptr);
KW_API kw_status kw_host_free(kw_ctx* ctx, void* hptr);

/* ------------------------------------------------------------------------------------------------------------------
 * Device constants — replaces CudaDeviceConstants::uploadDeviceConstants (CudaDeviceConstants.cu:58-60)
 * and CudaParameters::setKernelConfiguration (CudaParameters.cpp:195-232; geometry is derived internally
 * from the CU count instead of SM count x 8).
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_set_constants(kw_ctx* ctx, const kw_constants* constants);
KW_API kw_status kw_get_constants(kw_ctx* ctx, kw_constants* out);

/* ------------------------------------------------------------------------------------------------------------------
 * FFT — replaces CufftComplexMatrix static plan factory + compute* members
 * (MatrixClasses/CufftComplexMatrix.cpp:82-130 plans ND, :144-426 plans 1D, :432-502 destroy, :508-534 exec ND,
 *  :540-692 exec 1D).  Unnormalised, forward sign -i, out-of-place, nx/2+1 bins along x.  Dimensions come from
 * kw_set_constants.  C2R may overwrite its input (as cuFFT may).
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_fft_create_plans_3d(kw_ctx* ctx);                         /* createR2CFftPlanND + createC2RFftPlanND */
KW_API kw_status kw_fft_create_plans_1d(kw_ctx* ctx, int axis);               /* create{R2C,C2R}FftPlan1D{X,Y,Z} */
KW_API kw_status kw_fft_destroy_plans(kw_ctx* ctx);                           /* destroyAllPlansAndStaticData */
KW_API kw_status kw_fft_r2c_3d(kw_ctx* ctx, const float* in, float* out);     /* computeR2CFftND */
KW_API kw_status kw_fft_c2r_3d(kw_ctx* ctx, float* in, float* out);           /* computeC2RFftND */
/* 1-D transforms along axis (0=x,1=y,2=z); the half-spectrum keeps the [z][y][x] order with the transformed
 * axis shortened to n/2+1 (the reference's transposed/padded layout for Y and Z is an implementation detail) */
KW_API kw_status kw_fft_r2c_1d(kw_ctx* ctx, int axis, const float* in, float* out);  /* computeR2CFft1D{X,Y,Z} */
KW_API kw_status kw_fft_c2r_1d(kw_ctx* ctx, int axis, float* in, float* out);        /* computeC2RFft1D{X,Y,Z} */

/* ------------------------------------------------------------------------------------------------------------------
 * Solver kernels — one entry per SolverCudaKernels wrapper (3-D, uniform grid)
 * ---------------------------------------------------------------------------------------------------------------- */
/* computeVelocityHeterogeneous (.cuh:92, .cu:184-243) when dt_rho0_sg* != NULL,
 * computeVelocityHomogeneousUniform (.cuh:107, .cu:278-335) when all three are NULL */
KW_API kw_status kw_compute_velocity(kw_ctx* ctx, float* ux_sgx, float* uy_sgy, float* uz_sgz, const float* ifft_x,
                                     const float* ifft_y, const float* ifft_z, const float* dt_rho0_sgx,
                                     const float* dt_rho0_sgy, const float* dt_rho0_sgz, const float* pml_x_sgx,
                                     const float* pml_y_sgy, const float* pml_z_sgz);
/* addTransducerSource (.cuh:132, .cu:463-497) */
KW_API kw_status kw_add_transducer_source(kw_ctx* ctx, float* ux_sgx, const uint64_t* velocity_source_index,
                                          const float* transducer_source_input, const uint64_t* delay_mask,
                                          uint64_t time_index);
/* addVelocitySource (.cuh:141-143, .cu:504-555) */
KW_API kw_status kw_add_velocity_source(kw_ctx* ctx, float* velocity, const float* velocity_source_input,
                                        const uint64_t* velocity_source_index, uint64_t time_index);
/* addPressureSource (.cuh:152, .cu:570-660) */
KW_API kw_status kw_add_pressure_source(kw_ctx* ctx, float* rho_x, float* rho_y, float* rho_z,
                                        const float* pressure_source_input, const uint64_t* pressure_source_index,
                                        uint64_t time_index);
/* insertSourceIntoScalingMatrix (.cuh:163-166, .cu:679-733) */
KW_API kw_status kw_insert_source_into_scaling_matrix(kw_ctx* ctx, float* scaled_source, const float* source_input,
                                                      const uint64_t* source_index, uint64_t source_size,
                                                      int many_flag, uint64_t time_index);
/* computeSourceGradient (.cuh:173-174, .cu:740-758) */
KW_API kw_status kw_compute_source_gradient(kw_ctx* ctx, float* source_spectrum, const float* source_kappa);
/* addVelocityScaledSource (.cuh:181-182, .cu:765-786) */
KW_API kw_status kw_add_velocity_scaled_source(kw_ctx* ctx, float* velocity, const float* scaled_source);
/* addPressureScaledSource (.cuh:191-192, .cu:795-826) */
KW_API kw_status kw_add_pressure_scaled_source(kw_ctx* ctx, float* rho_x, float* rho_y, float* rho_z,
                                               const float* scaled_source);
/* addInitialPressureSource (.cuh:208, .cu:864-927); c2 == NULL -> scalar */
KW_API kw_status kw_add_initial_pressure_source(kw_ctx* ctx, float* p, float* rho_x, float* rho_y, float* rho_z,
                                                const float* p0_source_input, const float* c2);
/* computeInitialVelocityHeterogeneous / HomogeneousUniform (.cuh:222,236, .cu:949-1040) */
KW_API kw_status kw_compute_initial_velocity(kw_ctx* ctx, float* ux_sgx, float* uy_sgy, float* uz_sgz,
                                             const float* dt_rho0_sgx, const float* dt_rho0_sgy,
                                             const float* dt_rho0_sgz);
/* computePressureGradient (.cuh:267, .cu:1139-1185) */
KW_API kw_status kw_compute_pressure_gradient(kw_ctx* ctx, float* fft_x, float* fft_y, float* fft_z,
                                              const float* kappa, const float* ddx_k_shift_pos,
                                              const float* ddy_k_shift_pos, const float* ddz_k_shift_pos);
/* computeVelocityGradient (.cuh:281, .cu:1210-1268) */
KW_API kw_status kw_compute_velocity_gradient(kw_ctx* ctx, float* fft_x, float* fft_y, float* fft_z,
                                              const float* kappa, const float* ddx_k_shift_neg,
                                              const float* ddy_k_shift_neg, const float* ddz_k_shift_neg);
/* computeVelocityGradientShiftNonuniform (.cuh:293, .cu:1285-1320): du?d? *= d?ud?n[coord] on a non-uniform grid;
 * KW_ERR_INVALID when Ny > 65535 */
KW_API kw_status kw_compute_velocity_gradient_shift_nonuniform(kw_ctx* ctx, float* duxdx, float* duydy, float* duzdz,
                                                               const float* dxudxn, const float* dyudyn,
                                                               const float* dzudzn);
/* computeDensityNonlinear (.cuh:306, .cu:1358-1440) / computeDensityLinear (.cuh:320, .cu:1470-1545); rho0 NULL -> scalar */
KW_API kw_status kw_compute_density_nonlinear(kw_ctx* ctx, float* rho_x, float* rho_y, float* rho_z,
                                              const float* pml_x, const float* pml_y, const float* pml_z,
                                              const float* duxdx, const float* duydy, const float* duzdz,
                                              const float* rho0);
KW_API kw_status kw_compute_density_linear(kw_ctx* ctx, float* rho_x, float* rho_y, float* rho_z, const float* pml_x,
                                           const float* pml_y, const float* pml_z, const float* duxdx,
                                           const float* duydy, const float* duzdz, const float* rho0);
/* computePressureTermsNonlinear (.cuh:335-338, .cu:1577-1695); b_on_a / rho0 NULL -> scalar */
KW_API kw_status kw_compute_pressure_terms_nonlinear(kw_ctx* ctx, float* density_sum, float* nonlinear_term,
                                                     float* velocity_gradient_sum, const float* rho_x,
                                                     const float* rho_y, const float* rho_z, const float* duxdx,
                                                     const float* duydy, const float* duzdz, const float* b_on_a,
                                                     const float* rho0);
/* computePressureTermsLinear (.cuh:348-350, .cu:1724-1790) */
KW_API kw_status kw_compute_pressure_terms_linear(kw_ctx* ctx, float* density_sum, float* velocity_gradient_sum,
                                                  const float* rho_x, const float* rho_y, const float* rho_z,
                                                  const float* duxdx, const float* duydy, const float* duzdz,
                                                  const float* rho0);
/* computeAbsorbtionTerm (.cuh:365-368, .cu:1812-1840) */
KW_API kw_status kw_compute_absorbtion_term(kw_ctx* ctx, float* fft_part1, float* fft_part2,
                                            const float* absorb_nabla1, const float* absorb_nabla2);
/* sumPressureTermsNonlinear (.cuh:388-391, .cu:1865-1945); c2 / absorb_tau+absorb_eta NULL -> scalars */
KW_API kw_status kw_sum_pressure_terms_nonlinear(kw_ctx* ctx, float* p, const float* nonlinear_term,
                                                 const float* absorb_tau_term, const float* absorb_eta_term,
                                                 const float* c2, const float* absorb_tau, const float* absorb_eta);
/* sumPressureTermsLinear (.cuh:411-414, .cu:1966-2045) */
KW_API kw_status kw_sum_pressure_terms_linear(kw_ctx* ctx, float* p, const float* absorb_tau_term,
                                              const float* absorb_eta_term, const float* density_sum, const float* c2,
                                              const float* absorb_tau, const float* absorb_eta);
/* One-term power-law absorption (new with this build; k-Wave's medium.alpha_mode = 'no_dispersion', absorbing_flag = 3:
 * eta = 0; = 'no_absorption', absorbing_flag = 4: tau = 0): the two-term sum above with the absent product removed, every
 * fp32 product and sum rounded on its own (no fma contraction), in this order:
 *   which == 0 (no_dispersion):  p = c2 * (first + (fft_divider * (term * coef)))   coef = absorb_tau
 *   which == 1 (no_absorption):  p = c2 * (first - (fft_divider * (term * coef)))   coef = absorb_eta
 * For finite inputs that is the two-term sum with the other coefficient exactly 0.  term = the inverse transform of
 * nabla1 * F{rho0 * sum du} (which == 0) or of nabla2 * F{sum rho} (which == 1); first = the nonlinear term or the density
 * sum.  c2 / coef NULL -> the scalars of kw_constants (coef: absorb_tau or absorb_eta by `which`).
 * kw_fused_absorption_pressure_one evaluates the same expression (same bits) in its x-inverse epilogue. */
KW_API kw_status kw_compute_absorbtion_term_one(kw_ctx* ctx, float* fft_part, const float* absorb_nabla);
KW_API kw_status kw_sum_pressure_terms_one_nonlinear(kw_ctx* ctx, float* p, const float* nonlinear_term,
                                                     const float* absorb_term, const float* c2, const float* coef,
                                                     int which);
KW_API kw_status kw_sum_pressure_terms_one_linear(kw_ctx* ctx, float* p, const float* absorb_term,
                                                  const float* density_sum, const float* c2, const float* coef, int which);
/* sumPressureNonlinearLossless (.cuh:429, .cu:2067-2200) */
KW_API kw_status kw_sum_pressure_nonlinear_lossless(kw_ctx* ctx, float* p, const float* rho_x, const float* rho_y,
                                                    const float* rho_z, const float* c2, const float* b_on_a,
                                                    const float* rho0);
/* sumPressureLinearLossless (.cuh:444, .cu:2224-2275) */
KW_API kw_status kw_sum_pressure_linear_lossless(kw_ctx* ctx, float* p, const float* rho_x, const float* rho_y,
                                                 const float* rho_z, const float* c2);
/* Stokes absorption (new with this build; k-Wave's medium.alpha_mode = 'stokes', absorbing_flag = 2): for alpha_power == 2
 * the power-law operators degenerate (nabla1 = |k|^0 = 1, eta ~ tan(pi) = 0) and the absorbing equation of state is
 * element-wise.  With rhoSum = (rho_x + rho_y) + rho_z and duSum = (duxdx + duydy) + duzdz, every fp32 product and sum
 * rounded on its own (no fma contraction), in this order:
 *   absorb = tau * (rho0 * duSum)
 *   first  = rhoSum                                               (linear)
 *          = (((b_on_a * rhoSum) * rhoSum) / (2 * rho0)) + rhoSum   (nonlinear: the nonlinear term of .cu:1588-1601)
 *   p      = c2 * (first + absorb)
 * tau = absorb_tau of the power law at alpha_power = 2 (-2 * alpha_Np * c0).  c2 / b_on_a / rho0 / tau NULL -> scalars.
 * kw_fused_density(terms == 4) evaluates the same expression (same bits) inside the density epilogue. */
KW_API kw_status kw_sum_pressure_stokes_nonlinear(kw_ctx* ctx, float* p, const float* rho_x, const float* rho_y,
                                                  const float* rho_z, const float* duxdx, const float* duydy,
                                                  const float* duzdz, const float* c2, const float* b_on_a,
                                                  const float* rho0, const float* absorb_tau);
KW_API kw_status kw_sum_pressure_stokes_linear(kw_ctx* ctx, float* p, const float* rho_x, const float* rho_y,
                                               const float* rho_z, const float* duxdx, const float* duydy,
                                               const float* duzdz, const float* c2, const float* rho0,
                                               const float* absorb_tau);
/* computeVelocityShiftInX/Y/Z (.cuh:482-499, .cu:2617-2710); spectrum in the layout of kw_fft_r2c_1d(axis) */
KW_API kw_status kw_compute_velocity_shift(kw_ctx* ctx, int axis, float* spectrum, const float* shift_neg_r);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused spectral pipeline (MI355X fast path; csrc/kw_fused.hip).  Each entry computes one whole stage of the step —
 * FFTs, spectral multiply and the real-space update — with hand-written FFT passes, so the gradients and spectra never
 * make an HBM round trip as separate arrays.  Same arithmetic as the kernels cited; supported when each of Nx, Ny, Nz
 * is one of 16 32 48 64 72 80 96 100 108 112 120 128 140 144 160 168 180 192 196 200 216 224 240 252 256 280 288 300
 * 320 324 336 360 384 392 400 420 432 448 480 500 504 512 540 560 576 600 640 648 672 700 720 756 768 784 800 840 864
 * 896 900 960 1024 (2-D: Nx and Ny; with Nx one of 672 700 720 756 784 800 840 864 900 960 the Ny * Nz rows must also
 * be a multiple of 16 — kw_fused_supported says; other grids use the rocFFT entry points above).  kappa / nabla /
 * sourceKappa must first be imported into the pipeline's padded row layout.
 * ---------------------------------------------------------------------------------------------------------------- */
/* Multi-GPU (new with this build; the reference is single-GPU, Readme.md:12-13): Z-slab decomposition with one
 * all-to-all transpose per 3-D FFT.  A context in slab mode holds nz = nz_global/nranks planes of every real array
 * (kw_set_constants gets the LOCAL nz; fft_divider stays 1/(nx*ny*nz_global)) and, in k-space, ny/nranks rows with all
 * nz_global planes ("transposed" layout [nz_global][ny/nranks][P]); reduced operators (kappa, nabla, sourceKappa) are
 * supplied in that transposed layout.
 *
 * The exchange is an all-to-all of equal contiguous chunks (chunk q of `send` goes to rank q; chunk q of `recv` comes
 * from rank q).  Default: the library's own RCCL path — kw_comm_init gives the context a communicator and a
 * communication stream; every exchange is ncclGroupStart / ncclSend + ncclRecv per peer / ncclGroupEnd on that stream,
 * ordered against the context's stream by events (split-phase: the transpose of one array is in flight while the
 * passes of the others run); no host code but the enqueueing runs per exchange.
 *   rank 0: kw_comm_unique_id(id) -> distribute the KW_COMM_ID_BYTES bytes to all ranks by any means (file, socket,
 *   MPI, a torch.distributed store) -> every rank: kw_comm_init(ctx, nranks, rank, id)   [collective, blocks]
 *   -> kw_fused_set_slab(ctx, nranks, rank, nz_global, NULL, NULL) -> kw_fused_create(ctx).
 * One rank with a communicator runs the slab path exchanging with itself (rehearsal on a one-GPU machine). */
#define KW_COMM_ID_BYTES 128
KW_API kw_status kw_comm_unique_id(void* out_id, size_t bytes);  /* ncclGetUniqueId; bytes >= KW_COMM_ID_BYTES */
KW_API kw_status kw_comm_init(kw_ctx* ctx, uint32_t nranks, uint32_t rank, const void* unique_id);
KW_API kw_status kw_comm_destroy(kw_ctx* ctx);                    /* also done by kw_destroy */
KW_API kw_status kw_comm_info(kw_ctx* ctx, uint32_t* nranks, uint32_t* rank, uint64_t* exchanges_started);
/* the same two calls with the RCCL library named by the caller (a path or soname for dlopen; NULL = the default search:
 * the process's own librccl.so.1, then ROCm's) — e.g. a site build of RCCL, or a test double */
KW_API kw_status kw_comm_unique_id_from(const char* rccl_library, void* out_id, size_t bytes);
KW_API kw_status kw_comm_init_with(kw_ctx* ctx, const char* rccl_library, uint32_t nranks, uint32_t rank, const void* unique_id);
/* Device-initiated transport ("P2P"): the ranks map each other's exchange buffers — hipIpc handles between the
 * processes of one node, plain pointers between threads of one process — and every exchange is ONE small kernel on the
 * communication stream that stores this rank's chunks straight into the peers' receive buffers over xGMI, with a
 * credit / full flag rendezvous per peer (csrc/kw_comm.hip k_p2p_exchange).  Same split-phase contract and the same
 * schedules as the RCCL path; what it removes is the per-exchange fixed cost of a library group (launching thread and
 * communication kernel), which is what bounds small and chunked exchanges.  Single node.  Call order on every rank:
 *   kw_comm_init_p2p(ctx, nranks, rank)                 (with or without a prior kw_comm_init)
 *   kw_fused_set_slab(ctx, nranks, rank, nz_global, NULL, NULL);  kw_fused_create(ctx)
 *   kw_comm_p2p_export(ctx, blob, KW_COMM_P2P_BLOB_BYTES)          what this rank publishes: plain bytes
 *   < the caller gathers the blobs of all ranks, in rank order, by any means it has: MPI, a torch.distributed store,
 *     files — all_blobs = nranks * KW_COMM_P2P_BLOB_BYTES bytes, the same on every rank >
 *   kw_comm_p2p_connect(ctx, all_blobs)                  maps the peers' buffers; exchanges go P2P from here on
 * A rank that waits longer than kw_tuning::p2p_timeout_s for a peer stops waiting: the next exchange (or kw_sync of the
 * step loop) returns KW_ERR_COMM — a lost peer ends the run, it does not hang the GPU queue. */
#define KW_COMM_P2P_BLOB_BYTES 1024
KW_API kw_status kw_comm_init_p2p(kw_ctx* ctx, uint32_t nranks, uint32_t rank);
KW_API kw_status kw_comm_p2p_export(kw_ctx* ctx, void* blob, size_t bytes);
KW_API kw_status kw_comm_p2p_connect(kw_ctx* ctx, const void* all_blobs);
/* Link model for schedule studies on a one-GPU machine (tools/emulate_rank.py): ONE rank of an nranks run alone on the
 * GPU — the chunks for the absent peers are copied locally and every peer's transfer is held for latency_us +
 * bytes / link_gbs, as a link of that rate would.  In place of export / connect.  Results are not a simulation's. */
KW_API kw_status kw_comm_p2p_emulate(kw_ctx* ctx, float link_gbs, float latency_us);
/* -1 no communicator, 0 RCCL, 1 P2P not yet connected, 2 P2P, 3 P2P link model */
KW_API kw_status kw_comm_transport(kw_ctx* ctx, int* out_transport);
/* Override: a caller that owns its own communicator passes exchange(user, send, recv, bytes_per_peer), which must be
 * ordered after all prior work on the context's stream and complete (or stream-ordered) before it returns — e.g.
 * torch.distributed.all_to_all_single, or a host-staged all-to-all when several ranks share one GPU (tests).  The
 * callbacks return 0 on success; anything else aborts the step with KW_ERR_COMM. */
typedef int (*kw_exchange_fn)(void* user, void* send, void* recv, size_t bytes_per_peer);
KW_API kw_status kw_fused_set_slab(kw_ctx* ctx, uint32_t nranks, uint32_t rank, uint32_t nz_global,
                                   kw_exchange_fn exchange, void* user);   /* before kw_fused_create; NULL = RCCL path */
/* Optional split-phase form of the same all-to-all, so that transposes overlap with compute: start(user, send, recv,
 * bytes_per_peer, slot) begins the exchange (ordered after the work enqueued so far on the context's stream) and
 * returns; wait(user, slot) makes the context's stream wait for that exchange (slot in 0..5, one exchange in flight per
 * slot).  E.g. all_to_all_single(async_op=True) / work.wait().  Without it the blocking callback is used.
 * A spectral array travels as two pieces when its x-Nyquist bins are kept in the side array (even Nx, the default):
 * the rows on slot 0..2 and the side array on slot + 3 — the callbacks see two exchanges per array, the library's own
 * RCCL path puts both pieces into one group. */
typedef int (*kw_exchange_start_fn)(void* user, void* send, void* recv, size_t bytes_per_peer, int slot);
typedef int (*kw_exchange_wait_fn)(void* user, int slot);
KW_API kw_status kw_fused_set_slab_async(kw_ctx* ctx, kw_exchange_start_fn start, kw_exchange_wait_fn wait);
/* Strided form, for a caller-owned transport that can move PIECES of the arrays: for every peer q, `bytes` bytes at
 * send + q * stride_bytes + offset_bytes go to rank q and land at recv + (sender) * stride_bytes + offset_bytes
 * (stride == bytes, offset 0 is the plain all-to-all above).  start returns after beginning the exchange (or after
 * completing it, with wait == NULL); wait(user, slot) orders the context's stream after it; slot < 256.  With this form —
 * as with the library's own RCCL path — the pipeline runs its pipelined schedule: a third buffer set for the transposed
 * spectra, the forward transposes of the next stage started by the producing stage, small messages batched into one
 * exchange per stage and direction, and with KW_SLAB_CHUNKS=2..4 the plane-local tail of every stage (y-inverse,
 * x-inverse + epilogue, chained forward x / y) run per chunk of planes while the other chunks are on the wire
 * (KW_SLAB_PIPELINE=0: whole-array schedule). */
typedef int (*kw_exchange_piece_fn)(void* user, void* send, void* recv, size_t stride_bytes, size_t offset_bytes, size_t bytes,
                                    int slot);
KW_API kw_status kw_fused_set_slab_pieces(kw_ctx* ctx, kw_exchange_piece_fn start, kw_exchange_wait_fn wait);
KW_API kw_status kw_fused_scratch_bytes(kw_ctx* ctx, size_t* out_bytes_per_array);
/* like kw_fused_create but with caller-owned scratch (each of kw_fused_scratch_bytes bytes): s[3], and t[3] when
 * nranks > 1 — lets the caller register the buffers with its communication library */
KW_API kw_status kw_fused_create_with_scratch(kw_ctx* ctx, void* const s[3], void* const t[3]);
KW_API kw_status kw_fused_supported(kw_ctx* ctx, int* out_supported);
KW_API kw_status kw_fused_create(kw_ctx* ctx);   /* scratch + twiddles; needs kw_set_constants */
KW_API kw_status kw_fused_destroy(kw_ctx* ctx);
KW_API kw_status kw_fused_reduced_elems(kw_ctx* ctx, size_t* out_floats);  /* floats of one imported reduced array */
/* reduced real operator (kappa, nabla1/2, sourceKappa: [nz][ny][nx/2+1]; slab mode: the transposed [nz_global][ny/P][..])
 * -> the pipeline's private tile-blocked layout [ky][kx tile][kz][16] ("*_padded" arguments below) */
KW_API kw_status kw_fused_import_reduced(kw_ctx* ctx, float* dst_padded, const float* src_reduced);
/* computeVelocity (KSpaceFirstOrderSolver.cpp:2087-2119): R2C(p), computePressureGradient (.cu:1139-1157), 3x C2R,
 * computeVelocityHeterogeneous/HomogeneousUniform (.cu:184-215,278-308); dt_rho0_sg* NULL -> scalars */
KW_API kw_status kw_fused_velocity(kw_ctx* ctx, const float* p, float* ux_sgx, float* uy_sgy, float* uz_sgz,
                                   const float* dt_rho0_sgx, const float* dt_rho0_sgy, const float* dt_rho0_sgz,
                                   const float* pml_x_sgx, const float* pml_y_sgy, const float* pml_z_sgz,
                                   const float* kappa_padded, const float* ddx_k_shift_pos,
                                   const float* ddy_k_shift_pos, const float* ddz_k_shift_pos, int chain_u_spectra);
/* chain_u_spectra & KW_FUSED_CHAIN_U: the kernel that updates u also forward-transforms the updated rows along x into the
 * pipeline's scratch, so kw_fused_density(flags & KW_FUSED_U_IN_SCRATCH) skips re-reading u.  Only valid when nothing
 * else (velocity / transducer source injection) writes u in between.
 * chain_u_spectra & KW_FUSED_P_IN_SCRATCH: the spectrum of p was left in scratch by the previous
 * kw_fused_absorption_pressure(flags & KW_FUSED_CHAIN_P) and p has not been written since; p is not read. */
#define KW_FUSED_CHAIN_U       1
#define KW_FUSED_P_IN_SCRATCH  2
#define KW_FUSED_U_IN_SCRATCH 1 /* kw_fused_density: x-spectra of ux,uy,uz are already in scratch */
#define KW_FUSED_CHAIN_TERMS  2 /* kw_fused_density: chain the x-spectra of rho0*sum(du) and sum(rho) into scratch for
                                   kw_fused_absorption_pressure(terms_in_scratch = 1); only the term the pressure sum
                                   re-reads (t1 nonlinear / t0 linear) is stored, the other t arrays are left untouched */
/* second half of addInitialPressureSource (KSpaceFirstOrderSolver.cpp:2368-2395; .cu:949-982) */
KW_API kw_status kw_fused_initial_velocity(kw_ctx* ctx, const float* p, float* ux_sgx, float* uy_sgy, float* uz_sgz,
                                           const float* dt_rho0_sgx, const float* dt_rho0_sgy,
                                           const float* dt_rho0_sgz, const float* kappa_padded,
                                           const float* ddx_k_shift_pos, const float* ddy_k_shift_pos,
                                           const float* ddz_k_shift_pos);
/* computeVelocityGradient + computeDensity{Nonlinear,Linear} (KSpaceFirstOrderSolver.cpp:2126-2173; .cu:1210-1239,
 * 1358-1393, 1470-1497) and, when terms != 0, computePressureTerms{Linear(1),Nonlinear(2)} (.cu:1577-1602,1724-1742)
 * on the updated densities.  duxdx..duzdz may be NULL (gradients not stored).  terms==1: t0 = sum rho,
 * t1 = rho0 * sum du; terms==2: t0 = sum rho, t1 = nonlinear term, t2 = rho0 * sum du.
 * terms==3 (lossless media): the equation of state itself, sumPressure{Nonlinear,Linear}Lossless (.cu:2067-2084,
 * 2224-2236): t0 = p (output), t1 = c2 array or NULL for the scalar (INPUT, not written), t2 unused; with
 * KW_FUSED_CHAIN_TERMS the spectrum of the new p is left for kw_fused_velocity(KW_FUSED_P_IN_SCRATCH).
 * terms==4 (Stokes absorption, alpha_power == 2): as terms==3 with the absorbing term of kw_sum_pressure_stokes_* (same
 * association order, same bits) on the gradients of this step: t0 = p (output), t1 = c2 array or NULL, t2 = absorb_tau
 * array or NULL (both INPUTS, not written; NULL -> the scalar of kw_constants); chains the spectrum of p like terms==3.
 * terms==5 (one-term power law, no_dispersion) and terms==6 (no_absorption): the terms of 1 / 2 that
 * kw_fused_absorption_pressure_one reads, and no others.  `first` goes where 1 / 2 put it: t0 = sum rho (linear), t1 =
 * nonlinear term (nonlinear).  The one term of the absorption round trip goes where 1 / 2 put it as well: terms==5,
 * rho0 * sum du into t1 (linear) / t2 (nonlinear); terms==6, sum rho into t0 (rho0 * sum du is not computed).  With
 * KW_FUSED_CHAIN_TERMS that one term is not stored: its x-spectrum is left in scratch for
 * kw_fused_absorption_pressure_one(KW_FUSED_TERMS_IN_SCRATCH), and only `first` is written.  Unused t arrays may be NULL. */
KW_API kw_status kw_fused_density(kw_ctx* ctx, int nonlinear, const float* ux_sgx, const float* uy_sgy,
                                  const float* uz_sgz, float* rho_x, float* rho_y, float* rho_z, const float* pml_x,
                                  const float* pml_y, const float* pml_z, const float* rho0,
                                  const float* kappa_padded, const float* ddx_k_shift_neg,
                                  const float* ddy_k_shift_neg, const float* ddz_k_shift_neg, float* duxdx,
                                  float* duydy, float* duzdz, int terms, const float* b_on_a, float* t0, float* t1,
                                  float* t2, int flags);
/* absorbing branch of computePressure{Nonlinear,Linear} after the terms (KSpaceFirstOrderSolver.cpp:2196-2204,
 * 2231-2239; .cu:1812-1820,1865-1879,1966-1980): first = nonlinear term or density sum */
/* computeVelocityGradient alone (KSpaceFirstOrderSolver.cpp:2126-2143, SolverCudaKernels.cu:1210-1239): the three
 * gradients as arrays, for loops that put a step between them and the density update (non-uniform grids, :2145-2149) */
KW_API kw_status kw_fused_velocity_gradient(kw_ctx* ctx, const float* ux_sgx, const float* uy_sgy, const float* uz_sgz,
                                            float* duxdx, float* duydy, float* duzdz, const float* kappa_padded,
                                            const float* ddx_k_shift_neg_r, const float* ddy_k_shift_neg,
                                            const float* ddz_k_shift_neg, int flags /* KW_FUSED_U_IN_SCRATCH */);
KW_API kw_status kw_fused_absorption_pressure(kw_ctx* ctx, float* p, const float* velocity_gradient_term,
                                              const float* density_sum, const float* first,
                                              const float* nabla1_padded, const float* nabla2_padded, const float* c2,
                                              const float* absorb_tau, const float* absorb_eta, int flags);
/* the absorbing branch with one term (absorbing_flag 3 / 4; see kw_sum_pressure_terms_one_*): one forward transform of
 * `term`, times nabla_padded (nabla1 for which == 0, nabla2 for which == 1), one inverse, then p = c2 * (first +- ...) with
 * coef = absorb_tau / absorb_eta array or NULL for the scalar of kw_constants.  One exchange each way on slabs.  flags as
 * for kw_fused_absorption_pressure (TERMS_IN_SCRATCH: the term's spectrum was chained by kw_fused_density(terms 5 / 6)). */
KW_API kw_status kw_fused_absorption_pressure_one(kw_ctx* ctx, float* p, const float* term, const float* first,
                                                  const float* nabla_padded, const float* c2, const float* coef,
                                                  int which, int flags);
#define KW_FUSED_TERMS_IN_SCRATCH 1 /* kw_fused_absorption_pressure: the two terms' spectra were chained by kw_fused_density */
#define KW_FUSED_CHAIN_P          2 /* ... and the kernel that writes p forward-transforms it for the next kw_fused_velocity */
/* tuning probe: one pass of the pipeline over its scratch (0 y-pass, 1 line pass along z, 2 z-fused, 3 y-pass x3) */
KW_API kw_status kw_fused_probe(kw_ctx* ctx, int which, const float* padded_reduced_operator);
/* FFT part of scaleSource (KSpaceFirstOrderSolver.cpp:2346-2351; .cu:740-745), in place on scaled_source */
KW_API kw_status kw_fused_scale_source(kw_ctx* ctx, float* scaled_source, const float* source_kappa_padded);
/* Non-staggered velocity (computeShiftedVelocity, KSpaceFirstOrderSolver.cpp:2714-2735): one kernel per axis instead of
 * R2C + computeVelocityShiftIn{X,Y,Z} (SolverCudaKernels.cu:2617-2710) + C2R.  out = F^-1{ filter .* F{in} } along
 * `axis` (0 x, 1 y, 2 z) of the real [nz][ny][nx] array; filter = device array of N_axis complex values, the
 * Hermitian extension of the reference's half-length shift vector with the 1/N of the transform pair folded in:
 *   filter[k] = shift[k]/N (0 < k < N/2), filter[N-k] = conj(filter[k]), filter[0] = Re(shift[0])/N,
 *   filter[N/2] = Re(shift[N/2])/N  (what C2R keeps of those two bins).  Single-GPU pipeline only. */
KW_API kw_status kw_fused_shift_velocity(kw_ctx* ctx, int axis, const float* in, float* out, const float* filter);

/* ------------------------------------------------------------------------------------------------------------------
 * Sampling kernels — replace namespace OutputStreamsCudaKernels (OutputStreams/OutputStreamsCudaKernels.cuh:47-106)
 * ---------------------------------------------------------------------------------------------------------------- */
/* n_samples == 0 (for the post-processing entry points further down: n == 0) is KW_OK in every entry point of this
 * section: nothing is launched and no pointer is looked at.  max / min are fmaxf / fminf as CUDA defines them: a NaN
 * operand yields the other operand, +0 orders above -0. */
/* sampleIndex<op> (.cuh:58-62, .cu:83-126) */
KW_API kw_status kw_sample_index(kw_ctx* ctx, kw_reduce_op op, float* sampling_buffer, const float* source_data,
                                 const uint64_t* sensor_data, uint64_t n_samples);
/* the same for up to four operators of one field over one mask in one launch (e.g. -p --p_max): index and value are read
 * once; each buffer gets exactly what its own sampleIndex<op> call would give */
KW_API kw_status kw_sample_index_multi(kw_ctx* ctx, int n_ops, const kw_reduce_op* ops, float* const* sampling_buffers,
                                       const float* source_data, const uint64_t* sensor_data, uint64_t n_samples);
/* sampleCuboid<op> (.cuh:75-81, .cu:164-252): corners are 0-based inclusive (x,y,z), matrix_size = (nx,ny,nz) */
KW_API kw_status kw_sample_cuboid(kw_ctx* ctx, kw_reduce_op op, float* sampling_buffer, const float* source_data,
                                  const uint32_t top_left[3], const uint32_t bottom_right[3],
                                  const uint32_t matrix_size[3], uint64_t n_samples);
/* sampleAll<op> (.cuh:91-95, .cu:297-332) */
KW_API kw_status kw_sample_all(kw_ctx* ctx, kw_reduce_op op, float* sampling_buffer, const float* source_data,
                               uint64_t n_samples);
/* Compression streams (config 5).  The reference samples on the GPU (sampleIndex<kNone>) and correlates with the
 * basis on the CPU one step later (OutputStreams/IndexOutputStream.cpp:373-470); here gather + correlation are one
 * kernel and the accumulators c1/c2 ([n_samples][harmonics] complex) stay on the device:
 *   c1[i,h] += bE[h*b_size+step_local] * x[i];  c2[i,h] += bE_1[h*b_size+step_local] * x[i];
 *   mirror_first_half_frame: c2[i,h] += c1[i,h]  (first saved frame, :388,462-466).  c1 may equal c2 (--no_overlap). */
KW_API kw_status kw_sample_index_compress(kw_ctx* ctx, float* c1, float* c2, const float* source_data,
                                          const uint64_t* sensor_data, uint64_t n_samples, uint32_t harmonics,
                                          const float* bE, const float* bE_1, uint32_t b_size, uint32_t step_local,
                                          int mirror_first_half_frame);
/* --40-bit_complex (IndexOutputStream.cpp:410-436; codec Compression/CompressHelper.cpp:224-389): the accumulators are
 * [n_samples][harmonics] 5-byte packed complex numbers, decoded, updated and re-encoded at every sampled step; max_exp =
 * 138 (pressure) / 114 (velocity).  no_overlap: one buffer (c2 unused), c1 += bE*x + bE_1*x. */
KW_API kw_status kw_sample_index_compress_40b(kw_ctx* ctx, void* c1, void* c2, const float* source_data,
                                              const uint64_t* sensor_data, uint64_t n_samples, uint32_t harmonics,
                                              const float* bE, const float* bE_1, uint32_t b_size, uint32_t step_local,
                                              int mirror_first_half_frame, int no_overlap, int max_exp);
KW_API kw_status kw_intensity_avg_c_accumulate_40b(kw_ctx* ctx, float* iavg, const void* frame_p, const void* frame_u,
                                                   uint64_t n_samples, uint32_t harmonics, int max_exp_p, int max_exp_u);
/* IndexOutputStream::postSample for kIAvgC (IndexOutputStream.cpp:299-342): iavg[i] += sum_h Re(P[i,h]*conj(U[i,h]))/2 */
KW_API kw_status kw_intensity_avg_c_accumulate(kw_ctx* ctx, float* iavg, const float* frame_p, const float* frame_u,
                                               uint64_t n_samples, uint32_t harmonics);
/* buf[i] /= divisor — final division of I_avg_c by the frame count (IndexOutputStream.cpp:482-490) */
KW_API kw_status kw_divide(kw_ctx* ctx, float* buf, float divisor, uint64_t n);
/* ---- post-processing of stored series (KSpaceFirstOrderSolver.cpp:1231-1534 computeAverageIntensities, :1783-2080
 * computeQTerm).  The reference moves every spectrum to the host for the multiply; here the series stay on the device.
 * kw_time_shift_series: series[step][i] (device, steps x n, in place) is advanced by half a time step through its
 *   spectrum along the step axis: X[k] *= (1/steps) * shift[k], k = 0..steps/2 (:1437-1449); shift = device array of
 *   steps/2+1 complex values exp(i*pi*s(k)/steps) computed by the caller (:1253-1260).
 * kw_intensity_avg: iavg[i] = (sum over steps, in step order, of u[step][i]*p[step][i]) / steps (:1492-1513).
 * kw_q_term_sum: out[i] = -(a[i] + b[i] + c[i]) over the grid, c may be NULL in 2-D (:2014-2026). */
KW_API kw_status kw_time_shift_series(kw_ctx* ctx, float* series, const float* shift, uint64_t steps, uint64_t n);
KW_API kw_status kw_intensity_avg(kw_ctx* ctx, float* iavg, const float* p, const float* u, uint64_t steps, uint64_t n);
KW_API kw_status kw_q_term_sum(kw_ctx* ctx, float* out, const float* a, const float* b, const float* c, uint64_t n);
/* postProcessingRms (.cuh:103-105, .cu:359-378) */
KW_API kw_status kw_post_processing_rms(kw_ctx* ctx, float* sampling_buffer, float scaling_coeff, uint64_t n_samples);

/* ------------------------------------------------------------------------------------------------------------------
 * Weighted transducer arrays (new with this build): an array element of k-Wave's kWaveArray is a set of grid points
 * with band-limited interpolation weights.  Both directions are a sparse matrix in CSR form: ptr[0..rows] are 0-based
 * uint32 row offsets into entries[], and an entry is a 0-based column with its weight, read as one 8-byte load.  Both
 * kernels only gather, so every output value is a fixed function of the CSR and the input: the same bits on every run.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kw_csr_entry
{
  uint32_t col;    /* weighted source: element (0 .. n_elements-1); weighted sensor: linear grid index */
  float    weight;
} kw_csr_entry;
#define KW_ELEMENT_CHUNK 1024u /* entries per block of kw_sample_elements */
/* Weighted pressure source: the per-point series row of time step t,
 *   row[k] = sum over the entries j of row k, in CSR order, of weight_j * element_input[t * n_elements + col_j]
 * accumulated with fp32 fma from 0.  One thread per point.  ptr has n_points + 1 entries. */
KW_API kw_status kw_element_source_row(kw_ctx* ctx, float* row, const float* element_input, const uint32_t* ptr,
                                       const kw_csr_entry* entries, uint32_t n_points, uint32_t n_elements,
                                       uint64_t time_index);
/* Weighted pressure sensor: out[e] = sum over the entries j of row e of weight_j * p[col_j], for e < n_elements.
 * Row e is cut into ceil(len_e / KW_ELEMENT_CHUNK) chunks; chunk_ptr[0..n_elements] are the 0-based prefix sums of those
 * counts (computed once by the caller, n_chunks = chunk_ptr[n_elements]) and partials holds n_chunks floats of workspace.
 * One block per chunk: per-lane fma partial sums, then a fixed wave64 + LDS tree; a second launch adds an element's chunk
 * partials in chunk order.  No atomics.  An empty row gives 0. */
KW_API kw_status kw_sample_elements(kw_ctx* ctx, float* out, const float* p, const uint32_t* ptr,
                                    const kw_csr_entry* entries, uint32_t n_elements, uint64_t nnz,
                                    const uint32_t* chunk_ptr, uint32_t n_chunks, float* partials);
/* The velocity components of an array share one index set and one weight matrix: these two forms serve up to three fields
 * in one pass over the CSR, each entry read once.
 * kw_element_source_rows: rows[c] = the row kw_element_source_row gives for element_inputs[c] at time_index, bit for bit
 * (same CSR order, same fma chain from 0, one thread per point), for c = 0, 1, 2 in one launch.  rows and element_inputs
 * are host arrays of three device pointers; a component whose rows[c] is NULL is skipped and element_inputs[c] is then
 * never read, on the host or on the device.  With all three NULL nothing is launched. */
KW_API kw_status kw_element_source_rows(kw_ctx* ctx, float* const rows[3], const float* const element_inputs[3],
                                        const uint32_t* ptr, const kw_csr_entry* entries, uint32_t n_points,
                                        uint32_t n_elements, uint64_t time_index);
/* kw_sample_elements_multi: outs[f][e] = what kw_sample_elements gives on fields[f], bit for bit, for f < n_fields
 * (1 .. 3): the same chunks, per-lane stride, wave64 butterfly and four-wave pairing with one accumulator per field, then
 * one launch that adds the chunk partials of every field in chunk order.  outs and fields are host arrays of n_fields
 * device pointers; partials holds n_fields * n_chunks floats (field f's chunk b at f * n_chunks + b).  No atomics. */
KW_API kw_status kw_sample_elements_multi(kw_ctx* ctx, uint32_t n_fields, float* const outs[], const float* const fields[],
                                          const uint32_t* ptr, const kw_csr_entry* entries, uint32_t n_elements,
                                          uint64_t nnz, const uint32_t* chunk_ptr, uint32_t n_chunks, float* partials);

/* Per-entry time delays (new with this build): entry j of a CSR above may carry an integer delay d_j in time steps, at
 * most KW_ELEMENT_MAX_DELAY, so that one signal drives a focused or steered array and a sensor delivers delay-and-sum
 * series.  The delays travel beside the entries as uint32 values indexed like them; an entry stays one 8-byte load.
 * kw_element_source_rows_delayed: rows[c][k] = sum over the entries j of row k, in CSR order, of
 *     weight_j * element_inputs[c][(time_index - delays[j]) * n_elements + col_j],
 * fp32 fma from 0 as in kw_element_source_row(s), for c = 0, 1, 2 in one launch.  element_inputs[c] is the start of
 * component c's signals, signal_steps[c] rows of n_elements values; entry j is left out of component c's chain when
 * time_index < delays[j] or time_index - delays[j] >= signal_steps[c].  (With every delay 0 and time_index below every
 * signal_steps[c] the rows carry the bits of kw_element_source_rows; a time_index at or past the last row any entry can
 * reach gives rows of +0.)  rows, element_inputs and signal_steps are host arrays of three; a component whose rows[c]
 * is NULL is skipped and its other two values are never read.  With all three NULL nothing is launched. */
#define KW_ELEMENT_MAX_DELAY 65535u
KW_API kw_status kw_element_source_rows_delayed(kw_ctx* ctx, float* const rows[3], const float* const element_inputs[3],
                                                const uint64_t signal_steps[3], const uint32_t* ptr,
                                                const kw_csr_entry* entries, const uint32_t* delays, uint32_t n_points,
                                                uint32_t n_elements, uint64_t time_index);
/* kw_sample_elements_delayed: step n = rows_emitted of the delayed sensor,
 *     out_n[e] = sum over the entries j of element e of weight_j * field^(n - d_j)[col_j],
 * where field^(m) is what `fields` held at the call with rows_emitted == m and terms with n - d_j < 0 are dropped.
 * The caller has regrouped each element's entries by delay, stably (CSR order inside a group); a group is the set of
 * entries of one element with one delay.  entries holds the regrouped entries, group_ptr[0..n_groups] the groups'
 * offsets into it, group_delay[g] a group's delay, element_group_ptr[0..n_elements] the elements' offsets into the
 * groups, chunk_ptr[0..n_groups] the prefix sums of ceil(group length / KW_ELEMENT_CHUNK) (n_chunks in all) and
 * partials n_fields * n_chunks floats of workspace.  rings[f] holds ring_rows x n_elements floats, ring_rows above the
 * largest delay, zeroed by the caller before the call with rows_emitted == 0 and otherwise left to the calls; calls are
 * made with rows_emitted = 0, 1, 2, ... on one stream.
 * Two launches: the groups' chunk partials, with the device code of kw_sample_elements_multi on the groups as rows, so
 * a group's sum carries the bits kw_sample_elements gives for it as a row of its own; then one thread per element adds
 * each of its groups' sums, chunk partials in chunk order from 0, to ring row (rows_emitted + d) mod ring_rows in fp32,
 * writes row rows_emitted mod ring_rows to outs[f] and clears it to +0.  Column e of a ring belongs to one thread: no
 * atomics, and outs[f][e] is the sum of the element's group sums in descending delay order from +0 — the bits of
 * kw_sample_elements(_multi) when every delay is 0.  outs, fields and rings are host arrays of n_fields (1 .. 3) device
 * pointers.  A delay at or above ring_rows is folded into the ring (no access outside it) and gives wrong sums. */
KW_API kw_status kw_sample_elements_delayed(kw_ctx* ctx, uint32_t n_fields, float* const outs[],
                                            const float* const fields[], const uint32_t* group_ptr,
                                            const kw_csr_entry* entries, const uint32_t* group_delay,
                                            const uint32_t* element_group_ptr, uint32_t n_elements, uint32_t n_groups,
                                            uint64_t nnz, const uint32_t* chunk_ptr, uint32_t n_chunks, float* partials,
                                            float* const rings[], uint32_t ring_rows, uint64_t rows_emitted);

/* ------------------------------------------------------------------------------------------------------------------
 * Off-grid elements (new with this build): the weights of the arrays above from the elements' geometry — what k-Wave's
 * kWaveArray computes with getArrayGridWeights / offGridPoints.  An element is a set of integration points on its
 * surface; its weights are the band-limited interpolant (BLI) of those points, a truncated sinc stencil per point.
 *   Grid      nx x ny x nz points (a 2-D grid has nz == 1).
 *   Point     three coordinates in grid units, u = x / d + floor(N / 2) per axis (k-Wave's kgrid.x_vec), float64.  The
 *             call splits u, in float64, into the nearest index n = floor(u + 0.5) and the offset f = u - n in
 *             [-0.5, 0.5); f goes to the device as fp32.  A point whose n is outside 0 .. N - 1 is an error.
 *   Stencil   R = ceil(1 / (pi * bli_tolerance)) (0.05 gives 7; at most 64).  Point p of element e adds, to every grid
 *             point (n_x + d_x, n_y + d_y, n_z + d_z) with |d| <= R per axis that lies inside the grid,
 *               c = ((scale[e] * s(d_x, f_x)) * s(d_y, f_y)) * s(d_z, f_z),   s(d, f) = sinc(d - f),
 *             evaluated in fp32 as (-1)^d sin(pi f) / (pi (f - d)), 1 at f - d == 0 (exactly 0 off the point's own index
 *             when f == 0); on an axis of one point the factor is 1 and d = 0.  No entry is thresholded: the only
 *             truncation is the box of radius R, clipped at the grid's faces.
 *   Element   W[e][g] = sum over its points of c.  Each c is rounded to a multiple of 2^-40 and added with 64-bit integer
 *             atomics into the element's zeroed bounding box, so the sum is exact and the CSR is the same bits on every
 *             run and under any permutation of an element's points; it is rounded to fp32 once.  A cell is an entry iff
 *             its sum is not zero.  An element with |scale[e]| * (its point count) >= 2^22 is refused (KW_ERR_INVALID).
 *   Rounds    as many elements (in order) as fit `scratch_bytes` at 20 bytes per cell of their bounding boxes (the
 *             points' n, dilated by R and clipped; padded to 256 cells) share one round: a memset, four launches and one
 *             host round trip (two synchronisations: the entry count, then the entries).  scratch_bytes == 0: kw_tuning::offgrid_scratch_bytes.  An element whose box alone does
 *             not fit is refused with KW_ERR_ALLOC; kw_last_error names the element and the bytes it needs.
 * coords holds 3 * P doubles (x, y, z of point 0, then point 1, ...), point_ptr the n_elements + 1 offsets of the
 * elements' points (point_ptr[0] == 0, P = point_ptr[n_elements]), scale one factor per element; all host arrays, not
 * written; at most 2^32 points in one build.  Errors in them are KW_ERR_INVALID with the element and the point (counted within the element) named.
 * The result is a host-side CSR over the elements: row e holds element e's grid points, 0-based linear indices with x
 * fastest, strictly ascending, and their weights.  Elements without points give empty rows; n_elements == 0 an empty CSR.
 * The call allocates and frees its own device memory and synchronises the context's stream.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kw_offgrid kw_offgrid;
KW_API kw_status kw_offgrid_build(kw_ctx* ctx, const double* coords, const uint64_t* point_ptr, const float* scale,
                                  uint64_t n_elements, uint32_t nx, uint32_t ny, uint32_t nz, double bli_tolerance,
                                  uint64_t scratch_bytes, kw_offgrid** out);
/* the CSR of a build: its sizes, the n_elements + 1 row offsets, and copies of the entries (either may be NULL) */
KW_API kw_status kw_offgrid_size(kw_ctx* ctx, const kw_offgrid* h, uint64_t* out_n_elements, uint64_t* out_nnz);
KW_API kw_status kw_offgrid_ptr(kw_ctx* ctx, const kw_offgrid* h, uint64_t* out_ptr);
KW_API kw_status kw_offgrid_entries(kw_ctx* ctx, const kw_offgrid* h, uint64_t* out_index, float* out_weight);
KW_API kw_status kw_offgrid_free(kw_ctx* ctx, kw_offgrid* h);

/* ------------------------------------------------------------------------------------------------------------------
 * Bioheat (new with this build; what k-Wave's kWaveDiffusion computes): the element-wise kernels of the explicit k-space
 * time stepping of the Pennes equation  rho C dT/dt = div(K grad T) - rho_b C_b W_b (T - T_a) + Q  (csrc/kw_thermal.hip).
 * The FFT stages are the entry points above driven with thermal operators (host/ThermalSolver.cpp):
 * kw_fused_scale_source / kw_fused_initial_velocity / kw_fused_velocity_gradient, or kw_fft_r2c_3d / kw_fft_c2r_3d with
 * kw_compute_source_gradient / _pressure_gradient / _initial_velocity / _velocity_gradient.
 * n == 0 is KW_OK in both: nothing is launched and no pointer is looked at.
 *
 * kw_thermal_update: per point, with a = 1 / (rho C), P = rho_b C_b W_b a, in this fp32 order
 *     s = d0                      (d1 == d2 == NULL: Laplacian form, d0 = Laplacian of T, diff_scale = K)
 *       = (d0 + d1) + d2          (flux form: the three terms of div(K grad T), diff_scale = 1)
 *     r = (diff_scale * a) * s;   r = fma(-P, T - T_a, r);   r = fma(a, Q, r)  [Q != NULL and heat_on != 0]
 *     T = fma(dt, r, T)
 *   then on the updated T:  cem43 += (dt / 60) * R^(43 - T),  R = 0.5 for T >= 43, 0.25 for 37 <= T < 43, no increment
 *   below 37 (R^(43 - T) = exp2f(s (T - 43)), s = 1 or 2), and T_max = fmaxf(T_max, T) when T_max != NULL.
 *   a / P / T_a: an array, or NULL with the scalar beside it (a_s / P_s / T_a_s).  16-byte loads and stores when every
 *   pointer is 16-byte aligned (n % 4 tail element by element), element by element otherwise; at most CU count x 8 blocks
 *   of 256 threads stride over the array.
 * kw_thermal_dose: the dose increment alone, cem43[i] += (dt / 60) * R^(43 - T[i]), for callers that step T themselves.
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_thermal_update(kw_ctx* ctx, float* T, float* cem43, float* T_max, const float* d0, const float* d1,
                                   const float* d2, float diff_scale, const float* a, float a_s, const float* P, float P_s,
                                   const float* T_a, float T_a_s, const float* Q, float dt, int heat_on, uint64_t n);
KW_API kw_status kw_thermal_dose(kw_ctx* ctx, float* cem43, const float* T, float dt, uint64_t n);

/* ------------------------------------------------------------------------------------------------------------------
 * CW field propagator (new with this build; what k-Wave's acousticFieldPropagator computes): the steady-state pressure
 * of a continuous-wave source S(x) exp(i w t) in a homogeneous lossless medium, as the exact k-space solution of
 * p_tt - c0^2 lap(p) = S exp(i w t), p = p_t = 0 at t = 0, on a periodic grid at one late time T (csrc/kw_cw.hip,
 * host/CwPropagator.cpp).  Per bin, a = c0 |k|, d = a - w:
 *     G(a) = i [ sin(a T)/a - T exp(i (a + w) T/2) sinc(d T/2) ] / (a + w),   sinc(x) = sin(x)/x, sin(a T)/a -> T at a = 0
 * (the textbook (exp(i w T) - cos(a T) - i (w/a) sin(a T)) / (a^2 - w^2), regular at a = w and a = 0), and the complex
 * amplitude P(x) = p(x, T) exp(-i w T) = ifftn(G exp(-i w T) fftn(S)).  The field is carried as two real arrays, S = re +
 * i im: G depends on |k| only, so  Pr^ = Gr Sr^ - Gi Si^,  Pi^ = Gi Sr^ + Gr Si^  are Hermitian half-spectra.
 *
 * kw_cw_operator: g_re / g_im [nz][ny][nx/2+1] (the grid of kw_set_constants) <- Re / Im of G exp(-i w T) / (nx ny nz),
 *   evaluated in float64 on the device and rounded once (a T reaches thousands of radians).  w = 2 pi f0 [rad/s], T [s],
 *   dk? = 2 pi / (n? d?) [rad/m]; every scalar must be positive.  kw_fused_import_reduced moves each array into the
 *   pipeline's layout for kw_fused_cw_pair; kw_cw_mix reads them as they are.
 * kw_fused_cw_pair: re, im [nz][ny][nx], in place: (re + i im) <- ifftn((g_re + i g_im) fftn(re + i im)); the operators
 *   (imported) carry the 1/N.  x-forward and y-forward of both arrays, one z-pass that transforms both, mixes them in
 *   registers and transforms both back, y-inverse, x-inverse.  Single GPU, 3-D: KW_ERR_INVALID in slab mode or for Nz == 1.
 * kw_cw_mix: the same mix on two spectra of kw_fft_r2c_3d (interleaved complex, n_bins bins each), in place, for
 *   kw_fft_r2c_3d x 2 -> kw_cw_mix -> kw_fft_c2r_3d x 2 (grids off the fast path).  Per bin and per component (real and
 *   imaginary alike), in this fp32 order without contraction into fma:
 *     re' = (g_re * re) - (g_im * im),     im' = (g_im * re) + (g_re * im)
 * kw_cw_embed: ex_re / ex_im [ez][ey][ex] <- 0, except the corner [0, nz) x [0, ny) x [0, nx), which receives the source
 *   a, b [nz][ny][nx]: parts != 0: S = a + i b; parts == 0: S = a (cos b + i sin b) (amplitude, phase [rad]) — times the
 *   complex source scale: re = (Sr * scale_re) - (Si * scale_im), im = (Sr * scale_im) + (Si * scale_re), no contraction;
 *   with scale = (1, 0) the values are stored as they are (copies and zero fill are exact).
 * kw_cw_extract: the corner of the expanded pair cropped back to [nz][ny][nx]; each output may be NULL: out_re, out_im
 *   (copies), out_amp = sqrtf((re * re) + (im * im)), out_phase = atan2(im, re) evaluated in float64 and rounded once,
 *   out_q = q * ((re * re) + (im * im)) with q per point, or NULL and q_scalar (plane wave: q = alpha / (rho0 c0), alpha
 *   in Np/m, gives the volume rate of heat deposition).
 * embed / extract: 16-byte accesses when ex and nx are multiples of 4 and every pointer is 16-byte aligned, element by
 *   element otherwise; at most CU count x 8 blocks of 256 threads stride over the points.  A grid of 0 points (embed: of
 *   the expanded grid, extract: of the domain) and kw_cw_mix with n_bins == 0 are KW_OK: nothing is launched and no
 *   pointer is looked at.
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_cw_operator(kw_ctx* ctx, float* g_re, float* g_im, double c0, double w, double T, double dkx, double dky,
                                double dkz);
KW_API kw_status kw_fused_cw_pair(kw_ctx* ctx, float* re, float* im, const float* g_re_padded, const float* g_im_padded);
KW_API kw_status kw_cw_mix(kw_ctx* ctx, float* spec_re, float* spec_im, const float* g_re, const float* g_im, uint64_t n_bins);
KW_API kw_status kw_cw_embed(kw_ctx* ctx, float* ex_re, float* ex_im, const float* a, const float* b, int parts,
                             float scale_re, float scale_im, uint32_t ex, uint32_t ey, uint32_t ez, uint32_t nx, uint32_t ny,
                             uint32_t nz);
KW_API kw_status kw_cw_extract(kw_ctx* ctx, const float* ex_re, const float* ex_im, uint32_t ex, uint32_t ey, uint32_t ez,
                               uint32_t nx, uint32_t ny, uint32_t nz, float* out_re, float* out_im, float* out_amp,
                               float* out_phase, float* out_q, const float* q, float q_scalar);

/* ------------------------------------------------------------------------------------------------------------------
 * Angular-spectrum CW projector (what k-Wave's angularSpectrumCW computes): a complex pressure plane P0[y][x] carried to
 * the planes z_j = z0 + j dz, j < n_planes, of a homogeneous medium with wavenumber k [rad/m] and absorption alpha [Np/m]
 * (csrc/kw_angular.hip, host/AngularSpectrum.cpp).  Time factor exp(+i w t), outgoing waves exp(-i k r):
 *     P(., ., z) = ifft2( fft2(P0 embedded in nx x ny) H(kx, ky, z) ),      kr^2 = kx^2 + ky^2,  q = |k^2 - kr^2|^(1/2)
 *     kr^2 < k^2: H = exp(-i q z) exp(-alpha z k / q)     kr^2 = k^2: H = 1 (alpha = 0), 0 (alpha > 0)     kr^2 > k^2: H = exp(-q z)
 *     restriction: H = 0 where kr > kc(z) = k sqrt(D^2/2 / (D^2/2 + z^2)),  D = min((nx - 1) dx, (ny - 1) dy)
 * on the grid (nx, ny) of kw_set_constants; bins are counted k? = 2 pi / (n? d?) * min(i, n? - i).  No transform runs along
 * z.  The field is two real arrays and H depends on kr only: the 2x2 mix of kw_cw_mix gives Hermitian half-spectra.
 *
 * kw_angular_operator: tables <- five arrays of (nx/2 + 1) * ny 4-byte words, [ky][kx] each, evaluated in float64:
 *     a0, a1  uint32  round(frac(q z0 / 2 pi) 2^32), round(frac(q dz / 2 pi) 2^32) on kr^2 < k^2, else 0
 *     b0, b1  float   alpha z0 k / q * log2(e) and the same of dz (kr^2 < k^2); q z0 log2(e), q dz log2(e) (kr^2 > k^2); else 0
 *     alive   uint32  number of leading planes with kr <= kc(z_j) (n_planes without restriction); 0 on kr^2 = k^2, alpha > 0
 *   H of plane j, every step in float32 without contraction:
 *     angle = float(int32(a0 + j * a1)) * (2 pi 2^-32)      (the word wraps: exact phase, at most (j + 1) 2^-33 turns off)
 *     m = exp2f(-(b0 + (float(j) * b1))) * divider, 0 where j >= alive;   Hr = m * cos(angle),  Hi = -(m * sin(angle))
 *   (sincosf on the reduced argument; the hardware sine is not used).  n_planes <= 4096, z0 >= 0, dz > 0, alpha >= 0.
 *   imported (may be NULL; needs kw_fused_create): the same five tables in the pipeline's plane layout,
 *   kw_fused_angular_elems words each.
 * kw_fused_angular_elems: complex values of one 2-D source spectrum = words of one imported table (rows of the pipeline's
 *   pitch and, where the pipeline keeps it apart, the x-Nyquist column behind them).
 * kw_fused_angular_forward: spec_re / spec_im <- the 2-D spectra of plane 0 of re / im [nz][ny][nx] (x-forward and the
 *   forward y-pass on that plane; the leading planes that make up whole x tiles are read along with it).
 * kw_fused_angular_planes: re, im [nz][ny][nx] <- planes j0 ... j0 + nz - 1, nz = the context's plane count (the chunk):
 *   one launch k_yinv_angular (tile = (kx tile, plane): H of the plane from the table lines, the mix, both y-inverses over
 *   one exchange buffer; divider = 1 / (nx ny)) and the x-inverse of the two arrays.  Single GPU, nz > 1: KW_ERR_INVALID in
 *   slab mode or for Nz == 1.
 * kw_angular_mix: the twin on plain spectra: out_re / out_im [n_planes][n_bins] interleaved complex <- the mix of the
 *   source's spectra spec_re / spec_im [n_bins] with H of planes j0 ... from `tables` (natural order), for 2-D C2R
 *   transforms of each plane (grids off the fast path).  n_bins == 0 or n_planes == 0: KW_OK, nothing launched.
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_angular_operator(kw_ctx* ctx, uint32_t* tables, uint32_t* imported, double dx, double dy, double k,
                                     double alpha, double z0, double dz, uint32_t n_planes, int restriction);
KW_API kw_status kw_fused_angular_elems(kw_ctx* ctx, size_t* out_elems);
KW_API kw_status kw_fused_angular_forward(kw_ctx* ctx, const float* re, const float* im, float* spec_re, float* spec_im);
KW_API kw_status kw_fused_angular_planes(kw_ctx* ctx, const float* spec_re, const float* spec_im,
                                         const uint32_t* tables_imported, uint32_t j0, float* re, float* im);
KW_API kw_status kw_angular_mix(kw_ctx* ctx, float* out_re, float* out_im, const float* spec_re, const float* spec_im,
                                const uint32_t* tables, uint32_t n_bins, uint32_t n_planes, uint32_t j0, float divider);

/* ------------------------------------------------------------------------------------------------------------------
 * Time-domain angular-spectrum projector (what k-Wave's angularSpectrum computes): a real pressure record p0[t][y][x] on a
 * plane carried to a parallel plane at distance z >= 0 of a homogeneous medium (csrc/kw_angular_time.hip,
 * host/AngularSpectrumTime.cpp).  Time factor exp(+i w t), outgoing waves exp(-i k r).  The grid of
 * kw_set_constants is (nx, ny, nz) = (Ex, Ey, Lt): the time axis is where the pipeline has z; Ex and Lt even.
 *     p(., ., .; z) = irfftn( rfftn(p0 embedded in Lt x Ey x Ex) H(kx, ky, m; z) )                     axes (t, y, x)
 *     m' = min(m, Lt - m),  w = 2 pi m' / (Lt dt),  k = w / c0,  kr^2 = kx^2 + ky^2,  q = |k^2 - kr^2|^(1/2)
 *     bins are counted k? = 2 pi / (n? d?) * min(i, n? - i)
 *     m = 0 and m = Lt/2: H = 0 (the record's temporal mean is dropped)
 *     kr^2 < k^2: H0 = exp(-i q z) exp(-alpha(m') z k / q)     kr^2 = k^2: H0 = 1 (alpha = 0), 0 (alpha > 0)
 *     kr^2 > k^2: H0 = exp(-q z)
 *     retarded:    H0 <- H0 exp(+i k z)                        (plane z is reported at the times t_n + z / c0)
 *     restriction: H0 = 0 where kr^2 > k^2 (D^2/2) / (D^2/2 + z^2),  D = min((Ex - 1) dx, (Ey - 1) dy)
 *     H = H0 for 0 < m < Lt/2, conj(H0) for m > Lt/2
 * One real array is enough: H(-w) = conj H(w) and H depends on kr only, so the half-spectrum stays Hermitian.
 *
 * H per bin is ONE device function for the fused kernel and the twin, without contraction into fma:
 *   float64: kx, ky from the bin counts;  kr2 = (kx*kx) + (ky*ky);  k = dk * m' with dk = 2 pi / (Lt dt c0);  k2 = k*k;
 *            q = sqrt(fabs(k2 - kr2));  turns t = (qp - (retarded ? k : 0)) * z / 2 pi, qp = q when kr2 <= k2, 0 above;
 *            word = uint32(rint((t - floor(t)) * 2^32));  restriction test kr2 > k2 * cfac, cfac = (D^2/2) / (D^2/2 + z^2)
 *            computed once on the host
 *   float32: angle = float(int32(word)) * (2 pi 2^-32), one sincosf (the hardware sine is not used);  q32 = float(q);
 *            b = float(ak[m'] * z) / q32 (kr2 < k2, ak given), q32 * float(z log2(e)) (kr2 > k2), else 0;
 *            mag = exp2f(-b) * divider, 0 for m' = 0, m' = Lt/2, on kr2 = k2 with ak[m'] > 0, and beyond the restriction;
 *            Hr = mag * cos,  Hi = -(mag * sin), Hi negated for m > Lt/2;
 *            out = ((Hr * x.x) - (Hi * x.y), (Hr * x.y) + (Hi * x.x))
 *   A float32 product q z would be 3e-4 rad off a thousand wavelengths out; the phase word is exact to 2^-33 turns.
 *
 * kw_fused_angular_time_elems: complex values of one scratch array = the size of `kept`.
 * kw_fused_angular_time_forward: kept <- the (kx, ky, t) half-spectrum of vol [nz][ny][nx]: x-forward and y-forward of the
 *   one array, then a copy of scratch array 0, side array included.
 * kw_fused_angular_time_plane: vol_out [nz][ny][nx] <- the record on plane op->z: one launch k_zfused_time (lines of `kept`
 *   forward along t, H formed in registers — no operator array, no table in memory —, inverse along t into scratch array 0;
 *   divider = 1 / (nx ny nz)), the y-inverse and the storing x-inverse.  `kept` is not written.  Both: single GPU, nz > 1:
 *   KW_ERR_INVALID in slab mode or for Nz == 1.
 * kw_angular_time_mix: the twin: out_spec <- spec H on the natural [nz][ny][nx/2 + 1] half-spectrum of kw_fft_r2c_3d, out of
 *   place, for kw_fft_c2r_3d of each plane (grids off the fast path).  A context without bins: KW_OK, nothing launched.
 * kw_angular_time_embed: vol [lt][ey][ex] <- src [nt][ny][nx] in the corner, zero elsewhere.
 * kw_angular_time_reduce: p_max, p_min [ny][nx] <- max_t, min_t over t < nt of the corner of vol [lt][ey][ex]; series
 *   [nt][ny][nx] <- the corner itself.  Each output may be NULL.  Exact and deterministic (no float atomics): a block takes 16
 *   points and splits the record along t over its thread rows, so a small plane with a long record still fills the device.
 *   Both use 16-byte accesses when ex and nx are multiples of 4 and the pointers are 16-byte aligned; zero points: KW_OK.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kw_angular_time_op {   /* H of one plane */
  double dx, dy, dt, c0, z;           /* [m], [m], [s], [m/s], [m]; z >= 0 */
  const double* ak;                   /* device, nz/2 + 1 values alpha(m') k(m') log2(e); NULL = lossless */
  int32_t restriction, retarded;
} kw_angular_time_op;
KW_API kw_status kw_fused_angular_time_elems(kw_ctx* ctx, size_t* out_elems);
KW_API kw_status kw_fused_angular_time_forward(kw_ctx* ctx, const float* vol, float* kept);
KW_API kw_status kw_fused_angular_time_plane(kw_ctx* ctx, const float* kept, const kw_angular_time_op* op, float* vol_out);
KW_API kw_status kw_angular_time_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_angular_time_op* op,
                                     float divider);
KW_API kw_status kw_angular_time_embed(kw_ctx* ctx, float* vol, const float* src, uint32_t ex, uint32_t ey, uint32_t lt,
                                       uint32_t nx, uint32_t ny, uint32_t nt);
KW_API kw_status kw_angular_time_reduce(kw_ctx* ctx, const float* vol, uint32_t ex, uint32_t ey, uint32_t lt, uint32_t nx,
                                        uint32_t ny, uint32_t nt, float* p_max, float* p_min, float* series);

/* ------------------------------------------------------------------------------------------------------------------
 * k-space plane reconstruction (what k-Wave's kspacePlaneRecon computes): the record p[t][y][x] of a planar sensor to the
 * initial pressure p0[z][y][x] that produced it, homogeneous medium (csrc/kw_plane_recon.hip, host/PlaneRecon.cpp, DESIGN.md
 * "k-space plane reconstruction").  The grid of kw_set_constants is (nx, ny, nz) = (Ex, Ey, Lt), the time axis where the
 * pipeline has z.  The record is embedded, mirrored in time, in a zero volume v [Lt][Ey][Ex], Lt >= 2 Nt - 1:
 *     v[n] = p[n], 0 <= n < Nt;   v[Lt - n] = p[n], 1 <= n < Nt                     (even in t with period Lt)
 *     out = crop( positivity( 2 irfftn(G) ) )          axes (t -> z, y, x);  plane j at z_j = j c0 dt,  j < planes <= Nt
 *     S = fftn(v);  M = floor(Lt / 2);  m' = min(m, Lt - m);  bins are counted k? = 2 pi / (E? d?) * min(i, E? - i)
 *     dk = 2 pi / (Lt dt c0);  rho2 = (kx^2 + ky^2) / dk^2
 *     T[m'] = S[m'] w(m'):  w = sqrt(m'^2 - rho2) / m' where m'^2 >= rho2 and m' > 0;  w(0) = 1 if rho2 = 0;  else w = 0
 *     f = sqrt(m'^2 + rho2),  i0 = floor(f),  a = f - i0
 *     linear :  G[m] = T[i0] + a (T[min(i0 + 1, M)] - T[i0])          nearest:  G[m] = T[i0] if a < 1/2 else T[min(i0 + 1, M)]
 *     G[m] = 0 where f > M
 * The re-gridding from w to kz moves data between the bins of one (kx, ky) line; c0 enters through rho2 only.
 *
 * Per bin, TWO device functions shared by the fused kernel and the twin, without contraction into fma:
 *   float64: kx, ky from the bin counts;  kr2 = (kx*kx) + (ky*ky);  rho2 = kr2 / (dk*dk);  mm = double(m') * double(m');
 *            recon_w: d = mm - rho2, sqrt(d);   recon_f: f = sqrt(mm + rho2);   i0 = uint32(f);  f > M tested in float64
 *   float32: w = (float(sqrt(d)) / float(m')) * scale (d >= 0, m' > 0), scale (m' = 0, rho2 = 0), else 0;  scale = 2 / (Lt Ey Ex);
 *            T = (w * S.x, w * S.y);  a = float(f - double(i0));  G = (a * (T1 - T0)) + T0 per component, or the pick at a < 0.5f
 *
 * kw_fused_plane_recon: vol_out [nz][ny][nx] <- 2 irfftn(G) of vol_even [nz][ny][nx]: x-forward and y-forward of the one array,
 *   ONE launch k_zfused_recon (lines forward along t; T written back into the exchange buffer; a barrier; every bin gathers
 *   T[i0], T[i0 + 1] of its own line from LDS; inverse along t — no operator array, no index table in memory), the y-inverse
 *   and the storing x-inverse.  vol_out may be vol_even.  Single GPU, nz > 1: KW_ERR_INVALID in slab mode or for Nz == 1
 *   (2-D records: kw_fused_line_recon below).
 *   The stage does NOT check that vol_even is even in t: for a volume that is not, S[m] != S[Lt - m], the spectrum handed to
 *   the real inverse is not Hermitian and the result is not the inverse transform of G.
 * kw_plane_recon_mix: the twin: out_spec <- G on the natural [nz][ny][nx/2 + 1] half-spectrum of kw_fft_r2c_3d, out of place
 *   (it gathers), for kw_fft_c2r_3d (grids off the fast path; any nx, ny, nz, odd ones included).  A context without bins:
 *   KW_OK, nothing launched.
 * kw_plane_recon_embed: vol [lt][ey][ex] <- the mirrored embedding of src [nt][ny][nx], zero elsewhere; lt >= 2 nt - 1.
 * kw_plane_recon_crop: out [planes][ny][nx] <- the corner of vol [lt][ey][ex], planes <= lt; positivity != 0: x > 0 ? x : 0.
 *   Both exact; 16-byte accesses when ex and nx are multiples of 4 and the pointers are 16-byte aligned; zero points: KW_OK.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kw_plane_recon_op {
  double  dx, dy, dt, c0;             /* [m], [m], [s], [m/s] */
  int32_t interp;                     /* 0 = linear, 1 = nearest */
  int32_t reserved;                   /* 0 */
} kw_plane_recon_op;
KW_API kw_status kw_fused_plane_recon(kw_ctx* ctx, const float* vol_even, const kw_plane_recon_op* op, float* vol_out);
KW_API kw_status kw_plane_recon_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_plane_recon_op* op, float scale);
KW_API kw_status kw_plane_recon_embed(kw_ctx* ctx, float* vol, const float* src, uint32_t ex, uint32_t ey, uint32_t lt,
                                      uint32_t nx, uint32_t ny, uint32_t nt);
KW_API kw_status kw_plane_recon_crop(kw_ctx* ctx, float* out, const float* vol, uint32_t ex, uint32_t ey, uint32_t lt,
                                     uint32_t nx, uint32_t ny, uint32_t planes, int32_t positivity);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched k-space line reconstruction (what k-Wave's kspaceLineRecon computes, frame by frame): F records p[t][y] of a
 * linear array to the F images p0[x][y] that produced them, x_j = j c0 dt (csrc/kw_line_recon.hip, host/LineRecon.cpp,
 * DESIGN.md "k-space line reconstruction").  One frame is the plane reconstruction above with ONE lateral axis: the record
 * embedded mirrored in time in a zero plane v [Lt][Ey], S = fft2(v), and
 *     dk = 2 pi / (Lt dt c0);   ky = 2 pi / (Ey dy) * min(i, Ey - i);   rho2 = (ky * ky) / (dk * dk)          (float64)
 * with w, f, the interpolants, "G = 0 where f > M" and the float64 / float32 split exactly as documented there
 * (recon_w, recon_f, recon_scale, recon_pick: csrc/kw_recon_device.h, one copy for both operators);
 *     out = crop( positivity( 2 irfft2(G) ) ),  scale = 2 / (Lt Ey).   Frames are independent.
 *
 * Frames mode of the fused context.  kw_fused_set_frames(ctx, 1), before kw_fused_create (KW_ERR_STATE after it,
 *   KW_ERR_INVALID on a slab context): the constants (nx, ny, nz) = (Ey, Lt, F) then describe F independent planes — the
 *   sensor axis where the pipeline has x (contiguous, real-to-complex), t on y, the frame on z with NO transform along z and
 *   any F >= 1.  kw_fused_supported asks for fast-path nx and ny, the 2^32 index limits and, for the ten x lengths without
 *   masked x kernels, (ny nz) % (2 nl_x(nx)) == 0; also for nz <= 65535 (the frame is a block index) and P ny nz < 2^29
 *   (P = nx/2 + 1 rounded up to 16): the pass along t addresses a frame's lines by 32-bit byte offsets, so one scratch array
 *   ends below 4 GiB.  A frames context allocates ONE scratch array, the one its stage uses
 *   (kw_fused_create_with_scratch: s[0] alone is looked at).  The x-Nyquist side array is kept under the usual rule and is then
 *   [F][Lt].  Every other kw_fused_* stage, import and size query returns KW_ERR_INVALID on such a context ("frames mode").
 * kw_fused_line_recon: vol_out [F][Lt][Ey] <- 2 irfft2(G) of every plane of vol_even [F][Lt][Ey], three launches: the
 *   x-forward over all Lt F rows (a masked last tile where the row count asks for one), ONE launch k_yfused_line_recon
 *   (lines along t, tile position = the frame; k_zfused_recon's weight, barrier order and gather from LDS; rho2 from the
 *   column alone — no operator array, no index table) and the storing x-inverse.  No y-pass.  vol_out may be vol_even.
 *   op: kw_plane_recon_op with dx = the sensor pitch; dy is ignored.  KW_ERR_INVALID outside frames mode.  As for the plane
 *   stage, the evenness of vol_even in t is not checked.
 * kw_fft_create_plans_frames / kw_fft_r2c_frames / kw_fft_c2r_frames: nz batched 2-D real transforms of (nx, ny), natural
 *   layout [nz][ny][nx/2 + 1], any sizes; the 3-D plans are independent of them.
 * kw_line_recon_mix: the twin: out_spec <- G on those half-spectra, out of place (it gathers); any nx, ny, nz.  A context
 *   without bins: KW_OK, nothing launched.
 * kw_line_recon_embed: vol [frames][lt][ey] <- src [frames][nt][ny] mirrored along t, zero elsewhere; lt >= 2 nt - 1.
 * kw_line_recon_crop: out [frames][depth][ny] <- the corner of every plane of vol, depth <= lt; positivity as above.
 *   Both exact; 16-byte accesses when ey and ny are multiples of 4 and the pointers are 16-byte aligned; zero points: KW_OK.
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_fused_set_frames(kw_ctx* ctx, int on);
KW_API kw_status kw_fused_line_recon(kw_ctx* ctx, const float* vol_even, const kw_plane_recon_op* op, float* vol_out);
KW_API kw_status kw_fft_create_plans_frames(kw_ctx* ctx);
KW_API kw_status kw_fft_r2c_frames(kw_ctx* ctx, const float* in, float* out);
KW_API kw_status kw_fft_c2r_frames(kw_ctx* ctx, float* in, float* out);
KW_API kw_status kw_line_recon_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_plane_recon_op* op, float scale);
KW_API kw_status kw_line_recon_embed(kw_ctx* ctx, float* vol, const float* src, uint32_t ey, uint32_t lt, uint32_t frames,
                                     uint32_t ny, uint32_t nt);
KW_API kw_status kw_line_recon_crop(kw_ctx* ctx, float* out, const float* vol, uint32_t ey, uint32_t lt, uint32_t frames,
                                    uint32_t ny, uint32_t depth, int32_t positivity);

/* ------------------------------------------------------------------------------------------------------------------
 * Exact k-space propagator (what k-Wave's kspaceSecondOrder computes): an initial pressure p0[z][y][x] in a homogeneous
 * medium, lossless or power-law absorbing, to the pressure at any time t >= 0 with no time loop (csrc/kw_second_order.hip,
 * host/SecondOrder.cpp, DESIGN.md "Exact k-space propagator").  The grid of kw_set_constants is (nx, ny, nz) =
 * (Ex, Ey, Ez), the expanded periodic grid into whose corner p0 is embedded.
 *     p(., ., .; t) = irfftn( rfftn(p0 embedded) H(|k|; t) ),   |k|^2 = (kx^2 + ky^2) + kz^2         axes (z, y, x)
 *     bins are counted k? = 2 pi / (n? d?) * min(i, n? - i)
 *     lossless:  H = cos(c0 |k| t)
 *     absorbing: per mode p'' + 2 gamma p' + Omega^2 p = 0, p(0) = P0, p'(0) = 0 — the equation that the time loop's
 *                equation of state (absorb_tau on -d rho/dt, absorb_eta subtracted) gives for a homogeneous medium;
 *                a = alpha_coeff 100 (1e-6 / 2 pi)^y / (20 log10 e)  [Np (rad/s)^-y m^-1], converted on the host
 *       g = a c0^y |k|^(y-1)    T = tan(pi y / 2) (0 for y = 2)    B = 1 - 2 g T - g^2    r = sqrt(B)
 *       gamma = c0 |k| g        w_d = c0 |k| r
 *       H = exp(-gamma t) (cos(w_d t) + (g / r) sin(w_d t));    |k| = 0: H = 1
 *     Underdamped modes only: the caller keeps B >= 1/4 on every bin (SecondOrderParameters refuses alpha_coeff otherwise).
 * H is real and depends on |k| only, so the half-spectrum stays Hermitian and one real array is enough.
 *
 * H per bin is ONE device function (second_h) for the fused kernel and the twin, without contraction into fma:
 *   float64: kx, ky, kz from the bin counts;  kr2 = (kx*kx) + (ky*ky);  k2 = kr2 + (kz*kz);  k = sqrt(k2);  k2 == 0: H = divider
 *            absorbing: s = k (y = 2), sqrt(k) (y = 1.5) or pow(k, y - 1);  g = ac * s with ac = a c0^y from the host;
 *                       B = (1 - (twoT * g)) - (g*g) with twoT = 2 T from the host;  r = sqrt(B);  lossless: r = 1
 *            turns = ((k * r) * ct) / 2 pi with ct = c0 * t from the host;  word = uint32(rint((turns - floor(turns)) * 2^32))
 *   float32: angle = float(int32(word)) * (2 pi 2^-32), one sincosf (cosf when lossless; the hardware sine is not used);
 *            absorbing: E = exp2f(-float(((k * g) * ct) * log2(e)));  q = float(g / r);  H = (E * (cos + (q * sin))) * divider
 *            lossless:  H = cos * divider;        out = (H * x.x, H * x.y)
 *   |k|^(y-1) is evaluated once, in float64, for the phase and for E alike.  A float32 product c0 |k| t would be several
 *   1e-3 rad off at 10^4 turns; the phase word is exact to 2^-33 turns.
 *
 * kw_fused_second_order_elems: complex values of one scratch array = the size of `kept`.
 * kw_fused_second_order_forward: kept <- the (kx, ky, z) half-spectrum of vol [nz][ny][nx]: x-forward and y-forward, then a
 *   copy of scratch array 0, side array included — kw_fused_angular_time_forward's operation, one implementation.
 * kw_fused_second_order_time: vol_out [nz][ny][nx] <- the pressure at op->t: one launch k_zfused_second_order (lines of
 *   `kept` forward along z, H formed in registers from the column, the row and the bin m — no operator array, no table in
 *   memory —, inverse along z into scratch array 0; divider = 1 / (nx ny nz)), the y-inverse and the storing x-inverse.
 *   `kept` is not written.  Both: single GPU, nz > 1: KW_ERR_INVALID in slab mode, for Nz == 1 and on a frames context
 *   (kw_fused_second_order_frames_* are that context's entries).
 * kw_second_order_mix: the twin: out_spec <- spec H on the natural [nz][ny][nx/2 + 1] half-spectrum of kw_fft_r2c_3d, out
 *   of place, for kw_fft_c2r_3d (grids off the fast path; any nx, ny, nz, odd ones included).  A context without bins:
 *   KW_OK, nothing launched.
 * Embedding and crop: kw_angular_time_embed and kw_plane_recon_crop (a 3-D corner either way).  Sensor records and the
 * aggregates over the output times: kw_sample_index and kw_sample_all on the volume and on the crop.
 *
 * dp0/dt as a second initial condition (csrc/kw_second_order_pair.hip; k-Wave's source.dp0dt): p(0) = P0, p'(0) = V0 with
 * V0 = F{dp0dt embedded} [Pa/s], the same per-mode equation:
 *     p^(t) = Hc(|k|; t) P0 + Hs(|k|; t) V0          Hc = the H above
 *     lossless:  Hs = sin(c0 |k| t) / (c0 |k|)       absorbing: Hs = exp(-gamma t) sin(w_d t) / w_d       |k| = 0: Hs = t
 * Hs [s] is real and depends on |k| only.  (Hc, Hs) per bin is ONE device function (second_h_pair) for the fused passes and
 * the twins: second_h's float64 expressions in its order up to the phase word, ONE sincosf of the word's angle for both,
 *   float64: w = c0 * k (lossless), (c0 * k) * r (absorbing)
 *   float32: Hc = (E * (cos + (q * sin))) * divider;  Hs = ((E * sin) * float(1.0 / w)) * divider;  E = 1, q = 0 lossless
 *            k2 == 0: (divider, float(t) * divider);   out = ((Hc * x.x) + (Hs * y.x), (Hc * x.y) + (Hs * y.y))
 * kw_fused_second_order_time_pair: vol_out <- the pressure at op->t from kept_p and kept_v, each a kept spectrum of
 *   kw_fused_second_order_forward in an array of kw_fused_second_order_elems values: one launch
 *   k_zfused_second_order_pair (lines of both forward along z, the second one's requested while the first is transformed,
 *   the mix in registers, ONE inverse along z into scratch array 0), then the y-inverse and the storing x-inverse of
 *   kw_fused_second_order_time.  Neither kept array is written.  Its refusals are kw_fused_second_order_time's.
 * kw_second_order_mix_pair: the twin: out_spec <- Hc spec_p + Hs spec_v on the natural half-spectra, out of place
 *   (out_spec is neither input), any sizes.  A context without bins: KW_OK, nothing launched.
 * kw_fused_second_order_time and kw_second_order_mix are what they were: without dp0dt nothing else is launched.
 *
 * Not built: time-varying sources, heterogeneous media, Z-slabs, several output
 * times per z-pass, inverse passes restricted to the crop or to the sensor points, particle velocity.  (2-D: the batched
 * form on a frames context, below.)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kw_second_order_op {   /* H of one time */
  double  dx, dy, dz, c0, t;          /* [m], [m], [m], [m/s], [s]; t >= 0 */
  double  a, alpha_power;             /* a [Np (rad/s)^-y m^-1] and y; read when absorbing != 0 */
  int32_t absorbing;                  /* 0 = lossless */
  int32_t reserved;                   /* 0 */
} kw_second_order_op;
KW_API kw_status kw_fused_second_order_elems(kw_ctx* ctx, size_t* out_elems);
KW_API kw_status kw_fused_second_order_forward(kw_ctx* ctx, const float* vol, float* kept);
KW_API kw_status kw_fused_second_order_time(kw_ctx* ctx, const float* kept, const kw_second_order_op* op, float* vol_out);
KW_API kw_status kw_second_order_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_second_order_op* op,
                                     float divider);
KW_API kw_status kw_fused_second_order_time_pair(kw_ctx* ctx, const float* kept_p, const float* kept_v,
                                                 const kw_second_order_op* op, float* vol_out);
KW_API kw_status kw_second_order_mix_pair(kw_ctx* ctx, float* out_spec, const float* spec_p, const float* spec_v,
                                          const kw_second_order_op* op, float divider);

/* ------------------------------------------------------------------------------------------------------------------
 * Exact k-space propagator on frames: the batched 2-D form of the operator above (csrc/kw_second_order.hip,
 * host/SecondOrderFrames.cpp, DESIGN.md "Exact k-space propagator on frames").  F independent planes p0[f][y][x] that
 * share c0, the absorption and the output times; the grid of kw_set_constants is (nx, ny, nz) = (Ex, Ey, F), the fused
 * pipeline a frames context (kw_fused_set_frames): no transform along z.  One frame is the 3-D operator with the z axis
 * removed:
 *     p_f(., .; t) = crop( irfft2( rfft2(p0_f embedded in Ey x Ex) H(|k|; t) ) ),   |k|^2 = (kx*kx) + (ky*ky)
 *     bins are counted k? = 2 pi / (E? d?) * min(i, E? - i)
 * H is the H above, formed by the same device function (second_h) in the fused pass and in the twin: the bin along y
 * stands where the z bin does (dkz, ez := 2 pi / (Ey dy), Ey), kr2 = (kx*kx) of the column in float64 without contraction,
 * k2 = kr2 + (ky*ky), divider = 1 / (Ex Ey).  op is kw_second_order_op; dz is not looked at, the other validations are the
 * 3-D entries'.
 *
 * kw_fused_second_order_frames_elems: complex values of `kept` = one scratch array of the frames context: P Ey F and the
 *   x-Nyquist side array [F][Ey].
 * kw_fused_second_order_frames_forward: kept <- the (kx, y, frame) half-spectrum of vol [F][Ey][Ex]: the x-forward over
 *   all Ey F rows (a masked last tile where the row count asks for one), then a copy of scratch array 0, side array included.
 * kw_fused_second_order_frames_time: vol_out [F][Ey][Ex] <- every frame's pressure at op->t: ONE launch
 *   k_yfused_second_order (tile position = the frame; lines of `kept` forward along y, H formed in registers from the
 *   column and the bin — nothing read from memory for it —, inverse along y into scratch array 0; the side array's blocks
 *   take the column Ex/2 at NL frames each, those past the last frame store nothing) and the storing x-inverse.  `kept` is
 *   not written.
 * The three return KW_ERR_STATE before kw_fused_create and KW_ERR_INVALID outside frames mode (3-D, 2-D and slab
 * contexts); kw_fused_second_order_elems / _forward / _time keep refusing frames contexts.  kw_fused_supported's rules
 * for a frames context hold (at most 65535 frames, the scratch array below 2^29 complex values).
 * kw_second_order_frames_mix: the twin: out_spec <- spec H on the natural [F][Ey][Ex/2 + 1] half-spectra of
 *   kw_fft_r2c_frames, out of place, for kw_fft_c2r_frames; any sizes, odd ones included.  A context without bins: KW_OK,
 *   nothing launched.
 * Embedding and crop: kw_angular_time_embed and kw_plane_recon_crop with the frame count in the slowest position.  The
 * record: kw_sample_index on the expanded batch; the aggregates: kw_sample_all on the crop.
 * dp0/dt as a second initial condition: the 3-D section's operator and device function (second_h_pair), the bin along y
 * where the z bin stands.
 * kw_fused_second_order_frames_time_pair: vol_out <- every frame's pressure at op->t from kept_p and kept_v (each from
 *   kw_fused_second_order_frames_forward, kw_fused_second_order_frames_elems values): ONE launch k_yfused_second_order_pair
 *   (k_yfused_second_order's tiles and side blocks; both spectra forward along y, the mix in registers, ONE inverse) and the
 *   storing x-inverse.  Neither kept array is written.  KW_ERR_STATE before kw_fused_create, KW_ERR_INVALID outside frames
 *   mode, as kw_fused_second_order_frames_time.
 * kw_second_order_frames_mix_pair: the twin on the natural spectra [F][Ey][Ex/2 + 1], out of place, any sizes.  A context
 *   without bins: KW_OK, nothing launched.
 * Not built: dp0/dt in the line-sensor record below, time-varying sources, heterogeneous media, chunks of frames and
 * frames over several GPUs, particle velocity.  Several output times per pass and an x-inverse restricted to the rows that
 * hold sensors: served for a single row by the line-sensor record below, not otherwise.
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_fused_second_order_frames_elems(kw_ctx* ctx, size_t* out_elems);
KW_API kw_status kw_fused_second_order_frames_forward(kw_ctx* ctx, const float* vol, float* kept);
KW_API kw_status kw_fused_second_order_frames_time(kw_ctx* ctx, const float* kept, const kw_second_order_op* op,
                                                   float* vol_out);
KW_API kw_status kw_second_order_frames_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_second_order_op* op,
                                            float divider);
KW_API kw_status kw_fused_second_order_frames_time_pair(kw_ctx* ctx, const float* kept_p, const float* kept_v,
                                                        const kw_second_order_op* op, float* vol_out);
KW_API kw_status kw_second_order_frames_mix_pair(kw_ctx* ctx, float* out_spec, const float* spec_p, const float* spec_v,
                                                 const kw_second_order_op* op, float divider);

/* ------------------------------------------------------------------------------------------------------------------
 * Line-sensor record of the propagator on frames: what the row y = r dy of every frame records at many output times, with
 * no y-inverse and no x-inverse over the plane (csrc/kw_second_order_line.hip, host/SecondOrderFrames.cpp, DESIGN.md
 * "Line-sensor record of the propagator on frames").  Any context with constants (nx, ny, nz) = (Ex, Ey, F), any sizes,
 * odd ones included; the fused pipeline plays no part.
 *     p_f(x, y_r; t) = irfft_x[ G_f(kx; t) ],  kx = 0 ... Ex/2
 *     G_f(kx; t)     = sum over m = 0 ... Ey/2 of H(kx, m; t) Q_f(kx, m)
 *     Q_f(kx, m)     = q_f(kx, m) + q_f(kx, Ey - m);  bins 0 and (Ey even) Ey/2 pair with themselves: q_f(kx, m) alone
 *     q_f(kx, ky)    = rfft2(p0_f embedded)(kx, ky) exp(+2 pi i ky r / Ey) / (Ex Ey)
 * H is the H of the section above, which depends on ky through min(ky, Ey - ky) only.
 *
 * kw_second_order_line_elems: complex values of Q: (Ex/2 + 1) (Ey/2 + 1) F.
 * kw_second_order_line_prepare: q [Ex/2 + 1][Ey/2 + 1][F] <- the natural [F][Ey][Ex/2 + 1] spectra of kw_fft_r2c_frames.
 *   The phase of bin ky: the integer (ky r) mod Ey exactly, angle = 2 pi (that / Ey) and its cosine and sine in float64,
 *   each rounded to float32 once; q = ((X * phase) * divider) in float32 without contraction, divider = float(1 / (Ex Ey));
 *   the fold adds the two terms.  row < Ey; Ey/2 + 1 <= 65535 (a block index).
 * kw_second_order_line_record: g [F][n_times][Ex/2 + 1] (float2) <- Q, op (op->t is not looked at, op->dz neither) and the
 *   DEVICE array times [n_times] of float64 seconds, each >= 0 and finite (the caller checks them; the kernel reads no
 *   other memory by them), in any order.  ct = c0 * t in float64; per bin second_h's float64 expressions in its order —
 *   ((k * r) * ct) / 2 pi to the phase word, ((k * g) * ct) * log2(e), g / r, the three power paths, H = 1 at k = 0, no
 *   contraction — with the factors that do not depend on time formed once per bin and block (no table in memory).
 *   An accumulator takes its bins in ascending m, one fmaf(H, Q, acc) each, from zero: the bits of G_f(kx; t) do not depend
 *   on F, on the other times of the call or on n_times.  No atomics; nothing of size Ex Ey n_times exists.
 *   1 <= n_times <= 65535 * 256.
 * The x-inverse: kw_fft_c2r_frames on a context with constants (Ex, 1, F n_times) (a batched 1-D plan), then
 * kw_plane_recon_crop of Ex to Nx.
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_second_order_line_elems(kw_ctx* ctx, size_t* out_elems);
KW_API kw_status kw_second_order_line_prepare(kw_ctx* ctx, float* q, const float* spec, uint32_t row);
KW_API kw_status kw_second_order_line_record(kw_ctx* ctx, float* g, const float* q, const kw_second_order_op* op,
                                             const double* times, uint32_t n_times);

/* ------------------------------------------------------------------------------------------------------------------
 * Plane-sensor record of the 3-D propagator: what the plane z = r dz of the volume records at many output times, with no
 * inverse along z and no 3-D round trip per time (csrc/kw_second_order_plane.hip, host/SecondOrder.cpp, DESIGN.md
 * "Plane-sensor record of the propagator").  Any context with constants (nx, ny, nz) = (Ex, Ey, Ez), any sizes, odd ones
 * included; the fused pipeline plays no part.
 *     p(x, y, z_r; t) = irfft2_xy[ G(kx, ky; t) ],  kx = 0 ... Ex/2, ky = 0 ... Ey - 1
 *     G(kx, ky; t)    = sum over m = 0 ... Ez/2 of H(kx, ky, m; t) Q(kx, ky, m)
 *     Q(kx, ky, m)    = q(kx, ky, m) + q(kx, ky, Ez - m);  bins 0 and (Ez even) Ez/2 pair with themselves: q(kx, ky, m) alone
 *     q(kx, ky, kz)   = rfftn(p0 embedded)(kx, ky, kz) exp(+2 pi i kz r / Ez) / (Ex Ey Ez)
 * H is the H of "Exact k-space propagator", which depends on kz through min(kz, Ez - kz) and on ky through min(ky, Ey - ky).
 *
 * kw_second_order_plane_elems: complex values of Q: Ey (Ex/2 + 1) (Ez/2 + 1).
 * kw_second_order_plane_prepare: q [Ey][Ex/2 + 1][Ez/2 + 1] (m fastest) <- the natural [Ez][Ey][Ex/2 + 1] spectrum of
 *   kw_fft_r2c_3d, which is read only.  The phase of bin kz: the integer (kz r) mod Ez exactly, angle = 2 pi (that / Ez) and
 *   its cosine and sine in float64, each rounded to float32 once; q = ((X * phase) * divider) in float32 without
 *   contraction, divider = float(1 / (Ex Ey Ez)); the fold adds the two terms.  plane < Ez; q != spec; Ey <= 65535 and
 *   (Ez/2 + 1) / 32 <= 65535 (block indices).
 * kw_second_order_plane_record: g [n_times][Ey][Ex/2 + 1] (float2: the half-spectrum layout of kw_fft_c2r_frames on a context
 *   (Ex, Ey, n_times)) <- Q, op (op->t is not looked at) and the DEVICE array times [n_times] of float64 seconds, each >= 0
 *   and finite (the caller checks them; the kernel reads no other memory by them), in any order.  A block of k_plane_record
 *   owns 4 consecutive kx columns, the rows ky and Ey - ky (0 and, Ey even, Ey/2 stand alone) and 256 times; per bin the
 *   expressions of kw_second_order_line_record with kr2 = kx^2 + ky^2 as the z-pass forms it, one H for both rows.
 *   An accumulator takes its bins in ascending m, one fmaf(H, Q, acc) each, from zero: the bits of G(kx, ky; t) do not depend
 *   on the tile, on the other times of the call or on n_times.  No atomics; nothing of size Ex Ey Ez n_times exists.
 *   1 <= n_times <= 65535 * 256; g != q.
 * The inverse over the record: kw_fft_c2r_frames on a context with constants (Ex, Ey, n_times), then kw_plane_recon_crop of
 * (Ex, Ey) to (Nx, Ny).
 * ---------------------------------------------------------------------------------------------------------------- */
KW_API kw_status kw_second_order_plane_elems(kw_ctx* ctx, size_t* out_elems);
KW_API kw_status kw_second_order_plane_prepare(kw_ctx* ctx, float* q, const float* spec, uint32_t plane);
KW_API kw_status kw_second_order_plane_record(kw_ctx* ctx, float* g, const float* q, const kw_second_order_op* op,
                                              const double* times, uint32_t n_times);

#ifdef __cplusplus
}
#endif
#endif /* KWAVE_HIP_H */
