/*
 * kwave_host.h — C entry points of the C++ host layer (libkwave_host.so).
 *
 * The host layer is the MI355X build's mirror of the reference's caller side of the hot path:
 * Parameters / MatrixContainer / KSpaceFirstOrderSolver / OutputStreamContainer (k-wave-fluid-cuda_amd/host/).
 * These entry points exist so that non-C++ drivers (bench.py, pytest via ctypes) can run the *same* C++ time loop
 * the command-line program runs — they correspond to main()'s sequence in the reference (main.cpp:840-966):
 *   kwh_create   = Parameters::init + selectDevice + allocateMemory + loadInputData   (main.cpp:857-917)
 *   kwh_run      = the body of computeMainLoop for n steps                            (KSpaceFirstOrderSolver.cpp:885-935)
 *   kwh_finish   = last delayed flush + postProcessing                                (:937-942, :950-1053)
 * Input datasets are named exactly like the HDF5 input file's datasets (Utils/MatrixNames.h, main.cpp:446-563).
 */
#ifndef KWAVE_HOST_H
#define KWAVE_HOST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KWH_API __attribute__((visibility("default")))

typedef struct kwh_solver kwh_solver;

typedef struct kwh_dataset
{
  const char* name;     /* HDF5 dataset name, e.g. "c0", "ddx_k_shift_pos_r", "sensor_mask_index" */
  const void* data;     /* host pointer: float32 or uint64 */
  int32_t     dtype;    /* 0 = float ("float"), 1 = uint64 ("long") */
  int32_t     pad_;
  uint64_t    nx, ny, nz; /* (x,y,z) sizes = HDF5 dims reversed; complex datasets have the doubled x size halved here */
} kwh_dataset;

/* Weighted pressure source (new with this build; k-Wave's kWaveArray): instead of p_source_input, the datasets
 *   p_source_element_input  float  (1, p_source_flag, E)  one signal per element
 *   p_source_element_ptr    uint64 (1, 1, Npts + 1)       0-based CSR offsets, row k = point k of p_source_index
 *   p_source_element_index  uint64 (1, 1, nnz)            1-based element number of each entry
 *   p_source_element_weight float  (1, 1, nnz)            weight of each entry
 * make point k receive v_k(t) = sum_j weight_j * signal[t][element_j] (fp32 fma in CSR order); p_source_mode then applies
 * as to a p_source_many = 1 source with series row t = v(t).  p_source_input must be absent and p_source_many, if
 * given, 1.  kwh_create checks every CSR (offsets, counts, element and grid index ranges) and names the dataset.
 *
 * Weighted velocity source: the same for ux / uy / uz.  The components share u_source_index and therefore one CSR:
 *   u_source_element_ptr / _index / _weight   as p_source_element_*, row k = point k of u_source_index
 *   ux_ / uy_ / uz_source_element_input float (1, u?_source_flag, E)  one signal per element, per component
 * A component is active when its flag is above 0; the active components are all weighted or all plain, share E, and
 * may have different flags (a component stops when its own flag runs out).  u?_source_input must be absent,
 * u_source_many, if given, 1, and transducer_source_flag 0.  u_source_mode applies as to a u_source_many = 1 source.
 *
 * Per-entry time delays (optional; absent = all 0 and the undelayed kernels run), uint64 (1, 1, nnz), in time steps, one
 * value per entry of the CSR beside it, at most KW_ELEMENT_MAX_DELAY (kwave_hip.h):
 *   p_source_element_delay  point k receives v_k(t) = sum_j weight_j * signal[t - delay_j][element_j]; an entry is left
 *                           out while t < delay_j or once t - delay_j >= p_source_flag.  The source acts while
 *                           t < p_source_flag + the largest delay (capped by Nt).
 *   u_source_element_delay  the same for u_source_element_*, shared by the components; each component acts for its own
 *                           flag + the largest delay.
 *   sensor_element_delay    for sensor_element_* (p_elements, u*_elements, u*_non_staggered_elements alike):
 *                           out[t][e] = sum_j weight_j * field^(t - delay_j)[index_j] for t >= s, the sampling start; terms
 *                           with t - delay_j < s are dropped.  The entries of an element are regrouped by delay (stably)
 *                           and the group sums travel through a ring of (largest delay + 1) rows of E floats per field
 *                           (kw_sample_elements_delayed), which is part of the stream's checkpoint state ("Temp_<stream>"
 *                           in the reference-layout checkpoint file, behind the series in the file-less form).
 * kwh_create refuses, naming the dataset, a delay dataset whose length differs from its CSR's entry count, a delay above
 * the maximum, and a delay dataset without its CSR.  A slab rank's input may also hold the scalars
 * p_source_element_delay_max / u_source_element_delay_max (uint64): the largest delay of the whole array, not below the
 * rank's own, so that all ranks keep the source active for the same steps (dist.partition_problem writes them).  They are
 * read wherever they are present: in the input of a single-GPU run they lengthen the source's window in the same way (the
 * extra steps add rows of zeros), so leave them out there. */

/* what the reference takes from the command line for the loop (CommandLineParameters.cpp:264-292) */
typedef struct kwh_options
{
  int32_t  device_idx;                 /* -g ; <0 = first free */
  int32_t  fused_kernels;              /* 1: MI355X fused step kernels, 0: one launch per reference kernel */
  uint64_t sampling_start_time_index;  /* -s (0-based) */
  uint64_t benchmark_time_steps;       /* --benchmark (0 = use Nt) */
  int32_t  p_raw, p_rms, p_max, p_min, p_max_all, p_min_all, p_final;
  int32_t  u_raw, u_rms, u_max, u_min, u_max_all, u_min_all, u_final, u_non_staggered_raw;
  int32_t  p_c, u_non_staggered_c, i_avg_c, no_overlap;
  float    period;
  uint64_t mos, harmonics;
  /* Z-slab decomposition (one process per GPU).  With slab_ranks > 1 the datasets describe this rank's slab: "Nz" is
   * the local plane count, 3-D arrays / pml_z / pml_z_sgz are the local slices, source and sensor indices are local
   * (re-based, 1-based) indices; ddz_* stay global.  The all-to-all is the device library's RCCL path (comm_unique_id
   * below) unless exchange_fn (kw_exchange_fn of kwave_hip.h) overrides it. */
  uint64_t slab_ranks, slab_rank, nz_global;
  void*    exchange_fn;
  void*    exchange_user;
  void*    exchange_start_fn; /* optional kw_exchange_start_fn / kw_exchange_wait_fn pair (both or neither) */
  void*    exchange_wait_fn;
  void*    scratch[6]; /* optional caller-owned pipeline scratch (kw_fused_create_with_scratch), else all NULL */
  /* post-processed quantities (--I_avg, --Q_term, --Q_term_c; KSpaceFirstOrderSolver.cpp:977-1024): time-averaged
   * intensity from the stored p / u_non_staggered series, and Q = -div(I_avg) from it or from the compressed one */
  int32_t  i_avg, q_term, q_term_c;
  int32_t  u_c;        /* --u_c: compression coefficients of the staggered velocities (OutputStreamContainer.cpp:133-142) */
  float    frequency;  /* --frequency [Hz]: period = 1 / (frequency * dt) (Parameters.cpp:468-480); not together with period */
  int32_t  only_post_processing; /* --post: no time loop; I_avg / I_avg_c / Q_term / Q_term_c from the series stored in an
                                    existing output file (KSpaceFirstOrderSolver.cpp:373-415; kwh_post_process_output_file) */
  /* slab runs over the library's own RCCL path (the default multi-GPU exchange): KW_COMM_ID_BYTES bytes from
   * kw_comm_unique_id() on rank 0, the same on every rank; exchange_fn / exchange_start_fn must then be NULL.
   * With slab_ranks == 1 the rank exchanges with itself (rehearsal of the multi-GPU path on one GPU). */
  const void* comm_unique_id;
  int32_t  complex_40bit; /* --40-bit_complex: compression coefficients kept and stored as 5-byte complex numbers
                             (CompressHelper.cpp:224-389; BaseOutputStream.cpp:98-101: c_complex_size 1.25) */
  int32_t  reserved_;
  void*    exchange_piece_fn; /* optional kw_exchange_piece_fn (strided pieces; exchange_wait_fn, if set, is its wait):
                                 a caller-owned transport that lets the pipeline run its pipelined slab schedule.
                                 Give exchange_fn as well (used when the pipeline is told not to pipeline). */
  const void* tuning;         /* optional const kw_tuning* (kwave_hip.h): schedule parameters of the device library */
  int32_t  step_graph;        /* 1: replay the steady-state step from a recorded graph (launch-bound small grids; measured
                                 3-5 % slower than eager launches at 64^3 / 128^3, hence off by default) */
  int32_t  comm_p2p;          /* 1: slab exchange over the device library's P2P transport (kw_comm_init_p2p: mapped peer
                                 buffers, one store kernel per exchange) instead of RCCL groups; needs comm_allgather_fn.
                                 With comm_unique_id as well, the RCCL communicator is created first and stays behind it. */
  void*    comm_allgather_fn; /* kwh_allgather_fn: how the ranks trade their kw_comm_p2p_export blobs */
  void*    comm_allgather_user;
  const char* rccl_library;   /* optional library name / path for the RCCL binding (kw_comm_init_with); NULL = default */
  float    p2p_emulate_link_gbs;   /* > 0 with comm_p2p: link model instead of peers (kw_comm_p2p_emulate; schedule studies */
  float    p2p_emulate_latency_us; /*   with ONE rank of slab_ranks on a one-GPU machine, tools/emulate_rank.py) */
  int32_t  p_elements;        /* --p_elements: weighted sensor, stream "p_elements" of (Nt - s) rows of E values,
                                 p_elements[t][e] = sum_j sensor_element_weight[j] * p[sensor_element_index[j]] over row e
                                 of the CSR (sensor_element_ptr: E + 1 0-based offsets; sensor_element_index: 1-based
                                 linear grid indices).  Independent of sensor_mask_*.  Without the three datasets,
                                 kwh_create fails. */
  int32_t  u_elements;        /* --u_elements: the same weighted sensor over the staggered velocities: streams "ux_elements",
                                 "uy_elements" and (3-D) "uz_elements", each (Nt - s) rows of E values; the components are
                                 reduced together, one read of the CSR per step (kw_sample_elements_multi) */
  int32_t  u_non_staggered_elements; /* --u_non_staggered_elements: the same over the velocities shifted to the pressure
                                 grid (as --u_non_staggered_raw samples them): "ux_non_staggered_elements", ... */
} kwh_options;
/* gathers `bytes` bytes of every rank, in rank order, into all (nranks * bytes); the same result on every rank; 0 = ok.
 * Any transport the launcher has will do: MPI_Allgather, torch.distributed.all_gather on a gloo group, files. */
typedef int (*kwh_allgather_fn)(void* user, const void* mine, void* all, size_t bytes);

KWH_API const char* kwh_last_error(void);
KWH_API int      kwh_create(const kwh_dataset* datasets, size_t n_datasets, const kwh_options* options, kwh_solver** out);
KWH_API int      kwh_destroy(kwh_solver* s);
KWH_API int      kwh_run(kwh_solver* s, uint64_t n_steps);
KWH_API int      kwh_finish(kwh_solver* s);
KWH_API int      kwh_sync(kwh_solver* s);
KWH_API uint64_t kwh_time_index(const kwh_solver* s);
/* the underlying kw_ctx* (include/kwave_hip.h) — for HIP-event timing on the solver's stream */
KWH_API void*    kwh_context(kwh_solver* s);
/* copy a matrix (by reference name: "p","ux_sgx","rhox","kappa_r","absorb_tau", "c0" (= c^2 after pre-processing) ...)
 * from the device into dst; n = number of floats expected (checked) */
KWH_API int      kwh_get_matrix(kwh_solver* s, const char* name, float* dst, uint64_t n);
KWH_API int      kwh_matrix_size(kwh_solver* s, const char* name, uint64_t* n_floats);
/* scalar parameters computed by pre-processing: "absorb_tau","absorb_eta","c2","dt_rho0_sgx",...;
 * "fused_pipeline" = 1 when the grid runs on the hand-written FFT pipeline, 0 on the rocFFT path */
KWH_API int      kwh_get_scalar(kwh_solver* s, const char* name, float* out);
/* output streams by dataset name ("p","p_max","ux",...): size = points per step, steps = stored steps (1 for aggregates) */
KWH_API int      kwh_stream_info(kwh_solver* s, const char* name, uint64_t* size, uint64_t* steps);
KWH_API int      kwh_stream_read(kwh_solver* s, const char* name, float* dst, uint64_t n);
/* Checkpoint / restart (KSpaceFirstOrderSolver.cpp:1176-1224 save, :186-228 recover; MatrixContainer.cpp:504-537): the
 * state of a run is the seven arrays p, rhox, rhoy, rhoz, ux_sgx, uy_sgy, uz_sgz, the time index and the state of every
 * output stream.  These calls move that state in and out of a prepared solver; the HDF5 checkpoint file itself is
 * written by kwh_checkpoint_write / read by kwh_checkpoint_read (libkwave_host_h5.so). */
/* Compression helpers of the reference that run on the host (Compression/CompressHelper.cpp:146-216 findPeriod,
 * :298-389 convertFloatCTo40b, :224-289 convert40bToFloatC; exponent bias e = 138 pressure / 114 velocity).  The
 * solver uses findPeriod itself when compression streams are requested without a period (Parameters.cpp:488-512). */
KWH_API int      kwh_find_period(const float* signal, uint64_t length, float* period);
KWH_API int      kwh_pack_complex_40b(const float* re_im_pairs, uint64_t n, uint8_t* packed5n, int32_t e);
KWH_API int      kwh_unpack_complex_40b(const uint8_t* packed5n, uint64_t n, float* re_im_pairs, int32_t e);
KWH_API int      kwh_set_matrix(kwh_solver* s, const char* name, const float* src, uint64_t n);
KWH_API int      kwh_set_time_index(kwh_solver* s, uint64_t t_index);
KWH_API int      kwh_stream_count(kwh_solver* s, uint64_t* n);
KWH_API int      kwh_stream_name(kwh_solver* s, uint64_t i, char* out, uint64_t cap);
/* the same including the streams that only feed others and are not part of the output (the coefficient series behind
 * --I_avg_c / --Q_term_c alone, the intensities behind --Q_term alone): a checkpoint has to carry those too */
KWH_API int      kwh_stream_count_all(kwh_solver* s, uint64_t* n);
KWH_API int      kwh_stream_name_all(kwh_solver* s, uint64_t i, char* out, uint64_t cap);
/* dst == NULL: only the sizes are returned */
KWH_API int      kwh_stream_checkpoint(kwh_solver* s, const char* name, float* dst, uint64_t cap, uint64_t* n_floats,
                                       uint64_t* sampled_steps);
KWH_API int      kwh_stream_restore(kwh_solver* s, const char* name, const float* src, uint64_t n_floats,
                                    uint64_t sampled_steps);


/* ------------------------------------------------------------------------------------------------------------------
 * Bioheat solver (new with this build; what k-Wave's kWaveDiffusion computes): explicit k-space time stepping of the
 * Pennes equation  rho C dT/dt = div(K grad T) - rho_b C_b W_b (T - T_a) + Q  on a periodic 3-D grid (no PML), with the
 * CEM43 thermal dose accumulated on the GPU — the consumer of the acoustic solver's Q_term / Q_term_c.  A thermal solver
 * owns its own device context; acoustic and thermal solvers can share a process.  The scheme is in DESIGN.md.
 * Datasets (float unless noted; every medium dataset is a scalar or an Nx * Ny * Nz array):
 *   Nx Ny Nz (uint64), dx dy dz dt                  required; Nz == 1 (2-D) is refused
 *   T0                                              initial temperature [degC]
 *   thermal_conductivity, density, specific_heat    K [W/(m K)], rho [kg/m^3], C [J/(kg K)]; a scalar K selects the
 *                                                   Laplacian form of the diffusion term, an array the flux form
 *   thermal_conductivity_sgx / _sgy / _sgz          optional (all or none, arrays): K on the staggered grids; default: the
 *                                                   mean of each point and its +1 neighbour, the last point its own value
 *   blood_density, blood_specific_heat, blood_perfusion_rate, blood_ambient_temperature     all four or none, or
 *   perfusion_coeff [1/s] with blood_ambient_temperature
 *   Q                                               optional: volume rate of heat deposition [W/m^3]
 *   diffusion_coeff_ref                             optional: reference diffusivity of the k-space correction (default
 *                                                   max K / (rho C))
 *   sensor_mask_index (uint64, 1-based)             optional: T at those points after every step, stream "T_raw"
 * Of kwh_options the call reads device_idx, fused_kernels (1: the hand-written FFT pipeline where the grid is supported,
 * rocFFT elsewhere; 0: rocFFT); slab_ranks > 1 is refused.  A refusal names the dataset.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kwh_thermal kwh_thermal;
KWH_API int      kwh_thermal_create(const kwh_dataset* datasets, size_t n_datasets, const kwh_options* options, kwh_thermal** out);
KWH_API int      kwh_thermal_destroy(kwh_thermal* s);
/* n_steps steps; heat_on == 0 leaves Q out (cooling) */
KWH_API int      kwh_thermal_run(kwh_thermal* s, uint64_t n_steps, int heat_on);
KWH_API uint64_t kwh_thermal_time_index(const kwh_thermal* s);
/* "T", "cem43" [equivalent minutes at 43 degC], "T_max", "Q"; n = Nx * Ny * Nz (checked).  Setting "Q" on a solver created
 * without one gives it a heat source.  The running maximum is optional: setting "T_max" (to the current T, say) switches
 * it on, and from then on every step updates it; reading it before that is an error. */
KWH_API int      kwh_thermal_get_matrix(kwh_thermal* s, const char* name, float* dst, uint64_t n);
KWH_API int      kwh_thermal_set_matrix(kwh_thermal* s, const char* name, const float* src, uint64_t n);
/* volume [m^3] of the points whose cem43 is at least threshold_minutes (240 is the usual lesion threshold) */
KWH_API int      kwh_thermal_lesion_volume(kwh_thermal* s, float threshold_minutes, double* out_m3);
/* "T_raw": steps x points floats; dst == NULL returns the sizes alone */
KWH_API int      kwh_thermal_stream_read(kwh_thermal* s, const char* name, float* dst, uint64_t cap, uint64_t* size,
                                         uint64_t* steps);
/* "fused_pipeline": 1 on the hand-written FFT pipeline, 0 on the rocFFT path */
KWH_API int      kwh_thermal_get_scalar(kwh_thermal* s, const char* name, float* out);
/* the underlying kw_ctx* (include/kwave_hip.h) */
KWH_API void*    kwh_thermal_context(kwh_thermal* s);

/* ------------------------------------------------------------------------------------------------------------------
 * CW field propagator (new with this build; what k-Wave's acousticFieldPropagator computes): the steady-state complex
 * pressure amplitude P(x) of a continuous-wave source S(x) exp(i w t), w = 2 pi f0, in a homogeneous lossless medium, from
 * ONE forward and one inverse 3-D FFT of the source on an expanded periodic grid (kwave_hip.h "CW field propagator",
 * DESIGN.md) — instead of thousands of time steps.  A propagator owns its own device context and builds its operator
 * once; every run reuses it.
 *   T (0 = default): the evaluation time, by default the domain diagonal sqrt(sum (N_a d_a)^2) / c0.
 *   E (all 0 = default): the expanded grid; every side at least N_a + ceil(c0 T / d_a), so that no periodic image reaches
 *   the domain by T.  Default: the smallest fast-path line length of the fused pipeline at or above that; when an axis has
 *   none (above 1024) or with fused_kernels off, the smallest even number on every axis, which runs on rocFFT.  Given
 *   sides must be even and not below the rule.
 *   source scale: a complex factor on the source; (0, 0) = 1.  source_scale_kwave = 1 sets 2 i w c0 / dx, with which an
 *   amplitude p_s gives the steady state of the time loop's additive pressure source p_s sin(w t).
 * Refused, naming the parameter: Nx Ny Nz (0; Nz == 1: 2-D is not built), dx dy dz, c0, f0 (not positive, or above the
 * grid's Nyquist frequency c0 / (2 max d)), T, Ex Ey Ez (missing, odd, below the rule), E (2^32 points or more).
 * Of kwh_options the calls read device_idx and fused_kernels.  kwh_cw_plan validates and completes T and E without a
 * device; kwh_cw_create does the same and then needs one (its failure there is the device library's status, e.g.
 * KW_ERR_NO_DEVICE = 6).  Not built: absorbing or heterogeneous media, 2-D, Z-slabs, HDF5 files and the command line.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kwh_cw kwh_cw;
typedef struct kwh_cw_config
{
  uint64_t nx, ny, nz;      /* domain */
  double   dx, dy, dz;      /* [m] */
  double   c0, f0;          /* [m/s], [Hz] */
  double   t;               /* [s]; 0 = default */
  uint64_t ex, ey, ez;      /* expanded grid; 0 0 0 = default */
  double   source_scale_re, source_scale_im; /* 0 0 = 1 */
  int32_t  source_scale_kwave;
  int32_t  pad_;
} kwh_cw_config;
KWH_API int      kwh_cw_plan(const kwh_cw_config* config, const kwh_options* options, double* out_t, uint64_t out_expanded[3],
                             int32_t* out_fast_path);
KWH_API int      kwh_cw_create(const kwh_cw_config* config, const kwh_options* options, kwh_cw** out);
KWH_API int      kwh_cw_destroy(kwh_cw* s);
/* a, b: Nx * Ny * Nz floats each on the host ([Nz][Ny][Nx]); parts != 0: Re S, Im S; parts == 0: amplitude, phase [rad] */
KWH_API int      kwh_cw_run(kwh_cw* s, const float* a, const float* b, int parts);
/* the last run's result on the domain: "re", "im", "amplitude", "phase"; n = Nx * Ny * Nz (checked) */
KWH_API int      kwh_cw_get(kwh_cw* s, const char* name, float* dst, uint64_t n);
/* Q = q |P|^2 on the domain: q per point (n floats), or NULL and q_scalar.  Plane wave: q = alpha / (rho0 c0), alpha in
 * Np/m, gives the volume rate of heat deposition [W/m^3] that kwh_thermal_* takes as "Q". */
KWH_API int      kwh_cw_heat(kwh_cw* s, const float* q, float q_scalar, float* dst, uint64_t n);
/* the FFT round trip alone on the expanded pair as it stands (timing: tools/bench_cw.py) */
KWH_API int      kwh_cw_propagate(kwh_cw* s);
/* "fused_pipeline" (1 on the hand-written FFT pipeline, 0 on rocFFT), "t", "Ex", "Ey", "Ez", "runs",
 * "source_scale_re", "source_scale_im" */
KWH_API int      kwh_cw_get_scalar(kwh_cw* s, const char* name, double* out);
/* the underlying kw_ctx* (include/kwave_hip.h) */
KWH_API void*    kwh_cw_context(kwh_cw* s);

/* ------------------------------------------------------------------------------------------------------------------
 * Angular-spectrum CW projector (what k-Wave's angularSpectrumCW computes): a complex pressure plane P0 — a measured
 * hologram, or the plane in front of a simulated array — carried to the planes z_j = z0 + j dz, j < planes, of a
 * homogeneous medium that may absorb (alpha_np in Np/m at f0), by one 2-D FFT of the plane and one multiply and inverse
 * 2-D FFT per output plane (kwave_hip.h "Angular-spectrum CW projector").  Nothing is transformed or expanded
 * along z; the planes are computed in chunks of chunk_planes.
 *   E (0 0 = default): the expanded sides; default the smallest fast-path line length of the fused pipeline at or above
 *   2 N per axis; when an axis has none (above 1024) or with fused_kernels off, 2 N, which runs on rocFFT.  Given sides
 *   must be even and not below N.
 *   chunk_planes (0 = default): the smallest of 16, 32, 48, 64 that holds all the planes, 64 beyond that, reduced while the
 *   chunk (16 bytes per expanded point and plane) exceeds 1 GiB, 16 at least; on a fast-path grid a given value must be a
 *   fast-path length.
 *   angular_restriction != 0: components beyond kc(z) = k sqrt(D^2/2 / (D^2/2 + z^2)) are dropped on plane z.
 * Refused, naming the parameter: Nx Ny (0), dx dy, c0, f0 (not positive), z0 (< 0), dz (<= 0), planes (0, above 4096),
 * alpha_np (< 0), Ex Ey (missing, odd, below N), chunk_planes, E (2^32 points or more per chunk).
 * Of kwh_options the calls read device_idx and fused_kernels.  kwh_angular_plan validates and completes E and the chunk
 * without a device.  Not built: heterogeneous media, reverse projection (z < 0), non-uniform plane spacing,
 * 2-D (line -> plane), Z-slabs, HDF5 files and the command line, graphs.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kwh_angular kwh_angular;
typedef struct kwh_angular_config
{
  uint64_t nx, ny;          /* the plane */
  double   dx, dy;          /* [m] */
  double   c0, f0;          /* [m/s], [Hz] */
  double   z0, dz;          /* [m] */
  uint64_t planes;          /* Nz */
  double   alpha_np;        /* [Np/m]; 0 = lossless */
  uint64_t ex, ey;          /* expanded sides; 0 0 = default */
  uint64_t chunk_planes;    /* 0 = default */
  int32_t  angular_restriction;
  int32_t  pad_;
} kwh_angular_config;
KWH_API int      kwh_angular_plan(const kwh_angular_config* config, const kwh_options* options, uint64_t out_expanded[2],
                                  uint64_t* out_chunk_planes, int32_t* out_fast_path);
KWH_API int      kwh_angular_create(const kwh_angular_config* config, const kwh_options* options, kwh_angular** out);
KWH_API int      kwh_angular_destroy(kwh_angular* s);
/* a, b: Nx * Ny floats each on the host ([Ny][Nx]); parts != 0: Re P0, Im P0; parts == 0: amplitude, phase [rad] */
KWH_API int      kwh_angular_run(kwh_angular* s, const float* a, const float* b, int parts);
/* the last run's result [Nz][Ny][Nx]: "re", "im", "amplitude", "phase"; n = Nx * Ny * Nz (checked) */
KWH_API int      kwh_angular_get(kwh_angular* s, const char* name, float* dst, uint64_t n);
/* Q = q |P|^2: q per point (n floats), or NULL and q_scalar (kwh_cw_heat) */
KWH_API int      kwh_angular_heat(kwh_angular* s, const float* q, float q_scalar, float* dst, uint64_t n);
/* the chunks alone from the source spectra as they stand (timing: tools/bench_angular.py) */
KWH_API int      kwh_angular_project(kwh_angular* s);
/* "fused_pipeline", "Ex", "Ey", "chunk_planes", "planes", "runs" */
KWH_API int      kwh_angular_get_scalar(kwh_angular* s, const char* name, double* out);
/* the underlying kw_ctx* (include/kwave_hip.h) */
KWH_API void*    kwh_angular_context(kwh_angular* s);

/* ------------------------------------------------------------------------------------------------------------------
 * Time-domain angular-spectrum projector (what k-Wave's angularSpectrum computes): a pressure record p0[t][y][x] on a plane
 * — a pulsed hydrophone scan, or a cuboid of a time-loop run in front of an array — carried to the parallel planes at the
 * distances z[j] >= 0, j < n_planes, of a homogeneous medium with optional power-law absorption alpha_coeff f^alpha_power
 * (dB / (MHz^y cm), no dispersion).  The record is transformed once over (t, y, x); every plane costs one multiply by
 * H(kx, ky, w; z) and one inverse transform (kwave_hip.h "Time-domain angular-spectrum projector").  Results:
 * p_max = max_t p and p_min = min_t p per plane, and on request the record of one plane, all on the domain Nx x Ny (x Nt).
 *   E (0 0 = default): as kwh_angular_config.
 *   lt (0 = default): the expanded record length; default the smallest fast-path length at or above Nt, or Nt rounded up to
 *   even when there is none (above 1024) or with fused_kernels off.  A given lt must be even and not below Nt.
 *   angular_restriction != 0: on plane z the components with kr^2 > k^2 (D^2/2) / (D^2/2 + z^2) are dropped.
 *   retarded_time != 0: plane z is reported at the times t_n + z / c0.
 * The temporal mean and the temporal Nyquist bin of the record are dropped.
 * Refused, naming the parameter: Nx Ny Nt (0), dx dy dt c0 (not positive), alpha_coeff alpha_power (< 0), n_planes (0, above
 * 4096), z (NULL, an entry < 0), Ex Ey (missing, odd, below N), Lt (odd, below Nt), E (2^32 points or more).
 * Of kwh_options the calls read device_idx and fused_kernels.  kwh_angular_time_plan validates and completes (Ex, Ey, Lt)
 * without a device.  Not built: heterogeneous media, dispersion, reverse projection, 2-D, Z-slabs, HDF5 files and the
 * command line, graphs; several output planes per z-pass; the x- and y-inverse restricted to the crop; band limits other
 * than DC / Nyquist.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kwh_angular_time kwh_angular_time;
typedef struct kwh_angular_time_config
{
  uint64_t nx, ny, nt;      /* the record */
  double   dx, dy, dt;      /* [m], [m], [s] */
  double   c0;              /* [m/s] */
  double   alpha_coeff;     /* [dB / (MHz^y cm)]; 0 = lossless */
  double   alpha_power;     /* y */
  uint64_t ex, ey;          /* expanded sides; 0 0 = default */
  uint64_t lt;              /* expanded record length; 0 = default */
  uint64_t n_planes;        /* 1 ... 4096 */
  const double* z;          /* [m], n_planes distances */
  int32_t  angular_restriction;
  int32_t  retarded_time;
} kwh_angular_time_config;
KWH_API int      kwh_angular_time_plan(const kwh_angular_time_config* config, const kwh_options* options,
                                       uint64_t out_expanded[3], int32_t* out_fast_path);
KWH_API int      kwh_angular_time_create(const kwh_angular_time_config* config, const kwh_options* options,
                                         kwh_angular_time** out);
KWH_API int      kwh_angular_time_destroy(kwh_angular_time* s);
/* p0: Nx * Ny * Nt floats on the host ([Nt][Ny][Nx]): embed, transform, keep */
KWH_API int      kwh_angular_time_set_input(kwh_angular_time* s, const float* p0);
/* set_input and every plane; p_max / p_min [n_planes][Ny][Nx] stay on the device */
KWH_API int      kwh_angular_time_run(kwh_angular_time* s, const float* p0);
/* "p_max" or "p_min" of the last run; n = Nx * Ny * n_planes (checked) */
KWH_API int      kwh_angular_time_get(kwh_angular_time* s, const char* name, float* dst, uint64_t n);
/* plane j recomputed alone: dst [Nt][Ny][Nx], n = Nx * Ny * Nt (checked) */
KWH_API int      kwh_angular_time_series(kwh_angular_time* s, uint64_t j, float* dst, uint64_t n);
/* the planes alone from the kept spectrum as it stands (timing: tools/bench_angular_time.py) */
KWH_API int      kwh_angular_time_project(kwh_angular_time* s);
/* "fused_pipeline", "Ex", "Ey", "Lt", "planes", "runs" */
KWH_API int      kwh_angular_time_get_scalar(kwh_angular_time* s, const char* name, double* out);
/* the underlying kw_ctx* (include/kwave_hip.h) */
KWH_API void*    kwh_angular_time_context(kwh_angular_time* s);

/* ------------------------------------------------------------------------------------------------------------------
 * k-space plane reconstruction (what k-Wave's kspacePlaneRecon computes): the record p[t][y][x] of a planar sensor, sampled
 * at t_n = n dt, to the initial pressure p0 on the planes z_j = j c0 dt, j < planes <= Nt, of a homogeneous medium: one 3-D
 * FFT of the record mirrored in time, a re-gridding of every (kx, ky) line from w to kz with a weight, one inverse 3-D FFT
 * (kwave_hip.h "k-space plane reconstruction").  The result is planes x Ny x Nx on the domain.
 *   E (0 0 = default): the expanded sides; default (Nx, Ny), k-Wave's choice.  Given sides are not below N.
 *   lt (0 = default): the length of the mirrored record; default the smallest fast-path length at or above 2 Nt - 1, or
 *   2 Nt - 1 itself (odd, k-Wave's grid) when there is none (above 1024) or with fused_kernels off.  A given lt is not
 *   below 2 Nt - 1.  The fused stage runs when Ex, Ey and Lt are all fast-path lengths, the rocFFT twin otherwise.
 *   planes (0 = Nt).  interp: 0 linear, 1 nearest.  positivity != 0: the result is clamped at 0.
 * Refused, naming the parameter: Nx Ny Nt (0), dx dy dt c0 (not positive), planes (above Nt), interp (neither), Ex Ey
 * (missing, below N), Lt (below 2 Nt - 1), E (2^32 points or more).
 * Of kwh_options the calls read device_idx and fused_kernels.  kwh_plane_recon_plan validates and completes (Ex, Ey, Lt)
 * without a device.  2-D records: kwh_line_recon_* below.  Not built: heterogeneous media, Z-slabs, HDF5 files and the
 * command line, graphs, a half-length (DCT) time transform that would use the evenness, the x- and y-inverse restricted
 * to the crop, other interpolants.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kwh_plane_recon kwh_plane_recon;
typedef struct kwh_plane_recon_config
{
  uint64_t nx, ny, nt;      /* the record */
  double   dx, dy, dt;      /* [m], [m], [s] */
  double   c0;              /* [m/s] */
  uint64_t ex, ey;          /* expanded sides; 0 0 = default */
  uint64_t lt;              /* length of the mirrored record; 0 = default */
  uint64_t planes;          /* 1 ... Nt; 0 = Nt */
  int32_t  interp;          /* 0 = linear, 1 = nearest */
  int32_t  positivity;
} kwh_plane_recon_config;
KWH_API int      kwh_plane_recon_plan(const kwh_plane_recon_config* config, const kwh_options* options,
                                      uint64_t out_expanded[3], int32_t* out_fast_path);
KWH_API int      kwh_plane_recon_create(const kwh_plane_recon_config* config, const kwh_options* options,
                                        kwh_plane_recon** out);
KWH_API int      kwh_plane_recon_destroy(kwh_plane_recon* s);
/* p: Nx * Ny * Nt floats on the host ([Nt][Ny][Nx]); the result [planes][Ny][Nx] stays on the device */
KWH_API int      kwh_plane_recon_run(kwh_plane_recon* s, const float* p);
/* "p0" of the last run; n = Nx * Ny * planes (checked) */
KWH_API int      kwh_plane_recon_get(kwh_plane_recon* s, const char* name, float* dst, uint64_t n);
/* "fused_pipeline", "Ex", "Ey", "Lt", "planes", "dz", "runs" */
KWH_API int      kwh_plane_recon_get_scalar(kwh_plane_recon* s, const char* name, double* out);
/* the underlying kw_ctx* (include/kwave_hip.h) */
KWH_API void*    kwh_plane_recon_context(kwh_plane_recon* s);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched k-space line reconstruction (what k-Wave's kspaceLineRecon computes, frame by frame): `frames` records p[t][y] of
 * a linear array, sampled at t_n = n dt, to the images p0[x][y], x_j = j c0 dt, j < depth <= Nt, of a homogeneous medium —
 * the plane reconstruction above with one lateral axis (kwave_hip.h "Batched k-space line reconstruction").
 * Public names follow k-Wave: y is the sensor axis, t is time, x is depth.  The result is frames x depth x Ny.
 *   ey (0 = Ny): the expanded sensor axis, not below Ny.
 *   lt (0 = default): as for the plane reconstruction — the smallest fast-path length at or above 2 Nt - 1, or 2 Nt - 1
 *   itself when there is none (above 1024) or with fused_kernels off.  A given lt is not below 2 Nt - 1.
 *   depth (0 = Nt).  interp: 0 linear, 1 nearest.  positivity != 0: the result is clamped at 0.
 *   chunk_frames (0 = default): the frames that one context holds; default all frames, capped so that one chunk stays
 *   inside the index limits of the pass along t: P Lt chunk_frames < 2^29 bins (P = Ey/2 + 1 rounded up to 16; 4 GiB of
 *   spectrum) and at most 65535 frames.  A run goes chunk by chunk through that one context; a shorter last chunk runs as a full
 *   one whose surplus frames are zero records and are not copied out.  Frames are independent: on the fused path a frame's
 *   result does not depend on the chunking.
 *   The fused stage runs when the frames context of one chunk is supported (Ey and Lt fast-path lengths; for the ten
 *   lengths of Ey without masked x kernels, Lt chunk_frames a multiple of 16), the rocFFT twin otherwise.
 * Refused, naming the parameter: Ny Nt frames (0), dy dt c0 (not positive), depth (above Nt), interp (neither), Ey (below
 * Ny), Lt (below 2 Nt - 1), chunk_frames (above frames, above 65535, or too many bins), E (one frame of 2^29 bins or more).
 * Of kwh_options the calls read device_idx and fused_kernels.  kwh_line_recon_plan validates and completes
 * (Ey, Lt, depth, chunk_frames) without a device.  Not built: heterogeneous media, Z-slabs, HDF5 files and the command
 * line, graphs, the 2-D forms of the three projectors, frames spread over several GPUs.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kwh_line_recon kwh_line_recon;
typedef struct kwh_line_recon_config
{
  uint64_t ny, nt;          /* one frame */
  uint64_t frames;          /* F >= 1 */
  double   dy, dt;          /* [m], [s] */
  double   c0;              /* [m/s] */
  uint64_t ey;              /* expanded sensor axis; 0 = Ny */
  uint64_t lt;              /* length of the mirrored record; 0 = default */
  uint64_t depth;           /* 1 ... Nt; 0 = Nt */
  uint64_t chunk_frames;    /* 1 ... frames; 0 = default */
  int32_t  interp;          /* 0 = linear, 1 = nearest */
  int32_t  positivity;
} kwh_line_recon_config;
/* out_sizes: (Ey, Lt, depth, chunk_frames) */
KWH_API int      kwh_line_recon_plan(const kwh_line_recon_config* config, const kwh_options* options,
                                     uint64_t out_sizes[4], int32_t* out_fast_path);
KWH_API int      kwh_line_recon_create(const kwh_line_recon_config* config, const kwh_options* options,
                                       kwh_line_recon** out);
KWH_API int      kwh_line_recon_destroy(kwh_line_recon* s);
/* p: Ny * Nt * frames floats on the host ([frames][Nt][Ny]); the result [frames][depth][Ny] stays on the device */
KWH_API int      kwh_line_recon_run(kwh_line_recon* s, const float* p);
/* "p0" of the last run; n = Ny * depth * frames (checked) */
KWH_API int      kwh_line_recon_get(kwh_line_recon* s, const char* name, float* dst, uint64_t n);
/* "fused_pipeline", "Ey", "Lt", "depth", "frames", "chunk_frames", "dx", "runs" */
KWH_API int      kwh_line_recon_get_scalar(kwh_line_recon* s, const char* name, double* out);
/* the underlying kw_ctx* (include/kwave_hip.h) */
KWH_API void*    kwh_line_recon_context(kwh_line_recon* s);

/* ------------------------------------------------------------------------------------------------------------------
 * Exact k-space propagator (what k-Wave's kspaceSecondOrder computes): an initial pressure p0[z][y][x] on the domain
 * Nx x Ny x Nz of a homogeneous medium, lossless or with power-law absorption alpha_coeff f^alpha_power (dB / (MHz^y cm),
 * with its dispersion), to the pressure at any time t >= 0 — exactly, with no time loop, no CFL limit and no accumulated
 * stepping error.  p0 is transformed once; every output time costs one multiply by the real H(|k|; t) and one inverse
 * transform (kwave_hip.h "Exact k-space propagator").
 *   E (0 0 0 = default): the expanded periodic grid into whose corner the domain is embedded.  Default, with t_max > 0: per
 *   axis the smallest fast-path length at or above N + ceil(c0 t_max / d), or that number itself where there is none (above
 *   1024) or with fused_kernels off.  Given sides: all three, not below N; E = N is the periodic box.  t_max is then not read.
 *   The box is periodic: the result inside the domain is the free-space one for c0 t <= min over axes of (E - N) d; the
 *   scalar "t_free" reports that time.  Later times are not refused.
 *   Absorption: underdamped modes only — alpha_coeff is refused when B = 1 - 2 g tan(pi y / 2) - g^2, g = a c0^y |k|^(y-1),
 *   is below 1/4 at the smallest non-zero or at the largest |k| of the grid (B is concave in |k|^(y-1)).
 *   sensor_index: n_sensor 0-based flat indices into the domain [Nz][Ny][Nx]; kwh_second_order_run samples them at every
 *   time.  flags: which aggregates over the output times of a run are kept, each on the domain.
 * Refused, naming the parameter: Nx Ny Nz (0), dx dy dz c0 (not positive), t_max (not positive while the sides are by
 * default), alpha_coeff (< 0, the B rule), alpha_power (outside 0 <= y < 3, y = 1), Ex Ey Ez (missing, below N), E (2^32 points
 * or more), sensor_index (NULL, an entry outside the domain), t (negative or not finite), n_times (0).
 * Of kwh_options the calls read device_idx and fused_kernels.  kwh_second_order_plan validates and completes (Ex, Ey, Ez)
 * and the fast-path flag without a device.
 *   dp0/dt (k-Wave's source.dp0dt): kwh_second_order_set_dp0dt gives dp/dt at t = 0 [Pa/s] as a second initial condition,
 *   p^(t) = Hc P0 + Hs V0 per mode (kwave_hip.h); with dp0dt = -c0 df/dx beside p0 = f(x) it launches a one-way
 *   wave, and (p, dp/dt) of a snapshot continue a field.  It is independent of set_p0 — either may be called again in any
 *   order, neither resets the other; set_p0 stays required before field / run and may be all zeros —, NULL clears it and
 *   the propagator then launches what one without it launches.  The second kept spectrum is allocated at the first call.
 *   The scalar "has_dp0dt" reports 0 / 1.
 * Not built: time-varying sources,
 * heterogeneous media, Z-slabs, HDF5 files and the command line, graphs, several output times per z-pass, inverse passes restricted to the crop or to the sensor points (but for one plane z = const: the plane-sensor record below), particle velocity outputs.
 * ---------------------------------------------------------------------------------------------------------------- */
#define KWH_SECOND_ORDER_P_MAX   1
#define KWH_SECOND_ORDER_P_MIN   2
#define KWH_SECOND_ORDER_P_RMS   4
#define KWH_SECOND_ORDER_P_FINAL 8
typedef struct kwh_second_order kwh_second_order;
typedef struct kwh_second_order_config
{
  uint64_t nx, ny, nz;      /* the domain */
  double   dx, dy, dz;      /* [m] */
  double   c0;              /* [m/s] */
  double   alpha_coeff;     /* [dB / (MHz^y cm)]; 0 = lossless */
  double   alpha_power;     /* y */
  double   t_max;           /* [s]; sizes the default sides; 0 with given sides */
  uint64_t ex, ey, ez;      /* expanded sides; 0 0 0 = default */
  uint64_t n_sensor;
  const uint64_t* sensor_index; /* n_sensor indices into [Nz][Ny][Nx] */
  int32_t  flags;           /* KWH_SECOND_ORDER_P_* */
  int32_t  pad_;
} kwh_second_order_config;
KWH_API int      kwh_second_order_plan(const kwh_second_order_config* config, const kwh_options* options,
                                       uint64_t out_expanded[3], int32_t* out_fast_path);
KWH_API int      kwh_second_order_create(const kwh_second_order_config* config, const kwh_options* options,
                                         kwh_second_order** out);
KWH_API int      kwh_second_order_destroy(kwh_second_order* s);
/* p0: Nx * Ny * Nz floats on the host ([Nz][Ny][Nx]): embed, transform, keep; may be called again */
KWH_API int      kwh_second_order_set_p0(kwh_second_order* s, const float* p0);
/* dp0dt: Nx * Ny * Nz floats on the host ([Nz][Ny][Nx]), dp/dt at t = 0 [Pa/s]: embed, transform, keep; NULL clears it */
KWH_API int      kwh_second_order_set_dp0dt(kwh_second_order* s, const float* dp0dt);
/* the pressure at time t; the crop [Nz][Ny][Nx] stays on the device ("p") and goes to dst where dst is not NULL */
KWH_API int      kwh_second_order_field(kwh_second_order* s, double t, float* dst);
/* every time in the given order: row i of the record, the aggregates */
KWH_API int      kwh_second_order_run(kwh_second_order* s, const double* times, uint64_t n_times);
/* "p_raw" [n_times][n_sensor], "p_max", "p_min", "p_rms", "p_final" of the last run, "p" (the last field); n checked */
KWH_API int      kwh_second_order_get(kwh_second_order* s, const char* name, float* dst, uint64_t n);
/* "fused_pipeline", "Ex", "Ey", "Ez", "t_free", "runs", "has_dp0dt", "plane", "plane_chunk_times" */
KWH_API int      kwh_second_order_get_scalar(kwh_second_order* s, const char* name, double* out);
/* the underlying kw_ctx* (include/kwave_hip.h) */
KWH_API void*    kwh_second_order_context(kwh_second_order* s);

/* The plane-sensor record: the pressure on ONE plane z = plane dz of the domain at many output times — what a planar sensor
 * records, the input of kwh_plane_recon when times = n dt — without the inverse along z and without a 3-D round trip per
 * output time (kwave_hip.h "Plane-sensor record of the 3-D propagator"): per output time and (kx, ky) one sum over the
 * folded kz bins, then one batched 2-D inverse over the record itself.
 *   set_plane: 0 <= plane < Nz, in effect from the next set_p0 on; -1 switches the record off and frees its arrays.
 *     Refused as "plane" otherwise.
 *   set_plane_chunk_times: how many output times one pass takes (it bounds G [times][Ey][Ex/2 + 1]); 0: the default, as many
 *     as fit 256 MiB, one at the least.  Refused as "plane_chunk_times" when Ex Ey times reaches 2^32.  The scalars "plane"
 *     and "plane_chunk_times" report what is in effect.
 *   plane_record: dst [n_times][Ny][Nx] floats on the host, x fastest, or NULL (the passes run, nothing is copied); times in
 *     any order, each >= 0 and finite; t = 0 gives the plane of p0.  Refused: "plane_record: no plane set", "plane_record: no
 *     p0 since the plane was set", n_times (0), t, and while a dp0dt is set (the message names dp0dt and points to
 *     run(times); the record takes p0 alone).  field, run and plane_record may be interleaved: the record touches neither
 *     "p" nor the aggregates and the record of run.  A value's bits do not depend on the other times of the call or on the
 *     passes.  On the fast path set_p0 with a plane set runs one 3-D rocFFT of the embedded volume beside the fused forward
 *     and holds its spectrum (8 (Ex/2 + 1) Ey Ez bytes) until Q is formed.
 *   plane_plan: the checks of plane, chunk_times and n_times without a device; out: the times of one pass, the passes of
 *     n_times, the complex values of Q.
 * Not built: dp0/dt in the record, planes normal to x or y, several planes per call, equally spaced times by a recurrence
 * instead of one H per time, the 2-D inverse on the fused kernels, Z-slabs, HDF5 files and the command line. */
KWH_API int      kwh_second_order_plane_plan(const kwh_second_order_config* config, const kwh_options* options, int64_t plane,
                                             uint64_t chunk_times, uint64_t n_times, uint64_t out[3]);
KWH_API int      kwh_second_order_set_plane(kwh_second_order* s, int64_t plane);
KWH_API int      kwh_second_order_set_plane_chunk_times(kwh_second_order* s, uint64_t times);
KWH_API int      kwh_second_order_plane_record(kwh_second_order* s, const double* times, uint64_t n_times, float* dst);

/* ------------------------------------------------------------------------------------------------------------------
 * Exact k-space propagator on frames: the batched 2-D form of the propagator above — F independent initial pressures
 * p0[f][y][x] on the domain Nx x Ny, each carried to any time t >= 0 as
 *     p_f(., .; t) = crop( irfft2( rfft2(p0_f embedded in Ey x Ex) H(|k|; t) ) ),   |k|^2 = kx^2 + ky^2
 * with the H of the 3-D operator (kwave_hip.h "Exact k-space propagator on frames").  The frames share c0, the
 * absorption, the expanded plane, the output times and the sensor points; one pass serves the whole batch (the forward
 * side of kwh_line_recon: what a linear array records for many phantoms, with the same c0, dt and grid).
 *   E (0 0 = default): as above per axis, with t_max > 0; given sides: both, not below N.  "t_free" is taken over x and y.
 *   Absorption: the B rule above on the 2-D grid's smallest non-zero and largest |k|.
 *   frames: 1 ... 65535; there are no chunks of frames in this version.  A batch that the fused pipeline does not take for
 *   its size runs on rocFFT, like any grid off the fast path.
 *   sensor_index: n_sensor 0-based flat indices into ONE plane [Ny][Nx], applied to every frame.
 * Refused, naming the parameter: Nx Ny frames (0; frames above 65535), dx dy c0 (not positive), t_max (not positive while
 * the sides are by default), alpha_coeff (< 0, the B rule), alpha_power (outside 0 <= y < 3, y = 1), Ex Ey (missing, below N),
 * E (2^32 points or more), sensor_index (NULL, an entry outside the plane), t (negative or not finite), n_times (0).
 * flags: KWH_SECOND_ORDER_P_*.  kwh_second_order_frames_plan validates and completes (Ex, Ey) and the fast-path flag
 * without a device.  kwh_second_order_frames_set_dp0dt: dp/dt at t = 0 of every frame as a second initial condition, with
 * the rules of kwh_second_order_set_dp0dt; the scalar "has_dp0dt".  Not built: dp0/dt in the line-sensor record,
 * time-varying sources, heterogeneous media,
 * chunks of frames and frames over several GPUs, particle velocity outputs, HDF5 files and the command line, graphs.
 * Several output times per pass and an x-inverse restricted to the rows that hold sensors: for one row, the line-sensor
 * record below.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct kwh_second_order_frames kwh_second_order_frames;
typedef struct kwh_second_order_frames_config
{
  uint64_t nx, ny;          /* the domain of one frame */
  uint64_t frames;          /* F */
  double   dx, dy;          /* [m] */
  double   c0;              /* [m/s] */
  double   alpha_coeff;     /* [dB / (MHz^y cm)]; 0 = lossless */
  double   alpha_power;     /* y */
  double   t_max;           /* [s]; sizes the default sides; 0 with given sides */
  uint64_t ex, ey;          /* expanded sides; 0 0 = default */
  uint64_t n_sensor;
  const uint64_t* sensor_index; /* n_sensor indices into [Ny][Nx] */
  int32_t  flags;           /* KWH_SECOND_ORDER_P_* */
  int32_t  pad_;
} kwh_second_order_frames_config;
KWH_API int      kwh_second_order_frames_plan(const kwh_second_order_frames_config* config, const kwh_options* options,
                                              uint64_t out_expanded[2], int32_t* out_fast_path);
KWH_API int      kwh_second_order_frames_create(const kwh_second_order_frames_config* config, const kwh_options* options,
                                                kwh_second_order_frames** out);
KWH_API int      kwh_second_order_frames_destroy(kwh_second_order_frames* s);
/* p0: Nx * Ny * F floats on the host ([F][Ny][Nx]): embed, transform, keep; may be called again */
KWH_API int      kwh_second_order_frames_set_p0(kwh_second_order_frames* s, const float* p0);
/* dp0dt: Nx * Ny * F floats on the host ([F][Ny][Nx]), dp/dt at t = 0 [Pa/s]: embed, transform, keep; NULL clears it */
KWH_API int      kwh_second_order_frames_set_dp0dt(kwh_second_order_frames* s, const float* dp0dt);
/* every frame's pressure at time t; the crop [F][Ny][Nx] stays on the device ("p") and goes to dst where dst is not NULL */
KWH_API int      kwh_second_order_frames_field(kwh_second_order_frames* s, double t, float* dst);
/* every time in the given order: row i of the record, the aggregates */
KWH_API int      kwh_second_order_frames_run(kwh_second_order_frames* s, const double* times, uint64_t n_times);
/* "p_raw" [n_times][F][n_sensor], "p_max", "p_min", "p_rms", "p_final" of the last run ([F][Ny][Nx]), "p"; n checked */
KWH_API int      kwh_second_order_frames_get(kwh_second_order_frames* s, const char* name, float* dst, uint64_t n);
/* "fused_pipeline", "Ex", "Ey", "frames", "t_free", "runs", "has_dp0dt", "line_row", "line_chunk_times" */
KWH_API int      kwh_second_order_frames_get_scalar(kwh_second_order_frames* s, const char* name, double* out);
/* the underlying kw_ctx* (include/kwave_hip.h) */
KWH_API void*    kwh_second_order_frames_context(kwh_second_order_frames* s);

/* The line-sensor record: the pressure on ONE row y = row dy of every frame at many output times — what a linear array along
 * x records for F phantoms, the input of kwh_line_recon in its order "ty" with x as the array axis — without the y-inverse
 * and without the x-inverse over the plane (kwave_hip.h "Line-sensor record of the propagator on frames"): per output time
 * and kx one sum over the folded ky bins, then one batched 1-D inverse over the record itself.
 *   set_line_row: 0 <= row < Ny, in effect from the next set_p0 on; -1 switches the record off and frees its arrays.
 *     Refused as "line_row" otherwise.
 *   set_line_chunk_times: how many output times one pass takes (it bounds G [F][times][Ex/2 + 1]); 0: the default, as many
 *     as fit 256 MiB, one at the least.  Refused as "line_chunk_times" when Ex F times reaches 2^32.  The scalars
 *     "line_row" and "line_chunk_times" report what is in effect.
 *   line_record: dst [F][n_times][Nx] floats on the host, x fastest, or NULL (the passes run, nothing is copied); times in
 *     any order, each >= 0 and finite; t = 0 gives the row of p0.  Refused: "line_record: no line row set", "line_record: no
 *     p0 since the line row was set", n_times (0), t, and while a dp0dt is set (the message names dp0dt and points to
 *     run(times); the record takes p0 alone).  field, run and line_record may be interleaved: the record touches
 *     neither "p" nor the aggregates and the record of run.  A value's bits do not depend on F, on the other times of the call
 *     or on the passes.
 *   line_plan: the checks of row, chunk_times and n_times without a device; out: the times of one pass, the passes of
 *     n_times, the complex values of Q.
 * Not built: several rows, columns, arbitrary sensor points, the order "yt", frames over several GPUs.  (The plane-sensor
 * record of the 3-D propagator: kwh_second_order_plane_record above.) */
KWH_API int      kwh_second_order_frames_line_plan(const kwh_second_order_frames_config* config, const kwh_options* options,
                                                   int64_t row, uint64_t chunk_times, uint64_t n_times, uint64_t out[3]);
KWH_API int      kwh_second_order_frames_set_line_row(kwh_second_order_frames* s, int64_t row);
KWH_API int      kwh_second_order_frames_set_line_chunk_times(kwh_second_order_frames* s, uint64_t times);
KWH_API int      kwh_second_order_frames_line_record(kwh_second_order_frames* s, const double* times, uint64_t n_times,
                                                     float* dst);

#ifdef __cplusplus
}
#endif
#endif
