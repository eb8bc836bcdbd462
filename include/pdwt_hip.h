/*
 * pdwt_hip.h -- C-ABI of the MI355X-native PDWT hot path (libpdwt_hip.so).
 *
 * This is the drop-in boundary: every entry point below replaces one host-callable function of
 * the reference's level-driver layer (L2 in SURVEY.md section 1), which is the only thing the
 * reference's `Wavelets` class (src/wt.cu) calls to do device work.  Signatures are plain C:
 * device pointers, a host array of device pointers for the coefficient bands, a POD geometry
 * struct passed by value (== reference `w_info`, src/utils.h:9-19) and int error codes.  No HIP,
 * torch or C++ types appear, so the host side (include/wt.h + pdwt_amd/csrc/wt.cpp) builds with
 * a plain host compiler (g++) and any FFI (ctypes / Cython / cgo) can bind it.
 *
 * Differences from the reference seam, on purpose:
 *   - the filter bank is an ARGUMENT (per-instance state) instead of process-global
 *     __constant__ memory uploaded at construction (src/separable.cu:48-51, quirk B-1);
 *   - every function returns 0 on success or a negative PDWT_E* code (the reference's drivers
 *     always return 0 and never check a CUDA call, src/wt.cu:14-21 / B-10);
 *   - precision is a suffix (_f32/_f64) rather than a compile-time DTYPE macro, so one kernel
 *     library serves both libpdwt.so and libpdwtd.so (Makefile:29-39 of the reference).
 *
 * All device work is enqueued on ONE HIP stream per device (pdwt_get_stream(); owned by the library and
 * ordered against the NULL stream unless pdwt_set_stream / PDWT_STREAM_NONBLOCKING say otherwise); nothing
 * synchronises with the host except the functions documented to.
 */
#ifndef PDWT_HIP_H
#define PDWT_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDWT_MAX_FILTER_WIDTH 40 /* reference: MAX_FILTER_WIDTH, src/common.h:15 */

/* error codes (negative), 0 = success */
#define PDWT_OK 0
#define PDWT_EINVAL (-1)   /* bad argument (NULL pointer, bad geometry, hlen out of range) */
#define PDWT_EUNKNOWN (-2) /* unknown wavelet name (same value as src/separable.cu:42-45) */
#define PDWT_EHIP (-3)     /* a HIP runtime call failed (see pdwt_last_error_string) */
#define PDWT_ENOMEM (-4)
#define PDWT_ENOTSUP (-5)  /* the optional facility is not available here (RCCL cannot be loaded, a device list it cannot take): use the fallback */

/* == reference `struct w_info`, src/utils.h:9-19 (same field order, 6 x int32) */
typedef struct pdwt_info {
    int ndims;   /* 1 = (batched) 1D along rows, 2 = 2D */
    int Nr;      /* rows (1D: number of signals in the batch) */
    int Nc;      /* columns (1D: samples per signal) */
    int nlevels; /* decomposition levels */
    int do_swt;  /* 1 = stationary (undecimated, a-trous) transform */
    int hlen;    /* filter length */
} pdwt_info;

/* The four 1-D filters of a bank, indexed exactly like pywt.Wavelet.filter_bank /
 * the reference's c_kern_L/H/IL/IH (src/common.h:28-31): L=dec_lo, H=dec_hi, IL=rec_lo, IH=rec_hi. */
typedef struct pdwt_filters_f32 {
    int hlen;
    float L[PDWT_MAX_FILTER_WIDTH], H[PDWT_MAX_FILTER_WIDTH], IL[PDWT_MAX_FILTER_WIDTH], IH[PDWT_MAX_FILTER_WIDTH];
} pdwt_filters_f32;
typedef struct pdwt_filters_f64 {
    int hlen;
    double L[PDWT_MAX_FILTER_WIDTH], H[PDWT_MAX_FILTER_WIDTH], IL[PDWT_MAX_FILTER_WIDTH], IH[PDWT_MAX_FILTER_WIDTH];
} pdwt_filters_f64;

/* ---------------------------------------------------------------------------------------------
 * Device / memory plumbing.  Replaces the bare cudaMalloc/cudaMemcpy/cudaMemset/cudaFree calls
 * the reference's class makes (src/wt.cu:117-130,421-468; src/common.cu:400-488) and the
 * cudaGetDeviceProperties call in print_informations (src/wt.cu:543-549).
 * ------------------------------------------------------------------------------------------- */
int pdwt_device_count(void);                 /* >=0, or PDWT_EHIP */
int pdwt_set_device(int dev);                /* reference has none (TODO.txt:15) */
int pdwt_get_device(void);
int pdwt_device_name(char* buf, int buflen); /* src/wt.cu:543-549 */
void* pdwt_malloc(size_t nbytes);            /* NULL on failure */
int pdwt_free(void* dptr);
int pdwt_memset(void* dptr, int byte, size_t nbytes);              /* stream-ordered */
int pdwt_memcpy_h2d(void* dst, const void* src, size_t nbytes);    /* blocking */
int pdwt_memcpy_d2h(void* dst, const void* src, size_t nbytes);    /* blocking (syncs the stream) */
int pdwt_memcpy_d2d(void* dst, const void* src, size_t nbytes);    /* stream-ordered (both buffers owned by the library) */
/* device-to-device copy FROM OR TO A BUFFER OF THE CALLER (Wavelets(d_ptr, memisonhost=0), set_image(d_ptr, 1),
 * set_coeff(d_ptr, num, 1)): waits for the NULL stream first, copies, waits for the copy -- the blocking semantics
 * of the reference's cudaMemcpy (src/wt.cu:121-124,433-436), whatever stream the caller's producer ran on. */
int pdwt_memcpy_d2d_foreign(void* dst, const void* src, size_t nbytes);
int pdwt_sync(void);                         /* wait for the library stream of the current device */
void* pdwt_get_stream(void);                 /* the hipStream_t all launches go to (opaque) */
/* Streams.  By default all work of a device goes to ONE stream the library creates WITHOUT hipStreamNonBlocking: it
 * is ordered against the NULL stream in both directions (legacy default-stream semantics), so a reference program,
 * whose own kernels run on the NULL stream, needs no extra synchronisation.  PDWT_STREAM_NONBLOCKING=1 (environment,
 * read once) creates it non-blocking instead.  pdwt_set_stream(s, 1) makes the library enqueue on the caller's
 * stream `s` (NULL = the NULL stream) for the current device; pdwt_set_stream(NULL, 0) returns to the library stream. */
int pdwt_set_stream(void* user_stream, int use_it);
const char* pdwt_last_error_string(void);    /* text of the last failing HIP call (thread-local) */

/* timing helpers for bench.py: HIP events recorded on the library stream */
void* pdwt_event_create(void);
int pdwt_event_record(void* ev);
int pdwt_event_sync(void* ev);
float pdwt_event_elapsed_ms(void* ev_start, void* ev_stop); /* <0 on error */
int pdwt_event_destroy(void* ev);
/* Per-kernel timing: when enabled, every kernel launch of the library on this thread is bracketed
 * by HIP events; pdwt_ktime_read() synchronises and returns {launch count, total ms} for the
 * kernel `kernel_id` (PDWT_K_* below) since the last reset.  Off by default (no events recorded). */
/* stream capture of the launches of one transform into a graph (launch-bound small transforms; no reference
 * counterpart).  begin -> enqueue drivers as usual (nothing executes) -> end returns an executable graph. */
int pdwt_graph_allowed(void);
int pdwt_graph_capture_begin(void);
int pdwt_graph_capture_end(void** exec_out);
int pdwt_graph_launch(void* exec);
int pdwt_graph_destroy(void* exec);
/* ---------------------------------------------------------------------------------------------
 * Batched 2-D DWT (no reference counterpart: the reference has no batching, TODO.txt:15; BASELINE.json's north star asks for
 * batched images).  nimg equally sized float32 images, each with its own band table and scratch exactly as for
 * pdwt_forward_separable_f32 (pdwt_create_coeffs_buffer_f32, pdwt_tmp_elems); every level of ALL images runs in ONE launch.
 * create returns NULL when the geometry is outside the streaming level kernels (then run the images one by one); the object
 * only keeps device-side pointer tables: images, bands and scratch stay the caller's and must outlive it.
 * Round 5: `info` may also describe a Haar transform (hlen 2: one launch per level of the Haar kernels, any size, either precision) or,
 * in float32, an undecimated one (do_swt = 1: one launch per level of the fused SWT level kernels, banks of up to 40 taps; bands and
 * scratch as for pdwt_forward_swt_separable_f32) -- the same create / forward / inverse / destroy entry points.
 * ------------------------------------------------------------------------------------------- */
void* pdwt_batch2d_create_f32(int nimg, float* const* d_images, float** const* d_coeffs, float* const* d_tmps, pdwt_info info);
int pdwt_batch2d_forward_f32(void* batch, const pdwt_filters_f32* f);
int pdwt_batch2d_inverse_f32(void* batch, const pdwt_filters_f32* f);
void pdwt_batch2d_destroy(void* batch);
/* the same in double precision (libpdwtd): every level of all images in one launch of the fused double-precision level kernels; any even
 * bank of up to 40 taps, odd sizes included, every level at least 16 rows and the (padded) bank length in either direction; NULL otherwise.
 * The object of the _f64 create goes to the _f64 forward / inverse; a handle of the other precision is refused with PDWT_EINVAL (every
 * handle carries its kind).  Either destroy releases any handle. */
void* pdwt_batch2d_create_f64(int nimg, double* const* d_images, double** const* d_coeffs, double* const* d_tmps, pdwt_info info);
int pdwt_batch2d_forward_f64(void* batch, const pdwt_filters_f64* f);
int pdwt_batch2d_inverse_f64(void* batch, const pdwt_filters_f64* f);
void pdwt_batch2d_destroy_f64(void* batch);

/* In-kernel clock probe of the fused level kernels of dwt_lds.hip (the C5 kernels): while enabled, workgroup 0 of every such
 * launch records the shader-clock counter and the 100 MHz real-time counter at its start and end.  slot = direction * 8 + size
 * class (forward 0, inverse 8; class 0 = 16384 rows, 1 = 8192, 2 = 4096, ...): the last launch of that kind.  shader_mhz = the
 * clock the workgroup actually ran at, span_us its lifetime; 0 when nothing was recorded.  Synchronises the stream. */
/* The one exchange step of the batch split driven from ONE host process (include/wt_batch.h): all-reduce(SUM) of one double per device
 * over RCCL (xGMI).  in[i] / out[i] are device pointers on devices[i] (distinct devices; may alias); the reduction is enqueued on every
 * device's library stream and the sum is returned in *result.  RCCL is loaded at run time: pdwt_rccl_available() says whether it could
 * be; PDWT_ENOTSUP = not here / device list not usable -> add the per-device doubles on the host.  (One process per GPU: pdwt_amd/batch.py
 * does the same all-reduce through torch.distributed, backend "nccl" = RCCL.)  Reference: none (single-GPU, TODO.txt:15). */
int pdwt_rccl_available(void);
int pdwt_rccl_allreduce_sum_f64(int n, const int* devices, const double* const* in, double* const* out, double* result);
/* the double the reductions above work on: element pdwt_sum_result_index() of a scratch buffer holds the result of
 * pdwt_norm1_enqueue_* / the one-pass threshold; pdwt_sum_spare_index() is a free double behind it (all-reduce output) */
size_t pdwt_sum_result_index(void);
size_t pdwt_sum_spare_index(void);
/* One-time hardware self-check for a new stepping / firmware: the hand-counted `s_waitcnt vmcnt(N)` pipelines of the streaming kernels
 * rely on a wave's loads and stores retiring in order, stores issued with EXEC = 0 included (undocumented; established on gfx950 with
 * tools/probes/vmcnt_order.hip).  Runs a compact form of that probe on the current device (~10 ms, 0.8 GB of scratch it frees again) and
 * returns the number of registers that were read before their load had landed: 0 = the assumption holds; > 0 = run with PDWT_CASC=0
 * PDWT_STREAM=0 (compiler-counted kernels); < 0 = PDWT_E*. */
long long pdwt_selfcheck_vmcnt_order(void);
/* Bandwidth probe (measurement only, bench.py roofline.copy_ceiling): one launch on the library stream that copies `bytes` from src to dst
 * (mode 0), only reads src (1; dst needs 16 valid bytes) or only writes dst (2) with 16-byte accesses, eight in flight per lane, one
 * contiguous chunk per workgroup.  Time it with pdwt_event_*. */
int pdwt_probe_bandwidth(const void* src, void* dst, size_t bytes, int mode);
int pdwt_clock_probe_enable(int on);
int pdwt_clock_probe_read(int slot, double* shader_mhz, double* span_us);
/* diagnostic: enable(2) / enable(3) make EVERY workgroup of the forward / inverse launches record (the last launch wins);
 * dump copies nblocks x {clk0, t0, clk1, t1} (t in 100 MHz ticks) out.  tools/lds_trace.py */
int pdwt_clock_probe_dump(unsigned long long* out, int nblocks);
int pdwt_ktime_enable(int on);
int pdwt_ktime_reset(void);
int pdwt_ktime_read(int kernel_id, int* n_launches, double* total_ms);
const char* pdwt_kernel_name(int kernel_id); /* NULL if out of range */
int pdwt_kernel_count(void);

/* ---------------------------------------------------------------------------------------------
 * Filters.  Replaces w_compute_filters_separable (src/separable.cu:19-54, src/separable.h:5):
 * same name lookup (case-insensitive, 72 names of src/filters.cpp:5919-6002, haar aliases
 * short-circuit when !do_swt) and same return value (hlen, or -2 when unknown), but the taps are
 * written to *out (may be NULL to only query hlen) instead of device constant memory.
 * ------------------------------------------------------------------------------------------- */
int pdwt_compute_filters_separable_f32(const char* wname, int do_swt, pdwt_filters_f32* out);
int pdwt_compute_filters_separable_f64(const char* wname, int do_swt, pdwt_filters_f64* out);
int pdwt_num_wavelets(void);                  /* 72 */
const char* pdwt_wavelet_name(int idx);       /* table order of src/filters.cpp:5919-6002 */

/* ---------------------------------------------------------------------------------------------
 * Coefficient buffers.  Replace w_create/free/copy_coeffs_buffer[_1d]
 * (src/common.h:62-68, src/common.cu:400-488).  Layout (host array of device pointers):
 *   2D: [A_L, H1,V1,D1, ..., H_L,V_L,D_L] (3L+1 bands), 1D: [A_L, D1..D_L] (L+1 bands);
 *   level i band size = ceil-halved i times (src/utils.cu:24-27), SWT: all bands Nr x Nc;
 *   band 0 is allocated at level-1 size (it doubles as scratch, src/common.cu:421-423).
 * All bands live in ONE device allocation (band pointers are 256-byte aligned offsets into it),
 * zero-filled; free with pdwt_free_coeffs_buffer_*.
 * ------------------------------------------------------------------------------------------- */
float** pdwt_create_coeffs_buffer_f32(pdwt_info info);   /* dispatches on info.ndims */
double** pdwt_create_coeffs_buffer_f64(pdwt_info info);
int pdwt_free_coeffs_buffer_f32(float** coeffs, pdwt_info info);
int pdwt_free_coeffs_buffer_f64(double** coeffs, pdwt_info info);
int pdwt_copy_coeffs_buffer_f32(float** dst, float** src, pdwt_info info);
int pdwt_copy_coeffs_buffer_f64(double** dst, double** src, pdwt_info info);
/* number of bands and element count of band `num` (the arithmetic of src/wt.cu:441-465,480-504) */
int pdwt_num_bands(pdwt_info info);
long long pdwt_band_size(pdwt_info info, int num, int* band_Nr, int* band_Nc);

/* ---------------------------------------------------------------------------------------------
 * Transform drivers.  One per reference driver, same argument meaning:
 *   (d_image, d_coeffs /+host array of device ptrs+/, d_tmp /+2*Nr*Nc elements+/, info by value)
 * + the filter bank.  Observable effects are the reference's: forward fills every band and
 * leaves d_image intact; inverse overwrites d_image and clobbers band 0 (src/wt.cu:273-307,
 * SURVEY B-5/B-6).  Scratch usage inside d_tmp is an implementation detail.
 *   forward_separable      <- w_forward_separable        src/separable.cu:179-209
 *   forward_separable_1d   <- w_forward_separable_1d     src/separable.cu:214-236
 *   inverse_separable      <- w_inverse_separable        src/separable.cu:332-364
 *   inverse_separable_1d   <- w_inverse_separable_1d     src/separable.cu:368-395
 *   forward_swt_separable[_1d] <- src/separable.cu:496-537
 *   inverse_swt_separable[_1d] <- src/separable.cu:629-672
 *   haar_forward2d/inverse2d/forward1d/inverse1d <- src/haar.cu:61-119,163-221
 *
 * Buffers of the caller.  d_image, every band pointer and d_tmp (and the buffers of the 3-D drivers
 * below) need only be aligned to their element type: the kernels that use 16-byte accesses are
 * chosen only when every pointer they touch is 16-byte aligned, and a slower kernel with the same
 * result runs otherwise.  Bands may lie back to back.  d_tmp may hold anything on entry.  A driver
 * writes only: d_image (inverse); the bands within their sizes (pdwt_band_size; band 0 within its
 * level-1 allocation; the 1-D / 2-D inverse leaves every band but band 0 intact, the 3-D inverses
 * leave every band intact); and the first pdwt_tmp_elems(info) elements of d_tmp.  Nothing before or
 * behind any of these is written (tests/test_cabi_buffers_gpu.py).
 * ------------------------------------------------------------------------------------------- */
/* test / tuning knobs (not part of the reference seam; names and meaning in INTEGRATION.md).  Each knob is
 * initialised ONCE from its PDWT_<NAME> environment variable and changed at run time only through
 * pdwt_debug_set; e.g. "force_twopass" = 1 makes the 2D DWT drivers use the two-pass (row kernel + column
 * kernel) form instead of the fused level kernels.  Unknown key: PDWT_EINVAL.
 * pdwt_debug_get also serves read-only launch counters (launches since the process started) for the tests
 * that must know which of several kernels behind one timer id ran: stat_casc_spec_fwd / _inv, stat_lat_fwd /
 * _inv, stat_inv_casc3, stat_inv_cascw, stat_inv_casc2, stat_fwd1d_fused, stat_inv1d_fused,
 * stat_fwd1d_fused_ip, stat_inv1d_fused_ip, stat_ana_rows_tr, stat_syn_rows_tr, stat_ana_cols_ring,
 * stat_syn_cols_ring, stat_swt_ana_rows_lds, stat_swt_syn_rows_lds, stat_swt_ana_cols_ring,
 * stat_swt_syn_cols_ring, stat_swtf_fwd, stat_swtf_inv, stat_swtf_invp, stat_swtl2_fwd, stat_swtl2_inv,
 * stat_swtd_fwd, stat_swtd_inv (csrc/common.hpp: StatId). */
int pdwt_debug_set(const char* key, int value);
int pdwt_debug_get(const char* key, int* value);

/* minimum element count of the d_tmp scratch the drivers need (2*Nr*Nc as in src/wt.cu:128-130,
 * plus alignment slack for the sub-buffers carved out of it) */
size_t pdwt_tmp_elems(pdwt_info info);

#define PDWT_DECL_DRIVERS(T, S)                                                                               \
    int pdwt_forward_separable_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const pdwt_filters_##S* f);       \
    int pdwt_forward_separable_1d_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const pdwt_filters_##S* f);    \
    int pdwt_inverse_separable_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const pdwt_filters_##S* f);       \
    int pdwt_inverse_separable_1d_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const pdwt_filters_##S* f);    \
    int pdwt_forward_swt_separable_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const pdwt_filters_##S* f);   \
    int pdwt_forward_swt_separable_1d_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const pdwt_filters_##S* f);\
    int pdwt_inverse_swt_separable_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const pdwt_filters_##S* f);   \
    int pdwt_inverse_swt_separable_1d_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const pdwt_filters_##S* f);\
    int pdwt_haar_forward2d_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info);                                     \
    int pdwt_haar_inverse2d_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info);                                     \
    int pdwt_haar_forward1d_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info);                                     \
    int pdwt_haar_inverse1d_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info);
PDWT_DECL_DRIVERS(float, f32)
PDWT_DECL_DRIVERS(double, f64)

/* ---------------------------------------------------------------------------------------------
 * Coefficient utilities on the hot path (BASELINE.json north_star: soft_threshold, norm1).
 *   soft_thresh <- w_call_soft_thresh  src/common.cu:219-249 (+ kernels src/common.cu:13-52):
 *                  in-place copysign(max(|v|-beta,0),v) on every detail band, band 0 only when
 *                  do_thresh_appcoeffs; normalize>0 divides beta by sqrt(2) per level.
 *                  ONE launch for all bands (device-side band table) instead of L launches.
 *   norm1       <- Wavelets::norm1  src/wt.cu:398-418 (3L+1 cublas asum calls): sum of |c| over
 *                  ALL bands incl. band 0.  One reduction launch (wave64 shuffles -> LDS ->
 *                  per-block double partial) + one finalize launch; the result is accumulated in
 *                  double and rounded once; *out is written after a stream sync.
 * ------------------------------------------------------------------------------------------- */
int pdwt_soft_thresh_f32(float** d_coeffs, float beta, pdwt_info info, int do_thresh_appcoeffs, int normalize);
int pdwt_soft_thresh_f64(double** d_coeffs, double beta, pdwt_info info, int do_thresh_appcoeffs, int normalize);
int pdwt_norm1_f32(float** d_coeffs, pdwt_info info, float* out);
int pdwt_norm1_f64(double** d_coeffs, pdwt_info info, double* out);
/* Threshold and norm in ONE pass over the bands: soft_thresh as above and, as a by-product, sum |c| over ALL bands (the
 * approximation band included, thresholded or not) of the thresholded coefficients -- what pdwt_norm1 would return right
 * after.  `d_scratch`: device buffer of pdwt_sum_scratch_doubles() doubles, ANY contents (the entry point resets the
 * kernels' arrival counter on the library stream in front of every launch; no zero-fill is required of the caller),
 * reusable for any number of calls on the library stream -- one reduction at a time per buffer; no host synchronisation.
 * pdwt_sum_scratch_read copies the result out (synchronises the stream).  The block partials are added in a fixed
 * order by the last block to finish: run-to-run deterministic. */
size_t pdwt_sum_scratch_doubles(void);
int pdwt_soft_thresh_sum_f32(float** d_coeffs, float beta, pdwt_info info, int do_thresh_appcoeffs, int normalize, double* d_scratch);
int pdwt_soft_thresh_sum_f64(double** d_coeffs, double beta, pdwt_info info, int do_thresh_appcoeffs, int normalize, double* d_scratch);
int pdwt_sum_scratch_read(const double* d_scratch, double* out);
/* same reduction, result in double regardless of T (used to combine shards across GPUs) */
int pdwt_norm1_as_double_f32(float** d_coeffs, pdwt_info info, double* out);
int pdwt_norm1_as_double_f64(double** d_coeffs, pdwt_info info, double* out);
/* the same reduction, ENQUEUED only: partial sums and result go to `d_scratch` (pdwt_sum_scratch_doubles() doubles, owned by
 * the caller, any contents -- see above); pdwt_sum_scratch_read fetches the value later.  Lets a host thread start the reductions of several devices
 * before it waits for any of them (include/wt_batch.h). */
int pdwt_norm1_enqueue_f32(float** d_coeffs, pdwt_info info, double* d_scratch);
int pdwt_norm1_enqueue_f64(double** d_coeffs, pdwt_info info, double* d_scratch);

/* ---------------------------------------------------------------------------------------------
 * Remaining coefficient utilities of the class and the circular shift of
 * cycle spinning (row 2).  All in place on the band table, ONE launch each.
 *   hard_thresh       <- w_call_hard_thresh  src/common.cu:252-283 (+ kernels :57-94): v if |v| > beta else 0*v.
 *                        As in the reference the approximation band is thresholded with the UN-normalised beta
 *                        (it computes beta/sqrt(2)^L but passes beta, :262-270).
 *   proj_linf         <- w_call_proj_linf  src/common.cu:286-315 (+ :96-131): copysign(min(|v|,beta),v).
 *   shrink            <- w_shrink  src/common.cu:346-371 (3L+1 cublas scal): v / (1+beta).
 *   group_soft_thresh <- w_call_group_soft_thresh  src/common.cu:318-343 (+ :134-198): per position
 *                        r = max(1 - beta/||(h,v,d[,a])||_2, 0) (0 when the norm is 0), applied to h,v,d[,a];
 *                        the approximation joins the group at the last scale only (do_thresh_appcoeffs).
 *   norm2sq           <- Wavelets::norm2sq  src/wt.cu:370-395 (3L+1 cublas nrm2): sum of c^2 over all bands.
 *                        The reference's 1-D branch adds cublas_asum (sum |c|) of the detail bands (:389):
 *                        FIXED, the squared l2 norm is returned (knob "norm2sq_ref1d" = 1 reproduces the reference
 *                        value).  Accumulated in double, rounded once.
 *   add_coeffs        <- w_add_coeffs / w_add_coeffs_1d  src/common.cu:499-526 (3L+1 cublas axpy):
 *                        dst[k] += alpha*src[k] for every band (whole bands, also for odd sizes in 1-D where
 *                        the reference's Nc/2 sizing leaves the last column of each band out).
 *   circshift         <- w_call_circshift + w_kern_circshift  src/common.cu:202-211,378-396:
 *                        out[y][x] = in[(y-sr) mod Nr][(x-sc) mod Nc] (sr forced to 0 for ndims 1); inplace != 0
 *                        leaves the result in d_image (d_image2 is the copy), else in d_image2.
 * ------------------------------------------------------------------------------------------- */
#define PDWT_DECL_UTILS(T, S)                                                                                   \
    int pdwt_hard_thresh_##S(T** d_coeffs, T beta, pdwt_info info, int do_thresh_appcoeffs, int normalize);     \
    int pdwt_proj_linf_##S(T** d_coeffs, T beta, pdwt_info info, int do_thresh_appcoeffs);                      \
    int pdwt_shrink_##S(T** d_coeffs, T beta, pdwt_info info, int do_thresh_appcoeffs);                         \
    int pdwt_group_soft_thresh_##S(T** d_coeffs, T beta, pdwt_info info, int do_thresh_appcoeffs, int normalize); \
    int pdwt_norm2sq_##S(T** d_coeffs, pdwt_info info, T* out);                                                 \
    int pdwt_norm2sq_as_double_##S(T** d_coeffs, pdwt_info info, double* out);                                  \
    int pdwt_add_coeffs_##S(T** d_dst, T** d_src, pdwt_info info, T alpha);                                     \
    int pdwt_circshift_##S(T* d_image, T* d_image2, pdwt_info info, int sr, int sc, int inplace);
PDWT_DECL_UTILS(float, f32)
PDWT_DECL_UTILS(double, f64)

/* ---------------------------------------------------------------------------------------------
 * Non-separable 2-D transform with four arbitrary hlen x hlen kernels (custom banks only).
 *   <- w_forward / w_inverse / w_forward_swt / w_inverse_swt  src/nonseparable.cu:233-292, 408-452
 *      (+ kernels :114-226, 301-400).
 * d_kernels: DEVICE pointer to 4*hlen*hlen taps, row-major [y][x], in the order LL, LH, HL, HH -- the
 * contents of the reference's c_kern_LL/LH/HL/HH constant arrays (src/nonseparable.cu:7-11) -- the forward
 * set for the forward calls, the inverse set for the inverse calls.  Same d_image / d_coeffs / d_tmp contract
 * as the separable drivers.  For the named wavelets (outer-product kernels) use the separable drivers on a
 * band table with H and V exchanged instead: same result, O(hlen) per sample.
 * ------------------------------------------------------------------------------------------- */
#define PDWT_DECL_NONSEP(T, S)                                                                                     \
    int pdwt_forward_nonseparable_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const T* d_kernels);     \
    int pdwt_inverse_nonseparable_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const T* d_kernels);     \
    int pdwt_forward_swt_nonseparable_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const T* d_kernels); \
    int pdwt_inverse_swt_nonseparable_##S(T* d_image, T** d_coeffs, T* d_tmp, pdwt_info info, const T* d_kernels);
PDWT_DECL_NONSEP(float, f32)
PDWT_DECL_NONSEP(double, f64)

/* ---------------------------------------------------------------------------------------------
 * 3-D separable DWT (volumes; the reference rejects ndims == 3, src/wt.cu).  A row-major Nz x Nr x Nc volume, decimated and
 * periodised exactly like the 1-D level of the drivers above, applied along x (Nc), then y (Nr), then z (Nz) at every level.
 * Band order (pdwt_band_size3d, get_coeff): [A_L, then for levels L .. 1 the 7 detail bands of the level in the key order of
 * PyWavelets' dwtn: aad, ada, add, daa, dad, dda, ddd] -- first letter = z axis, 'a' = low-pass, 'd' = high-pass -- so band
 * 1 + 7*(L - lev) + k is detail k of level lev (1 = finest).  A level-lev band is div2^lev(Nz) x div2^lev(Nr) x div2^lev(Nc).
 * All bands live in ONE zero-filled device allocation at 256-byte aligned offsets; band 0 is A_L only (no scratch role: the
 * inverse leaves every band intact).  Levels are the caller's to clamp: at most ilog2(min(Nz, Nr, Nc) / (hlen - 1)).
 * Sizes: any Nz <= 65535 and Nr * Nc < 2^31 (a plane is indexed in 32 bits; the volume itself may exceed 2^31 elements);
 * anything else is PDWT_EINVAL / a NULL buffer / a scratch size of 0.
 * d_tmp: pdwt_tmp_elems3d(info) elements, about 1.13x the volume (the four x-y quadrants of level 1 + one level-1 approximation).
 * Kernels: pdwt_amd/csrc/dwt3d.hip, two launches per level and direction (an x-y tile kernel and a z kernel); the band table and
 * its walks (thresholds, norm1): pdwt_amd/csrc/vol3d.hpp, shared with the stationary transform.
 * The thresholds and norm1 follow the 2-D semantics (pdwt_soft_thresh_* / pdwt_hard_thresh_* / pdwt_norm1_*) with 7 detail
 * bands per level: normalize > 0 divides beta by sqrt(2) per level, the approximation takes beta / sqrt(2)^L (soft) or the
 * un-normalised beta (hard), norm1 sums |c| over all bands, band 0 included, in double.
 * ------------------------------------------------------------------------------------------- */
typedef struct pdwt_info3d {
    int Nz;      /* planes */
    int Nr;      /* rows per plane */
    int Nc;      /* columns per row */
    int nlevels; /* decomposition levels */
    int hlen;    /* filter length */
} pdwt_info3d;

int pdwt_num_bands3d(pdwt_info3d info);                                                    /* 7L+1, or PDWT_EINVAL */
long long pdwt_band_size3d(pdwt_info3d info, int num, int* band_Nz, int* band_Nr, int* band_Nc); /* elements, or PDWT_EINVAL */
size_t pdwt_tmp_elems3d(pdwt_info3d info);                                                 /* 0 for a bad geometry */
float** pdwt_create_coeffs_buffer3d_f32(pdwt_info3d info);
double** pdwt_create_coeffs_buffer3d_f64(pdwt_info3d info);
int pdwt_free_coeffs_buffer3d_f32(float** coeffs, pdwt_info3d info);
int pdwt_free_coeffs_buffer3d_f64(double** coeffs, pdwt_info3d info);
int pdwt_forward3d_separable_f32(float* d_image, float** d_coeffs, float* d_tmp, pdwt_info3d info, const pdwt_filters_f32* f);
int pdwt_forward3d_separable_f64(double* d_image, double** d_coeffs, double* d_tmp, pdwt_info3d info, const pdwt_filters_f64* f);
int pdwt_inverse3d_separable_f32(float* d_image, float** d_coeffs, float* d_tmp, pdwt_info3d info, const pdwt_filters_f32* f);
int pdwt_inverse3d_separable_f64(double* d_image, double** d_coeffs, double* d_tmp, pdwt_info3d info, const pdwt_filters_f64* f);
int pdwt_soft_thresh3d_f32(float** d_coeffs, float beta, pdwt_info3d info, int do_thresh_appcoeffs, int normalize);
int pdwt_soft_thresh3d_f64(double** d_coeffs, double beta, pdwt_info3d info, int do_thresh_appcoeffs, int normalize);
int pdwt_hard_thresh3d_f32(float** d_coeffs, float beta, pdwt_info3d info, int do_thresh_appcoeffs, int normalize);
int pdwt_hard_thresh3d_f64(double** d_coeffs, double beta, pdwt_info3d info, int do_thresh_appcoeffs, int normalize);
int pdwt_norm1_3d_f32(float** d_coeffs, pdwt_info3d info, double* out);   /* sum |c| in double (synchronises) */
int pdwt_norm1_3d_f64(double** d_coeffs, pdwt_info3d info, double* out);

/* ---------------------------------------------------------------------------------------------
 * 3-D stationary transform (undecimated, a-trous; the reference's do_swt with a third axis).  Same pdwt_info3d and volume
 * layout as the 3-D DWT above.  Level j applies the 1-D a-trous level of the SWT drivers (tap spacing f = 2^(j-1)) along x,
 * then y, then z; its input is the aaa band of level j-1.  The inverse undoes z, then y, then x.
 * Bands: 7L+1 FULL-SIZE (Nz x Nr x Nc) bands in the order of the 3-D DWT: [A_L, then for levels L .. 1: aad, ada, add, daa, dad,
 * dda, ddd], one zero-filled device allocation at 256-byte aligned offsets.  The inverse leaves every band intact: the
 * intermediate approximations pass through d_image.
 * Geometry: Nz <= 65535, Nr * Nc < 2^31, an even hlen of the bank table, and 1 <= nlevels <= ilog2(min(Nz, Nr, Nc) / (hlen - 1))
 * (so (hlen - 1) * 2^(L-1) < min(Nz, Nr, Nc)); anything else is PDWT_EINVAL / a NULL buffer / a scratch size of 0.
 * d_tmp: pdwt_tmp_elems_swt3d(info) elements, 4 volumes (the four x-y quadrants of a level).
 * Kernels: pdwt_amd/csrc/swt3d.hip, two launches per level and direction (an x-y tile kernel and a z kernel); band table: vol3d.hpp.
 * The thresholds and norm1 follow the 3-D DWT rules above with full-size bands.
 * ------------------------------------------------------------------------------------------- */
int pdwt_num_bands_swt3d(pdwt_info3d info);                                                    /* 7L+1, or PDWT_EINVAL */
long long pdwt_band_size_swt3d(pdwt_info3d info, int num, int* band_Nz, int* band_Nr, int* band_Nc); /* elements, or PDWT_EINVAL */
size_t pdwt_tmp_elems_swt3d(pdwt_info3d info);                                                 /* 0 for a bad geometry */
float** pdwt_create_coeffs_buffer_swt3d_f32(pdwt_info3d info);
double** pdwt_create_coeffs_buffer_swt3d_f64(pdwt_info3d info);
int pdwt_free_coeffs_buffer_swt3d_f32(float** coeffs, pdwt_info3d info);
int pdwt_free_coeffs_buffer_swt3d_f64(double** coeffs, pdwt_info3d info);
int pdwt_forward3d_swt_f32(float* d_image, float** d_coeffs, float* d_tmp, pdwt_info3d info, const pdwt_filters_f32* f);
int pdwt_forward3d_swt_f64(double* d_image, double** d_coeffs, double* d_tmp, pdwt_info3d info, const pdwt_filters_f64* f);
int pdwt_inverse3d_swt_f32(float* d_image, float** d_coeffs, float* d_tmp, pdwt_info3d info, const pdwt_filters_f32* f);
int pdwt_inverse3d_swt_f64(double* d_image, double** d_coeffs, double* d_tmp, pdwt_info3d info, const pdwt_filters_f64* f);
int pdwt_soft_thresh_swt3d_f32(float** d_coeffs, float beta, pdwt_info3d info, int do_thresh_appcoeffs, int normalize);
int pdwt_soft_thresh_swt3d_f64(double** d_coeffs, double beta, pdwt_info3d info, int do_thresh_appcoeffs, int normalize);
int pdwt_hard_thresh_swt3d_f32(float** d_coeffs, float beta, pdwt_info3d info, int do_thresh_appcoeffs, int normalize);
int pdwt_hard_thresh_swt3d_f64(double** d_coeffs, double beta, pdwt_info3d info, int do_thresh_appcoeffs, int normalize);
int pdwt_norm1_swt3d_f32(float** d_coeffs, pdwt_info3d info, double* out);   /* sum |c| in double (synchronises) */
int pdwt_norm1_swt3d_f64(double** d_coeffs, pdwt_info3d info, double* out);

/* -----------------------------------------------------------------------------------------------
 * Band statistics and one threshold per band, over an explicit list of bands: band k is d_ptr[k] with n[k] elements,
 * 1 <= nb <= 97 (the classes of wt.h / wt3d.h / swt3d.h build the list from their geometry).  Kernels: pdwt_amd/csrc/bandstats.hip.
 *
 * The stats entries fill out[k] for every band: n, sum |c|, sum c^2 and max |c| (accumulated in double; one launch for all
 * bands; bit-reproducible: no float atomics) and, where want_median[k] != 0, the exact median of |c| -- the mean of the
 * elements of rank (n-1)/2 and n/2, found by radix select (3 read passes of the asking bands in float, 6 in double) --
 * otherwise NaN.  want_median[k] == 2 asks for the median alone: band k is left out of the moments launch and its sums and max are
 * NaN.  want_median == NULL asks for no median.  n[k] == 0 gives zeros and a NaN median.  A NaN element orders
 * above +inf in the selection.  They SYNCHRONISE (one copy to the host at the end, like the norm1 entries) and so must not
 * be called between the begin and the end of a graph capture.
 *
 * The thresh entries apply op (0 soft, 1 hard) with beta[k] to band k, in place, in one launch; beta[k] < 0 leaves band k
 * alone.  Asynchronous, like the soft-threshold entries above.
 * nb < 1, nb > 97, a NULL d_ptr / n / out / beta or an unknown op: PDWT_EINVAL.
 * --------------------------------------------------------------------------------------------- */
typedef struct pdwt_band_stats {
    double n, sum_abs, sum_sq, max_abs, median_abs;
} pdwt_band_stats;
int pdwt_bandlist_stats_f32(const float* const* d_ptr, const size_t* n, int nb, const unsigned char* want_median, pdwt_band_stats* out);
int pdwt_bandlist_stats_f64(const double* const* d_ptr, const size_t* n, int nb, const unsigned char* want_median, pdwt_band_stats* out);
int pdwt_bandlist_thresh_f32(int op, float* const* d_ptr, const size_t* n, const float* beta, int nb);
int pdwt_bandlist_thresh_f64(int op, double* const* d_ptr, const size_t* n, const double* beta, int nb);

/* ---------------------------------------------------------------------------------------------
 * Band statistics and per-band thresholds over a REGULAR BATCH (pdwt_amd/csrc/bandbatch.hip): B images with the same nb <= 97
 * bands, band k of n[k] elements in every image.  d_ptr is a table of B * nb band pointers IN DEVICE MEMORY (band k of image b at
 * d_ptr[b * nb + k]; the caller builds it once and keeps it); n, want_median, beta and out are host arrays, read before the entry
 * returns (they go through a pinned staging buffer of the library: the caller may free them at once).  Band sizes, block layout
 * and betas reach the kernels through device memory, never through kernel arguments.  The number of launches and of copies to
 * the host is fixed per group (up to 8192 / nb images; a larger batch runs group after group) and does not depend on B inside a
 * group, with one exception: medians of bands of more than 2^19 elements are selected in rounds of 64 (image, band) pairs.
 *
 * The stats entries fill out[b * nb + k] with what pdwt_bandlist_stats_* gives for band k of image b, bit for bit in n, max |c|
 * and the median; want_median[k] (0 moments only, 1 moments and median, 2 the median alone; NULL: no median) holds for band k of
 * every image.  Sums are accumulated in double and combined in a fixed order (no float atomics: two runs give the same bits).
 * Launches: moments + combine, ONE selection launch for all asking bands of up to 2^19 elements (every radix pass inside it), and
 * for larger asking bands 3 (float) / 6 (double) histogram + pick launch pairs per round of 64 (image, band) pairs.  They
 * SYNCHRONISE (one copy to the host per group).
 *
 * The thresh entries apply op (0 soft, 1 hard) with beta[b * nb + k] to band k of image b, in place, in one launch per group;
 * beta < 0 leaves that band of that image alone.  The kernel runs asynchronously; beta has been consumed when the entry returns.
 * B < 1, nb < 1, nb > 97, a NULL d_ptr / n / out / beta or an unknown op: PDWT_EINVAL.
 * --------------------------------------------------------------------------------------------- */
int pdwt_bandbatch_stats_f32(const float* const* d_ptr, const size_t* n, int B, int nb, const unsigned char* want_median, pdwt_band_stats* out);
int pdwt_bandbatch_stats_f64(const double* const* d_ptr, const size_t* n, int B, int nb, const unsigned char* want_median, pdwt_band_stats* out);
int pdwt_bandbatch_thresh_f32(int op, float* const* d_ptr, const size_t* n, const float* beta, int B, int nb);
int pdwt_bandbatch_thresh_f64(int op, double* const* d_ptr, const size_t* n, const double* beta, int B, int nb);

/* ---------------------------------------------------------------------------------------------
 * 2-D wavelet packets (pdwt_amd/csrc/wpt2d.hip; the class: include/wpt.h).  The packet tree decomposes every band again: depth l
 * holds 4^l nodes of div2^l(Nr) x div2^l(Nc) elements, CONTIGUOUS in one array (node stride = the node's element count); node i has
 * the children 4i + {0: A, 1: H, 2: V, 3: D} at depth l + 1 -- the bands of the one-level 2-D transform of the drivers above
 * (periodised; the same arithmetic, the same meaning of H and V), for hlen == 2 the clamped 2x2 butterfly of the Haar drivers.
 *
 * The level entries run ONE depth step in ONE launch (one workgroup per tile and node).  d_parent: the array of depth l, nodes of
 * nr x nc elements; d_child: the array of depth l + 1, nodes of div2(nr) x div2(nc) elements.  d_nodes: DEVICE array of nnodes
 * parent indices, or NULL for the parents 0 .. nnodes-1.  forward reads parent d_nodes[k] and writes its four children
 * 4 * d_nodes[k] + 0..3; inverse reads those children and writes that parent; nothing else is touched, so a partial basis costs
 * work only on the parents named.  1 <= nnodes <= 16384 (a grid dimension), nr * nc < 2^31, an even f->hlen of 2 .. 40 and, for
 * hlen > 2, nr >= hlen and nc >= hlen, and at most 65535 rows of tiles (nr <= 262140 for hlen == 2, else about 2^21); anything else, or a NULL d_parent / d_child / f, is PDWT_EINVAL and nothing is launched.
 * Buffers need only be aligned to their element type.  Asynchronous on the library stream.
 *
 * node_cost: an additive cost of each of nnodes (<= 65535) contiguous nodes of node_elems elements in one launch, out[i] on the HOST:
 * kind 0 = sum |c| ("l1"), kind 1 = -sum c^2 ln c^2 over the non-zero c ("shannon").  Accumulated in double and combined in a
 * fixed order (no atomics: two runs give the same bits).  SYNCHRONISES.
 * ------------------------------------------------------------------------------------------- */
int pdwt_wpt2d_forward_level_f32(const float* d_parent, float* d_child, int nr, int nc, const int* d_nodes, int nnodes, const pdwt_filters_f32* f);
int pdwt_wpt2d_forward_level_f64(const double* d_parent, double* d_child, int nr, int nc, const int* d_nodes, int nnodes, const pdwt_filters_f64* f);
int pdwt_wpt2d_inverse_level_f32(float* d_parent, const float* d_child, int nr, int nc, const int* d_nodes, int nnodes, const pdwt_filters_f32* f);
int pdwt_wpt2d_inverse_level_f64(double* d_parent, const double* d_child, int nr, int nc, const int* d_nodes, int nnodes, const pdwt_filters_f64* f);
int pdwt_wpt2d_node_cost_f32(const float* d_nodes, size_t node_elems, int nnodes, int kind, double* out);
int pdwt_wpt2d_node_cost_f64(const double* d_nodes, size_t node_elems, int nnodes, int kind, double* out);

/* ---------------------------------------------------------------------------------------------
 * 2-D DWT with boundary modes (pdwt_amd/csrc/dwt_ext.hip; the class: include/wt_ext.h).  The only transform here that does not
 * periodise: a line x of n samples is extended past its ends by the mode (PyWavelets' names and semantics),
 *   0 zero       0
 *   1 constant   x[0] to the left, x[n-1] to the right
 *   2 symmetric  half-sample mirror, period 2n       ... x1 x0 | x0 x1 ...
 *   3 reflect    whole-sample mirror, period 2n - 2  ... x2 x1 | x0 x1 ...   (n == 1: the constant)
 *   4 periodic   x[j mod n]
 * and a bank of even length F gives N = (n + F - 1) / 2 coefficients per band (the full convolution at the odd indices):
 *   a[i] = sum_k L[k] xe[2i + 1 - k],  d[i] = sum_k H[k] xe[2i + 1 - k],            i = 0 .. N-1, k = 0 .. F-1
 *   x[k] = sum_i a[i] IL[k + F - 2 - 2i] + d[i] IH[k + F - 2 - 2i]  over the i whose tap index lies in 0 .. F-1,  k = 0 .. n-1
 * The inverse reads no sample outside 0 .. N-1: it needs no extension and does not depend on the mode.  In 2-D rows first, then
 * columns; the four bands have the orientation of the drivers above (A = row low / column low, H = row low / column high,
 * V = row high / column low, D = row high / column high), each ((nr + F - 1) / 2) x ((nc + F - 1) / 2), row-major.
 *
 * The level entries run ONE level in ONE launch.  forward reads the nr x nc image d_src and writes the four bands; inverse reads
 * the four bands and writes the nr x nc image d_dst.  An even f->hlen of 2 .. 40 (Haar included: the bank's own taps), nr and nc
 * >= hlen - 1, nr * nc < 2^31, at most 65535 rows of tiles (nr below about 2^21), mode 0 .. 4; anything else, or a NULL pointer, is
 * PDWT_EINVAL and nothing is launched.  Buffers need only be aligned to their element type.  Asynchronous on the library stream.
 *
 * Geometry of `levels` levels (1 .. 32) of an Nr x Nc image, no device needed: the band table is [A_L, H1, V1, D1, ..., H_L, V_L, D_L]
 * (level 1 the finest).  num_bands: 3 * levels + 1; band_shape: the elements of band num, its shape in band_Nr / band_Nc when given;
 * PDWT_EINVAL for sizes a level entry refuses or a bad num.  (The level clamp is the class's: include/wt_ext.h.)
 * ------------------------------------------------------------------------------------------- */
int pdwt_num_bands_ext(int Nr, int Nc, int hlen, int levels);
long long pdwt_ext_band_shape(int Nr, int Nc, int hlen, int levels, int num, int* band_Nr, int* band_Nc);
int pdwt_ext2d_forward_level_f32(const float* d_src, float* d_a, float* d_h, float* d_v, float* d_d, int nr, int nc, int mode, const pdwt_filters_f32* f);
int pdwt_ext2d_forward_level_f64(const double* d_src, double* d_a, double* d_h, double* d_v, double* d_d, int nr, int nc, int mode, const pdwt_filters_f64* f);
int pdwt_ext2d_inverse_level_f32(float* d_dst, const float* d_a, const float* d_h, const float* d_v, const float* d_d, int nr, int nc, const pdwt_filters_f32* f);
int pdwt_ext2d_inverse_level_f64(double* d_dst, const double* d_a, const double* d_h, const double* d_v, const double* d_d, int nr, int nc, const pdwt_filters_f64* f);

/* ---------------------------------------------------------------------------------------------
 * Batched 1-D DWT with boundary modes (pdwt_amd/csrc/dwt_ext1d.hip; the class: BoundaryWavelets1D, include/wt_ext.h): the
 * mathematics of the section above along the LAST axis only.  An nr x nc batch is nr independent lines of nc samples
 * (pywt.wavedec(x, w, mode, level, axis=-1)); one level gives N = (nc + F - 1) / 2 coefficients per band and row, the modes are the
 * numbers 0 .. 4 above, the inverse has no mode and trims like pywt.waverec.
 * Band table of `levels` levels (1 .. 32): [A_L, D_1, ..., D_L], level 1 the finest, band l row-major nr x N_l -- the order of
 * Wavelets with ndim = 1.  num_bands: levels + 1; band_len: the coefficients per row of band num; both need no device and return
 * PDWT_EINVAL for what the entries refuse.
 *
 * Every entry takes an even f->hlen of 2 .. 40 (Haar: the bank's own taps), nr >= 1, nc >= hlen - 1 (7 samples of db4), nr * nc
 * < 2^31 and a mode 0 .. 4; anything else, or a NULL pointer, is PDWT_EINVAL and nothing is launched.  Rows are not limited by a grid
 * dimension.  Buffers need only be aligned to their element type.  Asynchronous on the library stream.
 *
 * The level entries run ONE level in one launch of the per-level kernels: forward reads d_src (nr x nc) and writes d_a and d_d
 * (nr x N each); inverse reads them and writes d_dst (nr x nc).
 * The whole-transform entries take d_coeffs, a HOST table of levels + 1 device pointers in the band order above.  When a row fits
 * the LDS of a workgroup (pdwt_ext1d_fused: 1 / 0; float32 rows up to about 27 000 samples, float64 about 13 600) all levels run in
 * ONE launch that reads the batch once and writes every band once, and d_tmp is not used (may be NULL).  Otherwise they loop the level
 * kernels, keeping the intermediate approximations in d_tmp, which must hold pdwt_ext1d_tmp_elems elements (2 * nr * N_1; 0 for one
 * level).  They return PDWT_EXT1D_FUSED or PDWT_EXT1D_LEVELS to tell which path ran, or a negative error.  Both paths give the same
 * bits.  forward leaves d_src intact, inverse leaves the bands intact.
 * ------------------------------------------------------------------------------------------- */
#define PDWT_EXT1D_LEVELS 0 /* the per-level kernels ran */
#define PDWT_EXT1D_FUSED 1  /* one launch ran all levels */
int pdwt_num_bands_ext1d(int Nc, int hlen, int levels);
long long pdwt_ext1d_band_len(int Nc, int hlen, int levels, int num);
int pdwt_ext1d_fused(int Nc, int hlen, int levels, int elem_size);                      /* elem_size 4 or 8 */
long long pdwt_ext1d_tmp_elems(int Nr, int Nc, int hlen, int levels, int elem_size);
int pdwt_ext1d_forward_level_f32(const float* d_src, float* d_a, float* d_d, int nr, int nc, int mode, const pdwt_filters_f32* f);
int pdwt_ext1d_forward_level_f64(const double* d_src, double* d_a, double* d_d, int nr, int nc, int mode, const pdwt_filters_f64* f);
int pdwt_ext1d_inverse_level_f32(float* d_dst, const float* d_a, const float* d_d, int nr, int nc, const pdwt_filters_f32* f);
int pdwt_ext1d_inverse_level_f64(double* d_dst, const double* d_a, const double* d_d, int nr, int nc, const pdwt_filters_f64* f);
int pdwt_ext1d_forward_f32(const float* d_src, float* const* d_coeffs, int nr, int nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext1d_forward_f64(const double* d_src, double* const* d_coeffs, int nr, int nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext1d_inverse_f32(float* d_dst, float* const* d_coeffs, int nr, int nc, int levels, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext1d_inverse_f64(double* d_dst, double* const* d_coeffs, int nr, int nc, int levels, const pdwt_filters_f64* f, double* d_tmp);

/* ---------------------------------------------------------------------------------------------
 * Batched 2-D DWT with boundary modes (pdwt_amd/csrc/dwt_ext2db.hip; the class: BoundaryWaveletsImages, include/wt_ext.h): the
 * transform of "2-D DWT with boundary modes" on every image of a B x Nr x Nc stack -- pywt.wavedec2(x, w, mode, level,
 * axes=(-2, -1)).  Band table of `levels` levels (1 .. 32): [A_L, H1, V1, D1, ..., H_L, V_L, D_L], level 1 the finest; band num of
 * the batch is ONE contiguous B x nr_l x nc_l stack, image-major (band num of image b starts b * nr_l * nc_l elements in).  The
 * per-image shapes are those of pdwt_ext_band_shape.
 *
 * Every entry takes 1 <= B <= 65535, an even f->hlen of 2 .. 40 (Haar: the bank's own taps), nr and nc >= hlen - 1 at every level it
 * runs, nr * nc < 2^31, at most 65535 rows of tiles and a mode 0 .. 4; anything else, or a NULL pointer, is PDWT_EINVAL and nothing is
 * launched.  Offsets into the stacks are computed in size_t.  Buffers need only be aligned to their element type.  Asynchronous on the
 * library stream.
 *
 * The level entries run ONE level of all B images in one launch (the x-y tile kernels of the 3-D transform, the images as planes):
 * forward reads d_src (B x nr x nc) and writes the four stacks (B x N_r x N_c each); inverse reads them and writes d_dst.
 * The whole-transform entries take d_coeffs, a HOST table of 3 * levels + 1 device pointers in the band order above.  When the
 * pyramid of one image fits the LDS of a workgroup (pdwt_ext2db_fused: 1 / 0; LDS bytes: forward (Nr Nc + 2 Nr N_c1) elements plus
 * two index tables, inverse 2 N_r1 N_c1 + 2 Nr N_c1 elements, the larger within 160 KiB: float32 up to about 140 x 140, float64 about
 * 100 x 100 with a short bank) ALL levels of an image run in one workgroup and a transform is ONE launch, whatever levels and B: the
 * batch is read once, every band written once, and d_tmp is not used (may be NULL).  Otherwise they loop the level entries, keeping
 * the intermediate approximations in d_tmp, which must hold pdwt_ext2db_tmp_elems elements (2 * B * N_r1 * N_c1; 0 exactly when
 * fused).  They return PDWT_EXT2DB_FUSED or PDWT_EXT2DB_LEVELS to tell which path ran, or a negative error.  Both paths, and the 2-D
 * level entries applied image by image, give the same bits.  forward leaves d_src intact, inverse leaves the bands intact.
 * ------------------------------------------------------------------------------------------- */
#define PDWT_EXT2DB_LEVELS 0 /* the per-level kernels ran */
#define PDWT_EXT2DB_FUSED 1  /* one launch ran all levels */
int pdwt_ext2db_fused(int Nr, int Nc, int hlen, int levels, int elem_size);                      /* elem_size 4 or 8 */
long long pdwt_ext2db_tmp_elems(int B, int Nr, int Nc, int hlen, int levels, int elem_size);
int pdwt_ext2db_forward_level_f32(const float* d_src, float* d_a, float* d_h, float* d_v, float* d_d, int B, int nr, int nc, int mode, const pdwt_filters_f32* f);
int pdwt_ext2db_forward_level_f64(const double* d_src, double* d_a, double* d_h, double* d_v, double* d_d, int B, int nr, int nc, int mode, const pdwt_filters_f64* f);
int pdwt_ext2db_inverse_level_f32(float* d_dst, const float* d_a, const float* d_h, const float* d_v, const float* d_d, int B, int nr, int nc, const pdwt_filters_f32* f);
int pdwt_ext2db_inverse_level_f64(double* d_dst, const double* d_a, const double* d_h, const double* d_v, const double* d_d, int B, int nr, int nc, const pdwt_filters_f64* f);
int pdwt_ext2db_forward_f32(const float* d_src, float* const* d_coeffs, int B, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext2db_forward_f64(const double* d_src, double* const* d_coeffs, int B, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext2db_inverse_f32(float* d_dst, float* const* d_coeffs, int B, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext2db_inverse_f64(double* d_dst, double* const* d_coeffs, int B, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp);

/* ---------------------------------------------------------------------------------------------
 * Adjoints of the boundary-mode DWT (pdwt_amd/csrc/dwt_ext_adj.hip): the transposes W^T and S^T of the linear maps that
 * pdwt_ext2db_forward_* / pdwt_ext1d_forward_* (W, depends on the mode) and pdwt_ext2db_inverse_* / pdwt_ext1d_inverse_* (S) compute --
 * what a gradient needs.  With a signal extension W^T is not S.  One level along one line (the notation of the sections above),
 * cotangents abar, dbar of N entries:
 *   u[s]    = sum_i abar[i] L[2i + 1 - s] + dbar[i] H[2i + 1 - s]   over the i whose tap index lies in 0 .. F-1,  s = 2 - F .. 2N - 1
 *   xbar[k] = sum of u[s] over the s that the mode maps to sample k (s = k included), in ascending s
 * In 2-D the column adjoint runs before the row adjoint: xbar[y][x] is the sum over the pre-images sy of y (ascending) of the sum over
 * the pre-images sx of x (ascending) of the separable synthesis U[sy][sx] onto the extended grid.  Several levels run from the coarsest to
 * the finest; the xbar of a level is the A cotangent of the next finer one.  The sums are gathers in that fixed order (no atomics): a
 * result does not depend on B or on tiling, and two runs give the same bits.
 * The adjoint of the inverse, abar[i] = sum_k xbar[k] IL[k + F - 2 - 2i], is the FORWARD transform in mode 0 (zero) with the bank
 * L' = IL reversed, H' = IH reversed: the inverse_adjoint entries build that bank and run the forward entries (fused forms included);
 * their return code is that of the forward entry and their scratch is pdwt_ext2db_tmp_elems / pdwt_ext1d_tmp_elems.
 *
 * Sizes, modes, B and the band tables are those of the sections above; anything they refuse, or a NULL pointer, is PDWT_EINVAL and
 * nothing is launched.  forward_adjoint reads the cotangent bands (left intact) and writes d_dst (B x Nr x Nc / nr x nc);
 * inverse_adjoint reads d_src (left intact) and writes the bands.  d_coeffs is a HOST table.  Asynchronous on the library stream.
 * Scratch of forward_adjoint, in elements: the whole-transform entries need pdwt_ext2db_adjoint_tmp_elems (never 0) /
 * pdwt_ext1d_adjoint_tmp_elems (0 when all levels run in one launch: then d_tmp may be NULL); a level entry needs
 * B * ((nr + 2F - 3) * (nc + 2F - 3) - nr * nc) / nr * (2F - 3) (the halo of the extended grid; may be NULL in mode 0).
 * The 2-D whole transform loops the level kernels (PDWT_EXT2DB_LEVELS); the 1-D one returns PDWT_EXT1D_FUSED or PDWT_EXT1D_LEVELS,
 * fused when pdwt_ext1d_fused says so and one more padded detail line per row fits the LDS of a workgroup.  Both forms give the same bits.
 * ------------------------------------------------------------------------------------------- */
long long pdwt_ext2db_adjoint_tmp_elems(int B, int Nr, int Nc, int hlen, int levels, int elem_size);
int pdwt_ext2db_forward_adjoint_level_f32(float* d_dst, const float* d_a, const float* d_h, const float* d_v, const float* d_d, int B, int nr, int nc, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext2db_forward_adjoint_level_f64(double* d_dst, const double* d_a, const double* d_h, const double* d_v, const double* d_d, int B, int nr, int nc, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext2db_forward_adjoint_f32(float* d_dst, float* const* d_coeffs, int B, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext2db_forward_adjoint_f64(double* d_dst, double* const* d_coeffs, int B, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext2db_inverse_adjoint_f32(const float* d_src, float* const* d_coeffs, int B, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext2db_inverse_adjoint_f64(const double* d_src, double* const* d_coeffs, int B, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp);
long long pdwt_ext1d_adjoint_tmp_elems(int Nr, int Nc, int hlen, int levels, int elem_size);
int pdwt_ext1d_forward_adjoint_level_f32(float* d_dst, const float* d_a, const float* d_d, int nr, int nc, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext1d_forward_adjoint_level_f64(double* d_dst, const double* d_a, const double* d_d, int nr, int nc, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext1d_forward_adjoint_f32(float* d_dst, float* const* d_coeffs, int nr, int nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext1d_forward_adjoint_f64(double* d_dst, double* const* d_coeffs, int nr, int nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext1d_inverse_adjoint_f32(const float* d_src, float* const* d_coeffs, int nr, int nc, int levels, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext1d_inverse_adjoint_f64(const double* d_src, double* const* d_coeffs, int nr, int nc, int levels, const pdwt_filters_f64* f, double* d_tmp);

/* ---------------------------------------------------------------------------------------------
 * 3-D DWT with boundary modes (pdwt_amd/csrc/dwt_ext3d.hip; the class: BoundaryWavelets3D, include/wt_ext.h): the mathematics of
 * "2-D DWT with boundary modes" along x (the last axis), then y, then z of an nz x nr x nc volume -- pywt.wavedecn(vol, w, mode,
 * level).  One level gives eight bands of ((nz + F - 1) / 2) x ((nr + F - 1) / 2) x ((nc + F - 1) / 2), row-major; the modes are the
 * numbers 0 .. 4 above; the inverse runs z, y, x, has no mode and trims like pywt.waverecn.
 *
 * The level entries run ONE level in TWO launches (x-y on every plane through d_tmp, then z; the inverse z, then x-y).  d_bands is a
 * HOST array of 8 device pointers in the order aaa, aad, ada, add, daa, dad, dda, ddd (PyWavelets' dwtn keys; the first letter is
 * the z axis, a = low pass).  forward reads d_src and writes the eight bands; inverse reads them and writes d_dst.  d_tmp holds the
 * four x-y quadrants, 4 * nz * ((nr + F - 1) / 2) * ((nc + F - 1) / 2) elements (pdwt_ext3d_tmp_elems is enough); its contents
 * afterwards are unspecified.  Band aaa may be the buffer of d_src / d_dst itself (it is written after the input has been read): the
 * class keeps the approximation of a level in one scratch buffer that way.  forward leaves d_src intact otherwise, inverse leaves the
 * bands intact.
 * An even f->hlen of 2 .. 40 (Haar included: the bank's own taps), nz, nr and nc >= hlen - 1, nz <= 65535 (a grid dimension),
 * nr * nc < 2^31 (lanes across a plane), at most 65535 rows of tiles (nr below about 2^21), mode 0 .. 4; anything else, or a NULL
 * pointer (one of the eight included), is PDWT_EINVAL and nothing is launched.  Buffers need only be aligned to their element type.
 * Asynchronous on the library stream.
 *
 * Geometry of `levels` levels (1 .. 13) of an Nz x Nr x Nc volume, no device needed: the band table is that of the periodised 3-D
 * transform, [A_L, the 7 details of level L, ..., the 7 details of level 1] (detail k of level lev at 1 + 7 * (levels - lev) + k, in
 * the order aad .. ddd).  num_bands: 7 * levels + 1; band_shape: the elements of band num, its shape in band_Nz / band_Nr / band_Nc
 * when given; tmp_elems: the elements of scratch of an instance -- the four quadrants of level 1 plus one level-1 approximation, each
 * padded to a multiple of 64 elements; tmp_approx_offset: where that approximation starts in the scratch, in elements (the quadrants
 * of every level fit in front of it); all four PDWT_EINVAL for sizes a level entry refuses (band_shape also for a bad num).  (The
 * level clamp is the class's: include/wt_ext.h.)
 * ------------------------------------------------------------------------------------------- */
int pdwt_num_bands_ext3d(int Nz, int Nr, int Nc, int hlen, int levels);
long long pdwt_ext3d_band_shape(int Nz, int Nr, int Nc, int hlen, int levels, int num, int* band_Nz, int* band_Nr, int* band_Nc);
long long pdwt_ext3d_tmp_elems(int Nz, int Nr, int Nc, int hlen);
long long pdwt_ext3d_tmp_approx_offset(int Nz, int Nr, int Nc, int hlen);
int pdwt_ext3d_forward_level_f32(const float* d_src, float* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext3d_forward_level_f64(const double* d_src, double* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext3d_inverse_level_f32(float* d_dst, float* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext3d_inverse_level_f64(double* d_dst, double* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f64* f, double* d_tmp);

/* ---------------------------------------------------------------------------------------------
 * Adjoints of the 3-D boundary-mode DWT (pdwt_amd/csrc/dwt_ext3d_adj.hip): the transposes W^T and S^T of the linear maps that
 * pdwt_ext3d_forward_level_* (W, depends on the mode) and pdwt_ext3d_inverse_level_* (S) compute -- one level of a volume, in the
 * notation of "Adjoints of the boundary-mode DWT".  The forward level runs x-y, then z; its adjoint runs z, then x-y:
 *   along z, per column of each x-y quadrant q (cotangent stacks lo[q], hi[q] of hz = (nz + F - 1) / 2 planes)
 *     u[s]    = sum_i lo[i] L[2i + 1 - s] + hi[i] H[2i + 1 - s]   s = 2 - F .. 2 hz - 1, planes outside 0 .. hz - 1 count as 0
 *     Q[q][k] = sum of u[s] over the s that the mode maps to sample k, in ascending s (s = k in its place)
 *   then the 2-D level adjoint of the section above on the nz planes, with A, H, V, D = Q[0 .. 3] (q = 2 * x band + y band).
 * The sums are gathers in that fixed order (no atomics): a result does not depend on the tiling and two runs give the same bits.
 * The adjoint of the inverse level is the forward level in mode 0 (zero) with the bank L' = IL reversed, H' = IH reversed:
 * inverse_adjoint_level builds that bank, runs pdwt_ext3d_forward_level_* and returns its code.
 *
 * d_bands is the HOST array of 8 device pointers in the order aaa .. ddd of the level entries.  forward_adjoint_level reads the eight
 * cotangent bands (left intact) and writes d_dst (nz x nr x nc), which must not overlap them; inverse_adjoint_level reads d_src (left
 * intact, never the buffer of a band) and writes the eight bands.  d_tmp: pdwt_ext3d_adjoint_level_tmp_elems elements for either entry
 * -- the four quadrant cotangents, 4 * nz * ((nr + F - 1) / 2) * ((nc + F - 1) / 2) padded to a multiple of 64, then the nz frames of
 * the 2-D adjoint, nz * ((nr + 2F - 3) * (nc + 2F - 3) - nr * nc) at most; its contents afterwards are unspecified.
 * The sizes are those of the level entries above and of the 2-D level adjoint with B = nz; anything they refuse, a NULL pointer (one of
 * the eight included) or a bad mode is PDWT_EINVAL and nothing is launched (tmp_elems: PDWT_EINVAL).  Level entries only: the callers
 * loop the levels, from the coarsest to the finest for forward_adjoint (the d_dst of a level is the aaa cotangent of the next finer
 * one).  Asynchronous on the library stream; buffers need only be aligned to their element type.
 * pdwt_ext3d_adjoint_z_run (no device needed): the longest run [z0, z1) of samples along z that no cell of the extension repeats in
 * `mode`; a chunk of 16 samples from a multiple of 16 that lies inside it takes the path without a fold.
 * ------------------------------------------------------------------------------------------- */
long long pdwt_ext3d_adjoint_level_tmp_elems(int nz, int nr, int nc, int hlen);
int pdwt_ext3d_adjoint_z_run(int nz, int hlen, int mode, int* z0, int* z1);
int pdwt_ext3d_forward_adjoint_level_f32(float* d_dst, float* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext3d_forward_adjoint_level_f64(double* d_dst, double* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext3d_inverse_adjoint_level_f32(const float* d_src, float* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext3d_inverse_adjoint_level_f64(const double* d_src, double* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f64* f, double* d_tmp);

/* ---------------------------------------------------------------------------------------------
 * Batched 3-D DWT with boundary modes (pdwt_amd/csrc/dwt_ext3db.hip): the transform of the two sections above, W, its inverse S and
 * the adjoints W^T and S^T, on a contiguous stack of V volumes of Nz x Nr x Nc (volume-major), ALL `levels` levels in one call.  Volume
 * v of every result holds, bit for bit, what the chain of level entries above (pdwt_ext3d_forward_level_*, _inverse_level_*,
 * _forward_adjoint_level_*, _inverse_adjoint_level_*) gives on volume v alone, in every mode and either precision: the x-y passes are
 * the level entries' own launches on the V * nz planes of the stack (chunks of at most 65535 planes), the z passes put the (volume,
 * quadrant) pairs on the grid (chunks of at most 65535 pairs).  No atomics; nothing synchronises with the host between levels or
 * chunks: a call is asynchronous on the library stream.
 *
 * d_bands is a HOST table of 7 * levels + 1 device pointers in the order of pdwt_ext3d_band_shape: [A_L, the 7 details of level L,
 * ..., the 7 details of level 1], a level's details in the order aad, ada, add, daa, dad, dda, ddd.  Band k is ONE contiguous stack
 * V x nz_l x nr_l x nc_l (n_l = (n_{l-1} + F - 1) / 2, n_0 = N, F = f->hlen).  forward reads d_src and writes the bands; inverse reads
 * the bands and writes d_dst; forward_adjoint reads the cotangent bands and writes d_dst; inverse_adjoint (the forward in mode 0 with
 * the bank IL, IH reversed) reads d_src and writes the bands.  forward and inverse_adjoint leave d_src intact, inverse and
 * forward_adjoint leave the bands intact.  d_src / d_dst must not overlap a band or d_tmp.  Levels are NOT clamped: 1 .. 13.
 *
 * Scratch, in elements (pdwt_ext3db_tmp_elems for forward, inverse and inverse_adjoint; pdwt_ext3db_adjoint_tmp_elems for
 * forward_adjoint, which is never smaller and serves all four); contents afterwards are unspecified:
 *   tmp_elems         = 4 * V * Nz * nr_1 * nc_1                          the four x-y quadrant stacks of level 1
 *                     + (levels > 1 ? 2 * V * nz_1 * nr_1 * nc_1 : 0)     two approximation (cotangent) stacks, used in turn
 *   adjoint_tmp_elems = tmp_elems + max over l = 0 .. levels - 1 of V * nz_l * ((2 nr_{l+1} + F - 2) * (2 nc_{l+1} + F - 2) - nr_l * nc_l)
 *                                                                         the frames of the planes of the 2-D level adjoint
 *
 * PDWT_EINVAL (tmp_elems: PDWT_EINVAL too), before anything is launched or touched: a NULL pointer or a NULL entry of the table;
 * V < 1; mode outside 0 .. 4; levels outside 1 .. 13; a level whose nz_l x nr_l x nc_l volume the level entries refuse (an axis
 * shorter than F - 1, nz_l > 65535, ...); for the two adjoints also what the 2-D level adjoint refuses on a chunk of min(V * nz_l,
 * 65535) planes; and a stack of V * Nz >= 2^31 planes or V * Nz * Nr * Nc >= 2^40 elements (plane counts are ints; element
 * offsets are 64-bit).  Buffers need only be aligned to their element type.
 * ------------------------------------------------------------------------------------------- */
long long pdwt_ext3db_tmp_elems(int V, int Nz, int Nr, int Nc, int hlen, int levels);
long long pdwt_ext3db_adjoint_tmp_elems(int V, int Nz, int Nr, int Nc, int hlen, int levels);
int pdwt_ext3db_forward_f32(const float* d_src, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext3db_forward_f64(const double* d_src, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext3db_inverse_f32(float* d_dst, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext3db_inverse_f64(double* d_dst, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext3db_forward_adjoint_f32(float* d_dst, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext3db_forward_adjoint_f64(double* d_dst, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp);
int pdwt_ext3db_inverse_adjoint_f32(const float* d_src, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp);
int pdwt_ext3db_inverse_adjoint_f64(const double* d_src, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp);

/* ---------------------------------------------------------------------------------------------
 * Batched 1-D wavelet packets (pdwt_amd/csrc/wpt1d.hip; the class: WaveletPackets1D, include/wpt1d.h): the full binary tree of
 * every row of an Nr x Nc batch -- pywt.WaveletPacket(mode='periodization'), natural (Paley) order.  Depth l has 2^l nodes per row
 * of n_l = div2(n_{l-1}) samples (n_0 = Nc); node i has the children 2i (a) and 2i + 1 (d) of depth l + 1: the [A, D] bands of one
 * level of the periodised batched 1-D transform of the drivers above applied to that node (the same arithmetic; hlen == 2: the 1-D
 * Haar level).  Node 0 of depth l is A_l and node 1 is D_l of the ordinary transform.
 * Storage: ONE allocation per depth l = 1 .. L laid out (Nr, 2^l, n_l) row-major -- a row's depth-l line is one contiguous run of
 * 2^l * n_l elements, a node is a strided (Nr, n_l) view with a pitch of 2^l * n_l elements.  Depth 0 is the batch.
 *
 * No device needed.  geometry: the depth a batch of rows of Nc samples gets (levels < 1 asks for 1; clamped to
 * ilog2(Nc / (hlen - 1)) and to 12; 0 = too small, a bad Nc or a bad bank length) and, in n when given, n_0 .. n_L.  fused: 1 when
 * the whole tree of a row runs in one launch (ONE row's two LDS lines of adjacent depths, halos included, fit 160 KiB in both
 * directions: float32 rows up to about 20 000 samples, float64 about 10 000), else 0; PDWT_EINVAL when geometry gives 0 or elem_size
 * is not 4 or 8.  tmp_elems: the scratch the whole-transform entries need, which is 0 on both paths (kept for callers that size
 * buffers as for the boundary-mode entries); PDWT_EINVAL as fused, or for Nr < 1 or Nr * Nc >= 2^31.  frequency_order:
 * out[r] = r ^ (r >> 1), the natural index of the node of frequency rank r (Gray code; depth 0 .. 12).  state_table: the node states
 * of the inverse from a basis given as n (depth, idx) pairs, one byte per node, node i of depth l at (2^l - 1) + i, 2^(levels + 1)
 * bytes: 1 = a node of the basis (loaded), 2 = above the basis (synthesised from its children), 0 = below it (skipped);
 * PDWT_EINVAL unless every root-to-leaf path meets exactly one of the nodes.
 *
 * Device entries; an even f->hlen of 2 .. 40; anything out of range, or a NULL pointer, is PDWT_EINVAL and nothing is launched.
 * Buffers need only be aligned to their element type.  Asynchronous on the library stream unless stated.
 * The level entries run ONE depth step of nnodes (1 .. 4096) parents of n samples per row in one launch: forward reads d_parent
 * (nr, nnodes, n) and writes d_child (nr, 2 * nnodes, div2(n)); inverse reads d_child and writes the parents named by d_list, a
 * DEVICE array of count parent indices, or all nnodes when d_list is NULL.  nr * nnodes * n < 2^32.
 * The whole-transform entries take d_nodes, a HOST table of levels device pointers (d_nodes[l - 1] = the allocation of depth l);
 * levels must be what geometry gives for it.  forward fills every depth and leaves d_src intact.  inverse reconstructs d_dst
 * (nr x nc) under d_state, the DEVICE copy of a state_table whose root is 2.  They return PDWT_WP1_FUSED when one launch ran the
 * whole tree -- the inverse then writes d_dst ONLY -- or PDWT_WP1_LEVELS when the level kernels were looped -- the inverse then
 * writes every synthesised parent to its own allocation first; the nodes of the basis are never modified.  Same bits on both paths.
 * moments: out[4 * s + 0..3] = sum |c|, sum c^2, max |c|, -sum c^2 ln c^2 (zero terms skipped) of each of nseg contiguous segments
 * of n elements (a depth: nseg = nr * 2^l, segment s = row * 2^l + node), on the HOST; accumulated in double and combined in a
 * fixed order (no atomics: two runs give the same bits); nseg * n < 2^32.  SYNCHRONISES.
 * thresh: op 0 soft / 1 hard threshold (the formulas of pdwt_soft_thresh / pdwt_hard_thresh) in place on the elements of d_level
 * (nr, nnodes, n) whose node has d_flags[node] == 1 (DEVICE bytes, so a slice of a state_table serves).
 * pdwt_memcpy2d: height rows of width BYTES between pitched buffers (pitches in bytes, width <= both); kind 0 host to device,
 * 1 device to host (both synchronise), 2 device to device (asynchronous), 3 device to device from a foreign producer (waits for
 * the NULL stream first and for the copy).
 * ------------------------------------------------------------------------------------------- */
#define PDWT_WP1_LEVELS 0 /* the per-level kernels ran */
#define PDWT_WP1_FUSED 1  /* one launch ran the whole tree */
int pdwt_wp1_geometry(int Nc, int hlen, int levels, int* n);
int pdwt_wp1_fused(int Nc, int hlen, int levels, int elem_size);
long long pdwt_wp1_tmp_elems(int Nr, int Nc, int hlen, int levels, int elem_size);
int pdwt_wp1_frequency_order(int depth, int* out);
int pdwt_wp1_state_table(int levels, const int* depth, const int* idx, int n, unsigned char* out);
int pdwt_memcpy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, int kind);
int pdwt_wp1_forward_level_f32(const float* d_parent, float* d_child, int nr, int nnodes, int n, const pdwt_filters_f32* f);
int pdwt_wp1_forward_level_f64(const double* d_parent, double* d_child, int nr, int nnodes, int n, const pdwt_filters_f64* f);
int pdwt_wp1_inverse_level_f32(float* d_parent, const float* d_child, int nr, int nnodes, int n, const int* d_list, int count, const pdwt_filters_f32* f);
int pdwt_wp1_inverse_level_f64(double* d_parent, const double* d_child, int nr, int nnodes, int n, const int* d_list, int count, const pdwt_filters_f64* f);
int pdwt_wp1_forward_f32(const float* d_src, float* const* d_nodes, int nr, int nc, int levels, const pdwt_filters_f32* f);
int pdwt_wp1_forward_f64(const double* d_src, double* const* d_nodes, int nr, int nc, int levels, const pdwt_filters_f64* f);
int pdwt_wp1_inverse_f32(float* d_dst, float* const* d_nodes, int nr, int nc, int levels, const unsigned char* d_state, const pdwt_filters_f32* f);
int pdwt_wp1_inverse_f64(double* d_dst, double* const* d_nodes, int nr, int nc, int levels, const unsigned char* d_state, const pdwt_filters_f64* f);
int pdwt_wp1_moments_f32(const float* d_level, long long nseg, int n, double* out);
int pdwt_wp1_moments_f64(const double* d_level, long long nseg, int n, double* out);
int pdwt_wp1_thresh_f32(int op, float* d_level, int nr, int nnodes, int n, const unsigned char* d_flags, float beta);
int pdwt_wp1_thresh_f64(int op, double* d_level, int nr, int nnodes, int n, const unsigned char* d_flags, double beta);

/* ---------------------------------------------------------------------------------------------
 * Batched 2-D wavelet packets (pdwt_amd/csrc/wpt2db.hip; the class: WaveletPacketsImages, include/wpt_batch.h): the full quad-tree of
 * the "2-D wavelet packets" above on every image of a B x Nr x Nc stack, the same arithmetic and the same bits per image.
 * Storage: ONE allocation per depth l = 1 .. L laid out (B, 4^l, nr_l, nc_l) contiguous, image-major: image b's node i of depth l is
 * forest node b 4^l + i, its children are the forest nodes 4 (b 4^l + i) + 0..3 of depth l + 1.  Depth 0 is the stack of images.
 * 1 <= B <= 65535, Nr Nc < 2^31 and B 4^L <= 2^22; anything else, a NULL pointer, a bad bank length or levels that geometry does not
 * give back unchanged is PDWT_EINVAL and nothing is launched.
 *
 * No device needed.  geometry: WaveletPackets::geometry -- the depth an image of this size gets (levels < 1 asks for 1; clamped to
 * ilog2(min(Nr, Nc) / (hlen - 1)) and to 7; 0 = too small, a bad size or a bad bank length) and, in nr / nc when given, the node
 * shapes of depth 0 .. that depth.  fused: 1 when the whole tree of an image runs in the LDS of one workgroup, one launch per
 * direction (two image-sized buffers, the index tables and the state table fit 160 KiB: float32 up to about 128 x 128, float64 about
 * 96 x 96), else 0.  lds_bytes: the dynamic LDS of the forward (dir 0) / inverse (dir 1) fused launch of that plan, whether it fits or
 * not.  state_table: the node states of the inverse from a basis given as n (depth, idx) pairs, one byte per node, node i of depth l
 * at (4^l - 1) / 3 + i, (4^(levels + 1) - 1) / 3 bytes: 1 = a node of the basis (loaded), 2 = above the basis (synthesised from its
 * four children), 0 = below it (skipped); PDWT_EINVAL unless every root-to-leaf path meets exactly one of the nodes.
 * tmp_elems: the INTS of the device list buffer the per-depth form of the inverse reads, 0 when the fused form runs (the plan says
 * fused and allow_fused is set).  chunk_lists: fills that buffer on the HOST from a state table (lists == NULL: only counts) and
 * returns its ints: per depth the chunk-relative indices of the parents to synthesise.  A chunk of the per-depth form is 16384
 * forest parents, a whole number of images, so one list per depth serves every chunk.
 *
 * The whole-transform entries take d_nodes, a HOST table of levels device pointers (d_nodes[l - 1] = the allocation of depth l).
 * forward fills every depth and leaves d_src intact.  inverse reconstructs d_dst (B x Nr x Nc) under `state`, a HOST state_table
 * whose root is 2 (validated on every call); d_state is its DEVICE copy, read by the fused form; d_lists the DEVICE copy of
 * chunk_lists, read by the per-depth form when a depth holds both parents to synthesise and others (else it may be NULL).  They
 * return PDWT_WPTB_FUSED when one launch ran every tree -- the inverse then writes d_dst ONLY -- or PDWT_WPTB_LEVELS when the level
 * entries of wpt2d.hip were looped over the forest (allow_fused == 0, or an image beyond the budget) in chunks of at most 16384
 * parents -- the inverse then writes every synthesised parent to its own allocation first; the nodes of the basis are never
 * modified.  Same bits on both paths.  Buffers need only be aligned to their element type.  Asynchronous on the library stream.
 * ------------------------------------------------------------------------------------------- */
#define PDWT_WPTB_LEVELS 0 /* the level entries ran, depth by depth */
#define PDWT_WPTB_FUSED 1  /* one launch ran the whole tree of every image */
int pdwt_wptb_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc);
int pdwt_wptb_fused(int Nr, int Nc, int hlen, int levels, int elem_size);
long long pdwt_wptb_lds_bytes(int Nr, int Nc, int hlen, int levels, int elem_size, int dir);
long long pdwt_wptb_tmp_elems(int B, int Nr, int Nc, int hlen, int levels, int elem_size, int allow_fused);
int pdwt_wptb_state_table(int levels, const int* depth, const int* idx, int n, unsigned char* out);
long long pdwt_wptb_chunk_lists(int B, int levels, const unsigned char* state, int* lists);
int pdwt_wptb_forward_f32(const float* d_src, float* const* d_nodes, int B, int Nr, int Nc, int levels, const pdwt_filters_f32* f, int allow_fused);
int pdwt_wptb_forward_f64(const double* d_src, double* const* d_nodes, int B, int Nr, int Nc, int levels, const pdwt_filters_f64* f, int allow_fused);
int pdwt_wptb_inverse_f32(float* d_dst, float* const* d_nodes, int B, int Nr, int Nc, int levels, const unsigned char* state, const unsigned char* d_state,
                          const int* d_lists, const pdwt_filters_f32* f, int allow_fused);
int pdwt_wptb_inverse_f64(double* d_dst, double* const* d_nodes, int B, int Nr, int Nc, int levels, const unsigned char* state, const unsigned char* d_state,
                          const int* d_lists, const pdwt_filters_f64* f, int allow_fused);

#ifdef __cplusplus
}
#endif
#endif /* PDWT_HIP_H */
