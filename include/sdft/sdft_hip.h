/*
 * sdft/sdft_hip.h -- additions of the MI355X engine beyond the reference's C API.  Nothing here
 * alters the drop-in surface of sdft/sdft.h; a host that ignores this file behaves like one
 * built against the reference.  Included by sdft/sdft.h (needs its type selection).
 */

#ifndef SDFT_HIP_SDFT_HIP_H
#define SDFT_HIP_SDFT_HIP_H

#ifndef SDFT_HIP_SDFT_H
#error "include <sdft/sdft.h>, not <sdft/sdft_hip.h>"
#endif

#if defined(__cplusplus)
extern "C" {
#endif

/* ---- error channel -------------------------------------------------------------------------
   The reference has none (void returns, unchecked malloc; sdft.h:413-687).  Signatures are kept;
   on a HIP failure sdft_alloc* returns NULL, other calls leave their outputs untouched, and the
   text of the first failing HIP call is recorded per thread.  Never aborts. */
const char* sdft_hip_last_error(void);       /* NULL if nothing is recorded */
void        sdft_hip_clear_error(void);
/* A call that SUCCEEDED but has something to tell -- a poll loop of the exact-carry kernels timed out and the call was
   re-run with the serial carry pass (get_option "ring_recoveries" counts them) -- leaves a warning, never an error:
   its outputs and the stream state are valid and the host must not repeat it. */
const char* sdft_hip_last_warning(void);     /* NULL if nothing is recorded */
void        sdft_hip_clear_warning(void);

/* ---- device selection (one process per GPU is the intended multi-GPU model) ----------------- */
int         sdft_hip_device_count(void);
int         sdft_hip_set_device(int device); /* plans are created on the current device */
int         sdft_hip_get_device(void);
const char* sdft_hip_version(void);
int         sdft_hip_selftest(void);         /* 0 = cross-lane primitives behave as the kernels assume */
/* compiles the statements of a sdft_hip_op_expr operation (below) for `arch` (NULL: "gfx950") without running them:
   0, or -1 with the compiler's words in sdft_hip_last_error().  Needs no GPU. */
int         sdft_hip_check_expr(const char* expr, const char* arch);

/* measurement aid: average ms of a store-only kernel over `bytes` of device memory.
   pattern 0 = linear fill; pattern 1 = the forward kernel's tiling (rows of `row_slots` 16-byte
   slots, `lanes` slots per wave, `chunk_len` consecutive rows per wave); pattern 2 = one workgroup per time chunk writing
   whole rows in lockstep (`lanes` = rows per barrier); pattern 3 = the same with non-temporal stores; 4 = every XCD a contiguous
   eighth of the chunks (what ForwardArgs::xcd_map does in the analysis kernels); 5 = workgroups started at different row phases;
   6 = both; 100 + R = workgroup b takes the (b / R)-th chunk of region b mod R */
double      sdft_hip_store_ceiling(void* dst, size_t bytes, int pattern, unsigned row_slots, unsigned lanes,
                                   unsigned chunk_len, int reps);
/* Device memory for a DFT matrix, chosen for how fast it can be written: which physical memory backs a large allocation decides what
   the analysis' store stream reaches in it (5.85, 6.4 or 7.1 TB/s for 16 GB buffers of one process; reads do not care) and nothing
   can move a buffer afterwards.  Allocates up to `candidates` buffers of `bytes` (as many as fit beside each other), probes each with
   the store-only kernel above (2 launches), keeps the best and frees the others; *gbs (may be NULL) = the kept buffer's probe rate.
   Free with hipFree.  NULL on failure. */
void*       sdft_hip_malloc_matrix(size_t bytes, int candidates, double* gbs);
/* The same choice made inside ONE allocation, computed rather than searched (round 6, profiles/r06_stretch_map.txt): a large allocation is
   made of stretches of two or three KINDS of memory that alternate every 16-32 GiB (the first change lies 32 or 64 GiB into the allocation in
   every session kept), and the analysis' store stream -- every XCD writing its own eighth of the matrix at the same time -- reaches 6.8-7.1 TB/s
   when the matrix lies half in one kind and half in another, 5.6-5.85 when all of it is of one kind.  Allocates `arena_bytes` (>= bytes;
   bytes + 64 GiB has held a change of kind in every fresh process so far), finds the first change with small two-part store probes (2 GiB written each, steps
   of 16 GiB then bisection: <= 12 ms in all), returns the window centred on it and keeps the whole allocation until
   sdft_hip_free_matrix(window) -- NOT hipFree: the window is not the start of the allocation.  Two full-size probes check the result (the
   window, and a window at the allocation's start = what a plain hipMalloc would have been) and the better one is returned.  An allocation that
   holds no change of kind at all (seen in a process that had allocated and freed a lot before) is answered by a second allocation made while the first
   is held -- other memory by construction -- and the better of the two is kept; an arena too small for the two-part probes (< 3 GiB) is searched window
   by window (every 4 GiB, at most 8).  *gbs (may be NULL) = the window's probe rate.  NULL on failure; free: 0, or -1 for a pointer this call did
   not return.  Matrices below 64 MiB are not probed and get an allocation of their own size.  sdft_hip_matrix_placement tells how a window was placed. */
typedef struct
{
  size_t arena_bytes;      /* the allocation that holds the window */
  size_t window_offset;    /* of the window inside it */
  size_t boundary_offset;  /* where the kind of memory changes (0: no change found, the window came from the search or is the start) */
  int    pair_probes;      /* two-part probes of 2 GiB used to find it */
  int    window_probes;    /* full-size store-only probes (the start, the window; more only when the search ran) */
  double window_gbs;       /* store-only rate of the window, GB/s */
  double start_gbs;        /* ... of a window at the allocation's start */
  double probe_ms;         /* GPU time of all probes */
  int    arenas_tried;     /* 1; 2 when the first allocation held no change of kind and a second one was made beside it (the better is kept) */
} sdft_hip_placement_t;
void*       sdft_hip_malloc_matrix_in_arena(size_t bytes, size_t arena_bytes, double* gbs);
int         sdft_hip_matrix_placement(const void* window, sdft_hip_placement_t* out);
int         sdft_hip_free_matrix(void* window);
/* measurement aid: occupies `cus` CUs (nothing shares them) for `milliseconds` on a stream of its own and returns at once;
   cus = 0 waits for the release.  What a kernel keeps of its speed beside a kernel that holds part of the chip. */
int         sdft_hip_hold_cus(unsigned cus, double milliseconds);
/* the same for a load-only kernel (16-byte loads, four in flight per thread) */
double      sdft_hip_load_ceiling(const void* src, size_t bytes, int reps);
/* ... and for whole rows of `row_slots` 16-byte slots read in step by one workgroup per chunk of `chunk_len` rows
   (regions = 0: workgroup b -> chunk b; R: regions in turn, as store pattern 100 + R) */
double      sdft_hip_load_rows_ceiling(const void* src, size_t bytes, unsigned row_slots, unsigned chunk_len, unsigned regions, int reps);

/* ---- batched plans: `channels` independent streams with one launch per call ----------------
   The unit of sharding in the reference is the plan (no shared mutable state, sdft.h:145-182);
   a batch is the same thing laid out for one GPU.  With a batched plan
     sdft_sdft_n : samples [channels][nsamples],  dfts [channels][nsamples][dftsize]
     sdft_isdft_n: dfts as above,                 samples [channels][nsamples]          */
sdft_t*     sdft_hip_alloc_batch(const sdft_size_t dftsize, const sdft_window_t window,
                                 const sdft_double_t latency, const sdft_size_t channels) SDFT_HIP_SYMBOL(alloc_batch);
sdft_size_t sdft_hip_channels(const sdft_t* sdft) SDFT_HIP_SYMBOL(channels);

/* ---- fused analysis -> spectral operation -> synthesis -------------------------------------------
   The reference's contract materialises the (nsamples, dftsize) matrix between sdft_sdft_n and
   sdft_isdft_n (README.md:42-47 of the reference); a host that only wants the processed signal back
   pays two HBM streams of 16 KiB per sample for it.  sdft_hip_process_n computes
       out[t] = sdft_isdft( op( sdft_sdft(samples[t]) ) )
   with the same arithmetic and the same plan state update as the two calls, but the rows stay
   inside the workgroup that produced them (dftsize 8 ... 4096; other shapes, and the reference's summation
   order beyond 2048 double / 4096 float bins, run analysis + synthesis back to back through a workspace).
     sdft_hip_op_identity  params = NULL
     sdft_hip_op_gain      params = sdft_fd_t gains[dftsize]  (host or device): X'[k] = X[k] * gains[k]
     sdft_hip_op_shift     params = const long* (host): X'[k] = X[k - *params], zero outside the spectrum
     sdft_hip_op_cgain     params = sdft_fdx_t gains[dftsize] (host or device): X'[k] = X[k] * gains[k], complex
     sdft_hip_op_gain_rows / sdft_hip_op_cgain_rows   gains that change with time -- what a host of the reference does when
                           its loop over the matrix recomputes the mask every hop: params = const sdft_hip_gain_rows_t*
                           { gains[rows][dftsize] (real / complex; host or device), rows, hop }: vector r applies to the
                           call's samples [r*hop, (r+1)*hop), the last vector to everything after it.  Still one launch:
                           the folded coefficients of all vectors are formed by one small launch in front of it.
     sdft_hip_op_gate      params = sdft_fd_t[2] {threshold, floor} (host): X'[k] = X[k] if |X[k]| >= threshold, else
                           X[k] * floor (a spectral gate; floor = 0 removes the bin)
     sdft_hip_op_power     params = sdft_fd_t[2] {exponent, scale} (host): X'[k] = X[k] * scale * |X[k]|^(exponent-1), i.e.
                           |X'[k]| = scale * |X[k]|^exponent with the phase kept (spectral compression / expansion)
                           (gate and power are not linear in the spectrum: they run on the windowed rows inside the
                           row-group kernel, dftsize <= 2048 double / 4096 float, two passes beyond)
     sdft_hip_op_expr      the host's own operation, handed in as code: params = const sdft_hip_expr_t*
                           { expr, params, nparams }.  expr is a string of HIP C++ statements applied to every windowed
                           bin; in scope are  re, im  (sdft_fd_t; read and assign them: the value of bin k),  k, nbins
                           (unsigned),  t  (size_t: index of the sample within the call),  ch  (size_t: channel),
                           p[i]  (sdft_fd_t, read-only: the call's nparams parameters, copied from host memory with the call)
                           and HIP's math functions.  Example (a gate with a frequency-dependent threshold):
                               "if (re * re + im * im < p[0] * p[0] * (1 + k)) { re = 0; im = 0; }"
                           The statements are compiled into the fused kernel at run time (hiprtc: libhiprtc.so is opened
                           on first use; about a second per new expression and kernel shape, then cached for the life of
                           the process), so the call still moves no matrix; a hop (one time chunk) runs the hop kernel and
                           the row synthesis with the statements built in (two launches), rows beyond the row-group
                           kernel run analysis -> expression on the rows -> synthesis.
                           What sdft.h leaves to the host between sdft_sdft_n and sdft_isdft_n (README.md:42-47), on the GPU.
   dfts: NULL, or device memory of shape (nsamples, dftsize) that receives the processed spectrum
   (not with the shift).  Batched plans: samples / out [channels][nsamples].
   Results equal sdft_sdft_n + operation + sdft_isdft_n of the reference within the path's bar (1e-6
   relative at FD double, 1e-4 at FD float; measured 1e-13 / 1.2e-5); bit-identical on request (option
   "fused_exact" = 1) wherever the analysis is: calls shorter than 512 samples, FD float, FD double with
   carry = 1.  The stream state a call leaves behind is the one the two calls leave.  Returns 0, or -1
   with sdft_hip_last_error() set. */
enum sdft_hip_op { sdft_hip_op_identity = 0, sdft_hip_op_gain = 1, sdft_hip_op_shift = 2, sdft_hip_op_cgain = 3,
                   sdft_hip_op_gain_rows = 4, sdft_hip_op_cgain_rows = 5, sdft_hip_op_gate = 6, sdft_hip_op_power = 7,
                   sdft_hip_op_expr = 8 };
typedef struct { const void* gains; size_t rows; size_t hop; } sdft_hip_gain_rows_t;
typedef struct { const char* expr; const void* params; size_t nparams; } sdft_hip_expr_t;
int sdft_hip_process_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples, sdft_td_t* const out,
                       const int op, const void* params, sdft_fdx_t* dfts) SDFT_HIP_SYMBOL(process_n);

/* ---- decimated analysis --------------------------------------------------------------------------
   sdft_hip_sdft_every_n writes only the rows sdft_sdft_n would write for the call's samples first, first + every,
   first + 2*every, ... < nsamples -- a spectrogram at a hop of `every` samples -- without forming the others: the
   recurrence still steps every sample, the demodulation, the window and the store happen at the grid's samples only.
     rows = first < nsamples ? (nsamples - first + every - 1) / every : 0
   dfts is [rows][dftsize]; batched plans: samples [channels][nsamples], dfts [channels][rows][dftsize].  Each row is the
   row sdft_sdft_n gives (bit-identical wherever that call is: FD float, FD double with option "carry" = 1, calls shorter
   than 512 samples; within 1e-11 relative otherwise), and the stream state afterwards -- accumulators, fiddles, delay line,
   cursor -- is the one sdft_sdft_n of the same samples leaves: later sdft_sdft_n / sdft_isdft_n calls continue as if every
   row had been computed.
   The grid is local to the call (the plan keeps no grid state).  A host streaming in calls of any length passes, as the
   next call's first,
     first + rows * every - nsamples     (rows > 0)
     first - nsamples                    (rows == 0)
   and gets the rows one long call would give.  samples and dfts may each be host or device memory (option "async" applies
   to device pointers); dfts may be NULL when the call keeps no row, and then only advances the stream.  every == 1 with
   first == 0 is sdft_sdft_n itself.  Returns the number of rows written, or -1 with sdft_hip_last_error() set (a NULL plan,
   every == 0, or dfts == NULL with rows > 0; the stream state is then untouched). */
long sdft_hip_sdft_every_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                           const sdft_size_t every, const sdft_size_t first, sdft_fdx_t* dfts) SDFT_HIP_SYMBOL(sdft_every_n);

/* ---- power-spectrogram analysis ------------------------------------------------------------------
   sdft_hip_sdft_power_n writes |X|^2 of a band of bins on the row grid of sdft_hip_sdft_every_n: for the rows sdft_sdft_n would
   write for the call's samples first, first + every, ... < nsamples (rows, streaming and the next call's first exactly as above;
   every == 1 with first == 0 keeps every row) and the bins bin0 <= k < bin0 + nbins of each,
     power = re * re + im * im
   of the windowed, weighted bin as sdft_sdft_n stores it, evaluated in sdft_fd_t with two roundings for the products and one for
   the sum (no fused multiply-add) -- what numpy's d.real * d.real + d.imag * d.imag gives on that call's row.  The complex bin
   never reaches memory: the call stores half the bytes per bin of sdft_sdft_n and no second pass reads them back.
   power is [rows][nbins] real numbers, dense; batched plans: samples [channels][nsamples], power [channels][rows][nbins].  It
   need only be aligned to sizeof(sdft_fd_t).  The value is bit-identical to that expression wherever sdft_sdft_n is bit-identical
   to the reference (FD float, FD double with option "carry" = 1, calls shorter than 512 samples), else within 2.1e-11 of the
   largest power.  The stream state afterwards is the one sdft_sdft_n of the same samples leaves -- bins outside the band step
   every sample too -- so any other entry point may follow.  samples and power may each be host or device memory (option "async"
   applies to device pointers); power may be NULL when the call keeps no row.  The full grid with the full band is not
   sdft_sdft_n: the call always runs its own kernel ("last_kernel" = 5).  Returns the number of rows written (0 for
   nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan, every == 0, nbins == 0,
   bin0 + nbins > dftsize, or power == NULL with rows > 0. */
long sdft_hip_sdft_power_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                           const sdft_size_t every, const sdft_size_t first,
                           const sdft_size_t bin0, const sdft_size_t nbins,
                           sdft_fd_t* power) SDFT_HIP_SYMBOL(sdft_power_n);

/* ---- pooled power analysis -------------------------------------------------------------------------
   sdft_hip_sdft_power_sum_n sums |X|^2 over windows of rows, in the manner of Welch.  Let p[t][k] be the value
   sdft_hip_sdft_power_n stores for sample t and bin k at every == 1, first == 0 (formed the same way: in sdft_fd_t, two rounded
   products, one rounded sum, no fused multiply-add).  The grid points first, first + every, ... cut the call's samples into windows:
     head window  [0, min(first, nsamples))                                  present iff first > 0 and nsamples > 0: the end of
                                                                             a window a previous call began
     window j     [first + j * every, min(first + (j + 1) * every, nsamples))  for every j with first + j * every < nsamples;
                                                                             the last one may be short
   rows = (first > 0 && nsamples > 0 ? 1 : 0) + (rows of sdft_hip_sdft_every_n for the same nsamples, every, first).  Row r holds,
   for bin0 <= k < bin0 + nbins, the sum of p[t][k] over the r-th window (the head is row 0 when present), accumulated in
   sdft_fd_t.  sums is [rows][nbins], dense, aligned to sizeof(sdft_fd_t) only; batched plans: samples [channels][nsamples], sums
   [channels][rows][nbins].  Sums are returned, not means, because partial windows add: the next call's first is the one
   sdft_hip_sdft_every_n's contract gives (first + rows_of_the_grid * every - nsamples, or first - nsamples when first >=
   nsamples), and when it is not 0 the next call's row 0 completes this call's last row -- the host adds the two.  Divide a row
   by its window's length for a mean.  every == 1 with first == 0 gives sdft_hip_sdft_power_n's values bit for bit.
   Accuracy: the order in which a window's terms are added is the library's (time chunks cut windows).  Every term is
   non-negative, so with S the exact sum of the sdft_fd_t terms, L the window's length, u = 2^-24 (float) or 2^-53 (double) and
   gamma_n = n u / (1 - n u):  |sum - S| <= gamma_(L-1) S, element by element, wherever sdft_sdft_n is bit-identical to the
   reference (FD float, FD double with option "carry" = 1, calls shorter than 512 samples); elsewhere the term deviation of
   sdft_hip_sdft_power_n comes on top: 2.1e-11 of the largest power, times L.  The same plan, options and input give the same bits
   on every run (no floating-point atomics: pieces of a window are added in ascending time order).
   The stream state afterwards is the one sdft_sdft_n of the same samples leaves, so any other entry point may follow.  samples
   and sums may each be host or device memory (option "async" applies to device pointers).  The call is never resident,
   pipelined or fused and always runs its own kernel ("last_kernel" = 6).  Returns the number of rows written (0 only for
   nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan, every == 0, nbins == 0,
   bin0 + nbins > dftsize, or sums == NULL with rows > 0. */
long sdft_hip_sdft_power_sum_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                               const sdft_size_t every, const sdft_size_t first,
                               const sdft_size_t bin0, const sdft_size_t nbins,
                               sdft_fd_t* sums) SDFT_HIP_SYMBOL(sdft_power_sum_n);

/* ---- peak-hold analysis ----------------------------------------------------------------------------
   sdft_hip_sdft_power_peak_n holds the largest (hold = sdft_hip_hold_max: the peak spectrum of a spectrum analyser, crest factor
   against the mean) or the smallest (hold = sdft_hip_hold_min: the noise-floor tracker of minimum statistics) |X|^2 over windows
   of rows.  Grid, windows, head row, rows = (first > 0 && nsamples > 0 ? 1 : 0) + (rows of sdft_hip_sdft_every_n), the next
   call's first, the band, every > nsamples, host or device pointers (option "async" applies to device pointers) and the layout
   -- peaks is [rows][nbins], dense, aligned to sizeof(sdft_fd_t) only; batched plans: samples [channels][nsamples], peaks
   [channels][rows][nbins] -- are sdft_hip_sdft_power_sum_n's, unchanged.  Row r holds, for bin0 <= k < bin0 + nbins, the extreme
   over the r-th window of p[t][k], the value sdft_hip_sdft_power_n stores at every == 1, first == 0 (in sdft_fd_t: two rounded
   products, one rounded sum, no fused multiply-add).  One rule combines a held value m with a term p, in the kernels and for
   the host:
     max:  m = (p > m || p != p) ? p : m          min:  m = (p < m || p != p) ? p : m
   A window that holds a NaN term gives NaN (payload unspecified); otherwise the result is exactly one of the window's terms.
   Powers are +0 or larger, so signed zeros do not occur.  Every window has a sample, so the accumulators' start (-inf for max,
   +inf for min) never reaches the output.  With first > 0, row 0 completes the previous call's last row: the host combines the
   two by the same rule (fmax / fmin of finite values).
   Promised: (1) The same plan, options and input give the same bits on every run.  (2) every == 1 with first == 0 gives
   sdft_hip_sdft_power_n's values bit for bit, for either hold.  (3) Wherever sdft_sdft_n is bit-identical to the reference (FD
   float, FD double with option "carry" = 1, calls shorter than 512 samples) the value is the largest / smallest of the
   reference's powers over the window, bit for bit, for any every, first, band, cut of time into chunks, host staging and cut of a
   stream into calls: max and min are associative and commutative, so no order of combination shows.  (4) On the other routes
   the value is bit for bit the extreme of what sdft_hip_sdft_power_n stores at every == 1 when both calls cut time into chunks
   of the same length ("last_chunk_len"), and within 2.1e-11 of the call's largest power of the reference's extreme
   (sdft_hip_sdft_power_n's term deviation, with no factor for the window's length: |max a - max b| <= max |a - b|).  (5) The
   stream state afterwards is the one sdft_sdft_n of the same samples leaves -- bins outside the band step every sample too --
   so any other entry point may follow.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 11).  Returns the number of
   rows written (0 only for nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan,
   every == 0, nbins == 0, bin0 + nbins > dftsize, hold neither 0 nor 1, or peaks == NULL with rows > 0. */
enum sdft_hip_hold { sdft_hip_hold_max = 0, sdft_hip_hold_min = 1 };
long sdft_hip_sdft_power_peak_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                                const sdft_size_t every, const sdft_size_t first,
                                const sdft_size_t bin0, const sdft_size_t nbins,
                                const int hold, sdft_fd_t* peaks) SDFT_HIP_SYMBOL(sdft_power_peak_n);

/* ---- smoothed power analysis -----------------------------------------------------------------------
   The third detector of a spectrum analyser, beside the linear average (sdft_hip_sdft_power_sum_n) and the peak hold
   (sdft_hip_sdft_power_peak_n): the exponential average, the recursive periodogram of noise trackers (minimum statistics takes its
   minimum over this estimate), decision-directed SNR estimators, AGC and VAD front ends and spectrograms with a time constant,
     s[t][k] = a * s[t-1][k] + (1 - a) * |X[t][k]|^2
   advanced at EVERY sample of the call -- a sliding DFT has a spectrum at every sample -- and kept on a row grid, without storing
   a power per sample.  sdft_hip_sdft_power_smooth_n takes its grid (sampled: no head row, no windows), rows and the next call's
   first from sdft_hip_sdft_every_n and every > nsamples, the band and the pointer rules (host or device memory, each pointer on its
   own; option "async" applies to device pointers; smooth may be NULL when the call keeps no row) from sdft_hip_sdft_power_n,
   unchanged.  smooth is [rows][nbins], dense, aligned to sizeof(sdft_fd_t) only; batched plans: samples [channels][nsamples],
   smooth [channels][rows][nbins].
   The value, exactly.  Let p[t][k] be what sdft_hip_sdft_power_n stores at every == 1, first == 0.  In sdft_fd_t, with no fused
   multiply-add:
     a = (sdft_fd_t)decay     b = (sdft_fd_t)1 - a     s[-1] = state (zero if state == NULL)
     s[t] = fl( fl(a * s[t-1]) + fl(b * p[t]) )
   Row r is s at sample first + r * every, after that sample's update.  state is [channels][nbins] (the bins of the band only),
   read and written: on entry s before the call's first sample, on return s after its last.  It may be host or device memory
   whatever the other pointers are.  NULL: the call starts from zero and drops the end value.  A call that keeps no row still
   advances state.  A stream cut into calls passes state and sdft_hip_sdft_every_n's next first along.  exp(-1 / tau) is the decay of
   a time constant of tau samples.  A NaN or infinite power stays in s from then on.
   A call on host memory beyond option "stage_bytes" goes in time segments, calls in sequence with state passed along on the
   device; "last_segments" then answers their number.
   A long call cuts time into chunks ("last_chunks"); every chunk but the first runs the recursion from +0, and two small ordered
   kernels carry s across the chunks (the recursion is linear in s): a scan of the chunks' end values in ascending order, then
   smooth = fl(smooth + fl(P[j] * S)) for the rows of the later chunks, P[j] = fl(a^j) and S the value before the row's chunk.
   Six things are promised.
   (1) The same plan, options and input give the same bits on every run: no atomics.
   (2) A call of one time chunk ("last_chunks" = 1; every call shorter than 512 samples is one) is bit for bit the sequential
       expression above, evaluated on the reference's powers, wherever sdft_sdft_n is bit-identical to the reference (FD float, FD
       double with option "carry" = 1, calls shorter than 512 samples) -- for any every, first, band, pointer placement and staging.
   (3) A stream cut into one-chunk calls that pass state and the next first along has the bits of that sequential loop over the
       whole signal, wherever it is cut.
   (4) decay == 0 gives sdft_hip_sdft_power_n's values bit for bit for finite powers, on every route and any chunking (b == 1,
       P[j >= 1] == 0, and adding +0 changes nothing): those of the reference on the bit-identical routes, elsewhere what
       sdft_hip_sdft_power_n stores when it cuts time into chunks of the same length ("last_chunk_len"; at every == 1 it does).
   (5) Calls of several chunks: with u = 2^-24 (float) or 2^-53 (double), s the exact recursion on the sdft_fd_t terms and the
       rounded coefficients and M the largest of the incoming state and s[tau], tau <= t, barring underflow
         |smooth - s| <= 8 u M / (1 - a)
       (to first order 2 for the recursion itself, 3 for the scan, 3 (1 - a) for the last step; DESIGN.md has the derivation), and
       likewise the returned state.  On the routes that are not bit-identical the power call's term deviation comes on top: 2.1e-11
       of the largest power, with no factor 1 / (1 - a) because b / (1 - a) = 1.
   (6) The stream state of every channel is afterwards the one sdft_sdft_n of the same samples leaves -- bins outside the band
       step every sample too -- so any other entry point may follow.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 15).  Returns the number of rows
   written (0 for nsamples == 0), or -1 with sdft_hip_last_error() set, the stream state and *state untouched: a NULL plan,
   every == 0, nbins == 0, bin0 + nbins > dftsize, a decay that is NaN, negative or not below 1 after rounding to sdft_fd_t (a == 1
   never forgets), smooth == NULL with rows > 0, or a workspace that cannot be reserved. */
long sdft_hip_sdft_power_smooth_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                                  const sdft_size_t every, const sdft_size_t first,
                                  const sdft_size_t bin0, const sdft_size_t nbins,
                                  const double decay, sdft_fd_t* state, sdft_fd_t* smooth) SDFT_HIP_SYMBOL(sdft_power_smooth_n);

/* ---- smoothed peak-hold analysis -------------------------------------------------------------------
   What hosts compose from the three detectors above: the smallest (hold = sdft_hip_hold_min: the noise floor of minimum
   statistics, which takes its minimum over the smoothed estimate, not over raw powers) or the largest (hold = sdft_hip_hold_max:
   smoothed max-hold, envelope peak) of the SMOOTHED power over windows of samples, without storing a smoothed row per sample.
   The sequence is sdft_hip_sdft_power_smooth_n's, exactly: with p[t][k] what sdft_hip_sdft_power_n stores at every == 1,
   first == 0, in sdft_fd_t and with no fused multiply-add,
     a = (sdft_fd_t)decay     b = (sdft_fd_t)1 - a     s[-1] = state (zero if state == NULL)
     s[t] = fl( fl(a * s[t-1]) + fl(b * p[t]) )          at EVERY sample
   The grid, the windows, the head row, rows = (first > 0 && nsamples > 0 ? 1 : 0) + (rows of sdft_hip_sdft_every_n), the next
   call's first, every > nsamples, the band, host or device pointers (option "async" applies to device pointers) and the layout
   -- peaks is [rows][nbins], dense, aligned to sizeof(sdft_fd_t) only; batched plans: samples [channels][nsamples], peaks
   [channels][rows][nbins] -- are sdft_hip_sdft_power_peak_n's, unchanged.  Row r holds, for bin0 <= k < bin0 + nbins, the extreme
   by that call's rule (a NaN sticks, anything else is one of the terms) over the r-th window of s[t][k], s[t] taken after sample
   t's update.  state is [channels][nbins] (the bins of the band only), read and written as by sdft_hip_sdft_power_smooth_n: on
   entry s before the call's first sample, on return s after its last; host or device memory whatever the other pointers are;
   NULL: the call starts from zero and drops the end value.  A stream cut into calls passes state and the next first along and
   combines a call's head row (first > 0) with the previous call's last row by fmax / fmin.  s does not restart at a window: only
   the held extreme does.  A call on host memory beyond option "stage_bytes" goes in time segments, with state passed along on
   the device and head rows joined by the rule; "last_segments" then answers their number.
   A long call cuts time into chunks ("last_chunks").  The extreme of s over a window cannot be formed from a recursion started
   at +0 and corrected afterwards, so here the carries come before the rows: a first pass steps the recursion of every chunk for
   its end value only and writes no row, an ordered scan turns the end values into S_c, the value of s before chunk c (the scan
   of sdft_hip_sdft_power_smooth_n), and a second pass steps every chunk again from S_c and holds.  No row is corrected
   afterwards, and a long call steps the recurrence twice.
   Promised.
   (1) The same plan, options and input give the same bits on every run: no atomics.
   (2) A call of one time chunk ("last_chunks" = 1; every call shorter than 512 samples is one) is bit for bit the extreme over
       each window of the sequential expression above, evaluated on the reference's powers, wherever sdft_sdft_n is bit-identical
       to the reference (FD float, FD double with option "carry" = 1, calls shorter than 512 samples) -- for any every, first,
       band, hold, pointer placement and staging -- and the returned state is the loop's end value.  every == 1, first == 0 then
       gives sdft_hip_sdft_power_smooth_n's rows bit for bit.
   (3) A stream cut into one-chunk calls that pass state and the next first along, head rows joined by fmax / fmin, has the bits
       of (2) over the whole signal, wherever it is cut.
   (4) decay == 0 gives sdft_hip_sdft_power_peak_n's values bit for bit for finite powers, on every route and any chunking.
   (5) Calls of several chunks hold exactly: the rows at (every, first) are bit for bit the extreme over each window of the rows
       the same call gives at (1, 0) when both cut time alike ("last_chunk_len"), and the returned state is the last of those
       rows.  Against the exact recursion: with u = 2^-24 (float) or 2^-53 (double), s the exact recursion on the sdft_fd_t terms
       and the rounded coefficients, peak its extreme over the window and M the largest of the incoming state and s[tau],
       tau <= t, barring underflow
         |peaks - peak| <= 8 u M / (1 - a)
       and likewise the returned state (|ext(x') - ext(x)| <= max |x' - x|; inside a chunk the values are the sequential
       recursion from S_c, so an element's error is a convex mix of the scan's, 5, and the recursion's own, 2 -- DESIGN.md has
       the derivation; 8 is kept so that one bound serves both smoothed calls).  On the routes that are not bit-identical the
       power call's term deviation comes on top: 2.1e-11 of the largest power, with no factor 1 / (1 - a).
   (6) The stream state of every channel is afterwards the one sdft_sdft_n of the same samples leaves -- bins outside the band
       step every sample too -- so any other entry point may follow.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 17).  Returns the number of rows
   written (0 only for nsamples == 0), or -1 with sdft_hip_last_error() set, the stream state and *state untouched: a NULL plan,
   every == 0, nbins == 0, bin0 + nbins > dftsize, hold neither 0 nor 1, a decay that is NaN, negative or not below 1 after
   rounding to sdft_fd_t, peaks == NULL with rows > 0, or a workspace that cannot be reserved. */
long sdft_hip_sdft_smooth_peak_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                                 const sdft_size_t every, const sdft_size_t first,
                                 const sdft_size_t bin0, const sdft_size_t nbins,
                                 const double decay, const int hold,
                                 sdft_fd_t* state, sdft_fd_t* peaks) SDFT_HIP_SYMBOL(sdft_smooth_peak_n);

/* ---- power-moments analysis ------------------------------------------------------------------------
   The one statistic of the power that no pooled output yields because it is not linear in it: the second moment.  With the sum
   of the power it gives the variance of the power per bin, the spectral kurtosis (the RFI flagger of radio astronomy, the
   transient and bearing-fault detector of vibration analysis, a stationarity test on a PSD estimate) and the variance of a Welch
   estimate -- from ONE recurrence, without storing a power per sample.
   sdft_hip_sdft_power_moments_n takes its grid, windows, head row, rows = (first > 0 && nsamples > 0 ? 1 : 0) + (rows of
   sdft_hip_sdft_every_n), the next call's first, the band, every > nsamples and the pointer rules (host or device memory; option
   "async" applies to device pointers) from sdft_hip_sdft_power_sum_n, unchanged.  moments is [rows][nbins][2] of sdft_fd_t, dense,
   aligned to sizeof(sdft_fd_t) only; batched plans: samples [channels][nsamples], moments [channels][rows][nbins][2].  The pair of
   a window and a bin holds s1 at [..][0] and s2 at [..][1]:
     p  = the value sdft_hip_sdft_power_n stores at every == 1, first == 0:  fl( fl(re*re) + fl(im*im) )
     q  = fl(p * p)
     s1 = the sum of p over the window, formed exactly as sdft_hip_sdft_power_sum_n forms it
     s2 = the sum of q, accumulated in sdft_fd_t in the same order
   No fused multiply-add anywhere and no floating-point atomics; pieces of a window that a time chunk cuts are added in ascending
   time order.  Sums are returned, not means; with first > 0, row 0 completes the previous call's last row and the host adds both
   components.  q overflows in IEEE fashion (FD float: p > 1.8e19) and gives inf; nothing else is done about it.
   Six things are promised.
   (1) The same plan, options and input give the same bits on every run.
   (2) moments[..][0] is sdft_hip_sdft_power_sum_n's output bit for bit, for the same plan, options, samples, grid and band, on
       every route, as long as both calls cut time into chunks of the same length ("last_chunk_len") and run as one segment: true
       of device pointers, and of host memory within "stage_bytes".  The call takes that call's chunk choice and none of its own.
   (3) At every == 1, first == 0, s1 is sdft_hip_sdft_power_n's value and s2 is fl(p * p) of it, bit for bit, wherever sdft_sdft_n
       is bit-identical to the reference (FD float, FD double with option "carry" = 1, calls shorter than 512 samples) -- for any
       cut of time into chunks, any host staging and any cut of a stream into calls.  On the other routes they are those
       expressions on what sdft_hip_sdft_power_n stores on a twin plan that cuts time alike.
   (4) On the bit-identical routes and for other grids, with L the window's length, u = 2^-24 (float) or 2^-53 (double),
       gamma_n = n u / (1 - n u), and S1, S2 the exact sums of the sdft_fd_t terms p and q (all of them non-negative):
       |s1 - S1| <= gamma_(L-1) * S1   and   |s2 - S2| <= gamma_(L-1) * S2.
   (5) On the other routes sdft_hip_sdft_power_n's term deviation comes on top: with pmax the call's largest power and
       delta = 2.1e-11 * pmax,  L * delta  for s1 (as the pooled call has it) and  L * delta * (2 * pmax + delta)  for s2
       (from |p'^2 - p^2| = |p' - p| * |p' + p|).
   (6) The stream state of every channel is afterwards the one sdft_sdft_n of the same samples leaves -- bins outside the band
       step every sample too.  Any other entry point may follow.
   Consecutive rows of a sliding DFT overlap in all but one sample: an estimator built on s1 and s2 (the spectral kurtosis) keeps
   its mean for Gaussian noise, but not the variance a textbook derives for independent spectra.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 13).  Returns the number of rows
   written (0 only for nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan,
   every == 0, nbins == 0, bin0 + nbins > dftsize, moments == NULL with rows > 0, or a workspace that cannot be reserved. */
long sdft_hip_sdft_power_moments_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                                   const sdft_size_t every, const sdft_size_t first,
                                   const sdft_size_t bin0, const sdft_size_t nbins,
                                   sdft_fd_t* moments) SDFT_HIP_SYMBOL(sdft_power_moments_n);

/* ---- filterbank analysis ---------------------------------------------------------------------------
   Pooling of |X|^2 over frequency: mel, Bark and fractional-octave band energies, or the total power of a row, without storing
   and re-reading the powers.  A filterbank belongs to the plan.  sdft_hip_set_filterbank installs (copies) one; all four pointers
   are HOST memory.  Band b covers the bins band_bin0[b] <= k < band_bin0[b] + band_nbins[b] with the weights
   weights[off_b + (k - band_bin0[b])], off_b = band_nbins[0] + ... + band_nbins[b - 1].  Bands may overlap, repeat, come in any
   order and need not cover the spectrum; weights may be negative or zero.  nbands == 0 removes the filterbank.  Batched plans:
   one filterbank for all channels.  Returns 0, or -1 with sdft_hip_last_error() set and the plan's previous filterbank untouched:
   a NULL plan, a NULL array with nbands > 0, band_nbins[b] == 0, band_bin0[b] + band_nbins[b] > dftsize (or tables beyond 2^31
   bands / 2^32 weights).  sdft_hip_filterbank_bands: the installed filterbank's bands, 0 for none or a NULL plan. */
int         sdft_hip_set_filterbank(sdft_t* sdft, const sdft_size_t nbands, const sdft_size_t* band_bin0,
                                    const sdft_size_t* band_nbins, const sdft_fd_t* weights) SDFT_HIP_SYMBOL(set_filterbank);
sdft_size_t sdft_hip_filterbank_bands(const sdft_t* sdft) SDFT_HIP_SYMBOL(filterbank_bands);
/* sdft_hip_sdft_filterbank_n writes the band sums of the installed filterbank on the row grid of sdft_hip_sdft_every_n and
   sdft_hip_sdft_power_n: grid, rows, streaming and the next call's first are exactly theirs.  Let p[r][k] be what
   sdft_hip_sdft_power_n stores for row r and bin k.  Then
     out[r][b] = sum over the band's bins of fl(w * p)
   formed in sdft_fd_t: each product is rounded once, then the rounded products are added (no fused multiply-add anywhere).
   out is [rows][nbands] real numbers, dense, aligned to sizeof(sdft_fd_t) only; batched plans: samples [channels][nsamples], out
   [channels][rows][nbands].  samples and out may each be host or device memory (option "async" applies to device pointers); out
   may be NULL when the call keeps no row.
   Order of additions: the order inside a band is the library's own (a band's bins are added in ascending order inside a tile of
   bins, then the tiles' sums in ascending order).  Three things are promised.  (1) The same plan, options and input give the same
   bits on every run: no floating-point atomics.  (2) A row's bits depend only on the plan, the filterbank and that row's powers --
   not on nsamples, every, first, the time chunking, or where a stream was cut into calls.  (3) A band of one bin is exactly
   fl(w p), a band of two bins exactly fl(fl(w0 p0) + fl(w1 p1)): a filterbank of dftsize one-bin bands of weight 1 returns
   sdft_hip_sdft_power_n's values bit for bit on every route.
   Accuracy: with L the band's bin count, u = 2^-24 (float) or 2^-53 (double), gamma_n = n u / (1 - n u), eta the smallest positive
   subnormal of sdft_fd_t and T = sum |w_k| p_k in the reals:  |out - sum w_k p_k| <= gamma_L T + L eta, element by element (L
   rounded products and at most L - 1 additions, in any order), where p is the reference's wherever sdft_sdft_n is bit-identical
   to it (FD float, FD double with option "carry" = 1, calls shorter than 512 samples); elsewhere the term deviation of
   sdft_hip_sdft_power_n comes on top: 2.1e-11 of the largest power of the call's grid, times sum |w_k|.
   Bands that a tile boundary of the plan's geometry cuts pass through a plan-owned workspace of [channels][rows][pieces] numbers,
   grown on demand; a call whose workspace would exceed 64 MiB runs its time chunks in row segments (several launches that reuse
   the workspace), with the same bits and the same state.
   The stream state afterwards is the one sdft_sdft_n of the same samples leaves, so any other entry point may follow.  The call
   is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 7).  Returns the number of rows written
   (0 for nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan, no filterbank
   installed, every == 0, or out == NULL with rows > 0. */
long sdft_hip_sdft_filterbank_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                                const sdft_size_t every, const sdft_size_t first,
                                sdft_fd_t* out) SDFT_HIP_SYMBOL(sdft_filterbank_n);

/* ---- band-peak analysis ----------------------------------------------------------------------------
   The question a sliding DFT is most often run for: which bin is the peak, in each band, at each row, and how large is it --
   pitch and tone tracking, DTMF and FSK detection, dominant-frequency tracking, peak picking for sinusoidal modelling -- without
   storing and re-reading a power per bin.  sdft_hip_sdft_band_peak_n uses the plan's installed filterbank
   (sdft_hip_set_filterbank) and takes its grid, rows, streaming rule, the next call's first, every > nsamples and the pointer
   rules (host or device memory; option "async" applies to device pointers; peaks may be NULL when the call keeps no row) from
   sdft_hip_sdft_filterbank_n, unchanged.  peaks is [rows][nbands][2] of sdft_fd_t, dense, aligned to sizeof(sdft_fd_t) only;
   batched plans: samples [channels][nsamples], peaks [channels][rows][nbands][2].  [..][0] is the value, [..][1] the absolute bin
   index, stored as an exactly representable integer of sdft_fd_t; the call is refused when dftsize > 2^24 on an FD float plan.
   The value, exactly.  Let p_k be what sdft_hip_sdft_power_n stores for the row and bin k, w_k the band's weight for that bin and
   v_k = fl(w_k * p_k): one rounded product, no fused multiply-add.  The band's bins are scanned in ascending order:
     (m, i) = (v_first, first bin)
     for each later k:  if (v_k > m) || (v_k != v_k && m == m)  then (m, i) = (v_k, k)
   That is the lowest bin that attains the largest value, the lowest NaN bin if any value is NaN, and the first bin's bits among
   equal zeros of either sign: in numpy, i = np.argmax(v) and m = v[i].  The pieces of a band that a tile boundary of the plan's
   geometry cuts are combined in ascending tile order by the same rule, the lower piece the held pair and the higher piece the
   candidate; the rule is strict, so a tie across a tile boundary keeps the lower bin.
   Six things are promised.
   (1) The same plan, options and input give the same bits on every run: no atomics.
   (2) A row's pair depends only on the plan, the filterbank and that row's powers -- not on nsamples, every, first, the time
       chunking, the host staging, or where a stream was cut into calls.
   (3) Wherever sdft_sdft_n is bit-identical to the reference (FD float, FD double with option "carry" = 1, calls shorter than 512
       samples), value and bin are exactly the numpy expression on the reference's powers.  The value matches bit for bit; a
       NaN's payload is unspecified.
   (4) On the other routes value and bin are exactly that expression on what sdft_hip_sdft_power_n stores on a twin plan that cuts
       time into chunks of the same length ("last_chunk_len").  With pmax the largest power of the call's grid the value lies
       within 2.1e-11 * pmax * max|w| of the reference's (|max a - max b| <= max |a - b| and the power call's term deviation), and
       the bin can differ from the reference's only among bins whose reference values lie within twice that of the maximum.
   (5) A filterbank of dftsize one-bin bands of weight 1 returns sdft_hip_sdft_power_n's value bit for bit, with bin k, on every
       route.
   (6) The stream state of every channel is afterwards the one sdft_sdft_n of the same samples leaves.  Any other entry point may
       follow.
   Split bands pass through the filterbank call's plan-owned workspace with a pair per piece; a call whose workspace would exceed
   64 MiB runs its time chunks in row segments (several launches that reuse the workspace), with the same bits and the same state.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 14).  Returns the number of rows
   written (0 for nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan, no filterbank
   installed, every == 0, peaks == NULL with rows > 0, dftsize > 2^24 on an FD float plan, or a workspace that cannot be
   reserved. */
long sdft_hip_sdft_band_peak_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                               const sdft_size_t every, const sdft_size_t first,
                               sdft_fd_t* peaks) SDFT_HIP_SYMBOL(sdft_band_peak_n);

/* ---- pooled cross-spectrum analysis ----------------------------------------------------------------
   What relates the channels of a batched plan (sdft_hip_alloc_batch): the cross power spectral density
     S_ab[k] = sum over the samples t of a window of X_a[t][k] * conj(X_b[t][k])
   over Welch windows, without storing the complex rows of either channel.  With the auto-spectra S_aa and S_bb it gives
   coherence, transfer-function estimates, GCC-PHAT delays and the spatial covariance a beamformer needs.
   A list of channel pairs belongs to the plan.  sdft_hip_set_pairs installs (copies) one; both arrays are HOST memory.  Pairs may
   repeat, come in any order and have a == b (the auto-spectrum), so one call delivers S_aa, S_bb and S_ab from the same rows; a
   single-channel plan accepts only (0, 0).  npairs == 0 removes the list.  Returns 0, or -1 with sdft_hip_last_error() set and
   the previous list untouched: a NULL plan, a NULL array with npairs > 0, a channel index >= channels, more than 2^31 pairs.
   sdft_hip_pairs: the installed list's length, 0 for none or a NULL plan.
   Cost: every pair steps the recurrences of its two channels (one for a == b), so P pairs cost up to 2 P channels of
   sdft_hip_sdft_power_sum_n; a channel in no pair is stepped once more to keep its state.  The call is built for a few pairs per
   channel, not for an all-pairs covariance of many channels: that is sdft_hip_sdft_covariance_n below. */
int         sdft_hip_set_pairs(sdft_t* sdft, const sdft_size_t npairs,
                               const sdft_size_t* pair_a, const sdft_size_t* pair_b) SDFT_HIP_SYMBOL(set_pairs);
sdft_size_t sdft_hip_pairs(const sdft_t* sdft) SDFT_HIP_SYMBOL(pairs);
/* sdft_hip_sdft_cross_sum_n takes its grid, windows, head row, row count, streaming rule and the next call's first from
   sdft_hip_sdft_power_sum_n, unchanged: rows = (first > 0 && nsamples > 0 ? 1 : 0) + (rows of sdft_hip_sdft_every_n); sums are
   returned, not means; with first > 0, row 0 completes the previous call's last row (the host adds the two).
   Let A = (ar, ai) and B = (br, bi) be the windowed, weighted bins of the channels a and b of a pair as sdft_sdft_n stores them
   at sample t.  The term is A * conj(B), formed in sdft_fd_t with no fused multiply-add:
     re = fl( fl(ar*br) + fl(ai*bi) )        im = fl( fl(ai*br) - fl(ar*bi) )
   Row r of pair p holds, for bin0 <= k < bin0 + nbins, the sum of these terms over the r-th window, each component accumulated
   separately in sdft_fd_t; pieces of a window that a time chunk cuts are added in ascending time order (no floating-point
   atomics).  sums is [npairs][rows][nbins] complex numbers (re, im), dense, aligned to sizeof(sdft_fd_t) only; samples is
   [channels][nsamples].  samples and sums may each be host or device memory (option "async" applies to device pointers).
   Six things are promised.
   (1) The same plan, options and input give the same bits on every run.
   (2) Pair (a, a) has im == +0 exactly (for finite bins), and its re is formed from the same terms as sdft_hip_sdft_power_n's
       value: at every == 1, first == 0 it is that value bit for bit wherever the two calls start from the same carries -- on the
       bit-identical routes of (4) always, elsewhere when both cut time into chunks of the same length ("last_chunk_len").
   (3) Within one call, pair (b, a) is the complex conjugate of pair (a, b) bit for bit: the same re, im negated (as numbers: where
       two products cancel exactly both hold +0).  A repeated pair gives identical bits.
   (4) At every == 1, first == 0, each value is exactly the expression above on the two channels' sdft_sdft_n rows, wherever
       that call is bit-identical to the reference: FD float, FD double with option "carry" = 1, calls shorter than 512 samples.
   (5) Accuracy elsewhere on those bit-identical routes, per component: with L the window's length, u = 2^-24 (float) or 2^-53
       (double), gamma_n = n u / (1 - n u), T = sum |term| in the reals over the sdft_fd_t terms and S their exact sum,
       |sum - S| <= gamma_(L-1) T.  On the other routes the term deviation comes on top: the constant sdft_hip_sdft_power_n
       documents, 2.1e-11, times max|X_a| * max|X_b| over the call, times L (that call's derivation with |A||dB| + |B||dA| in
       place of 2|X||dX|).
   (6) The stream state afterwards is the one sdft_sdft_n of the same samples leaves for EVERY channel of the plan, whether it
       appears in no pair, in one or in many.  Any other entry point may follow.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 8).  Returns the number of rows
   written (0 for nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan, no pairs
   installed, every == 0, nbins == 0, bin0 + nbins > dftsize, or sums == NULL with rows > 0. */
long sdft_hip_sdft_cross_sum_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                               const sdft_size_t every, const sdft_size_t first,
                               const sdft_size_t bin0, const sdft_size_t nbins,
                               sdft_fdx_t* sums) SDFT_HIP_SYMBOL(sdft_cross_sum_n);

/* ---- smoothed cross-spectrum analysis ---------------------------------------------------------------
   The estimator an online multichannel host runs: the recursive cross-spectrum
     S_ab[t][k] = a * S_ab[t-1][k] + (1 - a) * X_a[t][k] conj(X_b[t][k])
   advanced at EVERY sample and kept on a row grid.  With S_aa and S_bb from the same call (the pairs (a, a) and (b, b)) it gives
   time-varying coherence, transfer functions and GCC-PHAT tracking; it is the forgetting-factor covariance of an online MVDR / GEV
   beamformer.  sdft_hip_sdft_cross_smooth_n uses the pair list of sdft_hip_set_pairs (repeats and a == b allowed, as for
   sdft_hip_sdft_cross_sum_n) and takes grid, rows, the next call's first, every > nsamples, the band and the pointer rules (host or
   device memory, each pointer on its own; option "async" applies to device pointers; smooth may be NULL when the call keeps no
   row) from sdft_hip_sdft_power_smooth_n, unchanged.  samples is [channels][nsamples]; smooth is [npairs][rows][nbins] complex
   (re, im), dense, aligned to sizeof(sdft_fd_t) only.
   The value, exactly.  With (re, im) the term of sdft_hip_sdft_cross_sum_n at sample t, A and B the windowed bins,
     re = fl( fl(A.re * B.re) + fl(A.im * B.im) )     im = fl( fl(A.im * B.re) - fl(A.re * B.im) )
     a = (sdft_fd_t)decay     b = (sdft_fd_t)1 - a
   each component separately runs s = fl( fl(a * s) + fl(b * term) ) in sdft_fd_t, no fused multiply-add.  Row r is s after the
   update of sample first + r * every.  state is [npairs][nbins] complex (the bins of the band only), read on entry and written on
   return, host or device memory whatever the other pointers are; NULL starts from zero and drops the end value.  It is written
   only after the whole call has succeeded.  A call that keeps no row still advances state.  A call on host memory beyond option
   "stage_bytes" goes in time segments with state passed along on the device; "last_segments" then answers their number.  A long
   call cuts time into chunks and carries s across them with the two ordered kernels of sdft_hip_sdft_power_smooth_n, which see a
   pair's row as 2 * nbins real numbers.
   Seven things are promised.
   (1) The same plan, options and input give the same bits on every run: no atomics.
   (2) A call of one time chunk ("last_chunks" = 1; every call shorter than 512 samples is one) is bit for bit the sequential
       expression above on the reference's rows, wherever sdft_sdft_n is bit-identical to the reference (FD float, FD double with
       option "carry" = 1, calls shorter than 512 samples) -- for any every, first, band, pointer placement and staging.
   (3) A stream cut into one-chunk calls that pass state and the next first along has the bits of that sequential loop over the
       whole signal, wherever it is cut.
   (4) Pair (a, a): re is sdft_hip_sdft_power_smooth_n's value for channel a bit for bit, given the same decay, the same grid and
       the re half of the state, on every route where both calls cut time alike ("last_chunk_len" equal); im stays +0 from a +0
       state.  Pair (b, a) equals the conjugate of pair (a, b) as numbers (zeros may differ in sign).  A repeated pair gives
       identical bits.
   (5) decay == 0 gives the every == 1 term of sdft_hip_sdft_cross_sum_n at the grid's samples, equal as numbers (a -0 term may
       come out as +0), on every route and any chunking.
   (6) Calls of several chunks: with u = 2^-24 (float) or 2^-53 (double), s the exact recursion on the sdft_fd_t terms and the
       rounded coefficients and M the running largest of the majorant m[t] = a * m[t-1] + b * |term[t]|, m[-1] = |state|, per
       component and barring underflow
         |smooth - s| <= 8 u M / (1 - a)
       (DESIGN.md has the derivation: that of sdft_hip_sdft_power_smooth_n with |s| <= m in the place of s >= 0), and likewise
       the returned state.  On the routes that are not bit-identical the cross-spectrum call's term deviation comes on top:
       2.1e-11 * max|X_a| * max|X_b|, with no factor 1 / (1 - a).
   (7) The stream state afterwards is the one sdft_sdft_n of the same samples leaves for EVERY channel of the plan, whether it
       appears in no pair, in one or in many.  Any other entry point may follow.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 16).  Returns the number of rows
   written (0 for nsamples == 0), or -1 with sdft_hip_last_error() set, the stream state and *state untouched: a NULL plan, no
   pairs installed, every == 0, nbins == 0, bin0 + nbins > dftsize, a decay that is NaN, negative or not below 1 after rounding to
   sdft_fd_t, smooth == NULL with rows > 0, or a workspace that cannot be reserved. */
long sdft_hip_sdft_cross_smooth_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                                  const sdft_size_t every, const sdft_size_t first,
                                  const sdft_size_t bin0, const sdft_size_t nbins,
                                  const double decay, sdft_fdx_t* state, sdft_fdx_t* smooth) SDFT_HIP_SYMBOL(sdft_cross_smooth_n);

/* ---- lag-product analysis --------------------------------------------------------------------------
   What a sliding DFT has over a hopped STFT is a row per sample, and the first thing a phase vocoder, a sinusoidal tracker, a
   reassignment or a Doppler (pulse-pair) estimator does with a row per sample is the phase advance of every bin from one sample to
   the next:
     R[k] = sum over the samples t of a window of X[t][k] * conj(X[t - 1][k])
   arg(R[k]) / (2 pi) * samplerate is the power-weighted mean frequency of bin k over the window (with hop 1: no unwrapping, no
   bin-centre correction), |R[k]| against sdft_hip_sdft_power_sum_n's sum its coherence.  The call keeps the phase that the power,
   pooled, peak-hold and filterbank calls discard, without storing the complex rows and with ONE recurrence per channel.
   sdft_hip_sdft_lag_sum_n takes its grid, windows, head row, row count, streaming rule, the next call's first, the band,
   every > nsamples and the pointer rules from sdft_hip_sdft_power_sum_n / sdft_hip_sdft_cross_sum_n, unchanged: rows =
   (first > 0 && nsamples > 0 ? 1 : 0) + (rows of sdft_hip_sdft_every_n); sums are returned, not means; with first > 0, row 0
   completes the previous call's last row (the host adds the two).
   Let A = (ar, ai) be the windowed, weighted bin sdft_sdft_n stores at sample t and B = (br, bi) the one it stores at sample
   t - 1.  The term is A * conj(B) in the cross-spectrum call's expression, formed in sdft_fd_t with no fused multiply-add:
     re = fl( fl(ar*br) + fl(ai*bi) )        im = fl( fl(ai*br) - fl(ar*bi) )
   Row r holds, for bin0 <= k < bin0 + nbins, the sum of these terms over the r-th window, each component accumulated separately
   in sdft_fd_t from a -0 start in ascending time order; pieces of a window that a time chunk cuts are added in ascending time
   order (no floating-point atomics).  sums is [rows][nbins] complex numbers (re, im), dense, aligned to sizeof(sdft_fd_t) only;
   batched plans: samples [channels][nsamples], sums [channels][rows][nbins], each channel by itself.  samples and sums may each
   be host or device memory (option "async" applies to device pointers).
   The row before the call's first sample is the row of the plan's state: the window applied to the demodulated state, which is
   acc where the cursor is 0 modulo 2 * dftsize and acc * conj(fid) elsewhere.  For a stream that is the last row the previous call
   produced, whichever entry point that call was; for a fresh or reset plan it is the zero row, so the first term is zero; after
   sdft_hip_set_state it is the row of the installed state.
   Five things are promised.
   (1) The same plan, options and input give the same bits on every run.
   (2) At every == 1, first == 0, each value is exactly the expression above on consecutive sdft_sdft_n rows, wherever that call
       is bit-identical to the reference: FD float, FD double with option "carry" = 1, calls shorter than 512 samples -- for any
       cut of time into chunks, any host staging and any cut of a stream into calls.  A term whose previous row is the zero row
       of a fresh plan is zero as a number; its sign is unspecified.
   (3) On those routes and for other grids, promise (5) of sdft_hip_sdft_cross_sum_n holds per component:
       |sum - S| <= gamma_(L-1) * sum |term|.
   (4) On the other routes that call's term deviation comes on top: 2.1e-11 times the call's largest |X|^2 times L.  The previous
       row at a chunk start comes from the chunk's own carry, which lies inside the same row deviation.
   (5) The stream state of every channel is afterwards the one sdft_sdft_n of the same samples leaves -- bins outside the band
       step every sample too.  Any other entry point may follow.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 12).  Returns the number of rows
   written (0 only for nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan,
   every == 0, nbins == 0, bin0 + nbins > dftsize, sums == NULL with rows > 0, or a workspace that cannot be reserved. */
long sdft_hip_sdft_lag_sum_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                             const sdft_size_t every, const sdft_size_t first,
                             const sdft_size_t bin0, const sdft_size_t nbins,
                             sdft_fdx_t* sums) SDFT_HIP_SYMBOL(sdft_lag_sum_n);

/* ---- array covariance analysis -----------------------------------------------------------------------
   The spatial covariance matrix per bin of an ARRAY of channels -- what MVDR / GEV beamformers, MUSIC and multichannel Wiener
   filters start from: the pooled cross-spectrum of ALL pairs of the array's channels.  As a pair list that costs two recurrences
   per pair; this call steps groups of channels instead (a wave takes a block of two groups, windows each channel once and forms
   every term between them in registers), so the recurrences grow with the number of blocks, not of pairs.
   An array belongs to the plan: an ordered list of nch DISTINCT channels of a batched plan, its elements.  sdft_hip_set_array
   installs (copies) one; chan is HOST memory, chan == NULL with nch > 0 means the channels 0 ... nch - 1, nch == 0 removes the
   list.  Returns 0, or -1 with sdft_hip_last_error() set and the previous list untouched: a NULL plan, an index >= channels, a
   repeated index, nch > channels.  The array is independent of the pair list of sdft_hip_set_pairs: both may be installed.
   sdft_hip_array_channels: the installed array's length, 0 for none or a NULL plan. */
int         sdft_hip_set_array(sdft_t* sdft, const sdft_size_t nch, const sdft_size_t* chan) SDFT_HIP_SYMBOL(set_array);
sdft_size_t sdft_hip_array_channels(const sdft_t* sdft) SDFT_HIP_SYMBOL(array_channels);
/* sdft_hip_sdft_covariance_n takes its grid, windows, head row, row count, streaming rule, the next call's first, the band
   arguments and the host / device pointer rules from sdft_hip_sdft_cross_sum_n, unchanged.
   cov is [T][rows][nbins] complex numbers (re, im), T = nch (nch + 1) / 2, dense, aligned to sizeof(sdft_fd_t) only: the upper
   triangle of the matrix in row-major order.  Element p(i, j) = i nch - i (i - 1) / 2 + (j - i), 0 <= i <= j < nch, holds the sum
   over each window of X_chan[i] * conj(X_chan[j]); the lower triangle is its conjugate, which the host mirrors.
   Three things are promised.
   (1) The same plan, options and input give the same bits on every run.
   (2) Element p(i, j) is, bit for bit, what sdft_hip_sdft_cross_sum_n returns for the pair (chan[i], chan[j]) from the same
       samples, wherever the two calls start from the same carries: on the bit-identical routes (FD float, FD double with option
       "carry" = 1, calls shorter than 512 samples) always, elsewhere when both cut time into chunks of the same length
       ("last_chunk_len"; option "chunk" sets it).  The call uses that call's term expression with the lower array index on
       side A (four rounded products, no fused multiply-add, -0 start), its additions in ascending time order, its workspace of
       cut windows and its ordered adder.  Hence p(i, i) has im == +0 and is the pooled power call's value, and promise (5) of
       sdft_hip_sdft_cross_sum_n (accuracy) holds for every element verbatim.
   (3) The stream state of every channel of the plan, in the array or not, is afterwards what sdft_sdft_n of the same samples
       leaves: every channel has exactly one writer.  Any other entry point may follow.
   Workspace (kept by the plan, grown on demand): where a call is cut into C > 1 time chunks, T * C * 2 * nbins complex numbers
   -- sdft_hip_sdft_cross_sum_n's, with T pairs.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 9).  Returns the number of rows
   written (0 for nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan, no array
   installed, every == 0, nbins == 0, bin0 + nbins > dftsize, cov == NULL with rows > 0, or a workspace that cannot be reserved. */
long sdft_hip_sdft_covariance_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                                const sdft_size_t every, const sdft_size_t first,
                                const sdft_size_t bin0, const sdft_size_t nbins,
                                sdft_fdx_t* cov) SDFT_HIP_SYMBOL(sdft_covariance_n);

/* ---- channel-mix analysis ------------------------------------------------------------------------------
   The step every consumer of the covariance call ends with -- an MVDR / GEV beamformer, a multichannel Wiener filter, a per-bin
   demixing matrix: a per-bin linear combination of the channels' spectra,
     Y_o[t][k] = sum over the elements i of W[o][i][k] * X_chan[i][t][k],
   formed in registers from the windowed bins, so that no channel's spectrum ever reaches memory.
   A mix belongs to the plan: an ordered list of nch DISTINCT channels of a batched plan (its elements; the rule is
   sdft_hip_set_array's: chan is HOST memory, chan == NULL means the channels 0 ... nch - 1) and nout weight tables.  weights is
   [nout][nch][dftsize] complex numbers in HOST memory and is applied as written: a host that wants w^H x passes conjugates.
   sdft_hip_set_mix installs (copies) one; nout == 0 removes the mix, whatever the other arguments.  Returns 0, or -1 with
   sdft_hip_last_error() set and the previous mix untouched: a NULL plan, weights == NULL with nout > 0, nch == 0 with nout > 0,
   nch > channels, an index >= channels, a repeated index, more than 65535 outputs, or a table that cannot be reserved.  The mix is
   independent of the pair list, the array and the filterbank: all may be installed.
   sdft_hip_mix_outputs: the installed mix's nout, 0 for none or a NULL plan. */
int         sdft_hip_set_mix(sdft_t* sdft, const sdft_size_t nout, const sdft_size_t nch, const sdft_size_t* chan,
                             const sdft_fdx_t* weights) SDFT_HIP_SYMBOL(set_mix);
sdft_size_t sdft_hip_mix_outputs(const sdft_t* sdft) SDFT_HIP_SYMBOL(mix_outputs);
/* sdft_hip_sdft_mix_n takes its grid, row count, streaming rule and the next call's first from sdft_hip_sdft_every_n (sampled
   rows, not pooled windows), and the band arguments and the host / device pointer rules from sdft_hip_sdft_power_n.  samples is
   [channels][nsamples]; out is [nout][rows][nbins] complex numbers (re, im), dense, aligned to sizeof(sdft_fd_t) only; it may be
   NULL when the call keeps no row.
   The value, exactly.  Let y_i = (yr, yi) be the windowed, weighted bin of element i as sdft_sdft_n stores it at the grid sample,
   and w_i = (wr, wi) its weight for this output and bin.  The term is formed in sdft_fd_t with no fused multiply-add,
     re = fl(fl(wr * yr) - fl(wi * yi))        im = fl(fl(wr * yi) + fl(wi * yr)),
   and the output is the sequential sum of the terms: the accumulator starts at -0, the terms are added in ascending element order
   i = 0 ... nch - 1, each component by itself, in sdft_fd_t.  The bits do not depend on how the kernel groups channels or outputs.
   (1) The same plan, options and input give the same bits on every run (no atomics).
   (2) The value is exactly that expression on the channels' sdft_sdft_n rows wherever that call is bit-identical to the
       reference: FD float, FD double with option "carry" = 1, calls shorter than 512 samples -- for any every, first, band, cut of
       time into chunks, or cut of a stream into calls.  A row's bits depend only on the plan, the mix and that row's bins.
   (3) A one-hot mix (weight 1 for one element, 0 for the others) returns sdft_hip_sdft_every_n's row of that channel as numbers,
       for finite bins; zeros may differ in sign.
   (4) On the other routes the row deviation sdft_hip_sdft_every_n documents comes on top: with E_i = 1e-11 times the largest
       |bin| of channel chan[i] over the call, each component moves by at most sum over i of (|wr_i| + |wi_i|) E_i  (from
       |d re| <= |wr| |d yr| + |wi| |d yi|), plus what the 3 nch roundings of a component make of it: gamma_(nch + 1) times
       sum over i of (|wr_i| + |wi_i|) (|yr_i| + |yi_i|), gamma_n = n u / (1 - n u), u = 2^-53.
   (5) The stream state of EVERY channel of the plan, in the mix or not, is afterwards what sdft_sdft_n of the same samples
       leaves: every channel has exactly one writer.  Any other entry point may follow.
   No workspace: the running sum of a row lives in the row itself between the groups of channels a wave takes.  Rows on their way
   to HOST memory are formed in device scratch, segment by segment, and copied out.
   The call is never resident, pipelined or fused and always runs its own kernel ("last_kernel" = 10).  Returns the number of rows
   written (0 for nsamples == 0), or -1 with sdft_hip_last_error() set and the stream state untouched: a NULL plan, no mix
   installed, every == 0, nbins == 0, bin0 + nbins > dftsize, out == NULL with rows > 0. */
long sdft_hip_sdft_mix_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples,
                         const sdft_size_t every, const sdft_size_t first,
                         const sdft_size_t bin0, const sdft_size_t nbins,
                         sdft_fdx_t* out) SDFT_HIP_SYMBOL(sdft_mix_n);

/* ---- streams ---------------------------------------------------------------------------------
   Every plan owns a HIP stream.  Calls with host pointers always return with the output
   complete.  Calls with device pointers do too unless option "async" is 1; then they return after
   enqueueing and sdft_hip_synchronize() (or the caller's own stream sync) completes them.
   Asynchronous analysis calls on the plan's OWN stream may run on internal streams beside it (option "pipeline"):
   sdft_hip_synchronize() and every later call of the plan wait for them, and so does the null stream (they are blocking
   streams like the plan's own: a plain hipMemcpy of the results sees them complete); a host that wants to queue its own work behind
   a call asks for the stream with sdft_hip_get_stream() -- from then on every kernel of the plan is on that stream -- or
   hands the plan a stream of its own with sdft_hip_set_stream(). */
int   sdft_hip_set_stream(sdft_t* sdft, void* hip_stream /* hipStream_t */) SDFT_HIP_SYMBOL(set_stream);
void* sdft_hip_get_stream(sdft_t* sdft) SDFT_HIP_SYMBOL(get_stream);
int   sdft_hip_synchronize(sdft_t* sdft) SDFT_HIP_SYMBOL(synchronize);
/* measurement aid: the reference driver's loop (test/test.c:69-83: sdft_sdft_n + sdft_isdft_n per hop of `hop` samples on one
   matrix) run `hops` times from C, as a C host runs it; seconds, or -1 */
double sdft_hip_time_hops(sdft_t* sdft, size_t hops, size_t hop, const sdft_td_t* samples, sdft_fdx_t* dfts, sdft_td_t* out) SDFT_HIP_SYMBOL(time_hops);

/* ---- options -----------------------------------------------------------------------------------
   Twenty-two keys.  The first twelve are for hosts; the defaults are the safe and (but for the host-memory choices, which only the host can
   make) the fast ones:
   "async"         0|1   see above
   "pipeline"      asynchronous analysis calls on the plan's own stream into matrices that do not overlap (a host that alternates between two
                       matrices) overlap: the state after a call comes from a small kernel ahead of the call's rows, the rows of consecutive
                       calls run on two internal streams; every other call of the plan and sdft_hip_synchronize wait for them.
                       1 (default) = calls of less than 2^29 bins, where the next call fills what a launch leaves idle -- a fixed 20-30 us per call:
                       n = 48 000, m = 1024: 82 against 75 % of the HBM peak, n = 131 072: 85 against 76 % (profiles/r06_pipelined_calls.txt); longer calls
                       amortise that by themselves and stay on one stream (n = 1e6: a tie at 85 %).  2 = calls of any
                       length, 0 = never.  Asynchronous synthesis calls that come back to back take the two streams in turn as well; a synthesis
                       never runs beside an analysis; either kind only once two of them have come in a row.  Off by itself on a caller's stream,
                       once sdft_hip_get_stream has been called, and with profiling.  get_option "last_pipelined", "pipelined_calls",
                       "pipelined_inverse_calls", "pipelined_ordered", "pipeline_streams" (10 x kind + pairs tried; kind 1 = ordinary
                       streams, 2 = by priority: what the plan falls back to when no ordinary pair runs concurrently, 0 = none found)
   "carry"         0 = chunk-parallel carries (FD double default; <= 1e-11 relative deviation from the
                       serial reference), 1 = exact serial carry pass (bit-identical; FD float always)
   "float_carry_parallel"  0 (default) | 1 = FD float plans take the chunk-parallel carries too: long calls run at
                       twice the speed and land closer to the double-precision result than the reference's float
                       arithmetic does, but NOT within 1e-4 of the float reference (which itself drifts about 2e-4
                       of the largest bin per 262144 samples); the state then differs from the reference's by the same
   "exact_inverse" 1 (default) = synthesis gives the reference's bits (bins of a row added in the reference's order, or --
                       float samples from double bins, up to 500 000
                       rows -- a tree sum whose rounding interval proves the reference's float, rows it cannot prove
                       added in order), 0 = wave-parallel tree sum, unverified
   "host_copy"     0 (default) = copies between the caller's host memory and the device go through pinned 2 MiB pieces of the
                       plan (beyond 64 KiB): the runtime is never handed caller memory to pin.  Its own path for pageable
                       memory pins the pages and remembers the pin by address; a host that frees the buffer, lets the heap
                       shrink and gets the address back later makes the next copy fault the GPU (process gone).  1 = the
                       runtime's path: faster (the reference driver's hop, 1.6 MB out and back: 128 against
                       197 us; long copies 55 against 26 GB/s) and safe for a host that allocates its buffers once and
                       keeps them, like the reference's driver (test/test.c:62-83) -- as is "host_register" = 1 (110 us);
                       get_option "host_copies_staged" counts the copies that went through the pieces
   "host_register" 0 (default) = host buffers are copied through staging buffers; 1 = host buffers of 1 MiB and more are
                       registered in place once (hipHostRegister, the last 8 page ranges are remembered) and the kernels
                       read and write them over PCIe: 139 -> 111 us per 100-sample hop of the reference's test driver.
                       ONLY for hosts that keep their buffers allocated while the plan lives (like test/test.c:62-64 of the
                       reference): a registration does not survive free() + malloc() handing the same address out again.
   "copy_threads"  2 (default) = worker threads of the copies between the caller's host memory and the plan's pinned slots (the host's
                       copy of one piece overlaps the DMA of the next; a hop-sized matrix is copied by the workers and the caller
                       together); 0 = the calling thread alone
   "pinned_io"     1 (default) = host sample buffers of up to 64 KiB (a hop of a host signal, the sample of sdft_sdft, the
                       result of sdft_isdft) travel through a pinned scratch of the plan that the kernels access directly
   "spin"          1 (default) = synchronous calls never sleep on the stream while they can still be running: calls of one
                       time chunk poll a completion word their kernel sets in pinned host memory (it is visible ~6 us
                       before the stream reports the kernel finished); other calls spin on the host clock until the call's
                       bytes could have moved at the chip's peak rate, then poll the stream (a sleeping wait wakes up 9 us
                       late on one box and 45 us late on another); 0 = sleep on the stream, 2 = poll from the start
   "profile"       0 off, 1 = HIP events around every stage, 2 = around the forward / inverse kernel only
                       (read with sdft_hip_get_profile; every event pair costs ~5 us of stream time)
   "resident"      0 (default) | 1 = the reference driver's loop -- sdft_sdft_n + sdft_isdft_n per hop, synchronous calls of one time chunk
                       (< 512 samples; synthesis of up to 1024 rows) on device pointers, single-channel plan on its own stream
                       (test/test.c:69-83 of the reference), and the single-sample calls sdft_sdft / sdft_isdft on a device row (the sample rides in
                       the call, the result comes back through pinned memory: 6.8 / 5.8 us per call against 11.8 / 9.9) -- is served by ONE kernel that stays on the chip: the host writes a call into a
                       cache line of pinned memory and rings a doorbell word, the kernel's workgroups run the same device functions the launches
                       run (bit-identical) and set the completion word: no launch and no stream query per call.  The kernel leaves by itself when
                       no call has come for 200 us (the first call after that starts it again), so a blocking hipMemcpy of the host -- which
                       waits for the plan's stream -- waits that long at most; every other entry point of the plan and sdft_hip_synchronize
                       retire it first.  Off by default: while it lives it holds 256 small workgroups and the plan's stream.
                       get_option "resident_calls", "resident_launches", "resident_missed" (calls that raced with the time-out and were
                       rung again), "resident_alive"
   Ten more pick a route the library otherwise picks by itself (a host that knows its shapes may, the tests do):
   "chunk"         samples per time chunk (0 = heuristic)
   "segments"      time segments of the exact carry pass overlapped with the forward launches (0 = heuristic)
   "chain"         exact carries: 1 (default) = relay form (seed table; identical waves take blocks of steps in turn, one dependent addition
                       per step on the chain; one relay launch beside one forward launch whose workgroups wait for their chunk's carries)
                       while bins x channels leave SIMDs idle, 0 = always the serial pass, 2 = relay form whenever the geometry allows
   "self_carry"    1 (default) = chunk-parallel FD double calls with 2*dftsize <= 4096 a power of two or 2/3/5-smooth run as ONE
                       launch: every workgroup derives its carry-in from the raw samples (fold + FFT in LDS);
                       0 = carries by a pre-pass (two more launches); calls of up to 2^19 samples per channel take it
   "hop_kernel"    1 (default) = calls of one time chunk run one fused launch (differences + analysis; a hop's samples in up to 8 time
                       parts, every (tile of bins, part) a workgroup: bit-identical), 0 = the general launches
   "fused_exact"   sdft_hip_process_n: 0 = folded form (window, operation and synthesis folded into per-bin
                       coefficients, sum over bins by a tree), 1 = bins summed in the reference's order by the
                       fastest route that gives those bits, 2 = in that order by the fused kernel,
                       -1 (default) = 1 when the host set carry = 1 at FD double, else 0
                       (float samples from double bins: the reference's bits are proven from the tree sum and a bound on
                       what any summation order can differ by; only samples whose bound straddles a rounding boundary of the
                       float are summed in order -- get_option "ordered_walks" counts them)
   "inverse_rows"  rows per wave of the exact inverse (0 = heuristic and tuner; 4, 8, 16, 32)
   "inverse_tune"  1 (default) = synthesis calls from 8 Ki rows on find the fastest of their bit-identical forms -- 4, 8, 16 or 32 rows
                       per wave, 256- or 512-byte row segments, the tree sum with the rounding-interval proof, whole rows read in step -- on the
                       host's own calls: the first calls of a shape take the forms in turn, timed by events, then the fastest serves the shape
                       (a few shapes are remembered: a host that alternates call lengths keeps what it has decided); 0 = the static choice.
                       get_option "last_inverse_tuned" = 10 x decided + form (0 tree sum, 1 32 rows, 2 16 rows, 3 16 rows x 512 B, 4 8 rows,
                       5 4 rows, 6 whole rows in step)
   "pointers"      0 (default) = every call asks the runtime what each pointer is (hipPointerGetAttributes: 0.06-0.16 us,
                       nothing is cached -- a buffer that was freed and whose address came back as the other kind of memory
                       is classified as what it is now), 1 = all device, 2 = all host (no query)
   "stage_bytes"   segment size of the host-pointer staging path
   A key the library does not know returns -1.
   TEST HOOKS.  Every other fork of the host logic is decided by the library alone in libsdft_hip.so.  The same sources built with
   -DSDFT_HIP_TEST_HOOKS (libsdft_hip_hooks.so, built beside the product by `python -m sdft_amd.build`; no host links it) accept the keys that force
   those forks, so that the tests can run every route against the reference and the probes under scripts/ can measure them:
   "rows_kernel", "row_slots_max", "interior", "fused", "fft_carry", "fold", "rows_f32", "hop_parts", "xcd_map", "chain_block", "relay_waves", "inverse_verify",
   "relay_flow", "relay_groups", "chain_debug", "inverse_nt", "inverse_nt_skip_mb", "inverse_step", "inverse_ordered", "host_direct", "copy_streams", "prefix_cells", "array_group", "mix_group", "mix_block" (sdft_capi.inc names what each selects);
   get_option "test_hooks" = 1 in that build.
   get_option additionally answers "tiles", "bins_per_lane", "row_slots", "last_chunks",
   "last_chunk_len", "last_kernel" (1 tiles, 2 row groups, 3 hop, 4 decimated analysis, 5 power-spectrogram analysis, 6 pooled power analysis, 7 filterbank analysis, 8 pooled cross-spectrum analysis, 9 array covariance analysis, 10 channel-mix analysis, 11 peak-hold analysis), 12 (lag-product analysis), 13 (power-moments analysis), 14 (band-peak analysis), 15 (smoothed power analysis), 16 (smoothed cross-spectrum analysis) or 17 (smoothed peak-hold analysis), "last_segments", "last_fused",
   "last_filterbank_launches" (forward_filterbank_kernel launches of the last filterbank call, over all of its host segments: more than its carry segments once its pieces exceed the workspace bound),
   "last_band_peak_launches" (its twin: forward_band_peak_kernel launches of the last band-peak call),
   "last_chain", "last_fused_exact", "last_fused_fold", "last_process_path" (1 fused kernel, 2 hop pair, 3 two-pass),
   "last_self" (no pre-pass launch), "last_prefix" (long calls: one pre-pass launch, prefix_cells_kernel), "last_inverse_nt" / "last_inverse_skip" (what the last synthesis launch used: non-temporal loads, rows read with ordinary loads),
   "array_group" (channels per group of a register block of sdft_hip_sdft_covariance_n),
   "mix_group" / "mix_block" (channels per group and outputs per block of a wave of sdft_hip_sdft_mix_n),
   "cursor", "device", "ring_recoveries" (calls re-run with the serial carry pass after a poll loop of
   the exact-carry kernels timed out: results stay valid, sdft_hip_last_warning() reports it), "flag_fallbacks". */
int  sdft_hip_set_option(sdft_t* sdft, const char* key, long value) SDFT_HIP_SYMBOL(set_option);
long sdft_hip_get_option(const sdft_t* sdft, const char* key) SDFT_HIP_SYMBOL(get_option);

/* accumulated device milliseconds and launch counts per stage {delta, carry, forward, inverse};
   synchronises, then resets the counters */
int  sdft_hip_get_profile(sdft_t* sdft, double ms[4], long calls[4]) SDFT_HIP_SYMBOL(get_profile);

/* ---- introspection (tests) ---------------------------------------------------------------------
   stream state copied to host buffers: acc, fid [channels][dftsize]; hist [channels][2*dftsize]
   in time order (oldest first); any pointer may be NULL */
int  sdft_hip_get_state(sdft_t* sdft, sdft_fdx_t* acc, sdft_fdx_t* fid, sdft_td_t* hist, size_t* cursor) SDFT_HIP_SYMBOL(get_state);

/* checkpoint / resume: installs a state read with sdft_hip_get_state into a plan of the same dftsize,
   window, latency, types and channel count (also one living on another GPU); NULL pointers leave
   that part untouched */
int  sdft_hip_set_state(sdft_t* sdft, const sdft_fdx_t* acc, const sdft_fdx_t* fid, const sdft_td_t* hist, size_t cursor) SDFT_HIP_SYMBOL(set_state);

/* host-only (no GPU needed): the plan tables exactly as uploaded; tw, syn [dftsize], wtab
   [2*dftsize], weights [2] = {analysis, synthesis}; any pointer may be NULL */
int  sdft_hip_plan_tables(const sdft_size_t dftsize, const sdft_double_t latency, sdft_fdx_t* tw,
                          sdft_fdx_t* syn, sdft_fdx_t* wtab, sdft_fd_t* weights) SDFT_HIP_SYMBOL(plan_tables);

#if defined(__cplusplus)
}
#endif

#endif /* SDFT_HIP_SDFT_HIP_H */
