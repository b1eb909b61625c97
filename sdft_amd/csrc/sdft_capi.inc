// sdft_capi.inc -- the C-ABI of one (TD, FD) instantiation.  Included by sdft_capi_<td><fd>.hip
// with SDFT_TD, SDFT_FD and SDFT_SUFFIX defined.  Every entry point is `extern "C"`, takes plain
// pointers and sizes, and replaces the reference function named in include/sdft/sdft.h.

#include "sdft_plan.hpp"

#pragma clang fp contract(off)

#define SDFT_CAT_(a, b) a##b
#define SDFT_CAT(a, b) SDFT_CAT_(a, b)
#define SDFT_FN(name) SDFT_CAT(SDFT_CAT(sdft_hip_, name), SDFT_CAT(_, SDFT_SUFFIX))

namespace {
using plan_t = sdfthip::Plan<SDFT_TD, SDFT_FD>;
using fdx_t = sdfthip::cx<SDFT_FD>;
inline plan_t* P(void* p) { return static_cast<plan_t*>(p); }
inline const plan_t* P(const void* p) { return static_cast<const plan_t*>(p); }
// the wrapper of a grid analysis call (Plan::sdft_*_n, which hands back its row count): NULL plan, the call, the rows as a long
template <class Call>
inline long grid_call(void* p, const char* fn, Call&& call)
{
  if (!p) { sdfthip::set_error(fn, "NULL plan"); return -1; }
  size_t rows = 0;
  if (!call(*P(p), rows)) return -1;
  if (rows > (size_t)LONG_MAX) { sdfthip::set_error(fn, "more rows than a long can count"); return -1; }
  return (long)rows;
}
#define SDFT_GRID_CALL(name, ...) grid_call(p, "sdft_hip_" #name, [&](plan_t& q, size_t& rows) { return q.name(__VA_ARGS__, rows); })
}

extern "C" {

// sdft.h:413
void* SDFT_FN(alloc_batch)(size_t dftsize, int window, double latency, size_t channels)
{
  plan_t* p = new (std::nothrow) plan_t();
  if (!p) { sdfthip::set_error("sdft_alloc", "out of host memory"); return nullptr; }
  if (!p->create(dftsize, window, latency, channels)) { p->destroy(); delete p; return nullptr; }
  return p;
}
void* SDFT_FN(alloc_custom)(size_t dftsize, int window, double latency) { return SDFT_FN(alloc_batch)(dftsize, window, latency, 1); }
// sdft.h:457
void* SDFT_FN(alloc)(size_t dftsize) { return SDFT_FN(alloc_batch)(dftsize, sdfthip::WIN_HANN, 1.0, 1); }
// sdft.h:466
void SDFT_FN(free)(void* p) { if (!p) return; P(p)->destroy(); delete P(p); }
// sdft.h:517
void SDFT_FN(reset)(void* p) { if (p) (void)P(p)->reset(); }
// sdft.h:535, :543, :551
size_t SDFT_FN(size)(const void* p) { return p ? P(p)->nbins : 0; }
int SDFT_FN(window)(const void* p) { return p ? P(p)->window : (int)sdfthip::WIN_BOXCAR; }
double SDFT_FN(latency)(const void* p) { return p ? P(p)->latency : 0.0; }
size_t SDFT_FN(channels)(const void* p) { return p ? P(p)->channels : 0; }

// sdft.h:562 -- single sample, dft of shape (dftsize)
void SDFT_FN(sdft)(void* p, SDFT_TD sample, void* dft)
{
  if (!p) return;
  sdfthip::Scoped<bool> sync(P(p)->async, false);
  (void)P(p)->sdft_n(1, &sample, static_cast<fdx_t*>(dft), 0 /* the by-value sample lives on the host stack */);
}
// sdft.h:607 -- dense (nsamples, dftsize); batched plans: x [channels][n], dfts [channels][n][dftsize]
void SDFT_FN(sdft_n)(void* p, size_t n, const SDFT_TD* x, void* dfts)
{
  if (p) (void)P(p)->sdft_n(n, x, static_cast<fdx_t*>(dfts));
}
// sdft.h:622
void SDFT_FN(sdft_nd)(void* p, size_t n, const SDFT_TD* x, void** dfts)
{
  if (p) (void)P(p)->sdft_nd(n, x, reinterpret_cast<fdx_t**>(dfts));
}
// sdft.h:635
SDFT_TD SDFT_FN(isdft)(void* p, const void* dft)
{
  SDFT_TD y = (SDFT_TD)0;
  if (p) (void)P(p)->isdft_one(static_cast<const fdx_t*>(dft), &y);
  return y;
}
// sdft.h:666
void SDFT_FN(isdft_n)(void* p, size_t n, const void* dfts, SDFT_TD* y)
{
  if (p) (void)P(p)->isdft_n(n, static_cast<const fdx_t*>(dfts), y);
}
// sdft.h:681
void SDFT_FN(isdft_nd)(void* p, size_t n, const void** dfts, SDFT_TD* y)
{
  if (p) (void)P(p)->isdft_nd(n, reinterpret_cast<const fdx_t**>(dfts), y);
}

// ---- additions beyond the reference (never altering the above) ------------------------------
// fused analysis -> spectral operation -> synthesis; see sdft_hip.h
int SDFT_FN(process_n)(void* p, size_t n, const SDFT_TD* x, SDFT_TD* y, int op, const void* params, void* dfts)
{
  return p && P(p)->process_n(n, x, y, op, params, static_cast<fdx_t*>(dfts)) ? 0 : -1;
}
// decimated analysis: the rows of sdft_n at the call's samples first, first + every, ... < n; see sdft_hip.h
long SDFT_FN(sdft_every_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, void* dfts)
{ return SDFT_GRID_CALL(sdft_every_n, n, x, every, first, static_cast<fdx_t*>(dfts)); }
// power-spectrogram analysis: re^2 + im^2 of a band of bins of the rows of that grid; see sdft_hip.h
long SDFT_FN(sdft_power_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, SDFT_FD* power)
{ return SDFT_GRID_CALL(sdft_power_n, n, x, every, first, bin0, nbins, power); }
// pooled power analysis: those powers at every sample, summed over the windows of the grid; see sdft_hip.h
long SDFT_FN(sdft_power_sum_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, SDFT_FD* sums)
{ return SDFT_GRID_CALL(sdft_power_sum_n, n, x, every, first, bin0, nbins, sums); }
// peak-hold analysis: the largest or the smallest of those powers over the windows of the grid; see sdft_hip.h
long SDFT_FN(sdft_power_peak_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, int hold, SDFT_FD* peaks)
{ return SDFT_GRID_CALL(sdft_power_peak_n, n, x, every, first, bin0, nbins, hold, peaks); }
// power-moments analysis: those powers and their squares, each summed over the windows of the grid; see sdft_hip.h
long SDFT_FN(sdft_power_moments_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, SDFT_FD* moments)
{ return SDFT_GRID_CALL(sdft_power_moments_n, n, x, every, first, bin0, nbins, moments); }
// smoothed power analysis: the one-pole average of those powers, advanced at every sample and kept on the grid; see sdft_hip.h
long SDFT_FN(sdft_power_smooth_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, double decay,
                                  SDFT_FD* state, SDFT_FD* smooth)
{ return SDFT_GRID_CALL(sdft_power_smooth_n, n, x, every, first, bin0, nbins, decay, state, smooth); }
// smoothed peak-hold analysis: the largest or smallest of that average over the windows of the grid; see sdft_hip.h
long SDFT_FN(sdft_smooth_peak_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, double decay, int hold,
                                 SDFT_FD* state, SDFT_FD* peaks)
{ return SDFT_GRID_CALL(sdft_smooth_peak_n, n, x, every, first, bin0, nbins, decay, hold, state, peaks); }
// filterbank analysis: weighted band sums of those powers on the grid; see sdft_hip.h
int SDFT_FN(set_filterbank)(void* p, size_t nbands, const size_t* band_bin0, const size_t* band_nbins, const SDFT_FD* weights)
{
  if (!p) { sdfthip::set_error("sdft_hip_set_filterbank", "NULL plan"); return -1; }
  return P(p)->set_filterbank(nbands, band_bin0, band_nbins, weights) ? 0 : -1;
}
size_t SDFT_FN(filterbank_bands)(const void* p) { return p ? P(p)->filterbank_bands() : 0; }
long SDFT_FN(sdft_filterbank_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, SDFT_FD* out)
{ return SDFT_GRID_CALL(sdft_filterbank_n, n, x, every, first, out); }
// band-peak analysis: per band of that filterbank the largest weighted power and its bin on the grid; see sdft_hip.h
long SDFT_FN(sdft_band_peak_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, SDFT_FD* peaks)
{ return SDFT_GRID_CALL(sdft_band_peak_n, n, x, every, first, peaks); }
// pooled cross-spectrum analysis: A conj(B) of the plan's channel pairs summed over the windows of the grid; see sdft_hip.h
int SDFT_FN(set_pairs)(void* p, size_t npairs, const size_t* pair_a, const size_t* pair_b)
{
  if (!p) { sdfthip::set_error("sdft_hip_set_pairs", "NULL plan"); return -1; }
  return P(p)->set_pairs(npairs, pair_a, pair_b) ? 0 : -1;
}
size_t SDFT_FN(pairs)(const void* p) { return p ? P(p)->pairs_count() : 0; }
long SDFT_FN(sdft_cross_sum_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, SDFT_FD* sums)
{ return SDFT_GRID_CALL(sdft_cross_sum_n, n, x, every, first, bin0, nbins, sums); }
// smoothed cross-spectrum analysis: the one-pole average of A conj(B) of those pairs, advanced at every sample and kept on the grid; see sdft_hip.h
long SDFT_FN(sdft_cross_smooth_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, double decay,
                                  SDFT_FD* state, SDFT_FD* smooth)
{ return SDFT_GRID_CALL(sdft_cross_smooth_n, n, x, every, first, bin0, nbins, decay, state, smooth); }
// lag-product analysis: X[t] conj(X[t - 1]) of every channel summed over those windows; see sdft_hip.h
long SDFT_FN(sdft_lag_sum_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, SDFT_FD* sums)
{ return SDFT_GRID_CALL(sdft_lag_sum_n, n, x, every, first, bin0, nbins, sums); }
// array covariance analysis: the cross-spectrum call's sums for all pairs of the channels of an array, by blocks; see sdft_hip.h
int SDFT_FN(set_array)(void* p, size_t nch, const size_t* chan)
{
  if (!p) { sdfthip::set_error("sdft_hip_set_array", "NULL plan"); return -1; }
  return P(p)->set_array(nch, chan) ? 0 : -1;
}
size_t SDFT_FN(array_channels)(const void* p) { return p ? P(p)->array_channels() : 0; }
long SDFT_FN(sdft_covariance_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, SDFT_FD* cov)
{ return SDFT_GRID_CALL(sdft_covariance_n, n, x, every, first, bin0, nbins, cov); }
// channel-mix analysis: per-bin weighted sums of the windowed bins of the channels of a mix on a row grid; see sdft_hip.h
int SDFT_FN(set_mix)(void* p, size_t nout, size_t nch, const size_t* chan, const SDFT_FD* weights)
{
  if (!p) { sdfthip::set_error("sdft_hip_set_mix", "NULL plan"); return -1; }
  return P(p)->set_mix(nout, nch, chan, reinterpret_cast<const sdfthip::cx<SDFT_FD>*>(weights)) ? 0 : -1;
}
size_t SDFT_FN(mix_outputs)(const void* p) { return p ? P(p)->mix_outputs() : 0; }
long SDFT_FN(sdft_mix_n)(void* p, size_t n, const SDFT_TD* x, size_t every, size_t first, size_t bin0, size_t nbins, SDFT_FD* out)
{ return SDFT_GRID_CALL(sdft_mix_n, n, x, every, first, bin0, nbins, out); }
int SDFT_FN(set_stream)(void* p, void* hip_stream) { return p && P(p)->set_stream(static_cast<hipStream_t>(hip_stream)) ? 0 : -1; }
// (a host that asks for the stream may queue work of its own behind a call: from here on every kernel of the plan is on it)
void* SDFT_FN(get_stream)(void* p)
{
  if (!p) return nullptr;
  (void)P(p)->pipe_join();
  P(p)->stream_exposed = true;
  return (void*)P(p)->stream;
}
int SDFT_FN(synchronize)(void* p) { return p && P(p)->synchronize() ? 0 : -1; }
// measurement aid: the reference driver's loop (test/test.c:69-83: sdft_sdft_n + sdft_isdft_n per hop on one buffer) run from C,
// as a C host runs it -- what an interpreter adds per call does not belong to the library.  Seconds for `hops` hops, or -1.
double SDFT_FN(time_hops)(void* p, size_t hops, size_t hop, const SDFT_TD* x, void* dfts, SDFT_TD* y)
{
  if (!p || !P(p)->synchronize()) return -1.0;
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < hops; ++i)
  {
    if (!P(p)->sdft_n(hop, x + i * hop, static_cast<fdx_t*>(dfts))) return -1.0;
    if (!P(p)->isdft_n(hop, static_cast<const fdx_t*>(dfts), y + i * hop)) return -1.0;
  }
  if (!P(p)->synchronize()) return -1.0;
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// options (include/sdft/sdft_hip.h documents them): the product library knows the twelve a host may want and ten that pick a route the
// library otherwise picks itself; the remaining path-forcing keys exist only in a build with -DSDFT_HIP_TEST_HOOKS (libsdft_hip_hooks.so:
// the tests run every route against the reference, the probes under scripts/ measure them) -- a key the build does not know returns -1
int SDFT_FN(set_option)(void* p, const char* key, long value)
{
  if (!p || !key) return -1;
  plan_t* q = P(p);
  // ---- for hosts ----
  if (!strcmp(key, "async")) { if (!value) (void)q->pipe_join(); q->async = value != 0; }
  else if (!strcmp(key, "pipeline")) { if (!value) (void)q->pipe_join(); q->opt_pipeline = value; }
  else if (!strcmp(key, "carry")) q->carry_mode = (value || (sizeof(SDFT_FD) == 4 && !q->opt_float_parallel)) ? sdfthip::CARRY_EXACT : sdfthip::CARRY_FAST;
  else if (!strcmp(key, "float_carry_parallel"))
  {
    q->opt_float_parallel = value != 0;
    if (sizeof(SDFT_FD) == 4) q->carry_mode = value ? sdfthip::CARRY_FAST : sdfthip::CARRY_EXACT;
  }
  else if (!strcmp(key, "exact_inverse")) q->opt_exact_inverse = value;
  else if (!strcmp(key, "host_copy")) q->io.opt_host_copy = value;
  else if (!strcmp(key, "host_register")) { q->io.opt_host_register = value; if (!value) q->io.forget_host_buffers(); }
  else if (!strcmp(key, "copy_threads")) { if (value != q->io.opt_copy_threads) q->io.pool.stop(); q->io.opt_copy_threads = value; }
  else if (!strcmp(key, "pinned_io")) q->opt_pinned_io = value;
  else if (!strcmp(key, "spin")) q->opt_spin = value;
  else if (!strcmp(key, "profile")) q->profile = (int)value;
  else if (!strcmp(key, "resident")) { if (!value) (void)q->resident_retire(); q->opt_resident = value; }
  // ---- routes the library otherwise picks itself ----
  else if (!strcmp(key, "chunk")) q->opt_chunk = value;
  else if (!strcmp(key, "segments")) q->opt_segments = value;
  else if (!strcmp(key, "chain")) q->opt_chain = value;
  else if (!strcmp(key, "self_carry")) q->opt_self = value;
  else if (!strcmp(key, "hop_kernel")) q->opt_hop_kernel = value;
  else if (!strcmp(key, "fused_exact")) q->opt_fused_exact = value;
  else if (!strcmp(key, "inverse_rows")) q->opt_inverse_rows = value;
  else if (!strcmp(key, "inverse_tune")) { q->opt_inverse_tune = value; for (auto& t : q->inv_tunes) t.reset_all(); }
  else if (!strcmp(key, "pointers")) q->opt_pointers = value;
  else if (!strcmp(key, "stage_bytes")) q->stage_bytes = value > 0 ? (size_t)value : q->stage_bytes;
#ifdef SDFT_HIP_TEST_HOOKS
  // ---- test hooks: every remaining fork of the host logic, forced ----
  else if (!strcmp(key, "interior")) q->opt_interior = value;                  // bin-owning lanes per wave of the independent-tile kernel
  else if (!strcmp(key, "inverse_verify")) q->opt_inverse_verify = value != 0; // 0: float samples from double bins always by the ordered sum (no tree sum + proof)
  else if (!strcmp(key, "rows_kernel")) q->opt_rows_kernel = value;            // 0: independent tiles even where the row fits the row-group kernel
  else if (!strcmp(key, "row_slots_max")) q->opt_row_slots_max = value;        // 1: the row-group kernel only for rows of one slot per lane
  else if (!strcmp(key, "fft_carry")) q->opt_fft_carry = value;                // 0: chunk partial sums by direct sums, 2: by FFT even for short chunks
  else if (!strcmp(key, "fused")) q->opt_fused = value;                        // 0: plain (unfused) arithmetic in the chunk-parallel FD double path
  else if (!strcmp(key, "fold")) q->opt_fold = value;                          // 0: the fused call keeps the windowed rows in LDS instead of the folded form
  else if (!strcmp(key, "rows_f32")) q->opt_rows_f32 = value;                  // 0: FD float rows by the generic row-group kernel, not the bin-pair kernel
  else if (!strcmp(key, "hop_parts")) q->opt_hop_parts = value;                // 1: a hop's samples in one part, n: n time parts
  else if (!strcmp(key, "xcd_map")) q->opt_xcd_map = value;                    // 0: workgroup b takes chunk b (no XCD-contiguous placement)
  else if (!strcmp(key, "chain_block")) q->opt_chain_L = value;                // relay form: steps per block (8 ... 128)
  else if (!strcmp(key, "chain_debug")) q->opt_chain_debug = value;            // relay form: bit 5 = a wave keeps the token (time-out test), 16 / 64 / 128 = statistics
  else if (!strcmp(key, "relay_waves")) q->opt_relay_waves = value;            // relay form: waves per relay
  else if (!strcmp(key, "relay_flow")) q->opt_relay_flow = value;              // 0: the forward launches wait for whole relay launches (segments), not per chunk
  else if (!strcmp(key, "relay_groups")) q->opt_relay_groups = value;          // 2: two relays per workgroup (half as many CUs; profiles/r06_relay_on_64_cus.txt)
  else if (!strcmp(key, "inverse_nt")) q->opt_inverse_nt = value;              // synthesis loads: 0 ordinary, 1 non-temporal, -1 by size
  else if (!strcmp(key, "inverse_nt_skip_mb")) q->opt_inverse_nt_skip_mb = value;  // MB read first with ordinary loads whatever the kind of load
  else if (!strcmp(key, "inverse_step")) q->opt_inverse_step = value;          // whole rows read in step: 1 always where it applies, -1 never
  else if (!strcmp(key, "inverse_ordered")) q->opt_inverse_ordered = value;    // whole rows, ordered sum: 1 always where it applies, -1 never
  else if (!strcmp(key, "host_direct")) q->io.opt_host_direct = value;         // 0: a hop-sized host matrix by DMA between staging matrix and pinned pieces
  else if (!strcmp(key, "copy_streams")) q->io.opt_copy_streams = value;       // 1: the DMAs of long host copies on one stream
  else if (!strcmp(key, "array_group")) q->opt_array_group = value;            // covariance call: channels per group (1, 2, 4), 0: the build's choice
  else if (!strcmp(key, "mix_group")) q->opt_mix_group = value;                // mix call: channels per group (2, 4, 8), 0: the build's choice
  else if (!strcmp(key, "mix_block")) q->opt_mix_block = value;                // mix call: outputs per block (1, 2, 4), 0: the build's choice
  else if (!strcmp(key, "prefix_cells")) q->opt_prefix_cells = value;          // prefix-cell route of long calls: 0 never, 1 beyond 2^19 samples, 2 whatever the length
#ifdef SDFT_SELF_STAMPS
  else if (!strcmp(key, "self_stamps")) q->opt_self_stamps = value;
#endif
#endif
  else return -1;
  return 0;
}
long SDFT_FN(get_option)(const void* p, const char* key)
{
  if (!p || !key) return -1;
  const plan_t* q = P(p);
  if (!strcmp(key, "async")) return q->async;
  if (!strcmp(key, "pipeline")) return q->opt_pipeline;
  if (!strcmp(key, "last_pipelined")) return q->last_pipelined;
  if (!strcmp(key, "pipelined_calls")) return (long)q->pipe_calls;
  if (!strcmp(key, "pipelined_ordered")) return (long)q->pipe_ordered;
  if (!strcmp(key, "pipelined_inverse_calls")) return (long)q->inv_calls;
  if (!strcmp(key, "last_inverse_pipelined")) return q->last_inverse_pipelined;
  if (!strcmp(key, "pipeline_streams")) return q->pipe_stream_kind * 10 + q->pipe_stream_attempts;
  if (!strcmp(key, "carry")) return q->carry_mode;
  if (!strcmp(key, "float_carry_parallel")) return q->opt_float_parallel;
  if (!strcmp(key, "ordered_walks")) return q->ordered_walks();
  if (!strcmp(key, "inverse_verify")) return q->opt_inverse_verify;
  if (!strcmp(key, "last_inverse_form")) return q->last_inverse_form;
  if (!strcmp(key, "chunk")) return q->opt_chunk;
  if (!strcmp(key, "interior")) return q->interior_lanes();
  if (!strcmp(key, "tiles")) return q->tiles();
  if (!strcmp(key, "bins_per_lane")) return plan_t::bins_per_lane();
  if (!strcmp(key, "last_chunks")) return q->last_chunks;
  if (!strcmp(key, "last_chunk_len")) return q->last_chunk_len;
  if (!strcmp(key, "cursor")) return (long)q->cursor;
  if (!strcmp(key, "last_kernel")) return q->last_kernel;
  if (!strcmp(key, "rows_kernel")) return q->opt_rows_kernel;
  if (!strcmp(key, "fused")) return q->opt_fused;
  if (!strcmp(key, "last_fused")) return q->last_fused;
  if (!strcmp(key, "last_segments")) return q->last_segments;
  if (!strcmp(key, "last_filterbank_launches")) return q->last_filterbank_launches;
  if (!strcmp(key, "last_band_peak_launches")) return q->last_band_peak_launches;
  if (!strcmp(key, "row_slots")) return q->row_slots();
  if (!strcmp(key, "device")) return q->device;
  if (!strcmp(key, "last_chain")) return q->last_chain;
  if (!strcmp(key, "last_fused_exact")) return q->last_fused_exact;
  if (!strcmp(key, "last_fused_fold")) return q->last_fused_fold;
  if (!strcmp(key, "last_process_path")) return q->last_process_path;
  if (!strcmp(key, "fused_exact")) return q->opt_fused_exact;
  if (!strcmp(key, "chain")) return q->opt_chain;
  if (!strcmp(key, "fold")) return q->opt_fold;
  if (!strcmp(key, "last_hop_pipe")) return q->last_hop_pipe;
  if (!strcmp(key, "spin")) return q->opt_spin;
  if (!strcmp(key, "inverse_step")) return q->opt_inverse_step;
  if (!strcmp(key, "inverse_ordered")) return q->opt_inverse_ordered;
  if (!strcmp(key, "inverse_nt_skip_mb")) return q->opt_inverse_nt_skip_mb;
  if (!strcmp(key, "last_inverse_nt")) return q->last_inverse_nt;
  if (!strcmp(key, "last_inverse_skip")) return q->last_inverse_skip;
  if (!strcmp(key, "hop_parts")) return q->opt_hop_parts;
  if (!strcmp(key, "xcd_map")) return q->opt_xcd_map;
  if (!strcmp(key, "inverse_tune")) return q->opt_inverse_tune;
  if (!strcmp(key, "last_inverse_tuned")) return q->last_inverse_tuned;
  if (!strcmp(key, "last_hop_parts")) return q->last_hop_parts;
  if (!strcmp(key, "self_carry")) return q->opt_self;
  if (!strcmp(key, "last_self")) return q->last_self;
  if (!strcmp(key, "last_prefix")) return q->last_prefix;
#ifdef SDFT_HIP_TEST_HOOKS
  if (!strcmp(key, "prefix_cells")) return q->opt_prefix_cells;
#endif
  if (!strcmp(key, "array_group")) return q->array_group();
  if (!strcmp(key, "mix_group")) return q->mix_group_size();
  if (!strcmp(key, "mix_block")) return q->mix_block_size();
  if (!strcmp(key, "host_register")) return q->io.opt_host_register;
  if (!strcmp(key, "host_register_hits")) return q->io.host_reg_hits;
  if (!strcmp(key, "host_copy")) return q->io.opt_host_copy;
  if (!strcmp(key, "copy_threads")) return q->io.opt_copy_threads;
  if (!strcmp(key, "copy_streams")) return q->io.opt_copy_streams;
  if (!strcmp(key, "copy_workers")) return (long)q->io.pool.workers();
  if (!strcmp(key, "host_copies_staged")) return q->io.pin_copies;
  if (!strcmp(key, "host_copy_memcpy_us")) return (long)q->io.pin_us_memcpy;
  if (!strcmp(key, "host_copy_device_us")) return (long)q->io.pin_us_device;
  if (!strcmp(key, "host_register_misses")) return q->io.host_reg_misses;
  if (!strcmp(key, "last_flow")) return q->last_flow;
  if (!strcmp(key, "flag_fallbacks")) return q->flag_fallbacks;
  if (!strcmp(key, "ring_recoveries")) return q->ring_recoveries;
  if (!strcmp(key, "rows_f32")) return q->opt_rows_f32;
  if (!strcmp(key, "last_rows_f32")) return q->last_rows_f32;
  if (!strcmp(key, "resident")) return q->opt_resident;
  if (!strcmp(key, "resident_calls")) return (long)q->res.calls;
  if (!strcmp(key, "resident_launches")) return (long)q->res.launches;
  if (!strcmp(key, "resident_missed")) return (long)q->res.missed;
  if (!strcmp(key, "resident_alive")) return q->res.alive ? 1 : 0;
  if (!strcmp(key, "test_hooks"))
  {
#ifdef SDFT_HIP_TEST_HOOKS
    return 1;
#else
    return 0;
#endif
  }
  return -1;
}
// accumulated per-stage device time: ms[4] = {delta, carry, forward, inverse}, calls[4]; resets the counters
int SDFT_FN(get_profile)(void* p, double* ms, long* calls)
{
  if (!p) return -1;
  plan_t* q = P(p);
  if (!q->synchronize()) return -1;
  for (int s = 0; s < sdfthip::ST_COUNT; ++s)
  {
    if (ms) ms[s] = q->prof_ms[s];
    if (calls) calls[s] = q->prof_calls[s];
    q->prof_ms[s] = 0; q->prof_calls[s] = 0;
  }
  return 0;
}
// measurement aid (option chain_debug bit 4): cycles per wave of the chain kernel's workgroup 0
int SDFT_FN(chain_stats)(void* p, unsigned long long* out32) { return p && P(p)->chain_stats(out32) ? 0 : -1; }
int SDFT_FN(relay_stamps)(void* p, unsigned long long* out, size_t count) { return p && P(p)->relay_stamps(out, count) ? 0 : -1; }
// stream state read-back (host buffers): acc, fid [channels][N]; hist [channels][2N] in time order
int SDFT_FN(get_state)(void* p, void* acc, void* fid, SDFT_TD* hist, size_t* cursor)
{
  return p && P(p)->get_state(static_cast<fdx_t*>(acc), static_cast<fdx_t*>(fid), hist, cursor) ? 0 : -1;
}
// checkpoint / resume: the inverse of get_state (host buffers; NULL pointers leave that part untouched)
int SDFT_FN(set_state)(void* p, const void* acc, const void* fid, const SDFT_TD* hist, size_t cursor)
{
  return p && P(p)->set_state(static_cast<const fdx_t*>(acc), static_cast<const fdx_t*>(fid), hist, cursor) ? 0 : -1;
}
// host-only: the plan tables exactly as uploaded (no GPU needed); tw, syn [N], wtab [2N] may be NULL
int SDFT_FN(plan_tables)(size_t dftsize, double latency, void* tw, void* syn, void* wtab, SDFT_FD* weights)
{
  sdfthip::Tables<SDFT_FD> t;
  t.build(dftsize, latency);
  if (tw) memcpy(tw, t.tw.data(), dftsize * sizeof(fdx_t));
  if (syn) memcpy(syn, t.syn.data(), dftsize * sizeof(fdx_t));
  if (wtab) memcpy(wtab, t.wtab.data(), 2 * dftsize * sizeof(fdx_t));
  if (weights) { weights[0] = t.aweight; weights[1] = t.sweight; }
  return 0;
}

}  // extern "C"
