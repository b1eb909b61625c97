// sdft_plan.hpp -- host side of the HIP engine: plan tables, device-resident stream state,
// chunk geometry, kernel launches.  One instance per (TD, FD) pair, see sdft_capi.inc.
// Citations are into /root/reference/c/src/sdft/sdft.h.

#pragma once

#include "sdft_kernels.hpp"
#include "sdft_forward_rows_f32.hpp"      // not part of the run-time-compiled text: plain analysis only
#include "sdft_resident.hpp"              // likewise: the opt-in resident kernel of the hop loop
#include "sdft_plan_logic.hpp"            // every decision that needs no HIP call (unit-tested on the CPU under sanitizers)
#include "sdft_host_io.hpp"               // the caller's host memory: classification, registration, copies through pinned slots

#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif
#include <chrono>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace sdfthip {

// ---- error channel (the reference has none: void returns, sdft.h:413-687) -----------------
void set_error(const char* what, const char* detail);   // sdft_common.hip
void set_warning(const char* what, const char* detail); // sdft_common.hip: something the host may want to know about a call that succeeded
bool lane_selftest();                                   // sdft_common.hip
// run-time compilation of a host's own spectral operation (sdft_common.hip)
bool rtc_kernel(const char* expr, const char* name_expr, int device, hipFunction_t* fn);
bool rtc_compile(const char* expr, const char* name_expr, const char* arch, std::string& lowered_name, std::vector<char>& code);


// ---- plan tables: the reference's own expressions (sdft.h:422-423, :439-446) evaluated on the
// host with the host libm, so the device tables are bit-identical to the oracle's ------------
template <typename FD> static inline FD host_cos(FD a);
template <> inline float  host_cos<float>(float a)   { return cosf(a); }
template <> inline double host_cos<double>(double a) { return cos(a); }
template <typename FD> static inline FD host_acos(FD a);
template <> inline float  host_acos<float>(float a)   { return acosf(a); }
template <> inline double host_acos<double>(double a) { return acos(a); }

// polar(r, t) of sdft.h:333-348.  The canonical oracle build (gcc -O2) merges the
// cos(t)/sin(t) pair into one glibc sincos() call, whose results differ from separate calls in
// the last bit for a few arguments; calling sincos explicitly keeps the tables bit-identical.
template <typename FD> static inline cx<FD> host_polar(FD r, FD t);
template <> inline cx<float> host_polar<float>(float r, float t)
{
  float s, c; sincosf(t, &s, &c); return cmake<float>(r * c, r * s);
}
template <> inline cx<double> host_polar<double>(double r, double t)
{
  double s, c; sincos(t, &s, &c); return cmake<double>(r * c, r * s);
}

template <typename FD>
struct Tables
{
  FD aweight, sweight;
  std::vector<cx<FD>> tw, syn, wtab;

  void build(size_t nbins, double latency)
  {
    aweight = (FD)(1) / (nbins * 2);                                    // :422
    sweight = (FD)(2);                                                  // :423
    tw.resize(nbins); syn.resize(nbins); wtab.resize(nbins * 2);
    const FD omega = (FD)(-2) * host_acos<FD>((FD)(-1)) / (nbins * 2);  // :439
    const FD gain = (FD)(+2) / ((FD)(1) - host_cos<FD>((FD)(omega * nbins * latency)));   // :440
    for (size_t k = 0; k < nbins; ++k)
    {
      const FD a = omega * k;                                           // :444
      const FD s = (FD)(omega * k * nbins * latency);                   // :445 (fd products, then * double)
      tw[k] = host_polar<FD>((FD)(1), a);
      syn[k] = host_polar<FD>(gain, s);
    }
    // W[j] = exp(-i*pi*j/N), j in [0, 2N): closed form of fid after j mod 2N rotations of bin 1
    // (only used to seed time chunks in the fast-carry mode)
    for (size_t j = 0; j < nbins * 2; ++j)
    {
      const double a = -3.14159265358979323846 * (double)j / (double)nbins;
      wtab[j] = (j < nbins) ? tw[j] : cmake<FD>((FD)cos(a), (FD)sin(a));
    }
  }
};

// the constants sdft_plan_logic.hpp is written against are the kernels'
static_assert(logic::kLanes == kWave && logic::kRowWaves == kRowWavesMax && logic::kRowSlots == kRowSlotsMax && logic::kTimeGroup == kGroup &&
              logic::kSumBlockLen == kSumBlock && logic::kHopSamples == kHopMax && kGroup % kRowGroup == 0, "sdft_plan_logic.hpp and the kernels disagree");
static_assert(logic::kWindowHann == WIN_HANN && logic::kWindowBlackman == WIN_BLACKMAN && logic::kWindowBoxcar == WIN_BOXCAR, "window numbering");
static_assert(logic::kWavesPerBlock == kWavesPerBlock && logic::kProcGroup == kProcGroup && logic::kProcRow == kProcRow, "sdft_plan_logic.hpp and the kernels disagree");
static_assert(sizeof(logic::Radices) == sizeof(RadixList), "radix lists");
static_assert(sizeof(logic::FilterbankPiece) == sizeof(FilterbankPiece) && sizeof(logic::FilterbankSplit) == sizeof(FilterbankSplit) &&
              logic::kFilterbankToWorkspace == kFilterbankToWorkspace, "filterbank tables");
static_assert(sizeof(logic::CrossItem) == sizeof(CrossItem) && offsetof(logic::CrossItem, out) == offsetof(CrossItem, out) &&
              offsetof(logic::CrossItem, writes_b) == offsetof(CrossItem, writes_b), "cross-spectrum items");
static_assert(sizeof(logic::CovItem) == sizeof(CovItem) && offsetof(logic::CovItem, b0) == offsetof(CovItem, b0) && offsetof(logic::CovItem, nb) == offsetof(CovItem, nb) &&
              offsetof(logic::CovItem, writes) == offsetof(CovItem, writes), "covariance items");
static_assert(sizeof(logic::MixItem) == sizeof(MixItem) && offsetof(logic::MixItem, no) == offsetof(MixItem, no) &&
              offsetof(logic::MixItem, writes) == offsetof(MixItem, writes), "mix items");

enum CarryMode : int { CARRY_FAST = 0, CARRY_EXACT = 1 };

enum ProfileStage : int { ST_DELTA = 0, ST_CARRY = 1, ST_FORWARD = 2, ST_INVERSE = 3, ST_COUNT = 4 };

// a value a member holds for a scope: the old one is back on every way out
template <typename T> struct Scoped
{
  T& ref; const T old;
  Scoped(T& r, T v) : ref(r), old(r) { r = v; }
  ~Scoped() { ref = old; }
  Scoped(const Scoped&) = delete;                          // (not assignable either: a reference member)
};

template <typename TD, typename FD>
class Plan
{
 public:
  using fdx = cx<FD>;

  size_t nbins = 0, channels = 1;
  int window = WIN_HANN;
  double latency = 1.0;
  Tables<FD> tab;

  int device = 0;
  int compute_units = 256;       // CUs of the plan's device (one row-group workgroup each)
  hipStream_t stream = nullptr;
  bool own_stream = false, async = false;

  // options
  int carry_mode = sizeof(FD) == 8 ? CARRY_FAST : CARRY_EXACT;
#ifdef SDFT_SELF_STAMPS
  long opt_self_stamps = 0;                                // development builds: device address of 8 stamp words
#endif
  long opt_inverse_verify = 1, last_inverse_form = 0;      // launch_inverse
  bool rtc_failed = false;                                 // launch_inverse returns void: a failed run-time compilation is reported here
  std::string user_expr;                                   // sdft_hip_process_n with an expression: the statements of the call in flight
  template <typename T> static const char* type_name() { return sizeof(T) == 8 ? "double" : "float"; }
  // FD float plans take the chunk-parallel carries too: 2x faster on long calls and closer to the double-precision
  // result than the reference's float arithmetic is, but not within 1e-4 of it (the float reference itself drifts
  // 2e-4 of the largest bin per 262144 samples: profiles/r03_float_parallel_carries.txt)
  long opt_float_parallel = 0;
  long opt_chunk = 0;            // forced chunk length (0 = heuristic)
  long opt_interior = 0;         // forced interior lanes per wave (0 = maximum)
  size_t stage_bytes = logic::kDefaultStageBytes;   // host-pointer path: staging segment size
  int profile = 0;               // 0 off, 1 = events around every stage, 2 = forward/inverse kernels only
  long opt_rows_kernel = 1;      // use the row-group forward kernel when the row fits one workgroup
  long opt_xcd_map = 1;          // every XCD takes a contiguous eighth of a launch's (channel, chunk) workgroups (ForwardArgs::xcd_map)
  long opt_pinned_io = 1;        // small host sample buffers travel through a pinned scratch the kernels access directly
  long opt_pointers = 0;         // 0 = ask the runtime on every call (hipPointerGetAttributes, ~0.1 us), 1 = all device, 2 = all host
  long opt_inverse_rows = 0;     // rows per wave of the exact inverse (0 = heuristic; 4, 8, 16, 32)
  size_t inverse_capacity[2] = {0, 0};   // waves the chip holds at once of the 4-row and the 8-row form (occupancy x CUs), 0: not asked yet
  // Synthesis reads the matrix with non-temporal loads (-1 = by size, 0 / 1).  The host pattern is analysis -> synthesis of the
  // same matrix: the analysis leaves the matrix's last 256 MiB dirty in the Infinity Cache, and ordinary loads of the rest
  // push those lines out to HBM while they read -- streaming loads leave them where the next analysis overwrites them.
  // Measured after a write (profiles/r04_synthesis_streaming_loads.txt): 706 MB f64f64 217 -> 176 us, f32f64 193 -> 153 us,
  // 2.1 GB 461 -> 392 us; a matrix that fits the cache (192 MB) 51 -> 58 us and 8-16 GB +5 %: hence the size window.
  long opt_inverse_nt = -1;
  long opt_inverse_nt_skip_mb = -1;                         // -1: 1536 MB of matrices from 6 GiB on (logic::inverse_ordinary_rows); 0: none
  // long synthesis calls: the fastest of the bit-identical streaming forms is found on the host's own calls (launch_inverse)
  long opt_inverse_tune = 1, last_inverse_tuned = 0;
  // (two tuners: a synthesis that follows an analysis call reads a matrix whose tail is still dirty in the Infinity Cache, one that
  // follows another synthesis does not -- which form and which kind of load is fastest differs between the two, and a host may do both)
  logic::TunerTable inv_tunes[2];                           // (each a few shapes: a host that alternates call lengths keeps what it has decided)
  bool inv_after_write = false;                              // the synthesis call being launched directly follows an analysis call
  hipEvent_t tune_evs[2][logic::TunerTable::kSlots][logic::FormTuner::kMax][2] = {};     // a pair of events per candidate form and tuner
  bool ensure_tune_events()
  {
    if (tune_evs[0][0][0][0]) return true;
    for (auto& kind : tune_evs)
      for (auto& tuner : kind)
        for (auto& pair : tuner)
          for (hipEvent_t& e : pair)
            if (hipEventCreate(&e) != hipSuccess)
            {
              (void)hipGetLastError(); e = nullptr;
              destroy_tune_events();
              return false;
            }
    return true;
  }
  void destroy_tune_events()
  {
    for (auto& kind : tune_evs) for (auto& tuner : kind) for (auto& q : tuner) for (hipEvent_t& f : q) if (f) { (void)hipEventDestroy(f); f = nullptr; }
  }
  long opt_exact_inverse = 1;    // inverse sums bins in the reference's order (bit-identical)
  long opt_row_slots_max = 2;    // largest slots-per-lane the row-group kernel may use (1 = rows <= 1024*BPL only)
  long opt_fused = 1;            // fused multiply-add arithmetic in the chunk-parallel FD double path
  long last_fused = 0;
  long opt_fft_carry = 1;        // FFT form of the chunk partial sums when 2N is a power of two
  long opt_hop_kernel = 1;       // single-chunk calls: fused delta + forward launch (forward_hop_kernel)
  long opt_fused_exact = -1;     // fused analysis->synthesis: 0 = folded / tree sum; 1 = bins summed in the reference's order
                                 // (the fastest route that gives those bits), 2 = in that order by the fused kernel;
                                 // -1 = in order exactly when the host asked for exact carries at FD double (carry = 1)
  long last_fused_exact = 0, last_fused_fold = 0, last_process_path = 0;   // last_process_path: 1 fused kernel, 2 hop pair, 3 two-pass segments
  long opt_spin = 1;             // synchronous short calls poll the stream instead of sleeping on it
  long opt_self = 1;             // chunk-parallel FD double calls, 2N a power of two: self-carried chunks (no pre-pass launches; logic::kSelfMax)
  long last_self = 0;
  long opt_prefix_cells = 1;     // test hook: the prefix-cell route of long calls (logic::ForwardQuery::prefix_cells)
  long last_prefix = 0;          // the last analysis call took it (one pre-pass launch: prefix_cells_kernel)

  long last_kernel = 0;          // 1 = forward_kernel (independent tiles), 2 = forward_rows_kernel, 3 = hop, 4 = forward_every_kernel, 5 = forward_power_kernel, 6 = forward_pooled_power_kernel, 7 = forward_filterbank_kernel, 8 = forward_cross_sum_kernel, 9 = forward_covariance_kernel, 10 = forward_mix_kernel, 11 = forward_power_peak_kernel, 12 = forward_lag_sum_kernel, 13 = forward_power_moments_kernel, 14 = forward_band_peak_kernel, 15 = forward_power_smooth_kernel, 16 = forward_cross_smooth_kernel, 17 = forward_smooth_peak_kernel

  // device-resident stream state
  DevBuf<fdx> d_tw, d_syn, d_wtab;
  // acc / fid / delay line are double-buffered: single-chunk calls read one set and write the other
  DevBuf<fdx> d_accs[4], d_fids[4];                        // state slots: a call reads [st_cur], writes [st_cur ^ 1] (pipelined calls: the next of the ring of four)
  int st_cur = 0;
  fdx* acc_p() { return d_accs[st_cur].p; }
  fdx* fid_p() { return d_fids[st_cur].p; }
  DevBuf<TD> d_hist[4];
  int hist_cur = 0;
  size_t cursor = 0;             // reference cursor (:153)

  // exact-carry mode overlaps the serial pass with the forward kernel: the pass runs on `aux`
  // in time segments, each segment's forward launch on `stream` waits for its event
  hipStream_t aux = nullptr;
  std::vector<hipEvent_t> seg_events;
  hipEvent_t ev_delta = nullptr;
  DevBuf<fdx> d_run_acc[2], d_run_fid[2];
  long opt_segments = 0;         // 0 = heuristic
  long last_segments = 1;

  // exact carries, chain form: fid at every fseed_L-th cursor of the canonical rotation sequence
  // (built on first use); fid_canonical = the stream's fid state is on that sequence (false after
  // a chunk-parallel call seeded fid from the closed-form table, or after set_state, until the
  // next roll-over puts it back to exactly 1)
  DevBuf<fdx> d_fseed;
  unsigned fseed_L = 0;
  bool fid_canonical = true;
  long opt_chain = 1;            // 0 = always the serial pass (carry_exact_kernel), 1 = heuristic, 2 = chain form whenever possible
  long opt_chain_L = 0, opt_chain_debug = 0;
  long last_hop_pipe = 0;
  long opt_hop_parts = 0, last_hop_parts = 1;   // ... in time parts (0 = by the launch's size, 1 = never, n = that many)
  long opt_fold = 1;             // fused call, tree-sum flavour: window, operation and synthesis folded into per-bin coefficients
  long opt_relay_waves = 0;      // waves per workgroup of the relay form (0 = default)
  DevBuf<unsigned long long> d_chain_stats;
  long last_chain = 0;

  // workspace
  DevBuf<FD> d_delta;
  DevBuf<fdx> d_carry, d_seed;
  DevBuf<FD> d_prefix;                                     // prefix cells [channels][chunks][2N]
  DevBuf<TD> d_stage_td;
  DevBuf<fdx> d_stage_fdx;
  DevBuf<fdx*> d_rowptr;
  DevBuf<FD> d_psum_ws, d_psum_head;                       // pooled power analysis: pieces of cut windows [channels][chunks][2][band]; a segment's head row
  // smoothed power analysis: the chunks' end values [channels][chunks][band]; s between the caller's state and the kernels (and
  // between the segments of a call) [channels][band]; P[j] = fl(a^j), j = 0 ... chunk length, rebuilt when (a, length) changes
  DevBuf<FD> d_smooth_ws, d_smooth_state, d_smooth_pw;
  FD smooth_pw_a = (FD)-1;                                   // (no decay is negative: nothing is cached yet)
  size_t smooth_pw_len = 0;
  // smoothed cross-spectrum analysis: d_smooth_ws and d_smooth_pw above serve it with pairs for channels and (re, im) rows of twice
  // the band; its s between the caller's state and the kernels [pairs][band] complex, and a segment's rows on their way to a host buffer
  DevBuf<FD> d_cross_smooth_state, d_cross_smooth_stage;
  // filterbank analysis: the installed filterbank (sdft_hip_set_filterbank) as the host gave it, its decomposition for the plan's
  // tiles (logic::filterbank_layout), the device copies the kernels read, and the workspace of split bands [channels][rows][slots]
  struct Filterbank
  {
    std::vector<size_t> bin0, nbins;
    std::vector<FD> weights;
    logic::FilterbankLayout layout;
    long interior = -1;                                      // option "interior" the layout was made for
  } fbank;
  DevBuf<FilterbankPiece> d_fb_pieces;
  DevBuf<unsigned> d_fb_tile0;
  DevBuf<FilterbankSplit> d_fb_splits;
  DevBuf<FD> d_fb_weights, d_fb_ws;
  // cross-spectrum analysis: the installed pair list (sdft_hip_set_pairs) as the host gave it, its work items (logic::cross_items)
  // and their device copy, the workspace of cut windows [items][chunks][2][band] complex, and a segment's head rows [pairs][band]
  struct Pairs
  {
    std::vector<size_t> a, b;
    std::vector<logic::CrossItem> items;
  } pairs;
  DevBuf<CrossItem> d_cross_items;
  DevBuf<FD> d_cross_ws, d_cross_head, d_cross_stage;     // (d_cross_stage: a segment's sums on their way to a host buffer)
  // covariance analysis: the installed array (sdft_hip_set_array), its work items (logic::covariance_items) for groups of `group`
  // channels and their device copy, the array's channels on the device, and the workspace, head rows and stage as above with the
  // array's nch (nch + 1) / 2 output indices for pairs
  struct Array
  {
    std::vector<size_t> chan;
    std::vector<logic::CovItem> items;
    int group = 0;
  } array;
  DevBuf<CovItem> d_cov_items;
  DevBuf<unsigned> d_cov_chan;
  DevBuf<FD> d_cov_ws, d_cov_head, d_cov_stage;
  long opt_array_group = 0;                                // test hook: channels per group (1, 2, 4), 0: the build's choice
  // channel-mix analysis: the installed mix (sdft_hip_set_mix) -- its channels, its work items (logic::mix_items) for blocks of
  // `block` outputs and their device copy, the channels and the weight table [nout][nch][N] on the device -- and the stage of a
  // segment's rows on their way to a host buffer
  struct Mix
  {
    std::vector<size_t> chan;
    std::vector<logic::MixItem> items;
    size_t nout = 0;
    int block = 0;
  } mix;
  DevBuf<MixItem> d_mix_items;
  DevBuf<unsigned> d_mix_chan;
  DevBuf<fdx> d_mix_weights;
  DevBuf<FD> d_mix_stage;
  long opt_mix_group = 0, opt_mix_block = 0;               // test hooks: channels per group (2, 4, 8), outputs per block (1, 2, 4), 0: the build's choice

  // profile: HIP events on the plan's stream, one pair per stage launch, collected lazily so
  // that back-to-back asynchronous calls are never serialised by the measurement
  std::vector<hipEvent_t> ev_pool[ST_COUNT];
  size_t ev_used[ST_COUNT] = {};
  double prof_ms[ST_COUNT] = {};
  long prof_calls[ST_COUNT] = {};

  // last launch geometry (introspection for tests / bench)
  long last_chunks = 0, last_chunk_len = 0, last_tiles = 0, last_interior = 0, last_pipelined = 0;
  long last_filterbank_launches = 0;                         // forward_filterbank_kernel launches of the last filterbank call
  long last_band_peak_launches = 0;                          // forward_band_peak_kernel launches of the last band-peak call

  bool create(size_t dftsize, int win, double lat, size_t nch)
  {
    nbins = dftsize; window = win; latency = lat; channels = nch ? nch : 1;
    if (window < 0 || window > 3) window = WIN_BOXCAR;      // reference: unknown window -> default branch (:394)
    tab.build(nbins, latency);
    SDFT_TRY(hipGetDevice(&device));
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) compute_units = cus; else (void)hipGetLastError(); }
    if (!lane_selftest()) return false;
    SDFT_TRY(hipStreamCreate(&stream));
    own_stream = true;
    if (const char* e = getenv("SDFT_HIP_CARRY"))
      carry_mode = (!strcmp(e, "exact") || !strcmp(e, "1")) ? CARRY_EXACT : CARRY_FAST;
    if (sizeof(FD) == 4) carry_mode = CARRY_EXACT;         // float FD follows the reference's rounding (unless "float_carry_parallel")
    if (const char* e = getenv("SDFT_HIP_CHUNK")) opt_chunk = atol(e);
    if (const char* e = getenv("SDFT_HIP_INTERIOR")) opt_interior = atol(e);
    if (nbins == 0) return true;
    const size_t nb = nbins, span = 2 * nbins;
    if (!d_tw.reserve(nb) || !d_syn.reserve(nb) || !d_wtab.reserve(span)) return false;
    for (int q = 0; q < 4; ++q)
      if (!d_accs[q].reserve(channels * nb) || !d_fids[q].reserve(channels * nb) || !d_hist[q].reserve(channels * span)) return false;
    if (!to_device(d_tw.p, tab.tw.data(), nb * sizeof(fdx))) return false;
    if (!to_device(d_syn.p, tab.syn.data(), nb * sizeof(fdx))) return false;
    if (!to_device(d_wtab.p, tab.wtab.data(), span * sizeof(fdx))) return false;
    return reset();
  }

  void destroy()
  {
    (void)hipSetDevice(device);
    (void)resident_retire();
    resident_release();
    (void)pipe_join();
    if (stream) (void)hipStreamSynchronize(stream);
    d_tw.release(); d_syn.release(); d_wtab.release();
    release_pipe();
    for (int q = 0; q < 4; ++q) { d_accs[q].release(); d_fids[q].release(); d_hist[q].release(); }
    d_delta.release(); d_carry.release(); d_seed.release(); d_prefix.release();
    d_stage_td.release(); d_stage_fdx.release(); d_rowptr.release(); d_fseed.release();
    d_psum_ws.release(); d_psum_head.release();
    d_smooth_ws.release(); d_smooth_state.release(); d_smooth_pw.release(); d_cross_smooth_state.release(); d_cross_smooth_stage.release();
    d_fb_pieces.release(); d_fb_tile0.release(); d_fb_splits.release(); d_fb_weights.release(); d_fb_ws.release();
    d_cross_items.release(); d_cross_ws.release(); d_cross_head.release(); d_cross_stage.release();
    d_cov_items.release(); d_cov_chan.release(); d_cov_ws.release(); d_cov_head.release(); d_cov_stage.release();
    d_mix_items.release(); d_mix_chan.release(); d_mix_weights.release(); d_mix_stage.release();
    d_gain.release(); d_stage_y.release(); d_chain_stats.release();
    d_alpha.release(); d_beta.release(); d_partial.release(); d_tickets.release();
    if (h_done_flag) { (void)hipHostFree(h_done_flag); h_done_flag = nullptr; }
    if (h_io) { (void)hipHostFree(h_io); h_io = nullptr; d_io = nullptr; }
    io.release_pin();
    if (h_status) { (void)hipHostFree(h_status); h_status = nullptr; }
    io.forget_host_buffers();
    if (d_started) { (void)hipFree(d_started); d_started = nullptr; }
    d_ready.release();
    d_done_count.release(); d_walked.release();
    d_run_acc[0].release(); d_run_acc[1].release(); d_run_fid[0].release(); d_run_fid[1].release();
    if (aux) { (void)hipStreamSynchronize(aux); (void)hipStreamDestroy(aux); aux = nullptr; }
    for (hipEvent_t e : seg_events) (void)hipEventDestroy(e);
    seg_events.clear();
    if (ev_delta) { (void)hipEventDestroy(ev_delta); ev_delta = nullptr; }
    destroy_tune_events();
    for (int st = 0; st < ST_COUNT; ++st)
    {
      for (hipEvent_t e : ev_pool[st]) (void)hipEventDestroy(e);
      ev_pool[st].clear(); ev_used[st] = 0;
    }
    if (own_stream && stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }

  // a host driving several GPUs from one process may have switched the current device
  std::chrono::steady_clock::time_point call_start;         // when the entry point in progress began (finish() counts from here)
  bool bind()
  {
    flag_pending = false; flag_wanted = false; pipe_allowed = false; call_start = std::chrono::steady_clock::now();
    SDFT_TRY(hipSetDevice(device));
    return res.alive ? resident_retire() : true;             // (option "resident": whatever is not one of its calls ends the kernel first)
  }

  // sdft.h:517-529
  bool reset()
  {
    if (!pipe_join()) return false;
    cursor = 0; hist_cur = 0; st_cur = 0; fid_canonical = true;
    if (nbins == 0) return true;
    if (!bind()) return false;
    const size_t nb = nbins, span = 2 * nbins;
    SDFT_TRY(hipMemsetAsync(d_hist[0].p, 0, channels * span * sizeof(TD), stream));
    SDFT_TRY(hipMemsetAsync(acc_p(), 0, channels * nb * sizeof(fdx), stream));
    std::vector<fdx> ones(channels * nb, cmake<FD>((FD)1, (FD)0));
    if (!to_device(fid_p(), ones.data(), ones.size() * sizeof(fdx))) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    return true;
  }

  bool set_stream(hipStream_t s)
  {
    if (!pipe_join()) return false;
    if (stream) SDFT_TRY(hipStreamSynchronize(stream));
    if (own_stream && stream) (void)hipStreamDestroy(stream);
    stream = s; own_stream = false;
    return true;
  }

  bool synchronize()
  {
    if (res.alive && !resident_retire()) return false;
    if (!pipe_join()) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (status_armed)
    {
      if (aux) SDFT_TRY(hipStreamSynchronize(aux));
      if (ring_gave_up())
      {
        set_error("carry_ring_kernel", "a poll loop timed out in an asynchronous call: its output and the stream state are invalid (reset the plan or restore a state)");
        (void)collect_profile();
        return false;
      }
    }
    return collect_profile();
  }

  // ---- profiling ---------------------------------------------------------------------------
  bool prof_on(int st) const { return profile == 1 || (profile == 2 && (st == ST_FORWARD || st == ST_INVERSE)); }
  bool prof_begin(int st, hipStream_t on = nullptr)
  {
    if (!prof_on(st)) return true;
    if (ev_used[st] + 2 > ev_pool[st].size())
    {
      hipEvent_t a, b;
      SDFT_TRY(hipEventCreate(&a)); SDFT_TRY(hipEventCreate(&b));
      ev_pool[st].push_back(a); ev_pool[st].push_back(b);
    }
    SDFT_TRY(hipEventRecord(ev_pool[st][ev_used[st]], on ? on : stream));
    return true;
  }
  bool prof_end(int st, hipStream_t on = nullptr)
  {
    if (!prof_on(st)) return true;
    SDFT_TRY(hipEventRecord(ev_pool[st][ev_used[st] + 1], on ? on : stream));
    ev_used[st] += 2;
    return true;
  }
  bool collect_profile()
  {
    for (int st = 0; st < ST_COUNT; ++st)
    {
      for (size_t i = 0; i + 1 < ev_used[st]; i += 2)
      {
        SDFT_TRY(hipEventSynchronize(ev_pool[st][i + 1]));
        float ms = 0.f;
        SDFT_TRY(hipEventElapsedTime(&ms, ev_pool[st][i], ev_pool[st][i + 1]));
        prof_ms[st] += ms; prof_calls[st] += 1;
      }
      ev_used[st] = 0;
    }
    return true;
  }

  // ---- geometry and time chunking: sdft_plan_logic.hpp ---------------------------------------------------------------
  static int bins_per_lane() { return logic::bins_per_lane(sizeof(fdx)); }
  int halo_bins() const { return logic::halo_bins(window); }
  int halo_lanes() const { return logic::halo_lanes(window, sizeof(fdx)); }
  long interior_lanes() const { return logic::interior_lanes(window, sizeof(fdx), opt_interior); }
  long tiles() const { return logic::tiles(nbins, window, sizeof(fdx), opt_interior); }
  bool rows_kernel_ok(bool row_pointers) const { return logic::rows_kernel_ok(nbins, sizeof(fdx), row_pointers, opt_rows_kernel != 0, opt_row_slots_max); }
  long row_slots() const { return logic::row_slots(nbins, sizeof(fdx)); }       // slots per lane (1 or 2) ...
  long row_waves() const { return logic::row_waves(nbins, sizeof(fdx)); }       // ... and physical waves of the row group
  logic::ChunkQuery chunk_query(size_t n, bool rows_kernel) const
  {
    logic::ChunkQuery q;
    q.n = n; q.channels = channels; q.nbins = nbins; q.rows_kernel = rows_kernel; q.exact = carry_mode == CARRY_EXACT; q.pipelined = pipe_this;
    q.forced_chunk = opt_chunk; q.row_waves = row_waves(); q.tiles = tiles(); q.compute_units = compute_units;
    return q;
  }

  // floor(2^32 / d) + 1, 0 for d <= 1: what flow_position divides a workgroup number by (ForwardArgs::inv_chunks, inv_channels)
  static unsigned inv32(unsigned d) { return d <= 1 ? 0u : (unsigned)((((unsigned long long)1) << 32) / d) + 1u; }
  // every launch is a 1-D grid (channels ride on grid.x); refuse what would not fit it
  static bool grid_fits(size_t blocks)
  {
    if (blocks <= 0x7fffffffull) return true;
    set_error("launch", "grid too large: channels x chunks x bins exceed 2^31 workgroups");
    return false;
  }

  // ---- exact carries, relay form: block length / seed table -----------------------------------------
  unsigned relay_block(long len) const { return logic::relay_block(nbins, len, sizeof(FD), sizeof(fdx), opt_chain_L); }
  // flow mode of the relay form (logic::forward_route)
  long opt_relay_flow = 1, last_flow = 0;
  DevBuf<unsigned> d_ready;
  unsigned ready_seq = 0;
  unsigned* d_started = nullptr;      // device word every relay workgroup bumps when it has started
  unsigned started_target = 0;
  // The forward launch must not take CUs the relays still need (a forward workgroup that waits for a relay which cannot
  // start would be a deadlock until the bounded polls run out): a one-wave gate kernel on the forward stream polls the
  // word until the relays of the call are resident (round 3 used hipStreamWaitValue32 for this: the runtime's wait packet
  // took 135 us to notice -- profiles/r04_relay_gate_trace.txt)
  // (asked by logic::forward_route before the call's workspace: the word is zeroed by the first flow call's carries stage, as
  // when the counter would wrap)
  bool gate_ok()
  {
    if (d_started) return true;
    if (hipMalloc((void**)&d_started, 8) != hipSuccess) { (void)hipGetLastError(); d_started = nullptr; return false; }
    started_target = ~0u;
    return true;
  }
  // relays (32 bins of a channel each), waves per relay.  (Two relays per workgroup -- the kernel has the form -- were measured
  // slower, 12 waves of products and two chains on one CU contend for issue: config 3 shape, 1.5 against 1.05 ms; the option is gone)
  static unsigned relay_waves_default() { return 8u; }
  long opt_relay_groups = 1;     // test hook: relays per workgroup (2: half as many CUs; FD float only)
  template <int L> unsigned relay_groups() const { return (unsigned)std::max(1L, std::min<long>(relay_limits<FD, L>::groups, opt_relay_groups)); }
  template <int L> unsigned relay_waves() const
  {
    const long mx = relay_limits<FD, L>::waves / (long)relay_groups<L>();
    return (unsigned)std::max(1L, std::min(mx, opt_relay_waves > 0 ? opt_relay_waves : (long)relay_waves_default()));
  }
  unsigned relay_groups_of(unsigned L) const { return L <= 64 ? relay_groups<64>() : relay_groups<128>(); }
  template <int L> bool launch_relay(ChainArgs<FD> cc, unsigned relays, hipStream_t on)
  {
    const unsigned waves = relay_waves<L>(), groups = relay_groups<L>();
    const unsigned blocks = (relays + groups - 1) / groups;
    cc.P = waves; cc.chunks_channels = (unsigned)channels;
    if constexpr (L * sizeof(FD) == 512)
    {
      // the longest block also exists as a measurement build
      if (cc.stats) { hipLaunchKernelGGL((carry_relay_kernel<FD, L, true>), dim3(blocks), dim3(kWave * waves * groups), 0, on, cc); SDFT_TRY(hipGetLastError()); return true; }
    }
    if constexpr (L * sizeof(FD) <= 512)
      hipLaunchKernelGGL((carry_relay_kernel<FD, L>), dim3(blocks), dim3(kWave * waves * groups), 0, on, cc);
    SDFT_TRY(hipGetLastError());
    return true;
  }
  bool ensure_fseed(unsigned L)
  {
    if (fseed_L == L && d_fseed.p) return true;
    if (!d_fseed.reserve((2 * nbins / L) * nbins)) return false;
    hipLaunchKernelGGL((fid_seed_kernel<FD>), dim3((unsigned)((nbins + kWave - 1) / kWave)), dim3(kWave), 0, stream,
                       (const fdx*)d_tw.p, d_fseed.p, (unsigned)nbins, L);
    SDFT_TRY(hipGetLastError());
    fseed_L = L;
    return true;
  }

  // ---- forward on device-resident buffers ------------------------------------------------
  // x: [channels] x n with stride x_stride; out: rows at out + ch*out_stride + t*N, or the row
  // pointer table `rows` (device array of channels*n device pointers)
  // Checked form (what every entry point calls).  The ring form of the exact carries ends its poll loops after a bounded
  // number of tries instead of hanging the GPU; a wave that ran out says so in a word of pinned host memory
  // (ChainArgs::status).  The state a call starts from stays intact until the next call (acc, fid and the delay line are
  // double-buffered, the cursor lives on the host), so a synchronous call that finds the word changed restores that
  // state and runs again with the serial pass: the outputs are the reference's bits either way, and
  // sdft_hip_last_error() tells the host that it happened.  Asynchronous calls are checked in synchronize(), which can
  // only report (the caller's buffers may have moved on).
  unsigned* h_status = nullptr;
  unsigned* d_status = nullptr;
  unsigned status_seen = 0;
  bool status_armed = false;       // a ring launch is in flight or unchecked
  long ring_recoveries = 0;
  bool ensure_status()
  {
    if (h_status) return true;
    if (hipHostMalloc((void**)&h_status, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); h_status = nullptr; return false; }
    *h_status = 0;
    if (hipHostGetDevicePointer((void**)&d_status, h_status, 0) != hipSuccess)
    {
      (void)hipGetLastError(); (void)hipHostFree(h_status); h_status = nullptr; return false;
    }
    return true;
  }
  // after the stream has drained: did a ring launch give up since the last look?
  bool ring_gave_up()
  {
    if (!status_armed || !h_status) return false;
    status_armed = false;
    const unsigned now = *(volatile unsigned*)h_status;
    if (now == status_seen) return false;
    status_seen = now;
    return true;
  }
  // What a forward call computes: one kind, and that kind's arguments (which the caller keeps alive for the call).  A
  // default-constructed bundle is the plain analysis: every row to out / rows.  The kinds from EVERY on carry the number of the
  // kernel that serves them (logic::ForwardKernel, option "last_kernel"); all but EVERY leave `out` unused.
  // FUSE: the fused call (process_n) -- synthesis in the same launch
  // EVERY: decimated analysis (sdft_every_n) -- only the rows of that grid are stored, by forward_every_kernel
  // POWER: power-spectrogram analysis (sdft_power_n) -- forward_power_kernel stores |X|^2 of its band on its grid
  // POWER_SUM: pooled power analysis (sdft_power_sum_n) -- forward_pooled_power_kernel sums it over the grid's windows
  // POWER_PEAK: peak-hold analysis (sdft_power_peak_n) -- forward_power_peak_kernel holds its largest (hold 0) or smallest (hold 1) over those windows; psum as POWER_SUM's
  // POWER_SMOOTH: smoothed power analysis (sdft_power_smooth_n) -- forward_power_smooth_kernel runs its one-pole average at every sample and stores it on the grid
  // FILTERBANK: filterbank analysis (sdft_filterbank_n) -- forward_filterbank_kernel stores the band sums of the plan's filterbank
  // BAND_PEAK: band-peak analysis (sdft_band_peak_n) -- forward_band_peak_kernel stores per band of that filterbank the largest weighted power and its bin, as a pair; fbk as FILTERBANK's, a pair for a number
  // CROSS_SUM: cross-spectrum analysis (sdft_cross_sum_n) -- forward_cross_sum_kernel sums A conj(B) of the plan's pairs over the grid's windows
  // SMOOTH_PEAK: smoothed peak-hold analysis (sdft_smooth_peak_n) -- forward_smooth_peak_kernel holds the largest or smallest of POWER_SMOOTH's average over POWER_PEAK's windows; in a call of several chunks after a carry pass of forward_power_smooth_kernel and smooth_scan_kernel
  // CROSS_SMOOTH: smoothed cross-spectrum analysis (sdft_cross_smooth_n) -- forward_cross_smooth_kernel runs the one-pole average of that term at every sample and stores it on the grid; the carry across chunks is POWER_SMOOTH's over 2 * band numbers per pair
  // LAG_SUM: lag-product analysis (sdft_lag_sum_n) -- forward_lag_sum_kernel sums X[t] conj(X[t - 1]) of every channel over those windows; cross has the plan's channels in the pairs' place and no items
  // POWER_MOMENTS: power-moments analysis (sdft_power_moments_n) -- forward_power_moments_kernel sums the power and its square of every channel over those windows, as (s1, s2) pairs; cross as LAG_SUM's
  // COVARIANCE: covariance analysis (sdft_covariance_n) -- forward_covariance_kernel does that for all pairs of the plan's array, by blocks
  // MIX: channel-mix analysis (sdft_mix_n) -- forward_mix_kernel stores the weighted sums of the plan's mix on the grid
  struct ForwardCall
  {
    enum Kind : int { PLAIN = 0, FUSE = -1, EVERY = logic::FK_EVERY, POWER = logic::FK_POWER, POWER_SUM = logic::FK_POWER_SUM, FILTERBANK = logic::FK_FILTERBANK,
                      CROSS_SUM = logic::FK_CROSS_SUM, COVARIANCE = logic::FK_COVARIANCE, MIX = logic::FK_MIX, POWER_PEAK = logic::FK_POWER_PEAK, LAG_SUM = logic::FK_LAG_SUM,
                      POWER_MOMENTS = logic::FK_POWER_MOMENTS, BAND_PEAK = logic::FK_BAND_PEAK, POWER_SMOOTH = logic::FK_POWER_SMOOTH, CROSS_SMOOTH = logic::FK_CROSS_SMOOTH, SMOOTH_PEAK = logic::FK_SMOOTH_PEAK };
    Kind kind = PLAIN;
    int hold = 0;                                            // POWER_PEAK, SMOOTH_PEAK
    const SmoothPeakArgs<FD>* speak = nullptr;               // SMOOTH_PEAK
    const PowerSmoothArgs<FD>* smooth = nullptr;             // POWER_SMOOTH
    const FuseArgs<TD, FD>* fuse = nullptr;                  // FUSE
    const EveryGrid* every = nullptr;                        // EVERY
    const PowerArgs<FD>* power = nullptr;                    // POWER
    const PowerSumArgs<FD>* psum = nullptr;                  // POWER_SUM, POWER_PEAK
    const FilterbankArgs<FD>* fbk = nullptr;                 // FILTERBANK, BAND_PEAK
    const CrossSumArgs<FD>* cross = nullptr;                 // CROSS_SUM, LAG_SUM, POWER_MOMENTS
    const CrossSmoothArgs<FD>* xsmooth = nullptr;            // CROSS_SMOOTH
    const CovarianceArgs<FD>* cov = nullptr;                 // COVARIANCE
    const MixArgs<FD>* mix = nullptr;                        // MIX
    static ForwardCall of(Kind k) { ForwardCall c; c.kind = k; return c; }
    static ForwardCall fused(const FuseArgs<TD, FD>& a) { ForwardCall c = of(FUSE); c.fuse = &a; return c; }
    static ForwardCall decimated(const EveryGrid& a) { ForwardCall c = of(EVERY); c.every = &a; return c; }
    static ForwardCall band_power(const PowerArgs<FD>& a) { ForwardCall c = of(POWER); c.power = &a; return c; }
    static ForwardCall power_sum(const PowerSumArgs<FD>& a) { ForwardCall c = of(POWER_SUM); c.psum = &a; return c; }
    static ForwardCall power_peak(const PowerSumArgs<FD>& a, int hold) { ForwardCall c = of(POWER_PEAK); c.psum = &a; c.hold = hold; return c; }
    static ForwardCall power_smooth(const PowerSmoothArgs<FD>& a) { ForwardCall c = of(POWER_SMOOTH); c.smooth = &a; return c; }
    static ForwardCall smooth_peak(const SmoothPeakArgs<FD>& a, int hold) { ForwardCall c = of(SMOOTH_PEAK); c.speak = &a; c.hold = hold; return c; }
    static ForwardCall filterbank(const FilterbankArgs<FD>& a) { ForwardCall c = of(FILTERBANK); c.fbk = &a; return c; }
    static ForwardCall band_peak(const FilterbankArgs<FD>& a) { ForwardCall c = of(BAND_PEAK); c.fbk = &a; return c; }
    static ForwardCall cross_sum(const CrossSumArgs<FD>& a) { ForwardCall c = of(CROSS_SUM); c.cross = &a; return c; }
    static ForwardCall cross_smooth(const CrossSmoothArgs<FD>& a) { ForwardCall c = of(CROSS_SMOOTH); c.xsmooth = &a; return c; }
    static ForwardCall lag_sum(const CrossSumArgs<FD>& a) { ForwardCall c = of(LAG_SUM); c.cross = &a; return c; }
    static ForwardCall power_moments(const CrossSumArgs<FD>& a) { ForwardCall c = of(POWER_MOMENTS); c.cross = &a; return c; }
    static ForwardCall covariance(const CovarianceArgs<FD>& a) { ForwardCall c = of(COVARIANCE); c.cov = &a; return c; }
    static ForwardCall channel_mix(const MixArgs<FD>& a) { ForwardCall c = of(MIX); c.mix = &a; return c; }
  };
  bool forward_device(size_t n, const TD* x, size_t x_stride, fdx* out, size_t out_stride, fdx* const* rows, const ForwardCall& c = ForwardCall())
  {
    const struct { size_t cursor; int st_cur, hist_cur; bool fid_canonical; } was{cursor, st_cur, hist_cur, fid_canonical};
    auto restore = [&] { cursor = was.cursor; st_cur = was.st_cur; hist_cur = was.hist_cur; fid_canonical = was.fid_canonical; };
    if (!forward_launch(n, x, x_stride, out, out_stride, rows, c))
    {
      // a launch that failed half-way (a host expression that does not compile, a grid that does not fit, an allocation)
      // must not leave the stream half-advanced: what was queued wrote the OTHER buffer set and the workspace only
      restore();
      return false;
    }
    if (last_chain < 2 || async) return true;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (aux) SDFT_TRY(hipStreamSynchronize(aux));
    if (!ring_gave_up()) return true;
    restore();
    const long saved = opt_chain;
    opt_chain = 0;
    const bool ok = forward_launch(n, x, x_stride, out, out_stride, rows, c) && (hipStreamSynchronize(stream) == hipSuccess);
    opt_chain = saved;
    ++ring_recoveries;
    // a recovered call is a valid call: it goes to the warning channel (and the counter), not to the error channel, so a
    // host that checks sdft_hip_last_error() after every call does not feed the samples twice
    if (ok) set_warning("carry_relay_kernel", "a poll loop timed out; the call was re-run with the serial carry pass (results are valid)");
    else
    {
      restore();
      set_error("carry_relay_kernel", "a poll loop timed out and the re-run with the serial carry pass failed");
    }
    return ok;
  }

  logic::ForwardQuery forward_query(size_t n, const fdx* out, size_t out_stride, fdx* const* rows, const ForwardCall& c) const
  {
    logic::ForwardQuery q;
    q.n = n; q.nbins = nbins; q.channels = channels; q.fd_bytes = sizeof(FD); q.fdx_bytes = sizeof(fdx);
    q.window = window; q.compute_units = compute_units; q.cursor = cursor; q.exact = carry_mode == CARRY_EXACT; q.fid_canonical = fid_canonical;
    q.fuse = c.kind == ForwardCall::FUSE;
    q.fuse_store = q.fuse && c.fuse->store;
    q.reference_order = q.fuse && wants_reference_order();
    q.coeff_ready = coeff_ready;
    q.every = c.kind == ForwardCall::EVERY;
    q.power = c.kind == ForwardCall::POWER;
    q.power_sum = c.kind == ForwardCall::POWER_SUM;
    q.power_peak = c.kind == ForwardCall::POWER_PEAK;
    q.power_smooth = c.kind == ForwardCall::POWER_SMOOTH;
    q.smooth_peak = c.kind == ForwardCall::SMOOTH_PEAK;
    q.filterbank = c.kind == ForwardCall::FILTERBANK;
    q.band_peak = c.kind == ForwardCall::BAND_PEAK;
    q.cross_sum = c.kind == ForwardCall::CROSS_SUM;
    q.cross_smooth = c.kind == ForwardCall::CROSS_SMOOTH;
    q.lag_sum = c.kind == ForwardCall::LAG_SUM;
    q.power_moments = c.kind == ForwardCall::POWER_MOMENTS;
    q.covariance = c.kind == ForwardCall::COVARIANCE;
    q.mix = c.kind == ForwardCall::MIX;
    q.power_every = q.power ? (size_t)c.power->every : (q.filterbank || q.band_peak) ? (size_t)c.fbk->every : q.mix ? (size_t)c.mix->every : 1;
    q.cross_items = c.cross ? c.cross->nitems : c.xsmooth ? c.xsmooth->nitems : q.covariance ? c.cov->nitems : q.mix ? c.mix->nitems : 0;
    q.row_pointers = rows != nullptr;
    q.out = reinterpret_cast<uintptr_t>(out);
    q.out_stride = out_stride;
    q.analysis_batch = calls.analysis_batch; q.pipe_wanted = pipe_wanted(nullptr); q.prev_out = prev_out;
    q.rows_kernel = opt_rows_kernel; q.row_slots_max = opt_row_slots_max; q.interior = opt_interior; q.chunk = opt_chunk; q.self = opt_self;
    q.fused = opt_fused; q.fold = opt_fold; q.fft_carry = opt_fft_carry; q.hop_kernel = opt_hop_kernel; q.chain = opt_chain; q.chain_L = opt_chain_L;
    q.relay_flow = opt_relay_flow; q.segments = opt_segments; q.xcd_map = opt_xcd_map; q.rows_f32 = opt_rows_f32; q.pipeline = opt_pipeline;
    q.prefix_cells = opt_prefix_cells;
    return q;
  }

  // The route (logic::forward_route) decides; this runs it: the hop and self-carried routes in a launch of their own, every
  // other route as delta -> carries -> forward
  bool forward_launch(size_t n, const TD* x, size_t x_stride, fdx* out, size_t out_stride, fdx* const* rows, const ForwardCall& c)
  {
    if (n == 0 || nbins == 0) return true;
    SDFT_TRY(hipSetDevice(device));
    flag_pending = false;                                    // only the hop kernel signals its completion
    calls.on_analysis(c.kind == ForwardCall::FUSE);          // (which kind of host is calling: logic::CallPattern)
    const logic::ForwardRoute r = logic::forward_route(forward_query(n, out, out_stride, rows, c), [this] { return gate_ok(); });
    pipe_this = r.pipelined;
    if (r.out.hi) prev_out = r.out;
    last_kernel = r.kernel; last_chunks = r.chunks; last_chunk_len = r.len; last_tiles = r.tiles; last_interior = r.interior;
    last_segments = r.segments; last_fused = r.fused; last_self = r.self; last_prefix = r.prefix; last_chain = r.carry == logic::CARRY_RELAY ? 3 : 0;
    if (r.kernel == logic::FK_HOP) { if (!pipe_join()) return false; return forward_hop(n, x, x_stride, out, out_stride, rows); }
    if (r.self || r.prefix) return forward_self(n, x, x_stride, out, out_stride, r.chunks, r.len, c, r.prefix);
    if (!pipe_join()) return false;

    // workspace
    const size_t nb = nbins, span = 2 * nbins;
    if (!d_delta.reserve(channels * n + 128)) return false;     // + slack: the exact pass prefetches bursts past a run
    if (!d_carry.reserve(channels * (size_t)r.chunks * nb)) return false;
    if (r.use_seed && !r.relay_L && !d_seed.reserve(channels * (size_t)r.chunks * nb)) return false;
    if (r.relay_L && !ensure_fseed(r.relay_L)) return false;
    if (r.segments > 1 || r.flow)
    {
      if (!aux) SDFT_TRY(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
      if (!ev_delta) SDFT_TRY(hipEventCreateWithFlags(&ev_delta, hipEventDisableTiming));
      while ((long)seg_events.size() < r.segments)
      {
        hipEvent_t e; SDFT_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        seg_events.push_back(e);
      }
      for (int q = 0; q < 2; ++q)
        if (!d_run_acc[q].reserve(channels * nb) || !d_run_fid[q].reserve(channels * nb)) return false;
    }

    DeltaIn<TD, FD> din;
    if (!forward_delta(r, n, x, x_stride, din) || !forward_carries(r, n, din) || !forward_rows_stage(r, n, out, out_stride, rows, c)) return false;

    // fid stays on the canonical rotation sequence unless this call seeded chunks from the closed-form
    // table; a call that crosses the roll-over with serial fid arithmetic puts it back
    if (!r.use_seed) fid_canonical = false;
    else if (cursor + n >= span) fid_canonical = true;
    cursor = (cursor + n) % span;
    st_cur ^= 1;
    return true;
  }
  // K0: differences + delay line -- unless the chunk-parallel carry kernel forms them itself
  bool forward_delta(const logic::ForwardRoute& r, size_t n, const TD* x, size_t x_stride, DeltaIn<TD, FD>& din)
  {
    const size_t span = 2 * nbins;
    if (!r.delta_in_carry)
    {
      if (!prof_begin(ST_DELTA)) return false;
      const size_t per_ch = (std::max(n, span) + kBlock - 1) / kBlock;
      if (!grid_fits(per_ch * channels)) return false;
      const bool single = r.chunks == 1;
      hipLaunchKernelGGL((delta_kernel<TD, FD>), dim3((unsigned)(per_ch * channels)), dim3(kBlock), 0, stream, x, x_stride,
                         d_hist[hist_cur].p, d_hist[hist_cur ^ 1].p, d_delta.p, n, span,
                         (const fdx*)acc_p(), (const fdx*)fid_p(), single ? d_carry.p : (fdx*)nullptr, single ? d_seed.p : (fdx*)nullptr,
                         (unsigned)per_ch);
      SDFT_TRY(hipGetLastError());
      if (!prof_end(ST_DELTA)) return false;
    }
    din.x = r.delta_in_carry ? x : nullptr; din.x_stride = x_stride;
    din.hist_in = d_hist[hist_cur].p; din.hist_out = d_hist[hist_cur ^ 1].p; din.delta_out = d_delta.p;
    hist_cur ^= 1;
    return true;
  }
  // carries: time segments of the exact pass on `aux` (each segment's forward launch on `stream` waits for its event), the relay
  // form (flow mode: one launch, the forward workgroups wait for their chunk's carries), or the pre-pass partial sums + scan
  bool forward_carries(const logic::ForwardRoute& r, size_t n, const DeltaIn<TD, FD>& din)
  {
    const size_t nb = nbins, span = 2 * nbins;
    const long chunks = r.chunks, segments = r.segments;
    if (r.flow && started_target > (1u << 30))
    {
      // a new start word, or long before the counter could wrap: drain both streams and begin it again (once per ~8 million calls)
      if (aux) SDFT_TRY(hipStreamSynchronize(aux));
      SDFT_TRY(hipStreamSynchronize(stream));
      SDFT_TRY(hipMemset(d_started, 0, 8));
      started_target = 0;
    }
    if (segments > 1 || r.flow)
    {
      SDFT_TRY(hipEventRecord(ev_delta, stream));                 // delta (and everything before) done
      SDFT_TRY(hipStreamWaitEvent(aux, ev_delta, 0));
    }
    // the stage's events go where its kernels go (the overlapped exact pass runs on `aux`)
    hipStream_t carry_stream = (segments > 1 || r.flow) ? aux : stream;
    if (!prof_begin(ST_CARRY, carry_stream)) return false;
    CarryArgs<FD> ca;
    ca.acc_next = nullptr; ca.fid_next = nullptr; ca.chunk0 = 0; ca.launch_chunks = (unsigned)chunks;
    ca.delta = d_delta.p; ca.tw = d_tw.p; ca.wtab = d_wtab.p; ca.carry = d_carry.p; ca.seed = d_seed.p;
    ca.acc_state = acc_p(); ca.fid_state = fid_p(); ca.n = n;
    ca.nbins = (unsigned)nb; ca.chunks = (unsigned)chunks; ca.chunk_len = (unsigned)r.len; ca.cursor0 = (unsigned)cursor;
    const unsigned bin_blocks = (unsigned)((nb + kBlock - 1) / kBlock), eblocks = (unsigned)logic::relays(nb);
    if (!grid_fits((size_t)bin_blocks * (size_t)chunks * channels) || !grid_fits(((nb + kScanBins - 1) / kScanBins) * channels) ||
        !grid_fits((size_t)eblocks * channels)) return false;
    if (r.carry == logic::CARRY_RELAY)
    {
      for (long sg = 0; sg < segments; ++sg)
      {
        const long j0 = chunks * sg / segments, j1 = chunks * (sg + 1) / segments;
        ChainArgs<FD> cc{};
        cc.delta = d_delta.p; cc.tw = d_tw.p; cc.fseed = d_fseed.p; cc.carry = d_carry.p;
        cc.acc_state = sg == 0 ? acc_p() : d_run_acc[(sg - 1) & 1].p;
        cc.acc_next = segments > 1 ? d_run_acc[sg & 1].p : nullptr;
        cc.n = n; cc.nbins = (unsigned)nb; cc.chunks = (unsigned)chunks; cc.chunk_len = (unsigned)r.len; cc.cursor0 = (unsigned)cursor;
        cc.chunk0 = (unsigned)j0; cc.launch_chunks = (unsigned)(j1 - j0); cc.L = r.relay_L; cc.P = 0; cc.chunk_shift = r.shift; cc.debug = (unsigned)opt_chain_debug & (47u | 128u); cc.stats = nullptr;
        if (opt_chain_debug & (16 | 64 | 128)) { if (!d_chain_stats.reserve(64 + 3 * 1024)) return false; cc.stats = d_chain_stats.p; }
        cc.status = ensure_status() ? d_status : nullptr;
        if (cc.status) status_armed = true;
        cc.ready = nullptr; cc.ready_seq = 0; cc.started = nullptr; cc.chunks_channels = (unsigned)channels;
        if (r.flow)
        {
          const size_t words = channels * (size_t)chunks * eblocks;
          if (d_ready.cap < words)
          {
            if (!d_ready.reserve(words)) return false;
            SDFT_TRY(hipMemsetAsync(d_ready.p, 0, d_ready.cap * sizeof(unsigned), carry_stream));
            ready_seq = 0;
          }
          if (++ready_seq == 0) { SDFT_TRY(hipMemsetAsync(d_ready.p, 0, d_ready.cap * sizeof(unsigned), carry_stream)); ready_seq = 1; }
          cc.ready = d_ready.p; cc.ready_seq = ready_seq; cc.started = d_started;
        }
        const unsigned cblocks = eblocks * (unsigned)channels;
        bool ok = true;
        switch (r.relay_L)
        {
          case 128: ok = launch_relay<128>(cc, cblocks, carry_stream); break;
          case 64:  ok = launch_relay<64>(cc, cblocks, carry_stream); break;
          case 32:  ok = launch_relay<32>(cc, cblocks, carry_stream); break;
          case 16:  ok = launch_relay<16>(cc, cblocks, carry_stream); break;
          default:  ok = launch_relay<8>(cc, cblocks, carry_stream); break;
        }
        if (!ok) return false;
        if (segments > 1 || r.flow) SDFT_TRY(hipEventRecord(seg_events[sg], aux));
        if (r.flow)
        {
          // the forward launch may go once every relay workgroup of this launch is resident
          const unsigned relays = cblocks, groups = relay_groups_of(r.relay_L);
          started_target += (relays + groups - 1) / groups;
          hipLaunchKernelGGL((relay_gate_kernel<FD>), dim3(1), dim3(kWave), 0, stream, (const unsigned*)d_started, started_target);
          SDFT_TRY(hipGetLastError());
        }
      }
    }
    else if (r.carry == logic::CARRY_SERIAL)
    {
      for (long sg = 0; sg < segments; ++sg)
      {
        const long j0 = chunks * sg / segments, j1 = chunks * (sg + 1) / segments;
        CarryArgs<FD> cs = ca;
        cs.chunk0 = (unsigned)j0; cs.launch_chunks = (unsigned)(j1 - j0);
        cs.acc_state = sg == 0 ? acc_p() : d_run_acc[(sg - 1) & 1].p;
        cs.fid_state = sg == 0 ? fid_p() : d_run_fid[(sg - 1) & 1].p;
        cs.acc_next = d_run_acc[sg & 1].p; cs.fid_next = d_run_fid[sg & 1].p;
        hipLaunchKernelGGL((carry_exact_kernel<FD>), dim3(eblocks * (unsigned)channels), dim3(kWave), 0,
                           segments > 1 ? aux : stream, cs);
        SDFT_TRY(hipGetLastError());
        if (segments > 1) SDFT_TRY(hipEventRecord(seg_events[sg], aux));
      }
    }
    else if (r.carry == logic::CARRY_SUMS)
    {
      // partial sums per chunk, then the scan over chunks
      const size_t span_bytes = span * sizeof(fdx);
      const unsigned sum_chunks = (unsigned)(chunks - (r.delta_in_carry ? 0 : 1));
      if (r.sums == logic::SUMS_FFT2)
      {
        unsigned lg = 0; while (((size_t)1 << lg) < span) ++lg;
        hipLaunchKernelGGL((chunk_fft_kernel<TD, FD>), dim3((unsigned)(sum_chunks * channels)), dim3(kBlock), span_bytes, stream, ca, lg, din);
      }
      else if (r.sums == logic::SUMS_FFT_MIXED)
        hipLaunchKernelGGL((chunk_fft_mixed_kernel<TD, FD>), dim3((unsigned)(sum_chunks * channels)), dim3(kBlock), 2 * span_bytes,
                           stream, ca, (unsigned)span, smooth_radices(span), din);
      else
      {
        if (!grid_fits((size_t)bin_blocks * sum_chunks * channels)) return false;
        hipLaunchKernelGGL((chunk_sum_kernel<TD, FD>), dim3((unsigned)((size_t)bin_blocks * sum_chunks * channels)), dim3(kBlock), 0, stream, ca, din);
      }
      SDFT_TRY(hipGetLastError());
      hipLaunchKernelGGL((carry_scan_kernel<FD>), dim3((unsigned)(((nb + kScanBins - 1) / kScanBins) * channels)),
                         dim3(kScanBins * kScanSlices), 0, stream, ca);
      SDFT_TRY(hipGetLastError());
    }
    // (CARRY_STATE, a single chunk: the stream state is the carry; delta_kernel has already copied it)
    return prof_end(ST_CARRY, carry_stream);
  }
  // K1: the rows, one launch per time segment (the new state goes to the other buffer set: the one a call started from survives
  // it, see forward_device)
  bool forward_rows_stage(const logic::ForwardRoute& r, size_t n, fdx* out, size_t out_stride, fdx* const* rows, const ForwardCall& c)
  {
    using K = ForwardCall;
    const FuseArgs<TD, FD>* const fuse = c.fuse;
    const size_t nb = nbins;
    const long chunks = r.chunks, segments = r.segments;
    // cross-spectrum, lag-product and power-moments analysis: the workspace of the windows a chunk boundary cuts (grown on demand, kept by the
    // plan); the work items take the channels' place in the launch
    CrossSumArgs<FD> cs{};
    if (c.cross)
    {
      cs = *c.cross;
      if (!d_cross_ws.reserve(logic::cross_sum_workspace(cs.nitems, (size_t)chunks, cs.nbins_out))) return false;
      cs.ws = chunks > 1 ? d_cross_ws.p : nullptr;
    }
    // covariance analysis: likewise, one workspace slot per output index
    CovarianceArgs<FD> cv{};
    if (c.cov)
    {
      cv = *c.cov;
      if (!d_cov_ws.reserve(logic::covariance_workspace(cv.nch, (size_t)chunks, cv.nbins_out))) return false;
      cv.ws = chunks > 1 ? d_cov_ws.p : nullptr;
    }
    const size_t launch_channels = c.cross ? cs.nitems : c.xsmooth ? c.xsmooth->nitems : c.cov ? cv.nitems : c.mix ? c.mix->nitems : channels;
    // pooled power and peak-hold analysis: the workspace of the windows a chunk boundary cuts (grown on demand, kept by the plan)
    PowerSumArgs<FD> ps{};
    if (c.psum)
    {
      ps = *c.psum;
      if (!d_psum_ws.reserve(logic::power_sum_workspace(channels, (size_t)chunks, ps.nbins_out))) return false;
      ps.ws = chunks > 1 ? d_psum_ws.p : nullptr;
    }
    // smoothed power analysis: the workspace of the chunks' end values and the table of the decay's powers (likewise; a call of one
    // chunk needs neither)
    PowerSmoothArgs<FD> sm{};
    if (c.smooth)
    {
      sm = *c.smooth;
      if (chunks > 1)
      {
        if (!d_smooth_ws.reserve(logic::power_smooth_workspace(channels, (size_t)chunks, sm.nbins_out))) return false;
        if (smooth_pw_a != sm.a || smooth_pw_len != (size_t)r.len)
        {
          const std::vector<FD> table = logic::power_smooth_table<FD>(sm.a, (size_t)r.len);
          smooth_pw_a = (FD)-1;                              // (a failure leaves no half-written table behind as a valid one)
          if (!d_smooth_pw.reserve(table.size()) || !to_device(d_smooth_pw.p, table.data(), table.size() * sizeof(FD))) return false;
          smooth_pw_a = sm.a; smooth_pw_len = (size_t)r.len;
        }
        sm.ends = d_smooth_ws.p; sm.pw = d_smooth_pw.p;
      }
    }
    // smoothed peak-hold analysis: the peak-hold call's workspace of cut windows, and for a call of several chunks the smoothed
    // power call's workspace and table; sc is what the carry pass and the scan see of the call -- no output, a grid that keeps no
    // row, the call's state buffers (the row pass writes state_out again, after the scan, with the bits of its last sample)
    SmoothPeakArgs<FD> sp{};
    PowerSmoothArgs<FD> sc{};
    if (c.speak)
    {
      sp = *c.speak;
      const unsigned band = sp.rows.nbins_out;
      if (!d_psum_ws.reserve(logic::power_sum_workspace(channels, (size_t)chunks, band))) return false;
      sp.rows.ws = chunks > 1 ? d_psum_ws.p : nullptr;
      if (chunks > 1)
      {
        if (!d_smooth_ws.reserve(logic::power_smooth_workspace(channels, (size_t)chunks, band))) return false;
        if (smooth_pw_a != sp.a || smooth_pw_len != (size_t)r.len)
        {
          const std::vector<FD> table = logic::power_smooth_table<FD>(sp.a, (size_t)r.len);
          smooth_pw_a = (FD)-1;                              // (as above)
          if (!d_smooth_pw.reserve(table.size()) || !to_device(d_smooth_pw.p, table.data(), table.size() * sizeof(FD))) return false;
          smooth_pw_a = sp.a; smooth_pw_len = (size_t)r.len;
        }
        sp.ends = d_smooth_ws.p;
        const logic::SmoothPeakCarryGrid none = logic::smooth_peak_carry_grid(n);
        sc = PowerSmoothArgs<FD>{nullptr, 0, sp.state_in, sp.state_out, d_smooth_ws.p, d_smooth_pw.p, sp.a, sp.b, none.every, none.first, sp.rows.bin0, band};
      }
    }
    // smoothed cross-spectrum analysis: the same workspace and table with the pairs for channels and rows of 2 * band numbers; xc is
    // what the scan and the fix-up see of the call
    CrossSmoothArgs<FD> xs{};
    PowerSmoothArgs<FD> xc{};
    if (c.xsmooth)
    {
      xs = *c.xsmooth;
      if (chunks > 1)
      {
        const size_t unit_row = logic::cross_smooth_unit_row(xs.nbins_out);
        if (!d_smooth_ws.reserve(logic::power_smooth_workspace(xs.npairs, (size_t)chunks, unit_row))) return false;
        if (smooth_pw_a != xs.a || smooth_pw_len != (size_t)r.len)
        {
          const std::vector<FD> table = logic::power_smooth_table<FD>(xs.a, (size_t)r.len);
          smooth_pw_a = (FD)-1;                              // (as above)
          if (!d_smooth_pw.reserve(table.size()) || !to_device(d_smooth_pw.p, table.data(), table.size() * sizeof(FD))) return false;
          smooth_pw_a = xs.a; smooth_pw_len = (size_t)r.len;
        }
        xs.ends = d_smooth_ws.p;
        xc = PowerSmoothArgs<FD>{xs.out, xs.out_stride, xs.state_in, xs.state_out, xs.ends, d_smooth_pw.p, xs.a, xs.b, xs.every, xs.first, 2u * xs.bin0, (unsigned)unit_row};
      }
    }
    // filterbank and band-peak analysis: the workspace of the bands a tile boundary cuts, [channels][rows of a launch][slots]
    // (likewise) of numbers or of pairs; the chunks go in launches whose rows keep it within its bound (logic::filterbank_next_span)
    FilterbankArgs<FD> fb{};
    const FilterbankArgs<FD>* const fbk = c.fbk;
    const bool peak = c.kind == K::BAND_PEAK;
    const size_t fb_rows = !fbk ? 0 : peak ? logic::band_peak_segment_rows(channels, fbk->nslots, sizeof(FD)) : logic::filterbank_segment_rows(channels, fbk->nslots, sizeof(FD));
    if (fbk)
    {
      fb = *fbk;
      size_t most = 0;
      for (long sg = 0; sg < segments && fb.nslots; ++sg)
        for (long ja = chunks * sg / segments, j1 = chunks * (sg + 1) / segments; ja < j1;)
        {
          const logic::FilterbankSpan sp = logic::filterbank_next_span(ja, j1, r.len, r.shift, n, (size_t)fb.every, (size_t)fb.first, fb_rows);
          most = std::max(most, sp.rows); ja = sp.jb;
        }
      if (!d_fb_ws.reserve(peak ? logic::band_peak_workspace(channels, most, fb.nslots) : logic::filterbank_workspace(channels, most, fb.nslots))) return false;
      fb.ws = d_fb_ws.p;
    }
    if (!prof_begin(ST_FORWARD)) return false;
    ForwardArgs<FD> fa{};
    fa.delta = d_delta.p; fa.tw = d_tw.p; fa.wtab = d_wtab.p; fa.carry = d_carry.p;
    fa.seed = (r.use_seed && !r.relay_L) ? d_seed.p : nullptr;
    fa.fseed = r.relay_L ? d_fseed.p : nullptr; fa.fseed_L = r.relay_L;
    fa.out = out; fa.out_stride = out_stride; fa.out_rows = rows;
    fa.acc_state = d_accs[st_cur ^ 1].p; fa.fid_state = d_fids[st_cur ^ 1].p; fa.n = n;
    fa.nbins = (unsigned)nb; fa.chunks = (unsigned)chunks; fa.chunk_len = (unsigned)r.len; fa.tiles = (unsigned)r.tiles;
    fa.interior_lanes = (unsigned)r.interior; fa.cursor0 = (unsigned)cursor; fa.chunk_shift = r.shift;
    fa.vec_store = r.vec_store ? 1 : 0;
    fa.wscale = (window == WIN_HANN) ? (FD)(tab.aweight * (FD)(0.25)) : tab.aweight;   // :371
    fa.done.flag = nullptr; fa.done.count = nullptr; fa.done.seq = 0; fa.done.total = 0;
    fa.ready = nullptr; fa.ready_seq = 0; fa.ready_n = 0; fa.ready_channels = (unsigned)channels; fa.ready_status = nullptr; fa.ready_status_seen = 0;
    fa.inv_channels = inv32((unsigned)channels);
    if (r.flow)
    {
      fa.ready = d_ready.p; fa.ready_seq = ready_seq; fa.ready_n = (unsigned)logic::relays(nb);
      fa.ready_status = ensure_status() ? d_status : nullptr;
      fa.ready_status_seen = fa.ready_status ? *(volatile unsigned*)h_status : 0u;
      if (fa.ready_status) status_armed = true;
    }
    if (r.arm_flag) fa.done = arm_flag((unsigned)(channels * (size_t)chunks));
    const bool exact_order = fuse && wants_reference_order();
    if (fuse) { last_fused_exact = exact_order; last_fused_fold = r.folded; }
    if (!fuse && r.kernel == logic::FK_ROWS) last_rows_f32 = r.rows_f32;
    for (long sg = 0; sg < segments; ++sg)
    {
      const long j0 = chunks * sg / segments, j1 = chunks * (sg + 1) / segments;
      const size_t groups = launch_channels * (size_t)(j1 - j0);
      fa.chunk0 = (unsigned)j0; fa.launch_chunks = (unsigned)(j1 - j0); fa.inv_chunks = inv32(fa.launch_chunks);
      fa.xcd_map = logic::xcd_groups(r.xcd_map, groups);
      fa.total_waves = (unsigned long long)groups * (unsigned long long)r.tiles;
      if (segments > 1) SDFT_TRY(hipStreamWaitEvent(stream, seg_events[sg], 0));      // (flow mode: the kernel waits chunk by chunk)
      const unsigned long long blocks = (fa.total_waves + kWavesPerBlock - 1) / kWavesPerBlock;
      const unsigned threads = (unsigned)(row_waves() * kWave);
      switch (c.kind)
      {
      case K::FUSE:
        // rows never leave the workgroup: synthesis in the same launch (caller checked rows_kernel_ok())
        if (r.folded) { if (!launch_process(fa, *fuse, (unsigned)groups, r.fused)) return false; }
        else if (r.kernel != logic::FK_ROWS) { set_error("sdft_hip_process_n", "rows of this length are fused in the folded form only"); return false; }
        else if (!launch_syn(fa, *fuse, (unsigned)groups, threads, r.fused && !exact_order, exact_order)) return false;
        break;
      case K::PLAIN:
        if (r.kernel == logic::FK_ROWS) launch_forward_rows(fa, (unsigned)groups, threads, r.fused, r.rows_f32);
        else launch_forward(fa, (unsigned)blocks);
        break;
      case K::FILTERBANK:
      case K::BAND_PEAK:
        for (long ja = j0; ja < j1;)
        {
          const logic::FilterbankSpan sp = logic::filterbank_next_span(ja, j1, r.len, r.shift, n, (size_t)fb.every, (size_t)fb.first, fb_rows);
          const size_t span_groups = channels * (size_t)(sp.jb - sp.ja);
          fa.chunk0 = (unsigned)sp.ja; fa.launch_chunks = (unsigned)(sp.jb - sp.ja); fa.inv_chunks = inv32(fa.launch_chunks);
          fa.xcd_map = logic::xcd_groups(r.xcd_map, span_groups);
          fa.total_waves = (unsigned long long)span_groups * (unsigned long long)r.tiles;
          const unsigned long long span_blocks = (fa.total_waves + kWavesPerBlock - 1) / kWavesPerBlock;
          if (!grid_fits(span_blocks)) return false;
          fb.ws_row0 = sp.row0; fb.ws_rows = sp.rows;
          if (peak) launch_forward_band_peak(fa, fb, (unsigned)span_blocks); else launch_forward_filterbank(fa, fb, (unsigned)span_blocks);
          SDFT_TRY(hipGetLastError());
          ++(peak ? last_band_peak_launches : last_filterbank_launches);
          if (fb.nsplits && sp.rows && !(peak ? launch_band_peak_rows(fb) : launch_filterbank_rows(fb))) return false;   // the split bands of these rows, before the next launch reuses the workspace
          ja = sp.jb;
        }
        break;
      case K::LAG_SUM: if (!grid_fits(blocks)) return false; launch_forward_lag_sum(fa, cs, (unsigned)blocks); break;
      case K::POWER_MOMENTS: if (!grid_fits(blocks)) return false; launch_forward_power_moments(fa, cs, (unsigned)blocks); break;
      case K::CROSS_SUM: if (!grid_fits(blocks)) return false; launch_forward_cross_sum(fa, cs, (unsigned)blocks); break;
      case K::COVARIANCE: if (!grid_fits(blocks)) return false; if (!launch_forward_covariance(fa, cv, (unsigned)blocks)) return false; break;
      case K::MIX: if (!grid_fits(blocks)) return false; if (!launch_forward_mix(fa, *c.mix, (unsigned)blocks)) return false; break;
      case K::POWER_PEAK: if (!grid_fits(blocks)) return false; launch_forward_power_peak(fa, ps, (unsigned)blocks, c.hold); break;
      case K::POWER_SUM: if (!grid_fits(blocks)) return false; launch_forward_power_sum(fa, ps, (unsigned)blocks); break;
      case K::POWER_SMOOTH: if (!grid_fits(blocks)) return false; launch_forward_power_smooth(fa, sm, (unsigned)blocks); break;
      case K::CROSS_SMOOTH: if (!grid_fits(blocks)) return false; launch_forward_cross_smooth(fa, xs, (unsigned)blocks); break;
      case K::SMOOTH_PEAK:                                   // one chunk: the rows at once; several: the carry pass first
        if (!grid_fits(blocks)) return false;
        if (chunks > 1) launch_forward_power_smooth(fa, sc, (unsigned)blocks); else launch_forward_smooth_peak(fa, sp, (unsigned)blocks, c.hold);
        break;
      case K::POWER: if (!grid_fits(blocks)) return false; launch_forward_power(fa, *c.power, (unsigned)blocks); break;
      case K::EVERY: if (!grid_fits(blocks)) return false; launch_forward_every(fa, *c.every, (unsigned)blocks); break;
      }
      SDFT_TRY(hipGetLastError());
    }
    SDFT_TRY(hipGetLastError());
    // the rows a chunk boundary cut, from the workspace: per channel for the pooled power and the peak-hold call (which holds instead
    // of adding); per pair for the cross-spectrum, the lag-product, the power-moments (their pairs are the plan's channels) and the covariance call,
    // whose complex sums (or pairs of sums) over nbins_out bins are real sums over 2 * nbins_out numbers -- the pooled power call's adder
    if (chunks > 1 && (c.psum || c.cross || c.cov))
    {
      const PowerSumArgs<FD> pieces = c.psum ? ps
                                    : c.cross ? PowerSumArgs<FD>{cs.row0, cs.row0_stride, cs.rest, cs.rest_stride, cs.ws, cs.every, cs.first, cs.bin0, 2u * cs.nbins_out}
                                              : PowerSumArgs<FD>{cv.row0, cv.row0_stride, cv.rest, cv.rest_stride, cv.ws, cv.every, cv.first, cv.bin0, 2u * cv.nbins_out};
      const size_t units = c.psum ? channels : c.cross ? cs.npairs : cv.npairs;
      if (!(c.kind == K::POWER_PEAK ? launch_peak_rows(pieces, n, chunks, r.len, r.shift, units, c.hold) : launch_power_sum_rows(pieces, n, chunks, r.len, r.shift, units))) return false;
      SDFT_TRY(hipGetLastError());
    }
    // the smoothed power call's carry across chunks: the scan of the end values, then what the chunks c >= 1 left out of their rows
    if (chunks > 1 && c.smooth)
    {
      if (!launch_smooth_scan(sm, n, chunks, r.len, r.shift, channels)) return false;
      const size_t kept = logic::every_rows(n, (size_t)sm.every, (size_t)sm.first);
      if (kept && !launch_smooth_fix(sm, kept, chunks, r.len, r.shift, channels)) return false;
      SDFT_TRY(hipGetLastError());
    }
    // the smoothed peak-hold call of several chunks: the scan turns the carry pass's end values into the chunks' starts, the row
    // pass runs over the same chunks (the segments' carries have all been waited for; it reads d_carry and writes the same half of
    // the stream state with the same values as the carry pass did), then the windows a chunk boundary cut
    if (chunks > 1 && c.speak)
    {
      if (!launch_smooth_scan(sc, n, chunks, r.len, r.shift, channels)) return false;
      for (long sg = 0; sg < segments; ++sg)
      {
        const long j0 = chunks * sg / segments, j1 = chunks * (sg + 1) / segments;
        const size_t groups = channels * (size_t)(j1 - j0);
        fa.chunk0 = (unsigned)j0; fa.launch_chunks = (unsigned)(j1 - j0); fa.inv_chunks = inv32(fa.launch_chunks);
        fa.xcd_map = logic::xcd_groups(r.xcd_map, groups);
        fa.total_waves = (unsigned long long)groups * (unsigned long long)r.tiles;
        const unsigned long long blocks = (fa.total_waves + kWavesPerBlock - 1) / kWavesPerBlock;
        if (!grid_fits(blocks)) return false;
        launch_forward_smooth_peak(fa, sp, (unsigned)blocks, c.hold);
        SDFT_TRY(hipGetLastError());
      }
      if (!launch_peak_rows(sp.rows, n, chunks, r.len, r.shift, channels, c.hold)) return false;
      SDFT_TRY(hipGetLastError());
    }
    // the smoothed cross-spectrum call's: the same two kernels over its pairs
    if (chunks > 1 && c.xsmooth)
    {
      if (!launch_smooth_scan(xc, n, chunks, r.len, r.shift, xs.npairs)) return false;
      const size_t kept = logic::every_rows(n, (size_t)xs.every, (size_t)xs.first);
      if (kept && !launch_smooth_fix(xc, kept, chunks, r.len, r.shift, xs.npairs)) return false;
      SDFT_TRY(hipGetLastError());
    }
    if (r.flow) SDFT_TRY(hipStreamWaitEvent(stream, seg_events[0], 0));          // the call ends when both launches have
    last_flow = r.flow;
    return prof_end(ST_FORWARD);
  }

  static RadixList smooth_radices(size_t span)
  {
    const logic::Radices r = logic::smooth_radices(span);
    RadixList rl; rl.count = r.count;
    for (int i = 0; i < 15; ++i) rl.r[i] = r.r[i];
    return rl;
  }
  size_t self_cells() const { return logic::self_cells(nbins, opt_self >= 1, sizeof(fdx)); }

  // ---- pipelined calls ------------------------------------------------------------------------------------------
  // Asynchronous analysis calls on the plan's own stream: consecutive calls' row kernels do not wait for each other.  What
  // ties call k + 1 to call k is the plan's state; self_state_kernel computes it from the call's samples ahead of the rows
  // (main stream: a chain of small kernels), the rows go to two streams in turn, each waiting for the state it reads only.
  // The next call's workgroups take the CUs as the previous call's leave them: launch gap, prologue (fold + FFT, no HBM
  // traffic) and the ragged end of a call are covered by the neighbour's stores.  State slots form a ring of four: the
  // state kernel of call k + 3 overwrites what the rows of call k read, and waits for them.
  // Anything else that touches the plan joins first (the main stream waits for the outstanding rows).  Off once the host has
  // asked for the stream (sdft_hip_get_stream: it may queue work of its own behind a call), with profiling, on a caller's stream.
  long opt_pipeline = 1;
  long pipe_stream_kind = 0, pipe_stream_attempts = 0;        // 1 = ordinary streams, 2 = by priority (0: none found, one stream)
  std::vector<hipStream_t> spare_streams;
  bool stream_exposed = false;
  hipStream_t row_streams[2] = {nullptr, nullptr};
  hipEvent_t ev_pre = nullptr, ev_rows[4] = {nullptr, nullptr, nullptr, nullptr};
  unsigned long long pipe_calls = 0, pipe_ordered = 0;
  // what the outstanding row launches write and which row stream each went to: a call whose matrix or samples overlap one of
  // them is ordered behind it, as one stream would have it (logic::RowRing decides, this class waits and records)
  logic::RowRing ring;
  logic::Range prev_out;                                     // the matrix of the previous analysis call (dense, row-group kernel)
  bool pipe_this = false;                                    // forward_launch: this call is pipelined (logic::ForwardRoute::pipelined)
  // Only calls whose every pointer is the caller's DEVICE memory may leave the plan's stream: the host-pointer routes reuse
  // the plan's staging buffers (d_stage_*, d_io, d_pin) on the main stream right behind a launch and promise the outputs
  // complete on return.  Set by the device/device branches of sdft_n / isdft_n for the duration of the call.
  bool pipe_allowed = false;
  bool ensure_pipe()
  {
    if (ev_pre) return true;
    // The two row streams must not share a hardware queue with each other or with the main stream: kernels of one queue
    // run one after the other, and the waits between the streams then only cost (the bench process measured 180 us per
    // pipelined call at n = 48 000 where a fresh process measured 128-140; the runtime deals its few hardware queues out
    // by its own rules).  So the streams are tried: a 200 us wave on each of the three at once (queue_probe_kernel), timed
    // by events -- they must have run at the same time.  Up to three pairs of ordinary streams, then one stream above and
    // one below the plan's priority (separate queue pools; 3-4 % slower than a good ordinary pair, the lower-priority
    // launch falls behind), else the plan stays on one stream.  Once per plan, a quarter of a millisecond per pair tried.
    {
      // (nothing in here is an error of the call: a plan that cannot have its streams stays on one stream)
      hipEvent_t ev[6] = {};
      auto release_events = [&]() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); };
      auto give_up = [&]() { (void)hipGetLastError(); release_events(); opt_pipeline = 0; pipe_stream_kind = 0; return false; };
      if (hipStreamSynchronize(stream) != hipSuccess) return give_up();
      for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) { e = nullptr; return give_up(); }
      auto concurrent = [&](hipStream_t a, hipStream_t b) -> int {
        hipStream_t st[3] = {stream, a, b};
        for (int i = 0; i < 3; ++i)
        {
          if (hipEventRecord(ev[2 * i], st[i]) != hipSuccess) return -1;
          hipLaunchKernelGGL((queue_probe_kernel<FD>), dim3(1), dim3(kWave), 0, st[i], 20000ull);
          if (hipEventRecord(ev[2 * i + 1], st[i]) != hipSuccess) return -1;
        }
        for (int i = 0; i < 3; ++i) if (hipStreamSynchronize(st[i]) != hipSuccess) return -1;
        // three waves of 200 us: from any start to any end less than two of them
        float span_ms = 0.f, worst = 0.f;
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j)
          {
            if (hipEventElapsedTime(&span_ms, ev[2 * i], ev[2 * j + 1]) != hipSuccess) return -1;
            worst = std::max(worst, span_ms);
          }
        return worst < 0.35f ? 1 : 0;
      };
      bool found = false;
      int lo = 0, hi = 0;                                     // (numerically: greatest = lowest priority)
      if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
      for (int attempt = 0; attempt < 4 && !found; ++attempt)
      {
        hipStream_t cand[2] = {nullptr, nullptr};
        const bool by_priority = attempt == 3;
        if (by_priority && lo == hi) break;
        for (int i = 0; i < 2; ++i)
        {
          // (blocking streams, like the plan's own: a host that reads its results with a plain hipMemcpy relies on the null
          // stream waiting for the plan's work, and that has to include the rows)
          const hipError_t e = by_priority ? hipStreamCreateWithPriority(&cand[i], hipStreamDefault, i == 0 ? hi : lo)
                                           : hipStreamCreateWithFlags(&cand[i], hipStreamDefault);
          if (e != hipSuccess) { if (cand[0]) (void)hipStreamDestroy(cand[0]); for (hipStream_t sp : spare_streams) (void)hipStreamDestroy(sp); spare_streams.clear(); return give_up(); }
        }
        const int ok = concurrent(cand[0], cand[1]);
        if (ok == 1) { row_streams[0] = cand[0]; row_streams[1] = cand[1]; found = true; pipe_stream_kind = by_priority ? 2 : 1; pipe_stream_attempts = attempt + 1; }
        else
        {
          (void)hipGetLastError();
          // (kept alive until the search is over: a destroyed stream's queue would be handed to the next candidate)
          spare_streams.push_back(cand[0]); spare_streams.push_back(cand[1]);
        }
      }
      for (hipStream_t sp : spare_streams) (void)hipStreamDestroy(sp);
      spare_streams.clear();
      if (!found) return give_up();
      release_events();
    }
    bool ok = hipEventCreateWithFlags(&ev_pre, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 4 && ok; ++i) ok = hipEventCreateWithFlags(&ev_rows[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i) ok = hipEventCreateWithFlags(&ev_inv[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) { release_pipe(); opt_pipeline = 0; pipe_stream_kind = 0; return false; }
    return true;
  }
  // Synthesis calls are stateless: consecutive asynchronous ones (a host that synthesises matrix after matrix) go to the two
  // row streams in turn as well -- n = 48 000: 148 -> 122 us per call, 66 -> 80 % of peak; n = 262 144: 82 -> 86 %
  // (two plans in turn, scripts/pair_overlap_probe.py ...) -- but never beside an analysis: a synthesis waits for the
  // rows of the analyses before it, an analysis for the syntheses before it (reads mixed into the write stream cost HBM
  // more than the overlap gains: 1.62 against 1.47 ms per pair at n = 262 144).
  // Only for hosts that do synthesise call after call: a host that alternates analysis and synthesis (the reference's loop)
  // would pay an event wait between streams per call and gain nothing, so the mode is learnt from the calls themselves --
  // on when a synthesis follows a synthesis, off when an analysis follows a lone synthesis.
  logic::CallPattern calls;                                   // ... learnt from the calls (the same for analyses)
  hipEvent_t ev_inv[2] = {nullptr, nullptr};                 // the last synthesis launch on each row stream
  logic::InverseStreams inv;
  unsigned long long inv_calls = 0;
  long last_inverse_pipelined = 0;
  bool pipe_join_inverses()
  {
    for (int i = 0; i < 2; ++i)
      if (inv.used[i]) { SDFT_TRY(hipStreamWaitEvent(stream, ev_inv[i], 0)); inv.used[i] = false; }
    return true;
  }
  bool pipe_join() { return pipe_join_rows() && pipe_join_inverses(); }
  bool pipe_join_rows()
  {
    if (!ring.open) return true;
    // the last launch on each row stream (among the four the ring remembers; older ones are ordered before them)
    int slots[2];
    const int count = ring.last_per_stream(slots);
    for (int i = 0; i < count; ++i) SDFT_TRY(hipStreamWaitEvent(stream, ev_rows[slots[i]], 0));
    ring.joined();
    return true;
  }
  void release_pipe()
  {
    for (int i = 0; i < 2; ++i) if (row_streams[i]) { (void)hipStreamSynchronize(row_streams[i]); (void)hipStreamDestroy(row_streams[i]); row_streams[i] = nullptr; }
    if (ev_pre) { (void)hipEventDestroy(ev_pre); ev_pre = nullptr; }
    for (int i = 0; i < 4; ++i) if (ev_rows[i]) { (void)hipEventDestroy(ev_rows[i]); ev_rows[i] = nullptr; }
    for (int i = 0; i < 2; ++i) { if (ev_inv[i]) { (void)hipEventDestroy(ev_inv[i]); ev_inv[i] = nullptr; } inv.used[i] = false; }
    ring.joined();
    (void)hipGetLastError();
  }
  bool pipe_wanted(const void* fuse) const
  {
    return !fuse && pipe_allowed && async && own_stream && !stream_exposed && opt_pipeline && profile == 0 && sizeof(FD) == 8;
  }
  bool launch_self_state(const ForwardArgs<FD>& fa, const SelfArgs<TD, FD>& sa, unsigned threads)
  {
    auto kern = self_state_kernel<TD, FD>;
    const size_t lds = self_cells() * sizeof(fdx);
    static thread_local int raised_on = -1;
    if (raised_on != device)
    {
      SDFT_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(96 * 1024)));
      raised_on = device;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)channels), dim3(threads), lds, stream, fa, sa);
    SDFT_TRY(hipGetLastError());
    return true;
  }

  // ---- self-carried chunks: the whole chunk-parallel call in one launch (SelfArgs in sdft_kernels.hpp) ----
  // prefix: the folded cells of every chunk come from one pre-pass launch (prefix_cells_kernel, logic::ForwardRoute::prefix);
  // one stream, never fused
  bool forward_self(size_t n, const TD* x, size_t x_stride, fdx* out, size_t out_stride, long chunks, long len,
                    const ForwardCall& c, bool prefix = false)
  {
    const FuseArgs<TD, FD>* const fuse = c.fuse;             // (the plain analysis or the fused call: no other kind has the form)
    const size_t nb = nbins, span = 2 * nbins;
    SelfArgs<TD, FD> sa;
    sa.x = x; sa.x_stride = x_stride;
    sa.hist_in = d_hist[hist_cur].p; sa.hist_out = d_hist[hist_cur ^ 1].p;
    sa.acc_in = d_accs[st_cur].p;
    sa.log2m = 0; sa.rl.count = 0;
    if ((span & (span - 1)) == 0) while (((size_t)1 << sa.log2m) < span) ++sa.log2m;
    else sa.rl = smooth_radices(span);
    sa.lds_deltas = 0;
    sa.prefix = nullptr;
#ifdef SDFT_SELF_STAMPS
    sa.stamps = reinterpret_cast<unsigned long long*>(opt_self_stamps);
#endif
    ForwardArgs<FD> fa{};
    fa.delta = nullptr; fa.tw = d_tw.p; fa.wtab = d_wtab.p; fa.carry = nullptr; fa.seed = nullptr; fa.fseed = nullptr; fa.fseed_L = 0;
    fa.out = out; fa.out_stride = out_stride; fa.out_rows = nullptr;
    fa.acc_state = d_accs[st_cur ^ 1].p; fa.fid_state = d_fids[st_cur ^ 1].p; fa.n = n;
    fa.total_waves = 0;
    fa.nbins = (unsigned)nb; fa.chunks = (unsigned)chunks; fa.chunk_len = (unsigned)len; fa.tiles = (unsigned)tiles();
    fa.interior_lanes = (unsigned)interior_lanes(); fa.cursor0 = (unsigned)cursor; fa.chunk_shift = 0;
    fa.chunk0 = 0; fa.launch_chunks = (unsigned)chunks; fa.inv_chunks = inv32(fa.launch_chunks);
    fa.xcd_map = logic::xcd_groups(opt_xcd_map != 0, channels * (size_t)chunks);
    fa.vec_store = 0;
    fa.wscale = (window == WIN_HANN) ? (FD)(tab.aweight * (FD)(0.25)) : tab.aweight;   // :371
    fa.done.flag = nullptr; fa.done.count = nullptr; fa.done.seq = 0; fa.done.total = 0;
    if (!grid_fits(channels * (size_t)chunks)) return false;
    if (channels * n * nb <= (fuse ? logic::kFlagMaxFused : logic::kFlagMax)) fa.done = arm_flag((unsigned)(channels * (size_t)chunks));
    const unsigned blocks = (unsigned)(channels * (size_t)chunks);
    const bool fused = opt_fused != 0;
    last_fused = fused; last_segments = 1; last_chain = 0;
    last_pipelined = 0;
    if constexpr (sizeof(FD) == 8)
    {
      // A host that writes call after call into ONE matrix gains nothing from two streams and would pay for the order
      // between them (an event wait across streams, satisfied or not, costs the row kernels 5-15 us per call: n = 48 000,
      // 165-171 against 157 us): a call whose matrix overlaps the previous call's takes the one-stream form.  A host that
      // alternates between two matrices is pipelined, each matrix on its own stream.
      const uintptr_t olo = reinterpret_cast<uintptr_t>(out), ohi = olo + ((channels - 1) * out_stride + n * nb) * sizeof(fdx);
      if (pipe_this && !fuse && ensure_pipe())
      {
        if (!pipe_join_inverses()) return false;             // never beside a synthesis
        const uintptr_t xlo = reinterpret_cast<uintptr_t>(x), xhi = xlo + ((channels - 1) * x_stride + n) * sizeof(TD);
        // samples that an outstanding launch is still writing (a matrix reinterpreted as samples): no overlap for this call
        if (ring.samples_overlap(xlo, xhi) && !pipe_join()) return false;
        const int s1 = (st_cur + 1) & 3, h1 = (hist_cur + 1) & 3;
        // Which row stream: the other one than the previous launch's -- unless this call's matrix overlaps what an
        // outstanding launch writes (a host that reuses one matrix): then the stream of the latest such launch, whose order
        // costs nothing (an event wait across streams costs ~15 us per call: n = 48 000 into one matrix 171 against 157 us)
        const logic::RowRing::Pick pk = ring.pick(olo, ohi);
        const int rsi = pk.stream;
        hipStream_t rs = row_streams[rsi];
        // the rows read the state everything queued on the main stream so far leaves behind
        SDFT_TRY(hipEventRecord(ev_pre, stream));
        SDFT_TRY(hipStreamWaitEvent(rs, ev_pre, 0));
        if (pk.behind)
        {
          ++pipe_ordered;
          if (pk.wait_launch >= 0) SDFT_TRY(hipStreamWaitEvent(rs, ev_rows[pk.wait_launch], 0));   // (overlapping launches on the other stream as well: the latest of them)
        }
        // the slot the state kernel writes was read by the rows of three calls ago
        if (ring.state_reader() >= 0) SDFT_TRY(hipStreamWaitEvent(stream, ev_rows[ring.state_reader()], 0));
        ForwardArgs<FD> fs = fa; SelfArgs<TD, FD> ss = sa;
        fs.acc_state = d_accs[s1].p; fs.fid_state = d_fids[s1].p; ss.hist_out = d_hist[h1].p;
        fs.done.flag = nullptr; fs.done.count = nullptr; fs.done.seq = 0; fs.done.total = 0;
        if (!launch_self_state(fs, ss, (unsigned)(row_waves() * kWave))) return false;
        ForwardArgs<FD> fr = fa; SelfArgs<TD, FD> sr = sa;
        fr.acc_state = nullptr; fr.fid_state = nullptr; sr.hist_out = nullptr;
        fr.done.flag = nullptr; fr.done.count = nullptr; fr.done.seq = 0; fr.done.total = 0;
        {
          Scoped<hipStream_t> on(stream, rs);
          if (!launch_forward_rows_self(fr, sr, blocks, (unsigned)(row_waves() * kWave), fused)) return false;
        }
        SDFT_TRY(hipEventRecord(ev_rows[ring.slot()], rs));
        ring.launched(olo, ohi, rsi);
        ++pipe_calls;
        last_pipelined = 1;
        st_cur = s1; hist_cur = h1;
        fid_canonical = false;                               // the rotation comes from the closed-form table (as the one-stream self form below)
        cursor = (cursor + n) % span;
        return true;
      }
    }
    if (!pipe_join()) return false;
    if constexpr (sizeof(FD) == 8)
    {
      if (prefix)
      {
        if (!d_prefix.reserve(channels * (size_t)chunks * span)) return false;
        PrefixArgs<TD, FD> pa;
        pa.x = x; pa.x_stride = x_stride; pa.hist_in = sa.hist_in; pa.prefix = d_prefix.p; pa.n = n;
        pa.span = (unsigned)span; pa.chunks = (unsigned)chunks; pa.chunk_len = (unsigned)len; pa.cursor0 = (unsigned)cursor;
        const size_t pblocks = ((span + kPrefixCells - 1) / kPrefixCells) * channels;
        if (!grid_fits(pblocks)) return false;
        if (!prof_begin(ST_CARRY)) return false;
        hipLaunchKernelGGL((prefix_cells_kernel<TD, FD>), dim3((unsigned)pblocks), dim3(kPrefixCells * kPrefixSlices), 0, stream, pa);
        SDFT_TRY(hipGetLastError());
        if (!prof_end(ST_CARRY)) return false;
        sa.prefix = d_prefix.p;
      }
    }
    if (!prof_begin(ST_FORWARD)) return false;
    if constexpr (sizeof(FD) == 8)
    {
      if (fuse)
      {
        last_fused_exact = 0; last_fused_fold = 1;
        if (!launch_process(fa, *fuse, blocks, fused, &sa)) return false;
      }
      else if (!launch_forward_rows_self(fa, sa, blocks, (unsigned)(row_waves() * kWave), fused)) return false;
    }
    SDFT_TRY(hipGetLastError());
    if (!prof_end(ST_FORWARD)) return false;
    hist_cur ^= 1; st_cur ^= 1;
    fid_canonical = false;                                   // chunks seeded fid from the closed-form table
    cursor = (cursor + n) % span;
    return true;
  }
  // ---- single-chunk calls (hop-wise streaming): one fused launch, tiles spread over the CUs ----
  bool forward_hop(size_t n, const TD* x, size_t x_stride, fdx* out, size_t out_stride, fdx* const* rows)
  {
    const size_t nb = nbins, span = 2 * nbins;
    const long ntiles = tiles(), inter = interior_lanes();
    HopArgs<TD, FD> ha;
    ha.x = x; ha.x_stride = x_stride;
    ha.hist_in = d_hist[hist_cur].p; ha.hist_out = d_hist[hist_cur ^ 1].p;
    ha.tw = d_tw.p;
    ha.acc_in = d_accs[st_cur].p; ha.fid_in = d_fids[st_cur].p;
    ha.acc_out = d_accs[st_cur ^ 1].p; ha.fid_out = d_fids[st_cur ^ 1].p;
    ha.out = out; ha.out_stride = out_stride; ha.out_rows = rows; ha.n = n;
    ha.total_waves = (unsigned long long)channels * (unsigned long long)ntiles;
    ha.nbins = (unsigned)nb; ha.tiles = (unsigned)ntiles; ha.interior_lanes = (unsigned)inter; ha.cursor0 = (unsigned)cursor;
    ha.vec_store = (bins_per_lane() == 2 && (nb % 2 == 0) && ((uintptr_t)out % 16 == 0) && (out_stride % 2 == 0) && !rows) ? 1 : 0;
    ha.wscale = (window == WIN_HANN) ? (FD)(tab.aweight * (FD)(0.25)) : tab.aweight;   // :371
    // one wave per workgroup while the launch is small (the tiles of a row land on different CUs);
    // four per workgroup once there are more waves than SIMDs anyway
    const bool wide = ha.total_waves > 2048;
    const unsigned long long blocks = wide ? (ha.total_waves + 3) / 4 : ha.total_waves;
    if (!grid_fits(blocks)) return false;
    // small launches of hop-sized calls: two waves per tile (recurrence | window + stores)
    const bool pipe = !wide && n <= (size_t)kHopMax;       // small launches: two waves per tile (forward_hop2_kernel)
    last_hop_pipe = pipe;
    // ... and the call's samples in time parts, every (tile, part) a workgroup on a CU of its own (forward_hop2_kernel): as many
    // parts as leave every workgroup a CU, at most 8, at least 12 samples each (the recurrence wave of a part runs the state
    // through the samples before it: what a part saves is the window, the demodulation and the stores of those samples)
    ha.parts = 1; ha.part_len = (unsigned)n;
    if (pipe)
    {
      const logic::HopParts hp = logic::hop_parts(n, ha.total_waves, compute_units, opt_hop_parts, flag_wanted && !async);
      ha.parts = hp.parts; ha.part_len = hp.part_len;
    }
    last_hop_parts = ha.parts;
    const unsigned hop2_blocks = (unsigned)blocks * ha.parts;
    ha.done = arm_flag(wide ? 0u : (pipe ? hop2_blocks : (unsigned)blocks));     // every workgroup reports
    ha.stamps = nullptr;
#ifdef SDFT_HOP_STAMPS
    if (d_partial.reserve(64)) { ha.stamps = reinterpret_cast<unsigned long long*>(d_partial.p); last_partial_elems = 0; hop2_stamps = true; }
#endif
    if (!prof_begin(ST_FORWARD)) return false;
    if (pipe) { if (rows) launch_hop2_t<true>(ha, hop2_blocks); else launch_hop2_t<false>(ha, hop2_blocks); }
    else if (rows) { if (wide) launch_hop_t<true, 4>(ha, (unsigned)blocks); else launch_hop_t<true, 1>(ha, (unsigned)blocks); }
    else      { if (wide) launch_hop_t<false, 4>(ha, (unsigned)blocks); else launch_hop_t<false, 1>(ha, (unsigned)blocks); }
    SDFT_TRY(hipGetLastError());
    if (!prof_end(ST_FORWARD)) return false;
    hist_cur ^= 1; st_cur ^= 1;
    last_kernel = 3;
    if (cursor + n >= span) fid_canonical = true;
    cursor = (cursor + n) % span;
    return true;
  }

  // fused call, one time chunk, folded form: one launch (process_hop2_kernel); the caller has folded the coefficients
  DevBuf<double> d_partial;
  DevBuf<unsigned> d_tickets;
  // completion word in pinned host memory: the kernels of short synchronous calls set it (signal_done), finish()
  // polls it.  flag_wanted: the public entry point has device pointers on both sides and will end in finish();
  // flag_pending: the call's LAST launch was armed (every entry point starts with both false, see bind()).
  unsigned* h_done_flag = nullptr;
  unsigned* d_done_flag = nullptr;
  DevBuf<unsigned> d_done_count;
  // fused call in the reference's order with float samples: samples whose sum was walked bin by bin (the others were
  // proven by the rounding interval of the tree sum: forward_rows_kernel<SYN = 2>); get_option "ordered_walks"
  DevBuf<unsigned> d_walked;
  unsigned* walked_counter()
  {
    if (!d_walked.p)
    {
      if (!d_walked.reserve(1)) { (void)hipGetLastError(); return nullptr; }
      if (hipMemsetAsync(d_walked.p, 0, sizeof(unsigned), stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    }
    return d_walked.p;
  }
  long ordered_walks() const
  {
    if (!d_walked.p) return 0;
    unsigned v = 0;
    if (hipStreamSynchronize(stream) != hipSuccess || hipMemcpy(&v, d_walked.p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (long)v;
  }
  unsigned flag_seq = 0;
  bool flag_pending = false, flag_wanted = false;
  bool ensure_flag()
  {
    if (h_done_flag) return true;
    if (!d_done_count.reserve(2)) return false;
    if (hipMemsetAsync(d_done_count.p, 0, 2 * sizeof(unsigned), stream) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipHostMalloc((void**)&h_done_flag, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); h_done_flag = nullptr; return false; }
    *h_done_flag = 0;
    if (hipHostGetDevicePointer((void**)&d_done_flag, h_done_flag, 0) != hipSuccess)
    {
      (void)hipGetLastError(); (void)hipHostFree(h_done_flag); h_done_flag = nullptr; return false;
    }
    return true;
  }
  DoneSignal arm_flag(unsigned total)
  {
    DoneSignal d; d.flag = nullptr; d.count = nullptr; d.seq = 0; d.total = total;
    flag_pending = false;
    if (flag_wanted && !async && !profile && opt_spin && total > 0 && ensure_flag())
    {
      d.flag = d_done_flag; d.count = d_done_count.p; d.seq = ++flag_seq;
      flag_pending = true;
    }
    return d;
  }
  bool process_hop(size_t n, const TD* x, size_t x_stride, TD* y, size_t y_stride)
  {
    const size_t nb = nbins, span = 2 * nbins;
    const size_t ptiles = (nb + kWave - 1) / kWave;
    if (!grid_fits(channels * ptiles)) return false;
    if (!d_partial.reserve(channels * ptiles * n + 8)) return false;     // + stamps of the development build
    last_partial_elems = channels * ptiles * n;
    if (d_tickets.cap < channels)
    {
      if (!d_tickets.reserve(channels)) return false;
      SDFT_TRY(hipMemsetAsync(d_tickets.p, 0, channels * sizeof(unsigned), stream));
    }
    ProcHopArgs<TD, FD> pa;
    pa.x = x; pa.x_stride = x_stride; pa.y = y; pa.y_stride = y_stride;
    pa.hist_in = d_hist[hist_cur].p; pa.hist_out = d_hist[hist_cur ^ 1].p;
    pa.tw = d_tw.p;
    pa.acc_in = d_accs[st_cur].p; pa.fid_in = d_fids[st_cur].p;
    pa.acc_out = d_accs[st_cur ^ 1].p; pa.fid_out = d_fids[st_cur ^ 1].p;
    pa.alpha = d_alpha.p; pa.beta = d_beta.p; pa.partial = d_partial.p; pa.tickets = d_tickets.p;
    pa.n = n; pa.nbins = (unsigned)nb; pa.tiles = (unsigned)ptiles; pa.cursor0 = (unsigned)cursor; pa.sweight = tab.sweight;
    pa.done = arm_flag((unsigned)channels);                  // every channel's last workgroup reports
    if (!prof_begin(ST_FORWARD)) return false;
    // two waves per tile (recurrence | coefficients + sums)
    if (!coeff_has_beta) hipLaunchKernelGGL((process_hop2_kernel<TD, FD, false>), dim3((unsigned)(channels * ptiles)), dim3(2 * kWave), 0, stream, pa);
    else                 hipLaunchKernelGGL((process_hop2_kernel<TD, FD, true>), dim3((unsigned)(channels * ptiles)), dim3(2 * kWave), 0, stream, pa);
    last_hop_pipe = 1;
    SDFT_TRY(hipGetLastError());
    if (!prof_end(ST_FORWARD)) return false;
    hist_cur ^= 1; st_cur ^= 1;
    last_kernel = 3; last_chunks = 1; last_chunk_len = (long)n; last_segments = 1; last_fused = 0;
    last_fused_exact = 0; last_fused_fold = 1;
    if (cursor + n >= span) fid_canonical = true;
    cursor = (cursor + n) % span;
    return true;
  }

  // folded form of the fused call (process_rows_kernel): per-bin coefficients from the plan's window and
  // synthesis tables and the call's operation, then one launch per overlap segment
  DevBuf<double> d_alpha, d_beta;
  bool coeff_ready = false, coeff_has_beta = false;
  unsigned coeff_rows = 1;
  int coeff_kind = -1; long coeff_shift = 0;
  bool fold_coefficients(const SpectralOp<FD>& op)
  {
    coeff_ready = false;
    if (!opt_fold || nbins < 8) return true;
    // identity and shift depend on the plan only: folded once; a gain array may change between calls
    if (!op_is_linear<FD>(op.kind)) return true;                                   // gate, power: the windowed rows are needed
    const bool has_array = op.kind == OP_GAIN || op.kind == OP_CGAIN;
    const unsigned rows = has_array && op.rows > 1 ? op.rows : 1u;
    if (rows > 65535u) return true;                                                // (grid.y) -- more gain vectors than that: two passes
    coeff_has_beta = !(latency == 1) || op.kind == OP_CGAIN;                     // im X enters through the synthesis twiddle or a complex gain
    coeff_rows = rows;
    if (!has_array && coeff_kind == op.kind && coeff_shift == op.shift && d_alpha.p) { coeff_ready = true; return true; }
    if (!d_alpha.reserve((size_t)rows * nbins) || !d_beta.reserve((size_t)rows * nbins)) return false;
    const FD w = (window == WIN_HANN) ? (FD)(tab.aweight * (FD)(0.25)) : tab.aweight;   // as ForwardArgs::wscale
    FD h0 = w, h1 = (FD)0, h2 = (FD)0;                                                   // taps of window_tap()
    if (window == WIN_HANN) { h0 = w + w; h1 = -w; }
    else if (window == WIN_HAMMING) { h0 = (FD)(0.54) * w; h1 = -((FD)(0.23) * w); }
    else if (window == WIN_BLACKMAN) { h0 = (FD)(0.42) * w; h1 = -((FD)(0.25) * w); h2 = (FD)(0.04) * w; }
    hipLaunchKernelGGL((fold_coeff_kernel<FD>), dim3((unsigned)((nbins + kBlock - 1) / kBlock), rows), dim3(kBlock), 0, stream,
                       d_alpha.p, d_beta.p, op, (const fdx*)d_syn.p, (unsigned)nbins, latency == 1 ? 1 : 0, h0, h1, h2);
    SDFT_TRY(hipGetLastError());
    coeff_kind = op.kind; coeff_shift = op.shift;
    coeff_ready = true;
    return true;
  }
  // ---- the kernel launches: run-time values -> template instantiations -------------------------------------------------
#include "sdft_plan_launch.inc"
#include "sdft_plan_resident.inc"

  // ---- inverse on device-resident buffers --------------------------------------------------
  bool inverse_device(size_t n, const fdx* in, size_t in_stride, const fdx* const* rows, TD* y, size_t y_stride,
                      const SpectralOp<FD>* op = nullptr)
  {
    if (n == 0) return true;
    SDFT_TRY(hipSetDevice(device));
    const bool ops_wanted = op && op->kind != OP_IDENTITY;
    last_inverse_pipelined = 0;
    // (whatever FD is: the synthesis has no state to carry from call to call)
    inv_after_write = calls.prev_was_analysis;
    calls.on_synthesis_begin();
    const bool inv_pipe = calls.inverse_batch && pipe_allowed && !rows && !ops_wanted && async && own_stream && !stream_exposed && opt_pipeline && profile == 0 &&
                          channels * n * nbins >= logic::kPipelineBinsMin && ensure_pipe();
    if (!(inv_pipe ? pipe_join_rows() : pipe_join())) return false;
    int si = 0;
    uintptr_t ylo = 0, yhi = 0;
    if (inv_pipe)
    {
      // the other stream than the previous synthesis -- the same one if the two write overlapping samples
      ylo = reinterpret_cast<uintptr_t>(y); yhi = ylo + ((channels - 1) * y_stride + n) * sizeof(TD);
      const uintptr_t ilo = reinterpret_cast<uintptr_t>(in), ihi = ilo + ((channels - 1) * in_stride + n * nbins) * sizeof(fdx);
      const logic::InverseStreams::Pick pk = inv.pick(logic::Range{ylo, yhi}, logic::Range{ilo, ihi});
      si = pk.stream;
      SDFT_TRY(hipEventRecord(ev_pre, stream));               // behind everything the main stream has been given (the joins above too)
      SDFT_TRY(hipStreamWaitEvent(row_streams[si], ev_pre, 0));
      // what the OTHER row stream still has outstanding: samples this call overwrites (a host that rotates three sample
      // buffers) or a matrix that was reinterpreted from them -- ordered behind it
      if (pk.wait_other) SDFT_TRY(hipStreamWaitEvent(row_streams[si], ev_inv[si ^ 1], 0));
    }
    Scoped<hipStream_t> on(stream, inv_pipe ? row_streams[si] : stream);
    if (!prof_begin(ST_INVERSE)) return false;
    InverseArgs<TD, FD> ia;
    ia.in = in; ia.in_stride = in_stride; ia.in_rows = rows; ia.syn = d_syn.p; ia.y = y; ia.y_stride = y_stride;
    ia.n = n; ia.nbins = (unsigned)nbins; ia.channels = (unsigned)channels; ia.sweight = tab.sweight;
    ia.op = SpectralOp<FD>{}; ia.op.kind = OP_IDENTITY; ia.op.rows = 1;
    ia.done.flag = nullptr; ia.done.count = nullptr; ia.done.seq = 0; ia.done.total = 0;
    {
      const size_t matrix_bytes = channels * n * nbins * sizeof(fdx);
      ia.nt = (int)logic::inverse_streaming_loads(matrix_bytes, opt_inverse_nt);
      ia.nt_skip = logic::inverse_ordinary_rows(matrix_bytes, nbins * sizeof(fdx), opt_inverse_nt_skip_mb);
    }
    const bool ops = op && op->kind != OP_IDENTITY;
    if (ops) ia.op = *op;
    const size_t total_rows = channels * n;
    const bool lat1 = (latency == 1);                                            // :639 exact compare
    if (ops) { if (lat1) launch_inverse<true, true>(ia, total_rows); else launch_inverse<false, true>(ia, total_rows); }
    else     { if (lat1) launch_inverse<true, false>(ia, total_rows); else launch_inverse<false, false>(ia, total_rows); }
    SDFT_TRY(hipGetLastError());
    if (rtc_failed) { rtc_failed = false; return false; }    // (the compiler's words are in the error channel already)
    if (!prof_end(ST_INVERSE)) return false;
    calls.on_synthesis_launched();
    if (inv_pipe)
    {
      SDFT_TRY(hipEventRecord(ev_inv[si], stream));
      inv.launched(si, logic::Range{ylo, yhi});
      ++inv_calls; last_inverse_pipelined = 1;
    }
    return true;
  }

  // synchronous calls: short ones poll the stream (a sleeping hipStreamSynchronize wakes up late --
  // tens of microseconds, more than a whole 100-sample hop takes on the device)
  size_t last_partial_elems = 0;
  bool hop2_stamps = false;
  bool chain_stats(unsigned long long* out32)
  {
#ifdef SDFT_HOP_STAMPS
    // development build: realtime stamps (100 MHz) of forward_hop2_kernel's workgroup 0 (recurrence wave: 0..2, window wave: 4..6)
    if (hop2_stamps && d_partial.p)
    {
      memset(out32, 0, 32 * sizeof(unsigned long long));
      SDFT_TRY(hipStreamSynchronize(stream));
      SDFT_TRY(hipMemcpy(out32, d_partial.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      hop2_stamps = false;
      return true;
    }
#endif
    if (!d_chain_stats.p) return false;
    SDFT_TRY(hipMemcpy(out32, d_chain_stats.p, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return true;
  }
  // development aid: the relay form's stamps (option chain_debug bit 7), 3 per turn of workgroup 0
  bool relay_stamps(unsigned long long* out, size_t count)
  {
    if (!d_chain_stats.p || d_chain_stats.cap < 64 + count) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (aux) SDFT_TRY(hipStreamSynchronize(aux));
    SDFT_TRY(hipMemcpy(out, d_chain_stats.p + 64, count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return true;
  }

  // Synchronous calls do not sleep on the stream (a sleeping hipStreamSynchronize wakes up tens of microseconds late):
  // they poll -- the completion word where the call's last kernel sets one, the stream otherwise -- for a bounded
  // wall-clock time (logic::sync_wait: min(20 ms, 200 us + 4 x what the call's bytes take at HBM speed); 50 ms for the word) and only then
  // block.  flag_fallbacks counts completion words that never became visible (get_option "flag_fallbacks").
  long flag_fallbacks = 0;
  static inline void cpu_relax()
  {
#if defined(__SSE2__)
    _mm_pause();
#endif
  }
  // hbm_bytes: what the call has to move through HBM at least (0: unknown -- sleep on the stream)
  size_t matrix_bytes(size_t n) const { return channels * n * nbins * sizeof(fdx); }
  bool finish(size_t hbm_bytes = 0)
  {
    if (async) return true;
    using clock = std::chrono::steady_clock;
    if (flag_pending)
    {
      // the kernel's completion word: visible ~6 us before the stream reports the kernel done
      flag_pending = false;
      volatile unsigned* f = h_done_flag;
      const clock::time_point t0 = clock::now();
      for (unsigned spins = 1;; ++spins)
      {
        if (*f == flag_seq)
        {
          // (the word says nothing about faults; a query of the stream here costs 5 us per hop -- measured 35 -> 46 us
          // for the two reference calls -- so a fault surfaces at the next call that touches the stream, as it does
          // for asynchronous calls)
          const hipError_t e = hipPeekAtLastError();
          if (e != hipSuccess) { set_error("completion word", hipGetErrorString(e)); (void)hipGetLastError(); return false; }
          return true;
        }
        if ((spins & 1023u) == 0 && clock::now() - t0 > std::chrono::milliseconds(50)) break;
      }
      ++flag_fallbacks;
      return synchronize();                                  // never seen: fall back to the stream
    }
    // The wait is the same on every box and never sleeps on the stream while the call can still be running: a sleeping
    // hipStreamSynchronize wakes up 9 us late on one box and 45 us late on another (round 4 slept for calls beyond 60 us and
    // lost 10 % of the north star's synchronous rate on the box it was not tuned on; profiles/r05_sync_completion.txt).  A call
    // cannot end before its bytes have moved at the chip's peak rate (logic::kPeakBytesPerUs -- the spec figure, a LOWER bound of the
    // time, not a tuned one): until then the host spins on its own clock without touching the runtime (queries that cannot
    // succeed yet only compete with the completion signal's handler for the runtime's locks), then it polls the stream.
    // Option "spin": 0 = sleep on the stream, 1 = this (default), 2 = poll from the start.
    if (opt_spin && hbm_bytes)
    {
      const logic::SyncWait w = logic::sync_wait(hbm_bytes);
      const clock::time_point t0 = clock::now();
      if (opt_spin == 1 && w.quiet_us > 0)
      {
        // (counted from the entry point's start: a call that has waited for its kernels already -- the exact-carry route
        // checks its poll loops' status word behind a synchronisation -- is not made to wait again)
        const auto quiet = std::chrono::nanoseconds((long long)(w.quiet_us * 1000.0));
        while (clock::now() - call_start < quiet) cpu_relax();
      }
      const auto budget = std::chrono::microseconds((long long)w.budget_us);
      for (unsigned spins = 1;; ++spins)
      {
        const hipError_t e = hipStreamQuery(stream);
        if (e == hipSuccess) return collect_profile();
        if (e != hipErrorNotReady) { set_error("hipStreamQuery", hipGetErrorString(e)); return false; }
        if ((spins & 15u) == 0 && clock::now() - t0 > budget) break;
      }
      (void)hipGetLastError();
    }
    return synchronize();
  }

  // calls whose kernels read and wrote the caller's host memory in place (map_host): always complete on return, and
  // through the stream's own synchronisation -- the point at which the runtime promises the host sees what the device
  // wrote over PCIe (a stream query that reports "done" first keeps the wait short; the synchronisation then returns at once)
  bool finish_mapped(size_t hbm_bytes)
  {
    Scoped<bool> sync(async, false);
    if (!finish(hbm_bytes)) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    return true;
  }

  // Pointer classification: every call asks the runtime (hipPointerGetAttributes).  Measured on MI355X / ROCm 7
  // (scripts/pointer_query_probe.hip, profiles/r04_pointer_query_cost.txt): 0.06-0.10 us per query for device and pinned
  // memory, 0.16 us for pageable host memory, with 2 or 2000 live allocations -- two orders of magnitude below a launch,
  // so nothing is cached and a buffer that was freed and whose address came back as the other kind of memory (hipMalloc
  // does hand a freed address out again) is classified as what it is now.  Option "pointers" = 1 / 2 declares every
  // pointer device / host memory (no query).
  bool on_device(const void* p)
  {
    if (opt_pointers == 1) return true;
    if (opt_pointers == 2) return false;
    return is_device_pointer(p);
  }

  // ---- the caller's host memory (sdft_host_io.hpp): registered in place, or copied through pinned slots of the plan ----------
  HostIo io;
  void* map_host(const void* p, size_t bytes, bool will_write = false) { return io.map_host(p, bytes, will_write); }
  // Both are complete on return as far as the caller's memory goes: to_device has read it, to_host has written it.
  bool copy_failed() { set_error("host copy", "a copy between host memory and the device through the plan's pinned slots failed"); return false; }
  bool to_device(void* dst, const void* src, size_t bytes)
  {
    if (bytes == 0) return true;
    if (!pipe_join()) return false;                          // (a no-op unless row streams hold outstanding launches)
    return io.to_device(dst, src, bytes, stream) || copy_failed();
  }
  bool to_host(void* dst, const void* src, size_t bytes)
  {
    if (bytes == 0) return true;
    if (!pipe_join()) return false;
    return io.to_host(dst, src, bytes, stream) || copy_failed();
  }

  // one strip per channel (no pitch limits, works for any size); kind says which side is the caller's host memory
  bool copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, hipMemcpyKind kind)
  {
    for (size_t c = 0; c < channels; ++c)
    {
      void* d = (char*)dst + c * dpitch;
      const void* s = (const char*)src + c * spitch;
      if (kind == hipMemcpyHostToDevice) { if (!to_device(d, s, width)) return false; }
      else if (kind == hipMemcpyDeviceToHost) { if (!to_host(d, s, width)) return false; }
      else { if (!pipe_join()) return false; SDFT_TRY(hipMemcpyAsync(d, s, width, kind, stream)); }
    }
    return true;
  }

  // Small host-side sample buffers (a hop of the host's signal, the by-value sample of sdft_sdft, the sample sdft_isdft
  // returns) do not go through the runtime's pageable copy path (5-10 us per copy): they travel through a pinned scratch
  // of the plan (logic::kSmallHostBytes, one direction per call) that the kernels read and write directly over PCIe, and the
  // call completes on the kernel's completion word.  Single-sample calls on a device row: 21.9 -> see profiles/r04_single_sample.txt.
  TD* h_io = nullptr;
  TD* d_io = nullptr;
  bool ensure_io()
  {
    if (h_io) return true;
    if (hipHostMalloc((void**)&h_io, logic::kSmallHostBytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); h_io = nullptr; return false; }
    if (hipHostGetDevicePointer((void**)&d_io, h_io, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(h_io); h_io = nullptr; d_io = nullptr; return false; }
    return true;
  }

  // the entry points of the C-ABI (sdft_n / isdft_n / _nd / single samples / the fused call / state access) and the routes
  // host memory takes through them
#include "sdft_plan_entry.inc"
};

}  // namespace sdfthip
