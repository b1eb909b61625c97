// sdft_plan_logic.hpp -- the host-side DECISIONS of the engine, free of any HIP dependency: launch geometry (lanes, tiles,
// row slots), time chunking, the block length of the exact-carry relay, which calls leave the plan's stream (call pattern,
// row-stream ring, address-range overlap), time parts of a hop, rows per wave of the synthesis, the routes of an analysis call
// (forward_route), a synthesis call (inverse_route), host memory through the entry points (host_route) and the fused call
// (process_route), the wait of a synchronous call, and the slot ring of the host-copy engine.  sdft_plan.hpp (Plan<TD, FD>) builds
// the queries, asks these functions and does the HIP calls (a check that needs one -- an allocation, the occupancy API -- is a
// callable the route asks only where it needs the answer);
// tests/cpp/plan_logic_test.cpp compiles this header alone with g++ -fsanitize=address,undefined (and the ring under
// -fsanitize=thread) in the `-m "not gpu"` suite (sanitizers on the host side).
// Citations are into /root/reference/c/src/sdft/sdft.h.

#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace sdfthip {
namespace logic {

// the kernels' constants this logic is written against (sdft_plan.hpp asserts that they are the kernels')
constexpr int kLanes = 64;              // lanes of a wave (kWave)
constexpr int kRowWaves = 16;           // waves of a row-group workgroup (kRowWavesMax)
constexpr int kRowSlots = 2;            // bins-per-lane slots of the row-group kernel (kRowSlotsMax)
constexpr int kTimeGroup = 8;           // samples per scalar-load burst of the time loops (kGroup)
constexpr int kSumBlockLen = 8;         // samples per block of the direct partial sums (kSumBlock)
constexpr int kHopSamples = 512;        // calls of one time chunk are shorter than this (kHopMax)
constexpr int kWindowHann = 1, kWindowBlackman = 3, kWindowBoxcar = 0;   // sdft.h:127-133

// ---- lanes, tiles, row groups ---------------------------------------------------------------------------------------------
inline int bins_per_lane(size_t fdx_bytes) { return fdx_bytes == 16 ? 1 : 2; }          // every lane stores 16 bytes
inline int halo_bins(int window) { return window == kWindowBlackman ? 2 : (window == kWindowBoxcar ? 0 : 1); }   // :350-402
inline int halo_lanes(int window, size_t fdx_bytes) { const int b = bins_per_lane(fdx_bytes); return (halo_bins(window) + b - 1) / b; }
// Bin-owning lanes of an independent-tile wave: a tile of 8*j lanes starts and ends on 128-byte lines, so no line is shared
// between two waves (n = 1e6, N = 1024, f64: 62 lanes 4.2 TB/s, 60 lanes 5.4, 56 lanes 5.6)
inline long interior_lanes(int window, size_t fdx_bytes, long forced)
{
  const long mx = kLanes - 2 * halo_lanes(window, fdx_bytes);
  const long v = forced > 0 ? std::min(forced, mx) : (mx / 8) * 8;
  return std::max(v, 1L);
}
inline long tiles(size_t nbins, int window, size_t fdx_bytes, long forced_interior)
{
  const long per = interior_lanes(window, fdx_bytes, forced_interior) * bins_per_lane(fdx_bytes);
  return (long)((nbins + (size_t)per - 1) / (size_t)per);
}
inline bool rows_kernel_ok(size_t nbins, size_t fdx_bytes, bool row_pointers, bool enabled, long slots_max)
{
  const size_t per = (size_t)(kLanes * kRowWaves * bins_per_lane(fdx_bytes));
  return enabled && !row_pointers && nbins >= 8 && nbins <= per * (size_t)std::min<long>(kRowSlots, std::max<long>(1, slots_max));
}
inline long row_slots(size_t nbins, size_t fdx_bytes)
{
  const size_t per = (size_t)(kLanes * kRowWaves * bins_per_lane(fdx_bytes));
  return (long)((nbins + per - 1) / per) <= 1 ? 1 : 2;
}
inline long row_waves(size_t nbins, size_t fdx_bytes)
{
  const size_t per = (size_t)(kLanes * bins_per_lane(fdx_bytes)) * (size_t)row_slots(nbins, fdx_bytes);
  return (long)((nbins + per - 1) / per);
}

// ---- time chunking ------------------------------------------------------------------------------------------------------------
struct ChunkQuery
{
  size_t n = 0, channels = 1, nbins = 0;
  bool rows_kernel = false;      // the row-group kernel takes the call: one workgroup per (channel, chunk)
  bool exact = false;            // exact carries (the reference's rounding sequence)
  bool pipelined = false;        // the call's rows run beside the neighbouring calls' (two row streams)
  long forced_chunk = 0;         // option "chunk"
  long target_waves = 0;         // option "target_waves"
  long row_waves = 1, tiles = 1; // of the plan's geometry
  int compute_units = 256;
};
struct Chunking { long chunks = 1, len = 0; };

// Enough workgroups to fill the chip, chunks not shorter than a minimum.  Row-group kernel: two rounds of the CUs (the carry
// pre-pass gets cheaper with fewer chunks: 1017 chunks 0.044 ms, 511 chunks 0.029 ms at n = 1e6); exact carries: 2048 chunks
// (8 overlap segments of >= 256 workgroups).  Calls below 36 000 samples are bound by the serial samples of one chunk
// (~0.36 us each), not by HBM: about 190 chunks of >= 32 samples.  WHOLE ROUNDS of the chip: a row group is one workgroup per
// CU, so 260 ... 500 workgroups on 256 CUs are one full round plus a partly filled one that takes just as long (n = 52 000:
// 260 chunks of 200 rows 226 us, 250 chunks of 208 rows 168 us): between one and two rounds the call takes ONE round of
// longer chunks.  Pipelined calls are the opposite case (the next call's workgroups fill whatever a launch leaves free, and a
// launch that fills the chip exactly keeps all workgroups in step): about 300 chunks of >= 160 rows whatever the length.
inline Chunking choose_chunks(const ChunkQuery& q)
{
  Chunking r;
  const long ch = (long)std::max<size_t>(q.channels, 1);
  const size_t n = q.n;
  if (q.rows_kernel && q.forced_chunk <= 0 && n >= (size_t)kHopSamples)
  {
    const long target_blocks = q.target_waves > 0 ? std::max(1L, q.target_waves / std::max(1L, q.row_waves)) : (q.exact ? 2048 : 512);
    long want = std::max(1L, (target_blocks + ch - 1) / ch);
    const bool mid = q.target_waves <= 0 && q.channels * n < 36000;
    if (mid) want = std::max(1L, std::min((190L + ch - 1) / ch, (long)(n / 32)));
    else want = std::max(1L, std::min(want, (long)(n / (q.exact ? 128 : 192))));
    if (!mid && q.pipelined && q.target_waves <= 0)
    {
      const long total = std::max(1L, (300L + ch - 1) / ch);
      want = std::max(1L, std::min(total, (long)(n / 160)));
    }
    else if (!mid && !q.exact && q.target_waves <= 0)
    {
      const long round = (long)q.compute_units;
      const long blocks = want * ch;
      if (blocks > round && blocks < 2L * round) want = std::max(1L, round / ch);
    }
    long len = (long)((n + (size_t)want - 1) / (size_t)want);
    len = ((len + kTimeGroup - 1) / kTimeGroup) * kTimeGroup;
    if (q.exact)
    {
      len = ((len + 31) / 32) * 32;                          // whole trips of the exact pass's inner loop
      if (mid && len > 32) len = ((len + 63) / 64) * 64;
      if (!mid && len > 64) len = ((len + 127) / 128) * 128; // whole blocks of the relay form
    }
    len = std::max(1L, std::min(len, (long)n));
    r.len = len; r.chunks = (long)((n + (size_t)len - 1) / (size_t)len);
    return r;
  }
  const long target = q.target_waves > 0 ? q.target_waves : 16384;
  const long min_len = 64;
  if (q.forced_chunk <= 0 && n < (size_t)kHopSamples) { r.chunks = 1; r.len = (long)n; return r; }   // short hops stay serial (and bit-exact)
  const long per = std::max(1L, ch * std::max(1L, q.tiles));
  long want = (target + per - 1) / per;
  long len;
  if (q.forced_chunk > 0) len = !q.exact ? ((q.forced_chunk + kSumBlockLen - 1) / kSumBlockLen) * kSumBlockLen : q.forced_chunk;
  else
  {
    want = std::max(1L, std::min(want, (long)(n / (size_t)min_len)));
    len = (long)((n + (size_t)want - 1) / (size_t)want);
    len = ((len + kTimeGroup - 1) / kTimeGroup) * kTimeGroup;
    if (q.exact) len = ((len + 31) / 32) * 32;
  }
  len = std::max(1L, std::min(len, (long)std::max<size_t>(n, 1)));
  r.len = len; r.chunks = (long)((n + (size_t)len - 1) / (size_t)len);
  return r;
}

// ---- decimated analysis (sdft_hip_sdft_every_n) --------------------------------------------------------------------------------
// Rows a call of n samples keeps: those at first, first + every, ... < n (the grid is call-local: every == 0 keeps none, the
// entry point refuses it).  A streaming host passes every_next_first(...) as the next call's first.
inline size_t every_rows(size_t n, size_t every, size_t first)
{
  return (every != 0 && first < n) ? (n - first - 1) / every + 1 : 0;          // (= ceil((n - first) / every), without overflow)
}
inline size_t every_next_first(size_t n, size_t every, size_t first)
{
  const size_t rows = every_rows(n, every, first);
  return rows ? first + rows * every - n : (first >= n ? first - n : 0);
}
// first of the part of a call that starts at sample t0 (host-pointer segments): the grid's first sample at or after t0, from t0
inline size_t every_first_from(size_t t0, size_t every, size_t first)
{
  if (first >= t0) return first - t0;
  const size_t past = (t0 - first) % every;
  return past ? every - past : 0;
}
// Time chunks of forward_every_kernel.  The kernel stores a row every `every` samples only: it is bound by the recurrence's
// arithmetic (about ten unfused operations per bin and sample), not by HBM.  So the grid is sized by waves, not by bytes: enough
// (chunk x tile x channel) waves for kEveryWavesPerSimd per SIMD of every CU, chunks not shorter than kEveryMinLen samples (each
// chunk pays a carry-in and a share of the carry pre-pass), calls below kHopSamples in one chunk (bit-identical, as the hop
// kernel's).  Exact carries: whole 128-sample blocks of the relay form.  The recurrence is a chain of dependent operations per
// wave, so it takes many waves to cover the latency: configs[1] at every = 100, 863 chunks of 1160 samples (this choice) 0.541 ms,
// chunks of 1024 / 2048 / 4632 (4 waves per SIMD) samples 0.524 / 0.542 / 0.582 ms (profiles/every_rates.txt).
constexpr long kEveryWavesPerSimd = 16, kEverySimds = 4, kEveryMinLen = 256;
struct EveryQuery
{
  size_t n = 0, channels = 1;
  long tiles = 1;                // bin tiles of the independent-tile geometry
  bool exact = false;
  long forced_chunk = 0;         // option "chunk"
  int compute_units = 256;
};
inline Chunking choose_grid_chunks(const EveryQuery& q, long min_len)
{
  Chunking r;
  const size_t n = q.n;
  if (n == 0) { r.chunks = 1; r.len = 0; return r; }
  long len;
  if (q.forced_chunk > 0) len = !q.exact ? ((q.forced_chunk + kSumBlockLen - 1) / kSumBlockLen) * kSumBlockLen : q.forced_chunk;
  else
  {
    if (n < (size_t)kHopSamples) { r.chunks = 1; r.len = (long)n; return r; }
    const long target = (long)std::max(q.compute_units, 1) * kEverySimds * kEveryWavesPerSimd;
    const long per = std::max(1L, (long)std::max<size_t>(q.channels, 1) * std::max(1L, q.tiles));
    long want = (target + per - 1) / per;
    want = std::max(1L, std::min(want, (long)(n / (size_t)min_len)));
    len = (long)((n + (size_t)want - 1) / (size_t)want);
    len = ((len + kTimeGroup - 1) / kTimeGroup) * kTimeGroup;
    if (q.exact) len = ((len + 127) / 128) * 128;
  }
  len = std::max(1L, std::min(len, (long)n));
  r.len = len; r.chunks = (long)((n + (size_t)len - 1) / (size_t)len);
  return r;
}
inline Chunking choose_every_chunks(const EveryQuery& q) { return choose_grid_chunks(q, kEveryMinLen); }

// ---- power-spectrogram analysis (sdft_hip_sdft_power_n) ------------------------------------------------------------------------
// |X|^2 of the bins [bin0, bin0 + nbins_out) of the rows of an every-grid, dense [channels][rows][nbins_out] real numbers.
// The band lies inside the plan's bins and is not empty (no overflow of bin0 + nbins_out)
inline bool power_band_ok(size_t nbins, size_t bin0, size_t nbins_out)
{
  return nbins_out != 0 && bin0 <= nbins && nbins_out <= nbins - bin0;
}
// Tile t of the independent-tile geometry owns the bins [t * per, min((t + 1) * per, nbins)), per = interior lanes x bins per lane
// (halo lanes own nothing); it forms rows only if one of them is in the band.  forward_power_kernel makes the same test per wave.
inline bool power_tile_emits(long tile, long interior, int bins_per_lane, size_t nbins, size_t bin0, size_t nbins_out)
{
  const size_t per = (size_t)interior * (size_t)bins_per_lane;
  const size_t own0 = (size_t)tile * per, own1 = std::min(own0 + per, nbins);
  return own0 < own1 && own0 < bin0 + nbins_out && bin0 < own1;
}
// elements from one channel's first power to the next channel's, and the place of bin k of row r in a channel
inline size_t power_channel_stride(size_t rows, size_t nbins_out) { return rows * nbins_out; }
inline size_t power_offset(size_t row, size_t k, size_t bin0, size_t nbins_out) { return row * nbins_out + (k - bin0); }
// Time chunks of forward_power_kernel.  A sparse grid is forward_every_kernel's case (arithmetic-bound: choose_every_chunks).  On
// a dense grid (every <= kTimeGroup: the kernel's burst path) every sample or so is a row, as in the tile kernel, so a short call
// is cut with the tile kernel's minimum (choose_chunks: 64 samples); both rules ask for the same number of waves, so long calls
// get the same chunks either way.  Measured, the dense grid wants no rule of its own: the kernel is bound by the arithmetic of
// its rows, not by their bytes, and is flat in the chunk length -- configs[1], all bins, this choice (863 chunks of 1160 samples)
// against chunks of 256 / 512 / 1024 / 2048 / 4632 / 9264: every = 1 2.237 against 2.198 / 2.035 / 2.097 / 1.978 / 2.261 /
// 2.908 ms (between two runs the best moved from 512 to 2048: noise), every = 16 0.664 against 0.711 / 0.641 / 0.622 / 0.656 /
// 0.767 / 1.033, every = 100 0.483 against 0.550 / 0.486 / 0.472 / 0.499 / 0.570 / 0.713 (profiles/power_rates.txt).
constexpr long kPowerDenseMinLen = 64;
inline long power_min_len(size_t every) { return every <= (size_t)kTimeGroup ? kPowerDenseMinLen : kEveryMinLen; }
inline Chunking choose_power_chunks(const EveryQuery& q, size_t every) { return choose_grid_chunks(q, power_min_len(every)); }

// ---- pooled power analysis (sdft_hip_sdft_power_sum_n) -------------------------------------------------------------------------
// The grid points first, first + every, ... cut the call's samples into windows; row r is the sum over the r-th window of the
// powers sdft_hip_sdft_power_n stores at every == 1.  A call with first > 0 begins with the head window [0, min(first, n)), the end
// of a window the previous call began (row 0); window j is [first + j * every, min(first + (j + 1) * every, n)).
inline size_t power_sum_head(size_t n, size_t first) { return first > 0 && n > 0 ? 1 : 0; }
inline size_t power_sum_rows(size_t n, size_t every, size_t first) { return power_sum_head(n, first) + every_rows(n, every, first); }
struct PowerSumWindow { size_t row, begin, end; };           // samples [begin, end) of the call, end <= n
// the window sample t < n lies in (every >= 1), and the window of row r < power_sum_rows(n, every, first)
inline PowerSumWindow power_sum_window(size_t t, size_t n, size_t every, size_t first)
{
  if (t < first) return {0, 0, std::min(first, n)};
  const size_t j = (t - first) / every, b = first + j * every;
  return {power_sum_head(n, first) + j, b, every < n - b ? b + every : n};
}
inline PowerSumWindow power_sum_row_window(size_t row, size_t n, size_t every, size_t first)
{
  const size_t head = power_sum_head(n, first);
  if (row < head) return {0, 0, std::min(first, n)};
  const size_t b = first + (row - head) * every;
  return {row, b, every < n - b ? b + every : n};
}
// Time chunk c of a launch is the samples [chunk_begin, chunk_end) (the kernels' t0 and t1: chunks of len samples, all but the
// first shifted down by `shift` in the ring form of the exact carries); chunk_of is the chunk of sample t
inline size_t chunk_begin(long c, long len, long shift) { return c ? (size_t)c * (size_t)len - (size_t)shift : 0; }
inline size_t chunk_end(long c, long len, long shift, size_t n) { return std::min((size_t)(c + 1) * (size_t)len - (size_t)shift, n); }
inline long chunk_of(size_t t, long len, long shift) { return (long)((t + (size_t)shift) / (size_t)len); }
// What a chunk [t0, t1) does with its windows.  A window that begins and ends inside the chunk is whole: the forward kernel stores
// its row.  At most two windows are cut by the chunk's ends: the one that began before t0 leaves its samples of the chunk as the
// chunk's head piece, the one that runs past t1 as its tail piece (a chunk that lies wholly inside one window has the head piece
// only).  Pieces go to the plan's workspace [channels][chunks][2][nbins_out], head in slot 0, tail in slot 1.
constexpr int kPowerSumHeadSlot = 0, kPowerSumTailSlot = 1;
struct PowerSumChunk
{
  bool head = false, tail = false;
  size_t head_row = 0, tail_row = 0;                         // the rows the pieces belong to
  size_t whole_row0 = 0, whole_rows = 0;                     // rows whole_row0 ... whole_row0 + whole_rows - 1 are stored from this chunk
};
inline PowerSumChunk power_sum_chunk(size_t t0, size_t t1, size_t n, size_t every, size_t first)
{
  PowerSumChunk p;
  if (t0 >= t1) return p;
  const PowerSumWindow a = power_sum_window(t0, n, every, first), b = power_sum_window(t1 - 1, n, every, first);
  p.head = a.begin < t0; p.head_row = a.row;
  p.tail = b.end > t1 && !(p.head && a.row == b.row); p.tail_row = b.row;
  p.whole_row0 = a.row + (p.head ? 1 : 0);
  const size_t past = b.row + (b.end > t1 ? 0 : 1);          // the first row after the whole ones
  p.whole_rows = past > p.whole_row0 ? past - p.whole_row0 : 0;
  return p;
}
inline size_t power_sum_slot(size_t channel, size_t chunks, size_t chunk, int slot, size_t nbins_out)
{
  return ((channel * chunks + chunk) * 2 + (size_t)slot) * nbins_out;
}
inline size_t power_sum_workspace(size_t channels, size_t chunks, size_t nbins_out) { return chunks > 1 ? channels * chunks * 2 * nbins_out : 0; }
// The chunks a row's window touches, c0 <= c1.  c1 == c0: the row is whole in that chunk.  Else the row is cut and is the sum, in
// this order, of the tail piece of chunk c0 and the head pieces of the chunks c0 + 1 ... c1 (pooled_power_rows_kernel: the thread
// of chunk c0 + 1 adds them; ascending order, so the same bits on every run).
struct PowerSumRowChunks { long c0, c1; };
inline PowerSumRowChunks power_sum_row_chunks(const PowerSumWindow& w, long len, long shift)
{
  return {chunk_of(w.begin, len, shift), chunk_of(w.end - 1, len, shift)};
}
// Time chunks of forward_pooled_power_kernel: every sample is a windowed power, whatever `every` is, so this is
// forward_power_kernel's dense grid (choose_power_chunks at every == 1: the tile kernel's minimum of 64 samples, the wave count of
// the arithmetic-bound kernels).  Shorter chunks than that cost a carry-in each and cut more windows; longer ones leave SIMDs idle.
// Measured, configs[1], all bins, this choice (863 chunks of 1160 samples) against chunks of 256 / 512 / 1024 / 2048 / 4632 / 9264:
// every = 100 1.520 against 1.566 / 1.508 / 1.537 / 1.658 / 1.850 / 2.348 ms, every = n (one window over all chunks: 863 pieces per
// bin for pooled_power_rows_kernel) 1.495 against 1.712 / 1.577 / 1.556 / 1.637 / 1.845 / 2.343 ms (profiles/power_sum_rates.txt).
inline Chunking choose_power_sum_chunks(const EveryQuery& q) { return choose_power_chunks(q, 1); }

// ---- peak-hold analysis (sdft_hip_sdft_power_peak_n) ---------------------------------------------------------------------------
// The pooled power call's grid, windows, head row, chunks, pieces and workspace with the other statistic: row r is the largest
// (hold 0) or the smallest (hold 1) of the window's powers.  One rule combines a held value m with a term p, in the kernel
// (forward_power_peak_kernel), the cut-window pass (peak_rows_kernel), the segment join (peak_join_kernel, or this function on a
// host buffer) and a host that joins the head row of a call to the last row of the call before it.  A NaN term takes the place
// of whatever is held and nothing replaces it, so a window with a NaN term gives NaN; without one the result is one of the terms.
// Every window and every piece of one has a sample: accumulators start at -inf (max) or +inf (min), which the first term replaces.
constexpr int kHoldMax = 0, kHoldMin = 1;                    // enum sdft_hip_hold
inline bool peak_hold_ok(int hold) { return hold == kHoldMax || hold == kHoldMin; }
template <typename T> inline T peak_hold(T m, T p, int hold)
{
  return hold == kHoldMin ? ((p < m || p != p) ? p : m) : ((p > m || p != p) ? p : m);
}

// ---- smoothed power analysis (sdft_hip_sdft_power_smooth_n) ----------------------------------------------------------------------
// The one-pole average of the power call's every == 1 term p, s[t] = fl(fl(a * s[t - 1]) + fl(b * p[t])) in FD, a = (FD)decay,
// b = fl(1 - a), advanced at EVERY sample of the call and kept on the power call's grid (rows: every_rows; the row of a grid point
// holds s after that sample's step).  It is the first statistic with memory across windows: s before a call's first sample comes
// from the caller's state [channels][nbins_out] and s after its last goes back there.  The pooled power call's route and chunk
// choice (choose_power_sum_chunks).  Chunk 0 starts from the state, every later chunk from +0 and so leaves a^(j + 1) * S_c out of
// its j-th sample, S_c the true s before the chunk.  Each chunk leaves the value it ends with, E_c, in the workspace
// [channels][chunks][nbins_out]; smooth_scan_kernel walks S_1 = E_0, S_{c + 1} = fl(fl(P[len_c] * S_c) + E_c) in ascending order,
// puts S_c in E_c's place and the last value into the state; smooth_fix_kernel adds fl(P[j + 1] * S_c) to the kept rows of the
// chunks c >= 1.  P[j] = fl(a^j) (power_smooth_table).  A call of one chunk needs none of this and is the sequential loop bit for bit.
// The decay a call may take: after rounding to FD neither NaN nor negative nor 1 or more (a == 1 never forgets: b == 0)
template <typename T> inline bool power_smooth_decay_ok(double decay)
{
  const T a = (T)decay;
  return a >= (T)0 && a < (T)1;                              // (false for NaN)
}
inline size_t power_smooth_slot(size_t channel, size_t chunks, size_t chunk, size_t nbins_out) { return (channel * chunks + chunk) * nbins_out; }
inline size_t power_smooth_workspace(size_t channels, size_t chunks, size_t nbins_out) { return chunks > 1 ? channels * chunks * nbins_out : 0; }
// P[j] = a^j for j = 0 ... len, formed from the rounded a in long double and rounded once to T (P[0] = 1 also at a == 0)
template <typename T> inline std::vector<T> power_smooth_table(T a, size_t len)
{
  std::vector<T> p(len + 1);
  for (size_t j = 0; j <= len; ++j) p[j] = (T)std::pow((long double)a, (long double)j);
  return p;
}
// what smooth_fix_kernel does with the row of sample t: its chunk and, in a chunk c >= 1, the entry of P that scales S_c -- the
// number of steps from the chunk's first sample up to and including t
struct PowerSmoothFix { long chunk; size_t power; };
inline PowerSmoothFix power_smooth_fix(size_t t, long len, long shift)
{
  const long c = chunk_of(t, len, shift);
  return {c, t - chunk_begin(c, len, shift) + 1};
}

// ---- smoothed cross-spectrum analysis (sdft_hip_sdft_cross_smooth_n) -------------------------------------------------------------
// The same recursion on each component of the cross-spectrum call's every == 1 term (re, im) of a pair, with the pair list's work
// items (cross_items) in the channels' place.  A unit of the carry is a pair and its row is the 2 * nbins_out real numbers
// (re, im) of the band: the scan and the fix-up above are real-valued and elementwise, so they serve unchanged with
// power_smooth_slot / power_smooth_workspace / power_smooth_fix taking (npairs, cross_smooth_unit_row(nbins_out)) for (channels,
// nbins_out).  The items of the pairs come first and in the pairs' order: item i < npairs is unit i.
inline size_t cross_smooth_unit_row(size_t nbins_out) { return 2 * nbins_out; }

// ---- smoothed peak-hold analysis (sdft_hip_sdft_smooth_peak_n) -------------------------------------------------------------------
// Row r holds, per bin, peak_hold over the r-th window of the peak-hold call's grid (power_sum_rows, power_sum_window) of the
// smoothed power call's sequence s[t], taken after sample t's step.  The extreme of s0[t] + a^j * S_c over a window is not a
// function of the extreme of s0[t], so the rows cannot be formed from +0 and fixed up: the carries come before the rows.  A call
// of several chunks runs forward_power_smooth_kernel on a grid that keeps no row (smooth_peak_carry_grid) for the chunks' end
// values E_c, smooth_scan_kernel for S_c, then forward_smooth_peak_kernel, whose chunk c >= 1 starts from S_c
// (power_smooth_slot), then peak_rows_kernel for the windows a chunk boundary cuts.  A call of one chunk is one launch and the
// sequential loop bit for bit.
// why a call is refused beyond the grid and the band: the hold first, then the decay (nullptr: neither)
template <typename T> inline const char* smooth_peak_refusal(int hold, double decay)
{
  if (!peak_hold_ok(hold)) return "hold must be sdft_hip_hold_max (0) or sdft_hip_hold_min (1)";
  if (!power_smooth_decay_ok<T>(decay)) return "decay must be at least 0 and less than 1 after rounding to sdft_fd_t";
  return nullptr;
}
// the grid the carry pass gives forward_power_smooth_kernel: its first point lies beyond the call's n samples, so no row is stored
struct SmoothPeakCarryGrid { size_t every, first; };
inline SmoothPeakCarryGrid smooth_peak_carry_grid(size_t n) { return {1, n}; }
// the scheme on a host, for one bin: p[0 .. n) are the terms, s_in the incoming state, the chunks are [c * len - shift, ...) as
// chunk_begin cuts them.  Writes s[t] after every sample to s_out[0 .. n) as the kernels form it -- the carry pass from +0, the
// scan with P[j] = power_smooth_table, the row pass from S_c -- and returns the state the call leaves (the last s).
template <typename T> inline T smooth_peak_scheme(const T* p, size_t n, T a, T s_in, long len, long shift, T* s_out)
{
  const T b = (T)1 - a;
  const long chunks = n ? chunk_of(n - 1, len, shift) + 1 : 0;
  const std::vector<T> pw = power_smooth_table<T>(a, (size_t)len);
  std::vector<T> start((size_t)std::max(chunks, 1L), s_in);
  T S = s_in;
  for (long c = 0; c < chunks; ++c)
  {
    const size_t t0 = chunk_begin(c, len, shift), t1 = std::min(n, chunk_begin(c + 1, len, shift));
    volatile T e = c ? (T)0 : s_in;                        // (volatile: each product and sum is rounded to T, no contraction)
    for (size_t t = t0; t < t1; ++t) { volatile T as = a * e, bp = b * p[t]; e = as + bp; }
    start[(size_t)c] = S;
    if (c == 0) S = e;
    else { volatile T ps = pw[t1 - t0] * S; S = ps + e; }
  }
  T s = s_in;
  for (long c = 0; c < chunks; ++c)
  {
    const size_t t0 = chunk_begin(c, len, shift), t1 = std::min(n, chunk_begin(c + 1, len, shift));
    volatile T v = start[(size_t)c];
    for (size_t t = t0; t < t1; ++t) { volatile T as = a * v, bp = b * p[t]; v = as + bp; s_out[t] = v; }
    s = v;
  }
  return s;
}

// ---- pooled cross-spectrum analysis (sdft_hip_sdft_cross_sum_n) ------------------------------------------------------------------
// Row r of pair p = (a, b) is the sum over the r-th window of the pooled power call's grid of A conj(B), A and B the windowed bins
// of the channels a and b.  A wave of forward_cross_sum_kernel steps the recurrences of the two channels of ONE work item, so the
// pair list becomes a table of items, once per sdft_hip_set_pairs: item p < npairs is pair p (out = p); after them comes one
// advance-only item {c, c, none} for every channel c that no pair names, so that every channel's state moves with the call.
// Exactly one item and side per channel writes that channel's state back: the first item that names it, side a before side b.
// (P pairs step up to 2P recurrences: a channel that is in many pairs is stepped once per pair.)
constexpr int kCrossNone = -1;
struct CrossItem
{
  unsigned a, b;
  int out;                                // the pair whose sums the item forms, kCrossNone: it only advances channel a (== b)
  unsigned short writes_a, writes_b;      // this side stores its channel's state on the last chunk
};
enum CrossCheck : int { CX_OK = 0, CX_NULL = 1, CX_CHANNEL = 2, CX_TOO_MANY = 3 };
// a pair list sdft_hip_set_pairs may install (npairs == 0 removes the list)
inline int cross_pairs_check(size_t channels, size_t npairs, const size_t* pair_a, const size_t* pair_b)
{
  if (npairs == 0) return CX_OK;
  if (!pair_a || !pair_b) return CX_NULL;
  if (npairs > ((size_t)1 << 31)) return CX_TOO_MANY;
  const size_t ch = std::max<size_t>(channels, 1);
  for (size_t p = 0; p < npairs; ++p)
    if (pair_a[p] >= ch || pair_b[p] >= ch) return CX_CHANNEL;
  return CX_OK;
}
// (of a list cross_pairs_check has passed)
inline std::vector<CrossItem> cross_items(size_t channels, size_t npairs, const size_t* pair_a, const size_t* pair_b)
{
  const size_t ch = std::max<size_t>(channels, 1);
  std::vector<CrossItem> items;
  std::vector<char> written(ch, 0);
  items.reserve(npairs + ch);
  for (size_t p = 0; p < npairs; ++p)
  {
    CrossItem it{(unsigned)pair_a[p], (unsigned)pair_b[p], (int)p, 0, 0};
    if (!written[it.a]) { it.writes_a = 1; written[it.a] = 1; }
    if (!written[it.b]) { it.writes_b = 1; written[it.b] = 1; }      // (a == b: side a has taken it)
    items.push_back(it);
  }
  for (size_t c = 0; c < ch; ++c)
    if (!written[c]) items.push_back(CrossItem{(unsigned)c, (unsigned)c, kCrossNone, 1, 0});
  return items;
}
// The workspace of the windows a chunk boundary cuts: power_sum_workspace / power_sum_slot with items for channels and, a complex
// sum being two real ones, 2 * nbins_out numbers for nbins_out (advance-only items come last and use none of it)
inline size_t cross_sum_workspace(size_t items, size_t chunks, size_t nbins_out) { return power_sum_workspace(items, chunks, 2 * nbins_out); }
inline size_t cross_sum_slot(size_t item, size_t chunks, size_t chunk, int slot, size_t nbins_out) { return power_sum_slot(item, chunks, chunk, slot, 2 * nbins_out); }
// numbers (not complex numbers) from one pair's first sum to the next pair's
inline size_t cross_pair_stride(size_t rows, size_t nbins_out) { return power_channel_stride(rows, 2 * nbins_out); }

// ---- lag-product analysis (sdft_hip_sdft_lag_sum_n) -----------------------------------------------------------------------------
// Row r of a channel is the sum over the r-th window of the pooled power call's grid of A conj(B), A the windowed bin of sample t
// and B that of sample t - 1 of the SAME channel: the cross-spectrum call's term, rows, workspace and strides with the plan's
// channels in the pairs' place, on the pooled power call's route (one recurrence per wave, its chunk choice).  The row before a
// chunk's first sample is demodulated from the chunk's carry-in (forward_lag_sum_kernel), so no carry pass and no launch changes.
inline size_t lag_sum_workspace(size_t channels, size_t chunks, size_t nbins_out) { return cross_sum_workspace(std::max<size_t>(channels, 1), chunks, nbins_out); }
inline size_t lag_sum_slot(size_t channel, size_t chunks, size_t chunk, int slot, size_t nbins_out) { return cross_sum_slot(channel, chunks, chunk, slot, nbins_out); }
inline size_t lag_channel_stride(size_t rows, size_t nbins_out) { return cross_pair_stride(rows, nbins_out); }
// (the time segments of a call on host memory: lag_sum_segment, beside stage_rows)

// ---- power-moments analysis (sdft_hip_sdft_power_moments_n) ---------------------------------------------------------------------
// Row r of a channel holds, per bin of the band, the pair (s1, s2): the sum over the r-th window of the pooled power call's grid of
// that call's term p, and the sum of q = fl(p * p).  A row of nbins_out pairs has the shape of the cross-spectrum call's row of
// nbins_out complex sums, so rows, workspace and strides are that call's with the plan's channels in the pairs' place, as the
// lag-product call has them -- on the pooled power call's route with ITS chunk choice (choose_power_sum_chunks, nothing of this
// call's own): [..][0] has the pooled call's bits only while both calls cut time alike.
inline size_t power_moments_workspace(size_t channels, size_t chunks, size_t nbins_out) { return cross_sum_workspace(std::max<size_t>(channels, 1), chunks, nbins_out); }
inline size_t power_moments_slot(size_t channel, size_t chunks, size_t chunk, int slot, size_t nbins_out) { return cross_sum_slot(channel, chunks, chunk, slot, nbins_out); }
inline size_t power_moments_channel_stride(size_t rows, size_t nbins_out) { return cross_pair_stride(rows, nbins_out); }
// (the time segments of a call on host memory: power_moments_segment, beside stage_rows)

// ---- array covariance analysis (sdft_hip_sdft_covariance_n) ------------------------------------------------------------------------
// The array is an ordered list of nch distinct channels of the plan (sdft_hip_set_array); the call returns the cross-spectrum
// call's sums for ALL pairs of its elements: the upper triangle in row-major order, element (i <= j) -- the pair of the channels
// (chan[i], chan[j]) -- at the output index covariance_pair_index.  As a pair list that steps two recurrences per pair; here the
// array is cut into groups of G consecutive elements (the last one may be shorter) and a wave of forward_covariance_kernel takes a
// BLOCK: group u on side A and group v >= u on side B, 2 G recurrences for G x G pairs.  A diagonal block (u == v) steps its one
// group once and forms the pairs (sa <= sb) of it; it is also the one item that writes the state of its channels back, so every
// array channel has exactly one writer.  After the blocks comes one advance-only item per plan channel that is not in the array.
enum ArrayCheck : int { AR_OK = 0, AR_CHANNEL = 1, AR_REPEAT = 2, AR_TOO_MANY = 3 };
constexpr size_t kArrayMaxChannels = 65535;                   // the pairs are counted in 32 bits
// a list sdft_hip_set_array may install (nch == 0 removes the list; chan == nullptr: the channels 0 ... nch - 1)
inline int array_check(size_t channels, size_t nch, const size_t* chan)
{
  const size_t ch = std::max<size_t>(channels, 1);
  if (nch > ch || nch > kArrayMaxChannels) return AR_TOO_MANY;
  if (!chan) return AR_OK;
  std::vector<char> seen(ch, 0);
  for (size_t i = 0; i < nch; ++i)
  {
    if (chan[i] >= ch) return AR_CHANNEL;
    if (seen[chan[i]]) return AR_REPEAT;
    seen[chan[i]] = 1;
  }
  return AR_OK;
}
inline size_t covariance_pairs(size_t nch) { return nch * (nch + 1) / 2; }
// i <= j < nch: i * nch - i (i - 1) / 2 + (j - i)
inline size_t covariance_pair_index(size_t nch, size_t i, size_t j) { return (i * (2 * nch - i + 1)) / 2 + (j - i); }
struct CovItem
{
  unsigned a0, b0;                        // a block: the first array element of side A and of side B (a0 <= b0; a0 == b0: diagonal);
                                          // an advance-only item: the PLAN channel, twice
  unsigned short na, nb;                  // elements on each side (1 ... G; advance-only: 1 and 0)
  unsigned short block, writes;           // block: forms pairs; writes: stores the state of side A's channels on the last chunk
};
// (of a list array_check has passed)
inline std::vector<CovItem> covariance_items(size_t channels, size_t nch, const size_t* chan, int G)
{
  const size_t ch = std::max<size_t>(channels, 1), g = (size_t)std::max(G, 1), groups = (nch + g - 1) / g;
  std::vector<CovItem> items;
  std::vector<char> in_array(ch, 0);
  for (size_t i = 0; i < nch; ++i) in_array[chan ? chan[i] : i] = 1;
  items.reserve(groups * (groups + 1) / 2 + ch);
  for (size_t u = 0; u < groups; ++u)
    for (size_t v = u; v < groups; ++v)
      items.push_back(CovItem{(unsigned)(u * g), (unsigned)(v * g), (unsigned short)std::min(g, nch - u * g), (unsigned short)std::min(g, nch - v * g),
                              1, (unsigned short)(u == v ? 1 : 0)});
  for (size_t c = 0; c < ch; ++c)
    if (!in_array[c]) items.push_back(CovItem{(unsigned)c, (unsigned)c, 1, 0, 0, 1});
  return items;
}
// the output index of the slots (sa, sb) of an item, or -1: the slot pair forms nothing (the kernel makes the same test)
inline long covariance_item_out(size_t nch, const CovItem& it, size_t sa, size_t sb)
{
  if (!it.block || sa >= it.na || sb >= it.nb || (it.a0 == it.b0 && sa > sb)) return -1;
  return (long)covariance_pair_index(nch, it.a0 + sa, it.b0 + sb);
}
// The workspace of the windows a chunk boundary cuts is the cross-spectrum call's with the nch (nch + 1) / 2 output indices for
// pairs: [pairs][chunks][2][nbins_out] complex, slot cross_sum_slot(p, ...)
inline size_t covariance_workspace(size_t nch, size_t chunks, size_t nbins_out) { return cross_sum_workspace(covariance_pairs(nch), chunks, nbins_out); }

// ---- channel-mix analysis (sdft_hip_sdft_mix_n) --------------------------------------------------------------------------------------
// A mix is an ordered list of nch distinct channels of the plan, as an array is, and nout weight tables [nch][dftsize] (sdft_hip_set_mix);
// output o of the call is, per row of an every-grid and per bin, the sum over the elements i of W[o][i][k] * X_chan[i][k].  A wave of
// forward_mix_kernel takes a BLOCK of up to O consecutive outputs and all the elements of the mix, group by group, so the items are
// the ceil(nout / O) blocks and, after them, one advance-only item per plan channel that is not in the mix.  The block of output 0
// is the one item that writes the state of the mix's channels back: every channel of the plan has exactly one writer.
enum MixCheck : int { MX_OK = 0, MX_CHANNEL = 1, MX_REPEAT = 2, MX_TOO_MANY = 3, MX_NO_WEIGHTS = 4, MX_NO_CHANNELS = 5, MX_TOO_MANY_OUTPUTS = 6 };
constexpr size_t kMixMaxOutputs = 65535;                      // an item counts its outputs in 16 bits
// a mix sdft_hip_set_mix may install (nout == 0 removes the mix, whatever the other arguments; chan == nullptr: the channels 0 ... nch - 1)
inline int mix_check(size_t channels, size_t nout, size_t nch, const size_t* chan, bool has_weights)
{
  if (nout == 0) return MX_OK;
  if (nout > kMixMaxOutputs) return MX_TOO_MANY_OUTPUTS;
  if (!has_weights) return MX_NO_WEIGHTS;
  if (nch == 0) return MX_NO_CHANNELS;
  switch (array_check(channels, nch, chan))
  {
    case AR_OK: return MX_OK;
    case AR_CHANNEL: return MX_CHANNEL;
    case AR_REPEAT: return MX_REPEAT;
    default: return MX_TOO_MANY;
  }
}
struct MixItem
{
  unsigned o0;                            // a block: its first output; an advance-only item: the PLAN channel
  unsigned short no, writes;              // no: outputs of the block (1 ... O; advance-only: 0); writes: stores state on the last chunk
};
// (of a mix mix_check has passed, nout > 0)
inline std::vector<MixItem> mix_items(size_t channels, size_t nch, const size_t* chan, size_t nout, int O)
{
  const size_t ch = std::max<size_t>(channels, 1), o = (size_t)std::max(O, 1), blocks = (nout + o - 1) / o;
  std::vector<MixItem> items;
  std::vector<char> in_mix(ch, 0);
  for (size_t i = 0; i < nch; ++i) in_mix[chan ? chan[i] : i] = 1;
  items.reserve(blocks + ch);
  for (size_t b = 0; b < blocks; ++b)
    items.push_back(MixItem{(unsigned)(b * o), (unsigned short)std::min(o, nout - b * o), (unsigned short)(b == 0 ? 1 : 0)});
  for (size_t c = 0; c < ch; ++c)
    if (!in_mix[c]) items.push_back(MixItem{(unsigned)c, 0, 1});
  return items;
}
// numbers (not complex numbers) from one output's first bin to the next output's, and the weight of (output, element, bin)
inline size_t mix_output_stride(size_t rows, size_t nbins_out) { return power_channel_stride(rows, 2 * nbins_out); }
inline size_t mix_weight_index(size_t nch, size_t nbins, size_t o, size_t i, size_t k) { return (o * nch + i) * nbins + k; }

// ---- filterbank analysis (sdft_hip_sdft_filterbank_n) --------------------------------------------------------------------------
// Band b of a filterbank covers the bins [band_bin0[b], band_bin0[b] + band_nbins[b]) with one weight per bin; row r of the output
// holds, per band, the sum of fl(weight * power) over the band's bins, the powers those sdft_hip_sdft_power_n stores for the row.
// Bands may overlap, repeat and come in any order.  What is refused: a band without bins, a band that ends past the plan's bins
// (no overflow of bin0 + nbins), and a filterbank whose tables would not fit the 32-bit fields of a piece.
enum FilterbankCheck : int { FB_OK = 0, FB_NULL = 1, FB_EMPTY_BAND = 2, FB_PAST_END = 3, FB_TOO_LARGE = 4 };
constexpr size_t kFilterbankMaxBands = (size_t)1 << 31;       // a piece's destination: 31 bits of band or slot, one flag
constexpr size_t kFilterbankMaxWeights = ((size_t)1 << 32) - 1;
inline int filterbank_check(size_t nbins, size_t nbands, const size_t* band_bin0, const size_t* band_nbins, bool weights_given)
{
  if (nbands == 0) return FB_OK;                            // (removes the filterbank)
  if (!band_bin0 || !band_nbins || !weights_given) return FB_NULL;
  if (nbands >= kFilterbankMaxBands) return FB_TOO_LARGE;
  size_t total = 0;
  for (size_t b = 0; b < nbands; ++b)
  {
    if (band_nbins[b] == 0) return FB_EMPTY_BAND;
    if (band_bin0[b] > nbins || band_nbins[b] > nbins - band_bin0[b]) return FB_PAST_END;
    if (band_nbins[b] > kFilterbankMaxWeights - total) return FB_TOO_LARGE;
    total += band_nbins[b];
  }
  return FB_OK;
}
// weights of the bands before band b (the offset of its first weight) are a running sum; all of them:
inline size_t filterbank_weights(size_t nbands, const size_t* band_nbins)
{
  size_t total = 0;
  for (size_t b = 0; b < nbands; ++b) total += band_nbins[b];
  return total;
}
// The independent-tile geometry gives tile t the bins [t * per, min((t + 1) * per, nbins)), per = interior lanes x bins per lane,
// and one wave; waves share no workgroup.  So every band is cut at the tile boundaries into PIECES, once per filterbank: a piece is
// the bins of one band inside one tile.  The wave of the tile forms the weighted sum of each of its pieces in ascending bin order.
// A band inside one tile has one piece, which is the band's value and goes straight to the output (dst = the band).  A band that
// crosses a boundary is SPLIT: its pieces get consecutive workspace slots in ascending tile order (dst = kFilterbankToWorkspace |
// slot) and filterbank_rows_kernel adds them in that order.  Neither order depends on the call, so a row's bits depend only on
// the plan, the filterbank and the row's powers.
constexpr uint32_t kFilterbankToWorkspace = 0x80000000u;
struct FilterbankPiece { uint32_t bin0, nbins, woff, dst; };      // bins [bin0, bin0 + nbins), weights from woff on in TILE order:
                                                                  // the pieces' weights one after the other as the pieces are sorted, so
                                                                  // that a tile's weights are one range (the kernel keeps its start in LDS)
struct FilterbankSplit { uint32_t band, slot0, pieces; };         // a split band: slots slot0 ... slot0 + pieces - 1
struct FilterbankLayout
{
  size_t nbands = 0, nslots = 0;                            // nslots: workspace slots per row and channel
  std::vector<FilterbankPiece> pieces;                      // sorted by tile, in band order inside a tile
  std::vector<size_t> wsrc;                                 // per piece: its first weight in the caller's band-ordered array
  std::vector<uint32_t> tile_piece0;                        // [tiles + 1]: tile t forms pieces[tile_piece0[t] ... tile_piece0[t + 1])
  std::vector<FilterbankSplit> splits;                      // in band order
};
// (of a filterbank filterbank_check has passed)
inline FilterbankLayout filterbank_layout(long tiles, long interior, int bins_per_lane, size_t nbands, const size_t* band_bin0, const size_t* band_nbins)
{
  FilterbankLayout l;
  l.nbands = nbands;
  const size_t per = (size_t)interior * (size_t)bins_per_lane, nt = (size_t)std::max(tiles, 1L);
  std::vector<size_t> count(nt + 1, 0);
  for (size_t b = 0; b < nbands; ++b)
    for (size_t t = band_bin0[b] / per; t <= (band_bin0[b] + band_nbins[b] - 1) / per; ++t) ++count[t + 1];
  for (size_t t = 0; t < nt; ++t) count[t + 1] += count[t];
  l.tile_piece0.resize(nt + 1);
  for (size_t t = 0; t <= nt; ++t) l.tile_piece0[t] = (uint32_t)count[t];
  l.pieces.resize(count[nt]);
  l.wsrc.resize(count[nt]);
  size_t woff = 0;
  for (size_t b = 0; b < nbands; ++b)
  {
    const size_t lo = band_bin0[b], hi = lo + band_nbins[b], t0 = lo / per, t1 = (hi - 1) / per;
    const size_t slot0 = l.nslots;
    if (t1 > t0)
    {
      l.splits.push_back(FilterbankSplit{(uint32_t)b, (uint32_t)slot0, (uint32_t)(t1 - t0 + 1)});
      l.nslots += t1 - t0 + 1;
    }
    for (size_t t = t0; t <= t1; ++t)
    {
      const size_t p0 = std::max(lo, t * per), p1 = std::min(hi, (t + 1) * per);
      const uint32_t dst = t1 > t0 ? (kFilterbankToWorkspace | (uint32_t)(slot0 + (t - t0))) : (uint32_t)b;
      l.wsrc[count[t]] = woff + (p0 - lo);
      l.pieces[count[t]++] = FilterbankPiece{(uint32_t)p0, (uint32_t)(p1 - p0), 0u, dst};
    }
    woff += band_nbins[b];
  }
  uint32_t at = 0;
  for (FilterbankPiece& p : l.pieces) { p.woff = at; at += p.nbins; }
  return l;
}
// The workspace holds the rows of ONE forward launch: [channels][rows of the launch][nslots] numbers, grown on demand and kept by
// the plan.  It is bounded: the time chunks of a call (whose carries exist before the first of them runs) go in as many launches,
// one after the other on the plan's stream, as keep each launch's rows within kFilterbankWorkspaceBytes, each followed by
// filterbank_rows_kernel on its rows -- row segments of one call, which change nothing in its values or its state.  A launch is
// at least one chunk: only a single chunk whose rows exceed the bound makes the workspace larger than that.
constexpr size_t kFilterbankWorkspaceBytes = (size_t)64 << 20;
inline size_t filterbank_slot(size_t channel, size_t rows, size_t row, size_t nslots, size_t slot) { return (channel * rows + row) * nslots + slot; }
inline size_t filterbank_workspace(size_t channels, size_t rows, size_t nslots) { return channels * rows * nslots; }
inline size_t filterbank_segment_rows(size_t channels, size_t nslots, size_t fd_bytes, size_t bound_bytes = kFilterbankWorkspaceBytes)
{
  const size_t row_bytes = std::max<size_t>(channels, 1) * nslots * fd_bytes;
  return row_bytes == 0 ? (size_t)-1 : std::max<size_t>(bound_bytes / row_bytes, 1);
}
// rows of the grid among the samples [0, t) of a call, and the rows the chunks [ja, jb) of a launch keep: row0 ... row0 + rows - 1
inline size_t filterbank_rows_before(size_t t, size_t every, size_t first) { return every_rows(t, every, first); }
struct FilterbankSpan { long ja, jb; size_t row0, rows; };
inline FilterbankSpan filterbank_span(long ja, long jb, long len, long shift, size_t n, size_t every, size_t first)
{
  const size_t r0 = filterbank_rows_before(chunk_begin(ja, len, shift), every, first), r1 = filterbank_rows_before(chunk_end(jb - 1, len, shift, n), every, first);
  return {ja, jb, r0, r1 - r0};
}
// the next launch of the chunks [ja, j1): as many chunks from ja on as keep at most max_rows rows, one at least
inline FilterbankSpan filterbank_next_span(long ja, long j1, long len, long shift, size_t n, size_t every, size_t first, size_t max_rows)
{
  FilterbankSpan s = filterbank_span(ja, ja + 1, len, shift, n, every, first);
  while (s.jb < j1)
  {
    const FilterbankSpan more = filterbank_span(ja, s.jb + 1, len, shift, n, every, first);
    if (more.rows > max_rows) break;
    s = more;
  }
  return s;
}

// ---- band-peak analysis (sdft_hip_sdft_band_peak_n) -----------------------------------------------------------------------------
// Per band of the installed filterbank and row of the filterbank call's grid the pair (m, i): with v_k = fl(w_k * p_k) over the
// band's bins in ascending order, i = np.argmax(v) and m = v[i] -- the lowest bin of the largest value, the lowest NaN bin if any
// value is NaN, the first bin's bits among equal zeros.  The pieces, the tile order, the slots and the launches by rows are the
// filterbank call's (filterbank_layout, filterbank_next_span); a slot holds a pair, so the workspace bound takes two numbers per slot.
// The rule is associative for ordered concatenation: the pieces of a split band, joined in ascending tile order with the lower
// piece held and the higher the candidate, give the bits of one walk over the whole band, for every cut of bins into tiles.
// The host's restatement of the rule (the kernels' band_peak_take; the tests hold it against np.argmax): is the candidate v, at a
// higher bin than the held m, taken?
template <typename T> inline bool band_peak_take(T m, T v) { return (v > m) || (v != v && m == m); }
constexpr size_t kBandPeakPair = 2;                         // numbers per band of a row, and per workspace slot: value, bin
inline size_t band_peak_segment_rows(size_t channels, size_t nslots, size_t fd_bytes, size_t bound_bytes = kFilterbankWorkspaceBytes)
{ return filterbank_segment_rows(channels, nslots, kBandPeakPair * fd_bytes, bound_bytes); }
inline size_t band_peak_workspace(size_t channels, size_t rows, size_t nslots) { return kBandPeakPair * filterbank_workspace(channels, rows, nslots); }
// the bin is stored as a number of FD: every bin of the plan must be one exactly (FD float: dftsize <= 2^24)
inline bool band_peak_bins_exact(size_t nbins, size_t fd_bytes) { return fd_bytes >= 8 ? nbins <= ((size_t)1 << 53) : nbins <= ((size_t)1 << 24); }

// ---- exact carries, relay form: block length = seed distance -----------------------------------------------------------
// divides 2N and the chunk length; L products live in L registers per lane (128 at FD float, 64 register pairs at FD double);
// the seed table (fid at every L-th cursor) stays below 256 MiB.  0: no block length fits (serial pass).
inline unsigned relay_block(size_t nbins, long chunk_len, size_t fd_bytes, size_t fdx_bytes, long forced)
{
  const size_t span = 2 * nbins;
  const unsigned top = fd_bytes == 4 ? 128u : 64u;
  for (unsigned cand : {128u, 64u, 32u, 16u, 8u})
  {
    if (cand > top) continue;
    if (forced > 0 && (unsigned)forced != cand) continue;
    if (span % cand == 0 && chunk_len > 0 && (size_t)chunk_len % cand == 0 && ((span / cand) * nbins * fdx_bytes) <= ((size_t)256 << 20)) return cand;
  }
  return 0;
}

// ---- radices of the mixed-radix FFT of `span` points (4, 2, 3, 5); count == 0: span has other prime factors --------------
struct Radices { unsigned char count = 0; unsigned char r[15] = {}; };
inline Radices smooth_radices(size_t span)
{
  Radices rl;
  size_t rem = span;
  if (rem == 0) return rl;
  for (unsigned f : {4u, 2u, 3u, 5u})
    while (rem % f == 0 && rl.count < 15) { rl.r[rl.count++] = (unsigned char)f; rem /= f; }
  if (rem != 1) rl.count = 0;
  return rl;
}
// LDS cells the in-kernel DFT of a self-carried chunk works in: 2N in place for powers of two, two buffers of 2N for the
// 2/3/5-smooth sizes (Stockham); 0: this 2N has neither form
inline size_t self_cells(size_t nbins, bool enabled, size_t fdx_bytes)
{
  const size_t span = 2 * nbins;
  if (span < 16 || span > 4096) return 0;
  if ((span & (span - 1)) == 0) return span;
  return (enabled && smooth_radices(span).count > 0 && 2 * span * fdx_bytes <= (size_t)80 * 1024) ? 2 * span : 0;
}

// ---- address ranges -------------------------------------------------------------------------------------------------------------
struct Range { uintptr_t lo = 0, hi = 0; };
inline bool overlap(uintptr_t alo, uintptr_t ahi, const Range& b) { return alo < b.hi && b.lo < ahi; }
inline bool overlap(const Range& a, const Range& b) { return a.lo < b.hi && b.lo < a.hi; }

// ---- which kind of host is calling: learnt from the calls ------------------------------------------------------------------
// Pipelining pays for a host that analyses call after call (or synthesises call after call); a host that alternates the two
// (the reference's loop, test/test.c:69-83) would pay an event wait between streams per call and gain nothing.  So a mode is
// on once two of a kind have come in a row and off again when the other kind follows a lone one.
struct CallPattern
{
  bool prev_was_inverse = false, inverse_batch = false;
  int inverse_run = 0;
  bool prev_was_analysis = false, analysis_batch = false;
  int analysis_run = 0;
  // an analysis call is about to be launched (fused = the fused analysis -> synthesis call, which is neither kind)
  void on_analysis(bool fused)
  {
    if (prev_was_inverse && inverse_run == 1) inverse_batch = false;
    prev_was_inverse = false; inverse_run = 0;
    if (prev_was_analysis && !fused) analysis_batch = true;
    prev_was_analysis = !fused;
    if (!fused) ++analysis_run;
  }
  // a synthesis call is about to be launched
  void on_synthesis_begin()
  {
    if (prev_was_inverse) inverse_batch = true;
    if (prev_was_analysis && analysis_run == 1) analysis_batch = false;
    prev_was_analysis = false; analysis_run = 0;
  }
  void on_synthesis_launched() { prev_was_inverse = true; ++inverse_run; }
};

// ---- pipelined analyses: the two row streams and the ring of four outstanding launches ------------------------------------
// Which row stream a launch goes to: the other one than the previous launch's -- unless the call's matrix overlaps what an
// outstanding launch writes: then the stream of the latest such launch (whose order costs nothing), and if launches on the
// other stream overlap as well, the latest of those is waited for by an event.
struct RowRing
{
  unsigned long long seq = 0;              // launches since the ring was last joined
  Range out[4];                            // what the outstanding launches write (by launch number & 3)
  int stream_of[4] = {0, 0, 0, 0};
  bool open = false;
  struct Pick { int stream = 0; bool behind = false; int wait_launch = -1; /* ring slot of a launch on the other stream to wait for */ };
  // do the call's SAMPLES lie in a matrix an outstanding launch is still writing?  (then everything joins first)
  bool samples_overlap(uintptr_t xlo, uintptr_t xhi) const
  {
    for (unsigned long long back = 1; back <= 3 && back <= seq; ++back)
      if (overlap(xlo, xhi, out[(seq - back) & 3])) return true;
    return false;
  }
  Pick pick(uintptr_t olo, uintptr_t ohi) const
  {
    Pick p;
    p.stream = seq ? (stream_of[(seq - 1) & 3] ^ 1) : 0;
    for (unsigned long long back = 1; back <= 3 && back <= seq; ++back)
      if (overlap(olo, ohi, out[(seq - back) & 3])) { p.stream = stream_of[(seq - back) & 3]; p.behind = true; break; }
    if (p.behind)
      for (unsigned long long back = 1; back <= 3 && back <= seq; ++back)
      {
        const int q = (int)((seq - back) & 3);
        if (stream_of[q] != p.stream && overlap(olo, ohi, out[q])) { p.wait_launch = q; break; }
      }
    return p;
  }
  // the state slot a launch's state kernel writes was read by the rows of three launches ago: their ring slot, or -1
  int state_reader() const { return seq >= 3 ? (int)((seq + 1) & 3) : -1; }
  int slot() const { return (int)(seq & 3); }
  void launched(uintptr_t olo, uintptr_t ohi, int stream) { out[seq & 3] = Range{olo, ohi}; stream_of[seq & 3] = stream; ++seq; open = true; }
  // the ring slots of the last launch on each row stream (older ones are ordered before them); returns how many
  int last_per_stream(int slots[2]) const
  {
    int count = 0;
    bool seen[2] = {false, false};
    for (unsigned long long back = 1; back <= 4 && back <= seq; ++back)
    {
      const int q = (int)((seq - back) & 3), rsi = stream_of[q];
      if (!seen[rsi]) { seen[rsi] = true; slots[count++] = q; }
    }
    return count;
  }
  void joined() { open = false; seq = 0; }
};

// ---- pipelined syntheses (stateless): two streams in turn ------------------------------------------------------------------
struct InverseStreams
{
  Range y[2];                              // the samples the last synthesis on each row stream writes
  bool used[2] = {false, false};
  int last = 1;
  struct Pick { int stream = 0; bool wait_other = false; };
  // the other stream than the previous synthesis -- the same one if the two write overlapping samples; what the OTHER row
  // stream still has outstanding (samples this call overwrites, or a matrix reinterpreted from them) is waited for
  Pick pick(const Range& yr, const Range& in) const
  {
    Pick p;
    p.stream = overlap(yr, y[last]) ? last : (last ^ 1);
    const int so = p.stream ^ 1;
    p.wait_other = used[so] && (overlap(yr, y[so]) || overlap(in, y[so]));
    return p;
  }
  void launched(int stream, const Range& yr) { used[stream] = true; last = stream; y[stream] = yr; }
};

// ---- calls of one time chunk: time parts -------------------------------------------------------------------------------------
// forward_hop2_kernel: every (tile, part) a workgroup on a CU of its own; as many parts as leave every workgroup a CU, at
// least 12 samples each; a synchronous call waits for the completion word, which the LAST of all workgroups sets after a
// ticket each: at most 4 parts there, 8 otherwise (profiles/r05_hop_time_parts.txt)
struct HopParts { unsigned parts = 1, part_len = 0; };
inline HopParts hop_parts(size_t n, unsigned long long tile_waves, int compute_units, long forced, bool waits_for_word)
{
  HopParts h; h.parts = 1; h.part_len = (unsigned)n;
  if (forced == 1 || n < 24) return h;
  const size_t room = std::max<size_t>(1, (size_t)std::max(compute_units, 1) / (size_t)std::max<unsigned long long>(1, tile_waves));
  const size_t most = waits_for_word ? 4 : 8;
  size_t parts = forced > 1 ? (size_t)forced : std::min<size_t>({most, room, n / 12});
  parts = std::max<size_t>(1, std::min(parts, n));
  const size_t plen = (n + parts - 1) / parts;
  h.part_len = (unsigned)plen; h.parts = (unsigned)((n + plen - 1) / plen);
  return h;
}

// ---- synthesis in the reference's order: rows per wave ---------------------------------------------------------------------
// 32 rows per wave for long FD-double calls, 16 for FD float and medium calls, 4 with an 8-deep ring below 64 Ki rows, one
// wave per row up to 1024 rows; where 4 rows per wave need a second, partly filled round of the chip and 8 rows per wave fit
// in one (capacities from the occupancy API), the 8-row form (profiles/r04_synthesis_rows_per_wave.txt)
inline long inverse_rows_per_wave(size_t total_rows, size_t fd_bytes, long forced, size_t capacity4, size_t capacity8, bool with_operation)
{
  long rw = forced > 0 ? forced : (total_rows <= 1024 ? 1 : total_rows < 65536 ? 4 : ((fd_bytes == 8 && total_rows >= (size_t)32 * 8192) ? 32 : 16));
  if (!with_operation && forced <= 0 && rw == 4 && capacity4 && capacity8)
  {
    const size_t groups4 = (total_rows + 3) / 4, groups8 = (total_rows + 7) / 8;
    if (groups4 > capacity4 && groups8 <= capacity8) rw = 8;
  }
  if (with_operation && rw != 1) rw = 16;                    // one streaming instantiation with the operation built in
  return rw;
}

// ---- which of several bit-identical kernel forms is the fastest HERE: measured on the calls themselves ---------------------
// The streaming synthesis has forms that give the same bits and differ by a few per cent either way from box to box (rows per
// wave, bytes per row segment, tree sum with the rounding-interval proof): round 4's fixed switch points were right on one
// lease and wrong on the next.  A host that repeats a call shape lets the plan find out: the first calls of the shape take
// the candidate forms in turn, each bracketed by a pair of events (two samples per form, the smaller one counts), then the
// fastest form serves the shape.  Until a sample's events have completed no new trial starts (the calls in between take
// form 0, the static choice, untimed); a new shape starts over.
struct FormTuner
{
  static constexpr int kMax = 6, kSamples = 2;
  size_t key = 0;
  int count = 0, chosen = -1;
  int samples[kMax] = {};
  bool inflight[kMax] = {};                                // a timed call of this form has been launched and not yet reported
  float best[kMax] = {};
  void reset(size_t k, int candidates)
  {
    key = k; count = candidates < 1 ? 1 : (candidates > kMax ? kMax : candidates); chosen = count == 1 ? 0 : -1;
    for (int i = 0; i < kMax; ++i) { samples[i] = 0; best[i] = 0.f; inflight[i] = false; }
  }
  // the form this call takes; timed: the caller brackets the launch with the form's pair of events, calls launched() and
  // reports the time once the events have completed (a host that queues calls faster than they run has several trials in
  // flight, one per form)
  int next(bool can_time, bool& timed)
  {
    timed = false;
    if (chosen >= 0) return chosen;
    int want = -1, open = 0;
    for (int i = 0; i < count; ++i)
    {
      if (samples[i] < kSamples) ++open;
      if (samples[i] < kSamples && !inflight[i] && (want < 0 || samples[i] < samples[want])) want = i;
    }
    if (open == 0)
    {
      chosen = 0;
      for (int i = 1; i < count; ++i) if (best[i] < best[chosen]) chosen = i;
      return chosen;
    }
    if (!can_time || want < 0) return 0;                      // (every open form is in flight: the static form, untimed)
    timed = true;
    return want;
  }
  void launched(int form) { if (form >= 0 && form < count) inflight[form] = true; }
  void report(int form, float ms)
  {
    if (form < 0 || form >= count) return;
    inflight[form] = false;
    if (!(ms > 0.f)) return;
    best[form] = samples[form] == 0 ? ms : (ms < best[form] ? ms : best[form]);
    ++samples[form];
  }
};

// A host may alternate between a few call lengths (hops of two sizes; staged host-pointer calls that end in a shorter tail segment): one tuner per
// kind of call would start over at candidate 0 on every change of shape and never settle.  A small table of tuners keyed by the shape, least recently
// used replaced: a shape that has decided stays decided while up to kSlots shapes interleave.
struct TunerTable
{
  static constexpr int kSlots = 3;
  FormTuner slot[kSlots];
  unsigned long stamp[kSlots] = {};                        // 0: never used
  unsigned long clock = 0;
  int find(size_t key, int candidates)
  {
    const int count = candidates < 1 ? 1 : (candidates > FormTuner::kMax ? FormTuner::kMax : candidates);
    int lru = 0;
    for (int i = 0; i < kSlots; ++i)
    {
      if (stamp[i] && slot[i].key == key && slot[i].count == count) { stamp[i] = ++clock; return i; }
      if (stamp[i] < stamp[lru]) lru = i;
    }
    slot[lru].reset(key, candidates);
    stamp[lru] = ++clock;
    return lru;
  }
  void reset_all() { for (int i = 0; i < kSlots; ++i) { slot[i].reset(0, 1); stamp[i] = 0; } clock = 0; }
};

// ---- pipelined analyses: where they pay ------------------------------------------------------------------------------------------
// The next call's workgroups fill what a launch leaves idle -- the launch gap, the prologue of the self-carried chunks, the ragged end: a fixed 20-30 us
// per call.  Interleaved in one process on two equally placed matrices (profiles/r06_pipelined_calls.txt): n = 24 000 +12 %, n = 48 000 +9 % (82 against
// 75 % of the HBM peak), n = 90 000 +6 %, n = 131 072 +11 % (85 against 76 %), n = 1e6 a tie (85 %: 2.4 ms per call amortise what pipelining hides, and the
// call's own cut -- two rounds of shorter chunks -- is as good as the pipelined one).  So: calls of less than 2^29 bins (half a million rows of 1024 bins,
// about a millisecond of store stream) by default.
// option: 0 never, 1 (default) calls below that size, 2 calls of any length.
constexpr size_t kPipelineBinsMax = (size_t)1 << 29;
inline bool pipeline_pays(const ChunkQuery& q, long option)
{
  if (option <= 0) return false;
  if (option >= 2) return true;
  return std::max<size_t>(q.channels, 1) * q.n * q.nbins < kPipelineBinsMax;
}

// ---- synthesis: are the matrix' loads non-temporal? ------------------------------------------------------------------------------
// Beyond 256 MiB (what fits the Infinity Cache reads faster through it).  Round 4 had stopped at 4 GiB, where non-temporal loads of a just-written
// matrix were 5 % slower; round 5 found why -- a non-temporal load of a line that sits DIRTY in the cache is slow -- and reads the rows that may be
// dirty with ordinary loads (inverse_ordinary_rows below): with that, non-temporal loads win on every matrix measured, just written or only read, by
// 3-10 % (profiles/r05_synthesis_streaming_loads_big.txt, r05_after_write_16gb.txt).  forced: the option (-1 = by size).
inline bool inverse_streaming_loads(size_t matrix_bytes, long forced)
{
  if (forced >= 0) return forced != 0;
  return matrix_bytes > ((size_t)256 << 20);
}

// ... and how many of the rows a synthesis reads FIRST (the matrix' end) take ordinary loads whatever the kind of load: a non-temporal load of a line that
// sits dirty in the 256 MiB Infinity Cache (what an analysis wrote last) is slow; ordinary loads of such lines are not, and 1.5 GB of them push everything
// dirty out on the way.  n = 1e6 x 1024 (16.4 GB), rows in step: after the analysis 2.74 (all non-temporal) / 2.75 (all ordinary) -> 2.55 ms, only read 2.45
// either way (profiles/r05_after_write_16gb.txt).  Matrices from 6 GiB on (below, none: 706 MB ... 2.1 GB read best without; around 4 GiB it depends on
// the form, which the tuner finds out); forced_mb: the option (-1 = this rule, 0 = none).
inline size_t inverse_ordinary_rows(size_t matrix_bytes, size_t row_bytes, long forced_mb)
{
  if (row_bytes == 0) return 0;
  const size_t mb = forced_mb >= 0 ? (size_t)forced_mb : (matrix_bytes >= ((size_t)6 << 30) ? (size_t)1536 : 0);
  return mb ? ((mb << 20) + row_bytes - 1) / row_bytes : 0;
}

// ---- fused call: waves of a workgroup and bins per lane (1, 2, 4) -----------------------------------------------------------
struct ProcessGeometry { long waves = 1, slots = 1; };
inline ProcessGeometry process_geometry(size_t nbins, size_t channels, size_t n, bool fused, size_t fd_bytes, long forced_slots)
{
  ProcessGeometry g;
  g.waves = std::min<long>(kRowWaves, (long)((nbins + kLanes - 1) / kLanes));
  const long want = forced_slots > 0 ? forced_slots : ((fused && fd_bytes == 8 && nbins >= 256) ? ((nbins >= 512 && channels * n >= 400000) ? 4 : 2) : 1);
  if (want > 1) g.waves = std::max(1L, std::min(g.waves, (long)((nbins + (size_t)(kLanes * want) - 1) / (size_t)(kLanes * want))));
  g.slots = (long)((nbins + (size_t)g.waves * kLanes - 1) / ((size_t)g.waves * kLanes));
  return g;
}

// ---- analysis: the route of a call (Plan::forward_launch runs it) ------------------------------------------------------------
constexpr int kWavesPerBlock = 4;                  // waves of a tile-kernel workgroup (kWavesPerBlock)
constexpr int kProcGroup = 8, kProcRow = 72;       // the fused kernel's transpose tile: samples per group, row stride (kProcGroup, kProcRow)
// (beyond kSelfMax a row-group analysis call takes the same kernel with the fold done once for all chunks by a pre-pass launch:
// ForwardRoute::prefix; the fused call and every shape without the self-carried form keep the partial sums + scan)
// That launch (prefix_cells_kernel) adds the n / 2N differences of a cell one after the other, on 2N / 32 workgroups per channel:
// every 512 rows of a cell are one load phase and 32 turns of 16 dependent additions through LDS, so its time grows with the rows
// per cell, which the partial sums + scan (parallel over the chunks, tens of microseconds whatever the length) do not.  The route
// is therefore bounded by rows per cell, kPrefixRowsMax = 9 passes of 512 rows; beyond it the partial sums + scan stay.
// MEASURED so far: the headline alone, 489 rows per cell, one pass: the launch takes 17 us where the partial sums + scan take 44 us
// (profiles/prefix_cells_ab.txt).  The bound itself is REASONED from that one figure: nine passes, about
// 5 us each, cost about what the partial sums + scan cost, and nine passes is the smallest bound under which m = 64 just beyond kSelfMax (4128
// rows) keeps the route.  scripts/prefix_cells_rows_ab.py measures both pre-passes from 258 to 625 000 rows per cell and is what
// should move this constant; its table has not been recorded yet.
constexpr size_t kPrefixRowsMax = 9 * 512;
inline size_t prefix_rows(size_t n, size_t nbins) { return (n + 2 * nbins - 1) / (2 * nbins); }   // rows per cell: the depth of prefix_cells_kernel's chain
constexpr size_t kSelfMax = (size_t)1 << 19;       // self-carried chunks for calls of up to this many samples per channel (the fold of a chunk's past grows with n) ...
constexpr size_t kSelfMaxFused = (size_t)1 << 16;  // ... of the fused call, which is bound by instruction issue (n = 131072: 99 -> 117 us self-carried)
constexpr size_t kFlagMax = (size_t)1 << 24;       // bin-samples up to which a row-group analysis call signals its own completion ...
constexpr size_t kFlagMaxFused = (size_t)1 << 26;  // ... and a fused call
constexpr size_t kPipelineBinsMin = (size_t)6 << 20;   // bin-samples from which a call may leave the plan's stream (analysis and synthesis)
constexpr size_t kSumsLds = (size_t)64 * 1024;     // LDS of a workgroup of the FFT forms of the chunk partial sums

// relays of the exact carries (32 bins of a channel each) = waves of the serial pass per channel
inline size_t relays(size_t nbins) { return (nbins + kLanes / 2 - 1) / (kLanes / 2); }

struct ForwardQuery
{
  size_t n = 0, nbins = 0, channels = 1, fd_bytes = 8, fdx_bytes = 16;
  int window = kWindowHann, compute_units = 256;
  size_t cursor = 0;
  bool exact = false;                     // exact carries (carry mode)
  bool fid_canonical = true;              // fid is on the canonical rotation sequence (the relay form's seed table)
  bool fuse = false, fuse_store = false;  // the fused call; it stores the processed spectrum too
  bool reference_order = false;           // the fused call sums bins in the reference's order
  bool coeff_ready = false;               // the fused call's folded coefficients are built
  bool every = false;                     // decimated analysis (forward_every_kernel)
  bool power = false;                     // power-spectrogram analysis (forward_power_kernel) on a grid of ...
  size_t power_every = 1;                 // ... every power_every-th sample
  bool power_sum = false;                 // pooled power analysis (forward_pooled_power_kernel)
  bool power_peak = false;                // peak-hold analysis (forward_power_peak_kernel): the pooled power call's route (never with power_sum)
  bool lag_sum = false;                   // lag-product analysis (forward_lag_sum_kernel): the pooled power call's route (never with power_sum or power_peak)
  bool power_moments = false;             // power-moments analysis (forward_power_moments_kernel): the pooled power call's route and chunk choice (never with power_sum, power_peak or lag_sum)
  bool power_smooth = false;              // smoothed power analysis (forward_power_smooth_kernel): the pooled power call's route and chunk choice (never with another of these)
  bool filterbank = false;                // filterbank analysis (forward_filterbank_kernel) on the grid of power_every
  bool band_peak = false;                 // band-peak analysis (forward_band_peak_kernel) on the grid of power_every: the filterbank call's route and chunk choice (never with filterbank)
  bool cross_sum = false;                 // pooled cross-spectrum analysis (forward_cross_sum_kernel) of ...
  size_t cross_items = 0;                 // ... this many work items (logic::cross_items), which take the channels' place in the launch
  bool smooth_peak = false;               // smoothed peak-hold analysis (forward_smooth_peak_kernel): the pooled power call's route and chunk choice (never with another of these)
  bool cross_smooth = false;              // smoothed cross-spectrum analysis (forward_cross_smooth_kernel): cross_sum's items, route and chunk choice (never with cross_sum)
  bool covariance = false;                // array covariance analysis (forward_covariance_kernel): cross_items counts its block items (logic::covariance_items)
  bool mix = false;                       // channel-mix analysis (forward_mix_kernel) on the grid of power_every: cross_items counts its items (logic::mix_items)
  bool row_pointers = false;              // rows go to a table of row pointers
  uintptr_t out = 0; size_t out_stride = 0;
  bool analysis_batch = false;            // CallPattern: analyses come call after call
  bool pipe_wanted = false;               // Plan::pipe_wanted: the plan and the call may leave the plan's stream
  Range prev_out;                         // the matrix of the previous dense row-group analysis
  // options
  long rows_kernel = 1, row_slots_max = 2, interior = 0, chunk = 0, self = 1, fused = 1, fold = 1, fft_carry = 1, hop_kernel = 1, chain = 1,
       chain_L = 0, relay_flow = 1, segments = 0, xcd_map = 1, rows_f32 = 1, pipeline = 1;
  long prefix_cells = 1;                  // test hook: 0 = never the prefix-cell route, 1 = calls beyond kSelfMax, 2 = whatever the length
};
enum ForwardKernel : int { FK_TILES = 1, FK_ROWS = 2, FK_HOP = 3, FK_EVERY = 4, FK_POWER = 5, FK_POWER_SUM = 6, FK_FILTERBANK = 7, FK_CROSS_SUM = 8, FK_COVARIANCE = 9, FK_MIX = 10, FK_POWER_PEAK = 11, FK_LAG_SUM = 12, FK_POWER_MOMENTS = 13, FK_BAND_PEAK = 14, FK_POWER_SMOOTH = 15, FK_CROSS_SMOOTH = 16, FK_SMOOTH_PEAK = 17 };     // = get_option "last_kernel"
// carries: the single chunk's are the stream state (delta_kernel copies it); pre-pass partial sums + scan (carries from the
// closed-form table); the serial exact pass (carry_exact_kernel); the relay form of the exact pass (carry_relay_kernel)
enum CarryForm : int { CARRY_STATE = 0, CARRY_SUMS = 1, CARRY_SERIAL = 2, CARRY_RELAY = 3 };
enum SumsForm : int { SUMS_NONE = -1, SUMS_DIRECT = 0, SUMS_FFT2 = 1, SUMS_FFT_MIXED = 2 };
struct ForwardRoute
{
  int kernel = FK_TILES;                  // FK_HOP: forward_hop takes the call
  bool self = false;                      // forward_self takes the call
  bool prefix = false;                    // forward_self takes the call with the folded cells of all chunks from one pre-pass launch (prefix_cells_kernel); never with self
  bool pipelined = false;                 // ... on the two row streams (Plan::pipe_this)
  Range out;                              // the matrix of a dense row-group analysis (the next call's prev_out), else empty
  long chunks = 1, len = 0, tiles = 1, interior = 1;
  unsigned relay_L = 0, shift = 0;        // CARRY_RELAY: block length; chunk j starts at sample j * len - shift
  long segments = 1;                      // time segments of the exact carries (serial pass on the side stream)
  bool flow = false;                      // relay form, flow mode: one relay launch, forward workgroups wait chunk by chunk
  int carry = CARRY_STATE, sums = SUMS_NONE;
  bool delta_in_carry = false;            // the partial-sums kernel forms the differences (no delta_kernel)
  bool use_seed = true;                   // fid comes from the serial rotation (else the closed-form table)
  bool fused = false;                     // fused multiply-add arithmetic (FD double, carries from the pre-pass)
  bool folded = false;                    // the fused call's folded form (process_rows_kernel)
  bool vec_store = false, rows_f32 = false, arm_flag = false, xcd_map = false;
};

// what the self-carried form needs of the plan and the call (the kernel that has it is chosen by the caller)
// (any_length: pipelined calls take the form whatever the length -- one stream runs long calls faster with the pre-pass,
// n = 1e6: 77.3 against 75.5 % of peak, but two matrices in turn, pipelined: 82.4 %)
inline bool self_eligible(const ForwardQuery& q, bool fused_call, bool any_length)
{
  const size_t most = fused_call ? std::min(kSelfMax, kSelfMaxFused) : kSelfMax;
  return q.fd_bytes == 8 && !q.exact && q.self && self_cells(q.nbins, q.self >= 1, q.fdx_bytes) != 0 && (q.n <= most || any_length);
}
inline ChunkQuery chunk_query(const ForwardQuery& q, bool rows_kernel, bool pipelined)
{
  ChunkQuery c;
  c.n = q.n; c.channels = q.channels; c.nbins = q.nbins; c.rows_kernel = rows_kernel; c.exact = q.exact; c.pipelined = pipelined;
  c.forced_chunk = q.chunk; c.row_waves = row_waves(q.nbins, q.fdx_bytes); c.tiles = tiles(q.nbins, q.window, q.fdx_bytes, q.interior);
  c.compute_units = q.compute_units;
  return c;
}

// gate_ok(): Plan::gate_ok (allocates the relays' start word on first use), asked only where flow mode is otherwise wanted
template <class GateOk>
inline ForwardRoute forward_route(const ForwardQuery& q, GateOk&& gate_ok)
{
  ForwardRoute r;
  const size_t nb = q.nbins, span = 2 * nb, n = q.n, ch = std::max<size_t>(q.channels, 1);
  const bool pow2 = (span & (span - 1)) == 0;
  // the decimated, the power-spectrogram, the pooled power, the peak-hold, the lag-product, the power-moments, the smoothed power, the filterbank, the band-peak, the cross-spectrum, the smoothed cross-spectrum, the smoothed peak-hold, the covariance and the mix analysis have the tile form only
  const bool grid = q.every || q.power || q.power_sum || q.power_peak || q.lag_sum || q.power_moments || q.power_smooth || q.smooth_peak || q.filterbank || q.band_peak || q.cross_sum || q.cross_smooth || q.covariance || q.mix;
  // (channel, chunk) groups of a tile launch per chunk: the two cross-spectrum, the covariance and the mix call's are their work items
  const size_t lanes = (q.cross_sum || q.cross_smooth || q.covariance || q.mix) ? std::max<size_t>(q.cross_items, 1) : ch;
  const bool rows = !grid && rows_kernel_ok(nb, q.fdx_bytes, q.row_pointers, q.rows_kernel != 0, q.row_slots_max);
  const bool folded = q.fuse && !q.reference_order && !q.fuse_store && q.fold && q.coeff_ready;
  // pipelined calls (forward_self): decided first because they take the self-carried form at any length and cut time differently
  // (calls of a few thousand rows gain a microsecond from it and cost the host seven runtime calls instead of one,
  // 19 against 3 us: n = 4096, m = 1024: 25.6 against 26.4 us per call; from n = 8192 on 30.4 against 32.9)
  if (!q.fuse && !q.row_pointers && q.out && rows)
  {
    r.out = Range{q.out, q.out + ((ch - 1) * q.out_stride + n * nb) * q.fdx_bytes};
    r.pipelined = q.analysis_batch && q.pipe_wanted && self_eligible(q, false, true) && n < ((size_t)1 << 31) && ch * n * nb >= kPipelineBinsMin &&
                  !overlap(r.out, q.prev_out) && pipeline_pays(chunk_query(q, true, false), q.pipeline);
  }
  // (the folded fused kernel and the row-group forward kernel have the self-carried form)
  bool self_form = self_eligible(q, q.fuse, r.pipelined) && (q.fuse ? folded : rows);
  if (self_form && q.fuse)
  {
    // the fused kernel folds into its transpose tiles: the 2N cells have to fit them, and it has one or two bins per lane
    const ProcessGeometry g = process_geometry(nb, ch, n, q.fused != 0, q.fd_bytes, 0);
    self_form = g.slots <= 2 && self_cells(nb, q.self >= 1, q.fdx_bytes) * q.fdx_bytes <= (size_t)g.waves * kProcGroup * kProcRow * sizeof(double);
  }
  if (!self_form) r.pipelined = false;
  Chunking c;
  if (grid)
  {
    EveryQuery e;
    e.n = n; e.channels = lanes; e.tiles = tiles(nb, q.window, q.fdx_bytes, q.interior); e.exact = q.exact; e.forced_chunk = q.chunk; e.compute_units = q.compute_units;
    c = (q.power_sum || q.power_peak || q.lag_sum || q.power_moments || q.power_smooth || q.smooth_peak || q.cross_sum || q.cross_smooth || q.covariance) ? choose_power_sum_chunks(e) : (q.power || q.filterbank || q.band_peak || q.mix) ? choose_power_chunks(e, q.power_every) : choose_every_chunks(e);
  }
  else c = choose_chunks(chunk_query(q, rows, r.pipelined));
  r.chunks = c.chunks; r.len = c.len;
  r.tiles = tiles(nb, q.window, q.fdx_bytes, q.interior); r.interior = interior_lanes(q.window, q.fdx_bytes, q.interior);
  r.kernel = q.mix ? FK_MIX : q.covariance ? FK_COVARIANCE : q.cross_smooth ? FK_CROSS_SMOOTH : q.cross_sum ? FK_CROSS_SUM : q.filterbank ? FK_FILTERBANK : q.band_peak ? FK_BAND_PEAK : q.smooth_peak ? FK_SMOOTH_PEAK : q.power_smooth ? FK_POWER_SMOOTH : q.power_moments ? FK_POWER_MOMENTS : q.lag_sum ? FK_LAG_SUM : q.power_peak ? FK_POWER_PEAK : q.power_sum ? FK_POWER_SUM : q.power ? FK_POWER : q.every ? FK_EVERY : rows ? FK_ROWS : FK_TILES;
  if (r.chunks == 1 && q.hop_kernel && nb >= 2 && !q.fuse && !grid) { r.kernel = FK_HOP; return r; }

  // self-carried chunks: every workgroup derives its carry-in from the raw samples (fold + one FFT in LDS) and forms
  // its own differences -- the call is ONE launch.  Kernels that have the form: the row-group forward kernel and the
  // folded fused kernel, FD double, 2N a power of two of at most 4096 cells.
  // (the fold of a chunk's past costs t0 / threads loads: hidden behind the other workgroups' row stores in the
  // analysis, which is bound by HBM -- n = 1e6: 2.885 -> 2.853 ms -- but not in the fused call, which is bound by
  // instruction issue: n = 48000: 45.9 -> 42.3 us, n = 131072: 99 -> 117 us; hence kSelfMaxFused)
  // (2N = 2/3/5-smooth: five Stockham stages with table look-ups -- n = 12000, N = 1000, chunks of 64 samples: 47 us with
  // the pre-pass, 55 us self-carried; n = 48000, chunks of 192: 192 -> 173 us)
  // Beyond kSelfMax (where the fold costs more than the other workgroups' stores hide) the fold is done ONCE: it is a prefix over
  // time of one real number per cursor, which one small launch writes for all chunks (prefix_cells_kernel); the row-group kernel
  // then reads its 2N cells instead of folding them and goes on as a self-carried chunk (FFT in LDS, own differences).  The fused
  // and the pipelined calls keep their forms, and so does every call of more than kPrefixRowsMax rows per cell.
  r.prefix = rows && !q.fuse && !r.pipelined && q.fd_bytes == 8 && !q.exact && q.self != 0 && self_cells(nb, q.self >= 1, q.fdx_bytes) != 0 &&
             q.prefix_cells != 0 && ((n > kSelfMax && prefix_rows(n, nb) <= kPrefixRowsMax) || q.prefix_cells == 2) && r.chunks > 1 && (pow2 || r.len > 64);
  // (a flag on top of the route below: Plan::forward_launch asks for it first and runs forward_self.  carry, sums, delta_in_carry,
  // use_seed and fused go on naming the partial sums + scan the same call takes without the flag -- tests/cpp/plan_logic_test.cpp
  // pins them for the headline and allows fused arithmetic only beside CARRY_SUMS -- and nothing reads them for a prefix call)
  r.self = self_form && !r.prefix && r.chunks > 1 && (pow2 || r.len > 64);
  if (r.self) return r;

  // exact carries: relay form (seed table + identical waves that take the blocks of L steps in turn, a block's products in
  // registers) while the serial pass would leave most SIMDs idle; the plain serial pass when bins x channels already
  // fill the chip.  The chunk grid is shifted so that every chunk but the first starts on a block boundary of the
  // cursor (chunk j starts at sample j*len - shift; one more chunk may be needed for the tail)
  const bool chain_ok = q.exact && r.chunks > 1 && q.chain && q.fid_canonical && (q.chain >= 2 || relays(nb) * ch <= 1024);
  r.relay_L = (chain_ok && n < ((size_t)1 << 31)) ? relay_block(nb, r.len, q.fd_bytes, q.fdx_bytes, q.chain_L) : 0u;
  if (r.relay_L)
  {
    r.shift = (unsigned)(q.cursor % r.relay_L);
    if (r.shift) r.chunks = (long)((n + r.shift + (size_t)r.len - 1) / (size_t)r.len);
  }
  if (r.chunks == 1) r.carry = CARRY_STATE;
  else if (q.exact) r.carry = r.relay_L ? CARRY_RELAY : CARRY_SERIAL;
  else
  {
    // form of the chunk-parallel partial sums: FFT when 2N is a power of two or 2/3/5-smooth (and fits LDS) -- but
    // direct sums for chunks of up to 64 samples, which need no barriers (n = 1024 / 4096, N = 1024: 28.0 / 32.1 ->
    // 24.2 / 28.3 us per call even with one launch more) -- and direct sums for every other size
    r.carry = CARRY_SUMS;
    const size_t span_bytes = span * q.fdx_bytes;
    const bool fft = q.fft_carry && !(r.len <= 64 && q.fft_carry != 2);
    if (fft && pow2 && span_bytes <= kSumsLds) r.sums = SUMS_FFT2;
    else if (fft && !pow2 && smooth_radices(span).count > 0 && 2 * span_bytes <= kSumsLds) r.sums = SUMS_FFT_MIXED;
    else r.sums = SUMS_DIRECT;
  }
  r.delta_in_carry = r.carry == CARRY_SUMS;                // K0: differences + delay line -- unless the partial sums form them
  r.use_seed = r.carry != CARRY_SUMS;
  if (r.carry == CARRY_SERIAL || r.carry == CARRY_RELAY)
  {
    // time segments: the serial pass of segment s+1 (few waves, latency-bound) runs on the side stream while the forward kernel
    // of segment s streams the matrix; up to 8 segments, each forward launch still filling the chip (>= 256 workgroups)
    const long launch_blocks = rows ? (long)ch * r.chunks : (long)lanes * r.chunks * r.tiles / kWavesPerBlock;
    r.segments = q.segments > 0 ? q.segments : std::max(1L, std::min(8L, launch_blocks / 256));
    // Relay form, flow mode: ONE relay launch for the whole call on the side stream and ONE forward launch whose workgroups wait
    // for their chunk's carries themselves (ForwardArgs::ready).  With segments and events the two passes barely overlap:
    // a 16-wave forward workgroup fills a CU's registers, so the relays of segment s+1 wait until the forward launch of
    // segment s has drained (config 3: chain 0.71 ms alone + forward 1.55 ms alone = 2.2 ms together).  Here the relays
    // hold their CUs from the start, the forward workgroups take whatever is free, in time order, and the whole chip
    // once the relays are through.  The forward launch is held back (relay_gate_kernel polls a word every relay workgroup
    // bumps at its start) until the relays are resident: a forward workgroup that waits for a relay which cannot start
    // would be a deadlock -- every wait in the kernels is bounded all the same, and a time-out re-runs the call (forward_device).
    r.flow = r.relay_L && q.relay_flow && q.segments <= 0 && (q.fuse || rows) && !grid && gate_ok();
    if (r.flow) r.segments = 1;
    r.segments = std::max(1L, std::min(r.segments, r.chunks));
  }
  // fused arithmetic only where the result is not claimed bit-identical: FD double with carries from the pre-pass
  r.fused = (rows || q.fuse) && q.fused && q.fd_bytes == 8 && !r.use_seed;
  r.folded = folded;
  r.vec_store = bins_per_lane(q.fdx_bytes) == 2 && nb % 2 == 0 && q.out % 16 == 0 && q.out_stride % 2 == 0 && !q.row_pointers;
  // FD float, rows of a multiple of 128 bins, dense aligned output: the bin-pair kernel (sdft_forward_rows_f32.hpp)
  r.rows_f32 = rows && !q.fuse && q.fd_bytes == 4 && q.rows_f32 && nb % (2 * kLanes) == 0 && r.vec_store;
  // short synchronous calls: the row-group kernels report their own completion (a word in pinned host memory
  // reaches the host before the stream does).  Worth it while the kernel has little to write back: n = 4096,
  // N = 1024: 49.7 -> 46.7 us per sdft_sdft_n, 40.4 -> 35.8 us per fused call; nothing at n = 48000.
  r.arm_flag = (rows || q.fuse) && r.segments == 1 && ch * n * nb <= (q.fuse ? kFlagMaxFused : kFlagMax);
  r.xcd_map = q.xcd_map && !r.flow;
  return r;
}
// ForwardArgs::xcd_map of a launch of `groups` (channel, chunk) workgroups
inline unsigned xcd_groups(bool on, size_t groups) { return (on && groups >= 16) ? (unsigned)groups : 0u; }

// ---- synthesis: the form of a call (Plan::launch_inverse runs it) --------------------------------------------------------------
constexpr size_t kInverseVerifyMax = 500000;      // rows up to which the tree sum with the rounding-interval proof serves sdft_isdft_n (beyond: the streaming kernel)
// the bit-identical forms (the numbering is get_option "last_inverse_tuned", + 10 once the tuner has settled) and two static ones:
// the tree sum without the reference's order (option exact_inverse = 0) and one wave per row
enum InverseForm : int { F_VERIFY = 0, F_32 = 1, F_16 = 2, F_16W = 3, F_8 = 4, F_4 = 5, F_STEP = 6, F_ORDERED = 7, F_8W = 8, F_TREE = 9, F_ROW = 10 };
// get_option "last_inverse_form": 0 tree sum, 1 streaming rows, 2 tree sum with the proof, 3 rows in step, 4 ordered rows
inline long inverse_form_code(int form) { return form == F_TREE ? 0 : form == F_VERIFY ? 2 : form == F_STEP ? 3 : form == F_ORDERED ? 4 : 1; }
inline long inverse_tuned_code(int form, bool settled) { return 10 * (settled ? 1 : 0) + form; }
// rows per wave of the streaming forms (what sizes their grid)
inline long inverse_form_rows(int form)
{
  return form == F_32 ? 32 : (form == F_16 || form == F_16W) ? 16 : (form == F_8 || form == F_8W) ? 8 : form == F_4 ? 4 : 1;
}

struct InverseQuery
{
  size_t n = 0, channels = 1, nbins = 0, td_bytes = 4, fd_bytes = 8;
  size_t in_stride = 0, y_stride = 0;
  uintptr_t in = 0;
  bool row_pointers = false, lat1 = true, ops = false;
  bool nt = false; size_t nt_skip = 0;                 // the matrix's loads are non-temporal but for its first nt_skip rows
  size_t capacity4 = 0, capacity8 = 0;                 // Plan::inverse_capacity as it stands (0: not asked yet)
  bool ordered_failed = false;                         // the static ordered launch did not go: the route without it
  // options
  long exact = 1, rows = 0, step = 0, ordered = 0, tune = 1, verify = 1, nt_skip_mb = -1;
};
struct InverseCandidate { int form = F_VERIFY; size_t nt_skip = 0; };
struct InverseRoute
{
  int form = F_TREE;                                   // the static form (tuned == false) ...
  long rows_per_wave = 1;                              // ... and its rows per wave (F_32 ... F_4 take forced ones as well: option inverse_rows)
  bool tuned = false;                                  // the tuner picks among the candidates; entry 0 is the static choice
  int count = 0;
  InverseCandidate cand[FormTuner::kMax];
};

// rows in step (inverse_rows_body): float samples from double bins at latency 1 (the term of a bin is +-re: one register per
// bin in flight; the general term needs both halves and the kernel's three groups in flight no longer fit 64 registers),
// dense rows of 64 ... 2048 bins; a form of the rounding-interval proof (option inverse_verify = 0 turns it off with the other one)
inline bool rows_in_step_ok(const InverseQuery& q)
{
  const size_t rows = q.channels * q.n;
  return q.lat1 && q.td_bytes == 4 && q.fd_bytes == 8 && q.verify && !q.row_pointers && q.nbins >= 64 && q.nbins <= 2048 && rows >= 64 && rows <= 0x7fffffffull * 4;
}
// whole rows, ordered sum (inverse_rows_ordered_kernel): every type pair, any latency; rows in one run (one channel, or channels
// without a gap between them), 16-byte loads -- and rows that fit the kernel's LDS (ordered_geometry(): ordered_rows_geometry::make)
template <class OrderedGeometry>
inline bool rows_ordered_ok(const InverseQuery& q, OrderedGeometry&& ordered_geometry)
{
  const size_t rows = q.channels * q.n;
  const bool one_run = q.channels == 1 || (q.in_stride == q.n * q.nbins && q.y_stride == q.n);
  const bool loads_ok = (q.in & 15) == 0 && (q.fd_bytes == 8 || q.nbins % 2 == 0);
  return !q.row_pointers && one_run && loads_ok && rows >= 64 && rows <= 0x7fffffffull && ordered_geometry();
}

// ordered_geometry(): as above; tune_events(): Plan::ensure_tune_events (creates the tuner's events on first use);
// capacity(c4, c8): Plan's occupancy query for the 4-row and the 8-row form.  Each is asked only where the route needs it.
template <class OrderedGeometry, class TuneEvents, class Capacity>
inline InverseRoute inverse_route(const InverseQuery& q, OrderedGeometry&& ordered_geometry, TuneEvents&& tune_events, Capacity&& capacity)
{
  InverseRoute r;
  const size_t rows = q.channels * q.n;
  const double matrix_bytes = (double)rows * (double)q.nbins * (double)(2 * q.fd_bytes);
  const bool exact_rows = q.exact && q.rows <= 0;      // the reference's order, rows per wave not forced
  const bool step_ok = rows_in_step_ok(q);
  // matrices from 6 GB on: the static choice too (n = 5e5 ... 1e6 x 1024, 64 x 48000 x 1024 / 2048, 250000 x 2048: +5 ... +10 % over
  // the best streaming form; 4 GB: a tie; below: the streaming forms, by up to 12 % -- profiles/r05_synthesis_rows_in_step.txt)
  const bool step_static = q.step >= 0 && step_ok && matrix_bytes >= 6.0e9;
  // (whole rows with the ordered sum: 6.85 TB/s at n = 1e6 x 1024 for every type pair -- rows in step 6.54, the tiles 5.8 ... 6.35;
  // profiles/r06_synthesis_forms.txt)
  const bool ordered_ok = !q.ops && exact_rows && q.ordered >= 0 && rows_ordered_ok(q, ordered_geometry);
  const bool ordered_static = ordered_ok && matrix_bytes >= 7.0e8;      // (48 000 x 1024 double bins: 6.1 TB/s against 5.7 for the best of the tiles; 200 000: 6.65 against 6.2)
  if (!q.ops)
  {
    const bool step_forced = exact_rows && q.step == 1 && q.ordered != 1 && step_ok;
    if (!q.ordered_failed && ordered_ok && !step_forced && (q.ordered == 1 || (ordered_static && !q.tune))) { r.form = F_ORDERED; return r; }
    if (exact_rows && ((q.step == 1 && step_ok) || (step_static && !q.tune))) { r.form = F_STEP; return r; }
  }
  if (!q.exact) { r.form = F_TREE; return r; }
  // the reference's summation order.  Measured (n=1e6, N=1024, f64): 32 rows per wave 2.75 ms, 16:
  // 2.82, 64: 3.6 (130 VGPRs); float bins and medium calls do best with 16; below 64 Ki rows a wave
  // with 16 rows and one tile of look-ahead is a chain of N/16 memory round trips (~70 us whatever
  // n is): 4 rows with an 8-deep ring (n = 12000: 33 us against 79, n = 48000: 153 against 178,
  // n = 131072: 397 against 355); short calls (a hop of 100 rows): one wave per row
  // float samples from double bins, medium calls: the tree-sum kernel with the rounding-interval test gives the same bits
  // without the chain of dependent additions (n = 4096: 22.5 -> 11.8 us, 48000: 145 -> 132 us, 200000: 585 -> 550 us;
  // from about half a million rows on the streaming kernel below is the faster one: 2.64 against 2.78 ms at n = 1e6)
  // Calls from 8 Ki rows on: the forms that stream at HBM speed differ by a few per cent either way from lease to lease -- 32 /
  // 16 / 8 / 4 rows per wave, 256- or 512-byte row segments, and (float samples from double bins) the tree sum with the
  // rounding-interval proof.  All give the same bits, so the plan measures them on the host's own calls (FormTuner;
  // scripts/synthesis_forms_ab.py: n = 1e6 tree sum +5.5 %, 262144 x 1024 f64f64 16 rows +19 %, m = 4096 FD float 512-byte
  // segments +13 %; round 4's fixed switch points flipped winner five times between 16 k and 65 k rows).  Candidate 0 is the
  // static choice.  Forced forms (options inverse_rows / inverse_rpi / inverse_verify = 0) and operations: static.
  const bool proof = q.td_bytes == 4 && q.fd_bytes == 8;
  if (!q.ops && q.tune && q.rows <= 0 && rows >= 8192 && tune_events())
  {
    r.tuned = true;
    const bool verify0 = proof && q.verify && rows <= kInverseVerifyMax;
    const long rw0 = inverse_rows_per_wave(rows, q.fd_bytes, 0, q.capacity4, q.capacity8, false);
    // candidates: up to kMax pairs (form, rows read first with ordinary loads).  The matrix streams past the caches (non-temporal loads) but for the
    // rows read first, which take ordinary loads: what an analysis left dirty in the Infinity Cache is slow to a non-temporal load.  1.5 GB of them
    // are the static choice from 6 GiB on and none below (inverse_ordinary_rows); between 2 and 16 GiB which is better depends on the form
    // and on whether the host has just written the matrix (4.3 GB: TD = FD = double 1007 -> 835 us with them, f32f64 733 -> 779), so there every
    // form is tried both ways (profiles/r05_after_write_16gb.txt)
    const bool both_loads = q.nt && q.nt_skip_mb < 0 && matrix_bytes >= 2.0 * 1073741824.0 && matrix_bytes < 16.0 * 1073741824.0;
    const size_t other_skip = q.nt_skip ? 0 : inverse_ordinary_rows((size_t)1 << 40, q.nbins * 2 * q.fd_bytes, -1);
    auto add = [&](int f)
    {
      for (int i = 0; i < r.count; ++i) if (r.cand[i].form == f) return;
      if (r.count < FormTuner::kMax) r.cand[r.count++] = InverseCandidate{f, q.nt_skip};
      if (both_loads && r.count < FormTuner::kMax) r.cand[r.count++] = InverseCandidate{f, other_skip};
    };
    add(ordered_static ? F_ORDERED : step_static ? F_STEP : verify0 ? F_VERIFY : (rw0 >= 32 ? F_32 : rw0 >= 16 ? F_16 : rw0 >= 8 ? F_8 : F_4));
    // (float samples from double bins: the two forms with the rounding-interval proof first)
    // (F_8W: 8 rows x 512 bytes, two tiles ahead -- the best of the tiles where rows are too long for the ordered form: 6.8 against 6.6 TB/s at
    // 500 000 x 2048 double; profiles/r06_synthesis_forms.txt)
    static constexpr int others_long[7] = {F_ORDERED, F_8W, F_STEP, F_VERIFY, F_16, F_32, F_16W}, others_medium[7] = {F_ORDERED, F_STEP, F_VERIFY, F_4, F_8, F_16, -1};
    int kinds = 1;
    for (int f : (rows >= 65536 ? others_long : others_medium))
    {
      if (r.count >= FormTuner::kMax || kinds >= (both_loads ? 3 : 4)) break;
      if (f == r.cand[0].form) continue;
      if (f < 0 || (f == F_ORDERED && !ordered_ok)) continue;
      if (f == F_8W && ordered_ok) continue;
      if (f == F_STEP && !(q.step >= 0 && step_ok)) continue;
      if (f == F_VERIFY && !(proof && q.verify)) continue;
      if (f == F_32 && q.fd_bytes != 8) continue;      // (64 registers of row segments: FD double only)
      add(f); ++kinds;
    }
    return r;
  }
  if (proof && q.verify && q.rows <= 0 && rows > 1024 && rows <= kInverseVerifyMax) { r.form = F_VERIFY; return r; }
  // (rows per wave: inverse_rows_per_wave; the capacities of the 4-row and the 8-row form come from the occupancy API)
  size_t c4 = q.capacity4, c8 = q.capacity8;
  if (!q.ops && q.rows <= 0 && c4 == 0 && rows > 1024 && rows < 65536) capacity(c4, c8);
  r.rows_per_wave = inverse_rows_per_wave(rows, q.fd_bytes, q.rows, c4, c8, q.ops);
  const long rw = r.rows_per_wave;
  r.form = (rw == 1 && rows <= 0x7fffffffull) ? F_ROW : rw >= 32 ? F_32 : rw >= 16 ? F_16 : rw >= 8 ? F_8 : F_4;
  return r;
}

// ---- synchronous completion -----------------------------------------------------------------------------------------------------
// A call cannot end before its bytes have moved at the chip's peak rate (the spec figure: a LOWER bound of the time, not a
// tuned one): until then the host spins on its own clock, then it polls the stream; never a sleeping wait while the call can
// still be running (it wakes up 9 us late on one box and 45 us late on another, profiles/r05_sync_completion.txt)
constexpr double kPeakBytesPerUs = 8.0e6;                    // HBM3E, 8 TB/s
struct SyncWait { double quiet_us = 0, budget_us = 0; };
inline SyncWait sync_wait(size_t hbm_bytes)
{
  SyncWait w;
  const double floor_us = (double)hbm_bytes / kPeakBytesPerUs;
  w.quiet_us = floor_us > 8.0 ? floor_us : 0.0;
  w.budget_us = std::min(20000.0, 200.0 + 4.0 * floor_us);
  return w;
}

// ---- host-pointer staging: rows per time segment ---------------------------------------------------------------------------
inline size_t stage_rows(size_t n, size_t row_bytes, size_t stage_bytes)
{
  const size_t seg = std::max<size_t>(1, stage_bytes / std::max<size_t>(row_bytes, 1));
  return std::min(seg, std::max<size_t>(n, 1));
}
// A grid analysis call (sdft_every_n and its eleven siblings) on host memory goes in time segments of at most this many samples:
// the rows a segment writes (row_bytes each, all channels / pairs / outputs of a row together; one row per `every` samples) and
// the samples it reads (sample_row_bytes per time step) stay within stage_bytes -- but a segment of host samples is never shorter
// than a hop.  whole_windows (the pooled calls): where the grid allows it a segment is made of whole windows, so that no row is
// made of two segments.  every <= n (the entry point has clamped it); samples_on_device / out_on_device: that side needs no staging.
inline size_t grid_segment(size_t n, size_t every, size_t first, size_t row_bytes, size_t sample_row_bytes, size_t stage_bytes,
                           bool samples_on_device, bool out_on_device, bool whole_windows)
{
  size_t seg = n;
  if (!out_on_device) seg = std::min(seg, stage_rows(n, row_bytes, stage_bytes) * every);
  if (!samples_on_device) seg = std::min(seg, std::max<size_t>((size_t)kHopSamples, stage_rows(n, sample_row_bytes, stage_bytes)));
  if (whole_windows && seg < n && seg > every && first % every == 0) seg -= seg % every;
  return seg;
}
// the lag-product call's: the cross-spectrum call's bounds with npairs = channels (channels * 2 * nbins_out numbers per row)
inline size_t lag_sum_segment(size_t n, size_t every, size_t first, size_t channels, size_t nbins_out, size_t fd_bytes, size_t td_bytes,
                              size_t stage_bytes, bool samples_on_device, bool sums_on_device)
{
  const size_t ch = std::max<size_t>(channels, 1);
  return grid_segment(n, every, first, ch * 2 * nbins_out * fd_bytes, ch * td_bytes, stage_bytes, samples_on_device, sums_on_device, true);
}
// the power-moments call's: the same bounds -- a row is channels * nbins_out pairs, twice the pooled call's bytes
inline size_t power_moments_segment(size_t n, size_t every, size_t first, size_t channels, size_t nbins_out, size_t fd_bytes, size_t td_bytes,
                                    size_t stage_bytes, bool samples_on_device, bool moments_on_device)
{
  const size_t ch = std::max<size_t>(channels, 1);
  return grid_segment(n, every, first, ch * 2 * nbins_out * fd_bytes, ch * td_bytes, stage_bytes, samples_on_device, moments_on_device, true);
}

// ---- host memory: the route of an analysis or a synthesis call (Plan::sdft_n / isdft_n run it) -----------------------------
// A call has a SAMPLES side ([channels][n] of TD: what the analysis reads and the synthesis writes) and a MATRIX side
// ([channels][n][N] bins: what the analysis writes and the synthesis reads); either may be the caller's host memory.
constexpr size_t kSmallHostBytes = (size_t)64 << 10;       // the plan's pinned scratch (h_io / d_io): host samples up to this size travel through it
constexpr size_t kDirectBytes = (size_t)4 << 20;           // a hop-sized matrix the kernels write / read in the pinned pieces themselves (both)
constexpr size_t kDefaultStageBytes = (size_t)1 << 30;     // option "stage_bytes": the staging segment of host-pointer calls
enum HostRouteKind : int { HR_DEVICE = 0, HR_SCRATCH = 1, HR_MAPPED = 2, HR_DIRECT = 3, HR_STAGED = 4 };
enum HostSamples : int { HS_AS_IS = 0, HS_IO = 1, HS_MAPPED = 2, HS_STAGE_TD = 3 };   // as they are, d_io, registered in place, d_stage_td
enum HostEnd : int { HE_FINISH = 0, HE_FINISH_MAPPED = 1, HE_SYNCHRONIZE = 2 };
struct HostQuery
{
  bool analysis = true;                                    // else synthesis
  bool samples_device = false, matrix_device = false;
  size_t samples_bytes = 0, matrix_bytes = 0;
  bool by_value = false;                                   // the sample of sdft_sdft / the result of sdft_isdft: host memory of the call's duration
  long pinned_io = 1, host_copy = 0, host_direct = 1;      // options
  size_t stage_bytes = kDefaultStageBytes, n = 0, row_bytes = 0;
};
struct HostRoute
{
  int route = HR_STAGED, samples = HS_AS_IS, end = HE_SYNCHRONIZE;
  bool flag_wanted = false, pipe_allowed = false, synchronous = false;
  bool refused = false;                                    // HR_DIRECT: the pinned pieces are busy and could not be drained -- the call fails
  size_t seg = 0;                                          // HR_STAGED: rows per time segment
};

// The callables are the checks with side effects, each asked at most once and only where the route needs the answer: Plan::ensure_io,
// HostIo::map_host of either side (it counts host_register_hits / misses), HostIo::ensure_pin / pin_idle.
template <class EnsureIo, class MapMatrix, class MapSamples, class EnsurePin, class PinIdle>
inline HostRoute host_route(const HostQuery& q, EnsureIo&& ensure_io, MapMatrix&& map_matrix, MapSamples&& map_samples,
                            EnsurePin&& ensure_pin, PinIdle&& pin_idle)
{
  HostRoute r;
  const bool sd = q.samples_device, md = q.matrix_device;
  // (a hop's samples are a different slice of the host's signal every call: a few hundred bytes go through the scratch or
  // the staging buffer, only buffers beyond 64 KiB are worth a registration)
  const bool small = q.samples_bytes <= kSmallHostBytes;
  if (sd && md)
  {
    r.route = HR_DEVICE; r.end = HE_FINISH; r.pipe_allowed = true;
    r.flag_wanted = true;                                  // a call of one time chunk may signal its own completion
    return r;
  }
  // small host samples, device matrix (hop-wise streaming from or to a host signal, sdft_sdft / sdft_isdft on a device row): the
  // kernel reads / writes the pinned scratch, completion by the kernel's word -- the call is complete on return like every
  // host-pointer call (hence synchronous)
  if (!sd && md && small && q.pinned_io && ensure_io())
  {
    r.route = HR_SCRATCH; r.samples = HS_IO; r.end = HE_FINISH; r.flag_wanted = r.synchronous = true;
    return r;
  }
  // host buffers mapped in place (HostIo::map_host): the kernels work on the caller's memory.  The matrix first, and the samples
  // whatever the matrix said: a matrix that was registered stays registered for the next call
  const bool matrix_ok = md || map_matrix();
  // analysis / synthesis: the by-value sample of sdft_sdft is never registered however many channels it has (it lives on the
  // host's stack); the by-value result of sdft_isdft is a buffer like any other
  const bool keep_off = q.analysis && q.by_value;
  const bool samples_mapped = !sd && !small && !keep_off && map_samples();
  if (matrix_ok && (sd || small || samples_mapped))
  {
    r.route = HR_MAPPED; r.samples = sd ? HS_AS_IS : small ? HS_STAGE_TD : HS_MAPPED;       // (small ones: one copy through device scratch)
    r.end = HE_FINISH_MAPPED;                              // host memory: complete on return, through the stream
    return r;
  }
  // a hop-sized matrix in host memory (the reference driver's 100 x 1000 bins = 1.6 MB, test/test.c:62-83): the kernels write it
  // into / read it from the plan's pinned pieces over PCIe -- no staging matrix, no DMA launch -- and the host copies it out / in
  // (scripts/host_hop_paths.py, profiles/r04_host_copy_paths.txt)
  if (!md && q.host_copy == 0 && q.host_direct && q.matrix_bytes <= kDirectBytes && (sd || small) && ensure_pin())
  {
    r.route = HR_DIRECT; r.end = HE_FINISH_MAPPED;
    if (!pin_idle()) { r.refused = true; return r; }
    r.samples = sd ? HS_AS_IS : (q.pinned_io && ensure_io()) ? HS_IO : HS_STAGE_TD;
    return r;
  }
  // staged (host pointers): time segments so that the staging matrix stays bounded; the stream state carries over from segment
  // to segment exactly like hop-wise calls do
  r.route = HR_STAGED; r.samples = sd ? HS_AS_IS : HS_STAGE_TD; r.end = HE_SYNCHRONIZE;
  r.seg = stage_rows(q.n, q.row_bytes, q.stage_bytes);
  return r;
}

// ---- fused analysis -> operation -> synthesis: the route of a call (Plan::process_n runs it) -----------------------------------
// fused call: bins summed in the reference's order?  (-1: exactly when the host asked for exact carries at FD double)
inline bool reference_order(long fused_exact, bool exact, size_t fd_bytes) { return fused_exact < 0 ? (exact && fd_bytes == 8) : fused_exact != 0; }
struct ProcessQuery
{
  ChunkQuery chunk;                                        // of the call; chunk.rows_kernel: the row-group kernel takes the plan's rows
  size_t fd_bytes = 8, fdx_bytes = 16;
  bool linear = true, user = false;                        // the operation: linear (identity, gain, shift, complex gain); the host's own statements
  size_t gain_rows = 1;                                    // gain vectors of a time-varying gain
  bool spectrum = false;                                   // the caller wants the processed spectrum (dfts)
  bool x_device = true, y_device = true;
  long fused_exact = -1, fold = 1, hop_kernel = 1, exact_inverse = 1, inverse_rows = 0;   // options
  size_t stage_bytes = kDefaultStageBytes;
  size_t workspace = 0;                                    // bins the plan's staging matrix holds already
};
// one launch of the folded hop kernel (process_hop2_kernel); the fused row kernels through forward_device; hop kernel + row
// synthesis (one time chunk, two launches); analysis and synthesis in time segments through a workspace
enum ProcessPath : int { PP_HOP_FOLDED = 0, PP_FUSED_ROWS = 1, PP_HOP_PAIR = 2, PP_SEGMENTS = 3 };   // (get_option "last_process_path": 1, 1, 2, 3)
struct ProcessRoute
{
  int path = PP_SEGMENTS;
  bool fold = false;                                       // the coefficients are folded (Plan::fold_coefficients) before the launch
  bool flag_wanted = false;
  size_t seg = 0;                                          // two passes: rows per segment
  bool rtc_hop = false, rtc_rows = false;                  // the host's statements: inverse_row_kernel / user_rows_kernel resolved up front
};

// free_bytes(): the device's free memory (0: unknown), asked only where a long call's workspace may outgrow stage_bytes
template <class FreeBytes>
inline ProcessRoute process_route(const ProcessQuery& q, FreeBytes&& free_bytes)
{
  ProcessRoute r;
  const size_t n = q.chunk.n, nb = q.chunk.nbins, ch = std::max<size_t>(q.chunk.channels, 1);
  const long chunks = choose_chunks(q.chunk).chunks;
  const bool hop = chunks == 1 && n <= (size_t)kHopSamples;
  const bool foldable = q.linear && !reference_order(q.fused_exact, q.chunk.exact, q.fd_bytes) && !q.spectrum && q.fold && nb >= 8;
  // reference order asked for on two-slot rows at FD float: the ordered walk (N dependent additions shared
  // by the four samples of a group) costs more than the synthesis pass it saves (N = 4096, n = 262144:
  // 5.7 ms against 4.1 ms for the two passes, which give the same bits); fused_exact = 2 insists on the kernel
  const bool walk_loses = row_slots(nb, q.fdx_bytes) == 2 && q.fd_bytes == 4 && q.chunk.exact && q.fused_exact == 1;
  r.flag_wanted = q.x_device && q.y_device;
  // calls of one time chunk: the folded form in one launch unless the reference's order is wanted -- then the hop kernel +
  // row synthesis pair below, which is bit-identical
  if (hop && foldable && q.hop_kernel && q.gain_rows <= 1) { r.path = PP_HOP_FOLDED; r.fold = true; return r; }
  // the folded form carries up to four bins per lane whatever the bin type is (N <= 4096); the forms that keep the
  // windowed rows in LDS stop at two slots of the row-group kernel (N <= 2048 double / 4096 float)
  // (many channels: one chunk per channel, however long, is no hop)
  if ((q.chunk.rows_kernel || (foldable && q.gain_rows <= 65535 && nb <= (size_t)4 * kLanes * kRowWaves)) && !hop && !walk_loses)
  {
    r.path = PP_FUSED_ROWS; r.fold = !q.spectrum;
    return r;
  }
  // short calls (one time chunk: the hop kernel and the row-per-wave synthesis, two launches) and shapes the row-group
  // kernel does not cover: analysis into the caller's matrix or a bounded workspace, synthesis with the operation applied
  // on the way in
  r.path = chunks == 1 ? PP_HOP_PAIR : PP_SEGMENTS; r.flag_wanted = false;
  const size_t row_bytes = ch * nb * q.fdx_bytes;
  r.seg = q.spectrum ? n : stage_rows(n, row_bytes, q.stage_bytes);
  // long calls run best in one piece (time segments restart the carry pipeline): unless the host has bounded it (option
  // stage_bytes), the workspace may take up to half of what the device has free
  if (!q.spectrum && r.seg < n && q.stage_bytes == kDefaultStageBytes)
    r.seg = q.workspace >= ch * nb * n ? n : std::max(r.seg, std::min(n, (free_bytes() / 2) / std::max<size_t>(row_bytes, 1)));
  if (q.user)
  {
    // a segment of up to 1024 rows is a hop: the statements run inside the row synthesis; longer ones (and a copy of the
    // spectrum) take user_rows_kernel.  The first and the last segment are the two lengths there are
    const size_t m_first = std::min(r.seg, n), m_last = n - ((n - 1) / r.seg) * r.seg;
    const bool hop_form = q.exact_inverse && q.inverse_rows <= 0;
    r.rtc_hop = hop_form && (ch * m_first <= 1024 || ch * m_last <= 1024);
    r.rtc_rows = !hop_form || ch * m_first > 1024 || ch * m_last > 1024 || q.spectrum;
  }
  return r;
}

// ---- host copies through pinned pieces: the slot ring --------------------------------------------------------------------------
// A copy of `bytes` bytes travels in pieces of `piece` bytes through a ring of `slots` pinned slots; piece i uses slot i % slots,
// so piece i may enter its slot once piece i - slots has left it.  Both directions are the same pipeline of two stages per
// piece: to the device  FILL (a host thread copies the caller's bytes into the slot) -> SEND (DMA out of the slot);
//        to the host    SEND (DMA into the slot) -> DRAIN (a host thread copies the slot into the caller's bytes).
struct PieceRing
{
  size_t bytes = 0, piece = 1;
  unsigned slots = 1;
  PieceRing(size_t total, size_t piece_bytes, unsigned ring_slots) : bytes(total), piece(std::max<size_t>(piece_bytes, 1)), slots(std::max(ring_slots, 1u)) {}
  size_t pieces() const { return (bytes + piece - 1) / piece; }
  size_t offset(size_t i) const { return i * piece; }
  size_t length(size_t i) const { return std::min(piece, bytes - std::min(bytes, i * piece)); }
  unsigned slot(size_t i) const { return (unsigned)(i % slots); }
  // the piece that must have left piece i's slot before i may enter it, or (size_t)-1
  size_t predecessor(size_t i) const { return i >= slots ? i - slots : (size_t)-1; }
};

}  // namespace logic
}  // namespace sdfthip
