// plan_logic_test.cpp -- unit tests of the engine's host-side decisions (sdft_amd/csrc/sdft_plan_logic.hpp: no HIP anywhere),
// compiled by tests/test_plan_logic_cpu.py with g++ -fsanitize=address,undefined and run in the `-m "not gpu"` suite
// (sanitizers for the host side).  Exits non-zero at the first violated property.

#include "sdft_plan_logic.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

using namespace sdfthip::logic;

static int failures = 0;
#define CHECK(cond, ...)                                                                    \
  do {                                                                                      \
    if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); \
      if (failures > 20) exit(1); }                                                         \
  } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static size_t rnd_in(size_t lo, size_t hi) { return lo + (size_t)(rnd() % (unsigned long long)(hi - lo + 1)); }

static void test_geometry()
{
  CHECK(bins_per_lane(16) == 1 && bins_per_lane(8) == 2, "lanes store 16 bytes");
  for (int window = 0; window < 4; ++window)
    for (size_t fdx : {(size_t)8, (size_t)16})
    {
      const long inter = interior_lanes(window, fdx, 0);
      CHECK(inter >= 8 && inter % 8 == 0 && inter + 2 * halo_lanes(window, fdx) <= kLanes, "window %d fdx %zu: %ld interior lanes", window, fdx, inter);
      CHECK(interior_lanes(window, fdx, 1000) == kLanes - 2 * halo_lanes(window, fdx), "forced interior is capped");
      for (size_t nbins : {(size_t)1, (size_t)7, (size_t)56, (size_t)57, (size_t)1000, (size_t)1024, (size_t)4096, (size_t)100000})
      {
        const long t = tiles(nbins, window, fdx, 0);
        const long per = inter * bins_per_lane(fdx);
        CHECK(t * per >= (long)nbins && (t - 1) * per < (long)nbins, "tiles cover the row exactly once: nbins %zu tiles %ld", nbins, t);
      }
    }
  // rows the row-group kernel takes: 8 ... 2048 bins of 16 bytes, ... 4096 bins of 8 bytes, never a row-pointer table
  CHECK(rows_kernel_ok(1024, 16, false, true, 2) && rows_kernel_ok(2048, 16, false, true, 2) && !rows_kernel_ok(2049, 16, false, true, 2), "FD double rows");
  CHECK(rows_kernel_ok(4096, 8, false, true, 2) && !rows_kernel_ok(4097, 8, false, true, 2) && !rows_kernel_ok(4096, 8, false, true, 1), "FD float rows");
  CHECK(!rows_kernel_ok(1024, 16, true, true, 2) && !rows_kernel_ok(1024, 16, false, false, 2) && !rows_kernel_ok(7, 16, false, true, 2), "exclusions");
  for (size_t fdx : {(size_t)8, (size_t)16})
    for (size_t nbins = 8; nbins <= (size_t)(kLanes * kRowWaves * bins_per_lane(fdx) * 2); nbins += 37)
    {
      const long s = row_slots(nbins, fdx), w = row_waves(nbins, fdx);
      CHECK((s == 1 || s == 2) && w >= 1 && w <= kRowWaves, "nbins %zu: %ld slots %ld waves", nbins, s, w);
      CHECK((size_t)(w * s * kLanes * bins_per_lane(fdx)) >= nbins, "the row group holds the row: nbins %zu", nbins);
    }
}

static void test_chunks()
{
  for (int it = 0; it < 200000; ++it)
  {
    ChunkQuery q;
    q.n = (it % 5 == 0) ? rnd_in(1, 600) : rnd_in(1, 3000000);
    q.channels = (it % 3 == 0) ? rnd_in(1, 600) : 1;
    q.nbins = rnd_in(1, 4096);
    q.rows_kernel = rnd() & 1; q.exact = rnd() & 1; q.pipelined = (rnd() & 3) == 0;
    q.forced_chunk = (rnd() & 7) == 0 ? (long)rnd_in(1, 100000) : 0;
    q.target_waves = (rnd() & 7) == 0 ? (long)rnd_in(1, 100000) : 0;
    q.row_waves = (long)rnd_in(1, 16); q.tiles = (long)rnd_in(1, 80); q.compute_units = (int)rnd_in(1, 304);
    const Chunking c = choose_chunks(q);
    CHECK(c.chunks >= 1 && c.len >= 1, "n %zu: %ld chunks of %ld", q.n, c.chunks, c.len);
    CHECK((size_t)c.chunks * (size_t)c.len >= q.n && (size_t)(c.chunks - 1) * (size_t)c.len < q.n, "chunks cover the call exactly once: n %zu %ld x %ld", q.n, c.chunks, c.len);
    if (q.forced_chunk <= 0 && q.n < (size_t)kHopSamples) CHECK(c.chunks == 1, "hop-sized calls are one chunk (bit-exact): n %zu", q.n);
    if (c.chunks > 1 && q.forced_chunk <= 0) CHECK(c.len % kTimeGroup == 0, "whole scalar-load groups: len %ld", c.len);
    if (c.chunks > 1 && q.exact && q.forced_chunk <= 0) CHECK(c.len % 32 == 0, "whole trips of the exact pass: len %ld", c.len);
    if (c.chunks > 1 && !q.exact && q.forced_chunk > 0) CHECK(c.len % kSumBlockLen == 0, "whole sum blocks: len %ld", c.len);
  }
  // the shapes the documents quote
  ChunkQuery q; q.rows_kernel = true; q.row_waves = 16; q.compute_units = 256; q.nbins = 1024;
  q.n = 48000; Chunking c = choose_chunks(q);
  CHECK(c.chunks == 250 && c.len == 192, "north star: %ld x %ld", c.chunks, c.len);
  q.n = 52000; c = choose_chunks(q);
  CHECK(c.chunks <= 256, "between one and two rounds of the chip a call takes ONE round: %ld chunks", c.chunks);
  q.n = 1000000; c = choose_chunks(q);
  CHECK(c.chunks > 256 && c.chunks <= 512, "two rounds at n = 1e6: %ld", c.chunks);
  q.pipelined = true; q.n = 48000; c = choose_chunks(q);
  CHECK(c.chunks == 300 && c.len == 160, "pipelined calls: about 300 chunks of >= 160 rows: %ld x %ld", c.chunks, c.len);
  // where pipelined calls pay: calls below 2^29 bins by default, any length on request, never when off
  q.pipelined = true;
  q.n = 48000; CHECK(pipeline_pays(q, 1) && pipeline_pays(q, 2) && !pipeline_pays(q, 0), "north star: pipelined by default");
  q.n = 131072; CHECK(pipeline_pays(q, 1), "n = 131072 gains 11 %%: pipelined");
  q.n = 1000000; CHECK(!pipeline_pays(q, 1) && pipeline_pays(q, 2), "n = 1e6 is a tie: one stream by default");
  q.n = 48000; q.channels = 64; CHECK(!pipeline_pays(q, 1), "one GPU's share of configs[4]: 3e9 bins");
  q.channels = 1;
  q.pipelined = false; q.exact = true; q.n = 262144; q.nbins = 4096; c = choose_chunks(q);
  CHECK(c.chunks == 2048 && c.len == 128, "configs[2]: %ld x %ld", c.chunks, c.len);
}

static void test_relay_and_radices()
{
  CHECK(relay_block(4096, 128, 4, 8, 0) == 128 && relay_block(1024, 192, 8, 16, 0) == 64 && relay_block(1000, 32, 4, 8, 0) == 16, "block lengths");
  CHECK(relay_block(7, 64, 4, 8, 0) == 0 && relay_block(1024, 100, 4, 8, 0) == 0 && relay_block(1024, 0, 4, 8, 0) == 0, "no block length fits");
  CHECK(relay_block(4096, 128, 4, 8, 32) == 32 && relay_block(4096, 128, 8, 16, 128) == 0, "forced");
  for (size_t nbins = 1; nbins < 5000; nbins += 3)
    for (long len : {8L, 32L, 96L, 128L, 640L, 1000L})
    {
      const unsigned L = relay_block(nbins, len, 4, 8, 0);
      if (L) CHECK((2 * nbins) % L == 0 && (size_t)len % L == 0 && L <= 128, "nbins %zu len %ld: L %u", nbins, len, L);
    }
  for (size_t span = 1; span <= 8192; ++span)
  {
    const Radices r = smooth_radices(span);
    size_t prod = 1;
    for (int i = 0; i < r.count; ++i) { CHECK(r.r[i] >= 2 && r.r[i] <= 5, "radix"); prod *= r.r[i]; }
    size_t rem = span;
    for (size_t f : {(size_t)2, (size_t)3, (size_t)5}) while (rem % f == 0) rem /= f;
    if (rem == 1 && span > 1) CHECK(r.count > 0 && prod == span, "a 2/3/5-smooth span factors completely: %zu", span);
    else CHECK(r.count == 0, "other prime factors: %zu", span);
  }
  CHECK(self_cells(1024, true, 16) == 2048 && self_cells(1000, true, 16) == 4000 && self_cells(1000, false, 16) == 0 && self_cells(1022, true, 16) == 0, "self cells");
  CHECK(self_cells(4096, true, 16) == 0 && self_cells(2048, true, 16) == 4096 && self_cells(4, true, 16) == 0, "self cells, limits");
}

static void test_call_pattern()
{
  CallPattern p;
  p.on_analysis(false); CHECK(!p.analysis_batch, "one analysis is not a run");
  p.on_analysis(false); CHECK(p.analysis_batch, "two analyses in a row");
  p.on_synthesis_begin(); p.on_synthesis_launched(); CHECK(p.analysis_batch && !p.inverse_batch, "a synthesis after a run of analyses");
  p.on_synthesis_begin(); p.on_synthesis_launched(); CHECK(p.inverse_batch, "two syntheses in a row");
  p.on_analysis(false); CHECK(p.inverse_batch, "an analysis after a run of syntheses keeps the mode");
  // the reference's loop: analysis, synthesis, analysis, synthesis ... : both modes go off and stay off
  CallPattern r;
  for (int i = 0; i < 6; ++i)
  {
    r.on_analysis(false);
    r.on_synthesis_begin(); r.on_synthesis_launched();
    if (i >= 1) CHECK(!r.analysis_batch && !r.inverse_batch, "alternating calls never leave the plan's stream (hop %d)", i);
  }
  // the fused call is neither kind
  CallPattern f;
  f.on_analysis(false); f.on_analysis(true); f.on_analysis(false);
  CHECK(!f.analysis_batch, "a fused call between two analyses breaks the run");
}

static void test_row_ring()
{
  RowRing ring;
  const uintptr_t A = 0x100000, B = 0x900000, S = 0x400000;
  RowRing::Pick p = ring.pick(A, A + S);
  CHECK(p.stream == 0 && !p.behind && ring.state_reader() < 0, "first launch");
  ring.launched(A, A + S, p.stream);
  p = ring.pick(B, B + S);
  CHECK(p.stream == 1 && !p.behind, "another matrix: the other stream");
  ring.launched(B, B + S, p.stream);
  p = ring.pick(A, A + S);
  CHECK(p.stream == 0 && p.behind && p.wait_launch < 0, "the first matrix again: behind its own launch, on its stream");
  ring.launched(A, A + S, p.stream);
  CHECK(ring.state_reader() == 0, "the fourth launch's state kernel waits for the rows of the first (slot 0)");
  p = ring.pick(A + S / 2, B + S / 2);
  CHECK(p.behind && p.wait_launch >= 0 && ring.stream_of[p.wait_launch] != p.stream, "a matrix across both: the other stream's launch is waited for");
  CHECK(ring.samples_overlap(B + 8, B + 16) && !ring.samples_overlap(0x10, 0x20), "samples inside an outstanding matrix");
  int slots[2];
  CHECK(ring.last_per_stream(slots) == 2 && ring.stream_of[slots[0]] != ring.stream_of[slots[1]], "join waits for the last launch on each stream");
  ring.joined();
  CHECK(!ring.open && ring.seq == 0 && ring.last_per_stream(slots) == 0, "joined");
  // random sequences: the pick is always one of the two streams, `behind` exactly when an outstanding launch overlaps
  for (int it = 0; it < 20000; ++it)
  {
    if ((rnd() & 31) == 0) ring.joined();
    const uintptr_t lo = (uintptr_t)rnd_in(0, 64) * 0x1000, hi = lo + (uintptr_t)rnd_in(1, 16) * 0x1000;
    bool any = false;
    for (unsigned long long back = 1; back <= 3 && back <= ring.seq; ++back) any = any || overlap(lo, hi, ring.out[(ring.seq - back) & 3]);
    const RowRing::Pick q = ring.pick(lo, hi);
    CHECK((q.stream == 0 || q.stream == 1) && q.behind == any, "pick: stream %d behind %d any %d", q.stream, (int)q.behind, (int)any);
    if (q.wait_launch >= 0) CHECK(ring.stream_of[q.wait_launch] != q.stream && overlap(lo, hi, ring.out[q.wait_launch]), "waited launch overlaps, other stream");
    ring.launched(lo, hi, q.stream);
  }
}

static void test_inverse_streams()
{
  InverseStreams inv;
  const Range y1{0x1000, 0x2000}, y2{0x3000, 0x4000}, y3{0x5000, 0x6000}, none{0, 0};
  InverseStreams::Pick p = inv.pick(y1, none); inv.launched(p.stream, y1);
  const int first = p.stream;
  p = inv.pick(y2, none); CHECK(p.stream != first && !p.wait_other, "two sample buffers: two streams"); inv.launched(p.stream, y2);
  p = inv.pick(y1, none); CHECK(p.stream == first && !p.wait_other, "the first buffer again: behind its writer, same stream"); inv.launched(p.stream, y1);
  // three buffers in rotation (the advisor's case): y3 -> y1's stream ... then y1 must wait for its earlier write on the other stream
  InverseStreams r;
  p = r.pick(y1, none); r.launched(p.stream, y1); const int sa = p.stream;
  p = r.pick(y2, none); r.launched(p.stream, y2);
  p = r.pick(y3, none); CHECK(p.stream == sa, "third buffer takes the first stream again"); r.launched(p.stream, y3);
  p = r.pick(y1, none); r.launched(p.stream, y1);
  p = r.pick(y2, none);
  CHECK(p.stream != r.last || p.wait_other || overlap(y2, r.y[p.stream]), "a write to y2 is ordered behind the outstanding write of y2");
  // a matrix that is an outstanding synthesis's samples reinterpreted
  InverseStreams m;
  p = m.pick(y1, none); m.launched(p.stream, y1);
  p = m.pick(y2, y1); CHECK(p.wait_other, "reads what the other stream is writing: waits");
}

static void test_small_decisions()
{
  HopParts h = hop_parts(100, 18, 256, 0, true);
  CHECK(h.parts == 4 && h.part_len == 25, "synchronous hop of the reference's test: %u x %u", h.parts, h.part_len);
  h = hop_parts(100, 18, 256, 0, false);
  CHECK(h.parts == 8 && h.part_len == 13, "asynchronous: %u x %u", h.parts, h.part_len);
  h = hop_parts(100, 200, 256, 0, false); CHECK(h.parts == 1, "no CU to spare: one part");
  h = hop_parts(23, 18, 256, 0, false); CHECK(h.parts == 1 && h.part_len == 23, "too short");
  h = hop_parts(100, 18, 256, 1, false); CHECK(h.parts == 1, "option: never");
  for (size_t n = 1; n < 600; ++n)
    for (long forced : {0L, 2L, 5L, 16L, 1000L})
    {
      h = hop_parts(n, 18, 256, forced, (n & 1) != 0);
      CHECK(h.parts >= 1 && (size_t)h.parts * h.part_len >= n && (size_t)(h.parts - 1) * h.part_len < n, "parts cover the call once: n %zu forced %ld: %u x %u", n, forced, h.parts, h.part_len);
    }
  CHECK(inverse_rows_per_wave(100, 8, 0, 0, 0, false) == 1 && inverse_rows_per_wave(48000, 8, 0, 0, 0, false) == 4 && inverse_rows_per_wave(1000000, 8, 0, 0, 0, false) == 32, "rows per wave");
  CHECK(inverse_rows_per_wave(1000000, 4, 0, 0, 0, false) == 16 && inverse_rows_per_wave(48000, 8, 0, 8192, 8192, false) == 8, "rows per wave: float bins; a second round avoided");
  CHECK(inverse_rows_per_wave(48000, 8, 0, 16384, 8192, false) == 4 && inverse_rows_per_wave(48000, 8, 0, 8192, 8192, true) == 16 && inverse_rows_per_wave(48000, 8, 32, 8192, 8192, false) == 32, "rows per wave: fits / operation / forced");
  ProcessGeometry g = process_geometry(1024, 1, 1000000, true, 8, 0);
  CHECK(g.slots == 4 && g.waves == 4, "fused call, long: %ld waves x %ld bins per lane", g.waves, g.slots);
  g = process_geometry(1024, 1, 48000, true, 8, 0); CHECK(g.slots == 2 && g.waves == 8, "fused call, north star: %ld x %ld", g.waves, g.slots);
  g = process_geometry(1024, 1, 48000, false, 4, 0); CHECK(g.slots == 1 && g.waves == 16, "FD float: %ld x %ld", g.waves, g.slots);
  for (size_t nbins = 8; nbins <= 4096; nbins += 11)
  {
    g = process_geometry(nbins, 1, 500000, true, 8, 0);
    CHECK((size_t)(g.waves * g.slots * kLanes) >= nbins && g.waves >= 1 && g.waves <= kRowWaves, "fused geometry holds the row: nbins %zu", nbins);
  }
  const SyncWait w = sync_wait((size_t)48000 * 1024 * 16);
  CHECK(w.quiet_us > 90 && w.quiet_us < 110 && w.budget_us > w.quiet_us * 2, "north star: quiet %.1f us budget %.1f us", w.quiet_us, w.budget_us);
  CHECK(sync_wait(1000).quiet_us == 0 && sync_wait((size_t)1 << 40).budget_us <= 20000.0, "short and huge calls");
  CHECK(stage_rows(1000, 16384, (size_t)1 << 30) == 1000 && stage_rows(1000000, 16384, (size_t)1 << 30) == 65536 && stage_rows(5, 0, 100) == 5 && stage_rows(10, 1000, 10) == 1, "staging segments");
}

static void test_form_tuner()
{
  FormTuner t;
  t.reset(1000, 3);
  bool timed = false;
  // a host that waits for every call: the candidates in turn, two samples each, the smaller one counts
  const float ms[3][2] = {{2.0f, 1.9f}, {1.5f, 1.6f}, {1.8f, 3.0f}};
  int seen[3] = {0, 0, 0};
  for (int i = 0; i < 6; ++i)
  {
    const int f = t.next(true, timed);
    CHECK(timed && f >= 0 && f < 3 && seen[f] < 2, "trial %d: form %d", i, f);
    t.launched(f); t.report(f, ms[f][seen[f]]); ++seen[f];
  }
  int f = t.next(true, timed);
  CHECK(!timed && f == 1 && t.chosen == 1, "the fastest form (by its smaller sample) is chosen: %d", f);
  CHECK(t.next(false, timed) == 1 && !timed, "and stays");
  // a host that queues calls faster than they run: one trial per form in flight, then the static form untimed
  t.reset(5000, 3);
  for (int i = 0; i < 3; ++i) { f = t.next(true, timed); CHECK(timed && f == i, "flood: form %d in flight", f); t.launched(f); }
  f = t.next(true, timed); CHECK(!timed && f == 0 && t.chosen < 0, "every open form in flight: the static form, untimed");
  t.report(1, 1.0f);
  f = t.next(true, timed); CHECK(timed && f == 1, "a form that has reported takes its second sample");
  t.reset(2000, 1); CHECK(t.next(true, timed) == 0 && !timed && t.chosen == 0, "one candidate: nothing to measure");
  t.reset(3000, 9); CHECK(t.count == FormTuner::kMax, "capped");
  t.reset(3000, 2);
  CHECK(t.next(false, timed) == 0 && !timed, "no timing possible: the static form");
  t.launched(1); t.report(7, 1.0f); t.report(1, -1.0f); CHECK(t.samples[1] == 0 && !t.inflight[1], "a failed sample frees the form and counts nothing");
  // a host that alternates between call lengths: each shape keeps its tuner (and what it decided); a fourth shape replaces the least recently used
  {
    TunerTable tab;
    const int a = tab.find(1000, 3), b = tab.find(2000, 3);
    CHECK(a != b && tab.slot[a].key == 1000 && tab.slot[b].key == 2000, "two shapes, two tuners");
    for (int i = 0; i < 6; ++i) { FormTuner& q = tab.slot[tab.find(1000, 3)]; const int g = q.next(true, timed); q.launched(g); q.report(g, 1.0f + g); (void)tab.find(2000, 3); }
    FormTuner& qa = tab.slot[tab.find(1000, 3)];
    CHECK(qa.next(true, timed) == 0 && qa.chosen == 0 && !timed, "the interleaved shape did not make the first one start over");
    CHECK(tab.slot[tab.find(2000, 3)].chosen < 0, "the second shape is still open");
    const int c = tab.find(3000, 3);
    CHECK(c != a && c != b, "a third shape takes the free slot");
    (void)tab.find(1000, 3); (void)tab.find(3000, 3);
    const int d = tab.find(4000, 2);
    CHECK(d == b && tab.slot[d].key == 4000 && tab.slot[d].count == 2 && tab.slot[d].chosen < 0, "a fourth shape replaces the least recently used (2000)");
    CHECK(tab.slot[tab.find(1000, 3)].chosen == 0, "... and the decided one is still there");
    CHECK(tab.find(1000, 4) >= 0 && tab.slot[tab.find(1000, 4)].count == 4, "another candidate count is another tuner");
    tab.reset_all();
    CHECK(tab.slot[tab.find(1000, 3)].chosen < 0, "reset_all forgets");
  }
  // the kind of load of the synthesis by the size of the matrix: the window of round 4, the very large matrices of round 5, the option
  const size_t MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;
  CHECK(!inverse_streaming_loads(200 * MiB, -1) && inverse_streaming_loads(300 * MiB, -1) && inverse_streaming_loads(4 * GiB, -1), "the window");
  CHECK(inverse_streaming_loads(4 * GiB + 1, -1) && inverse_streaming_loads(16 * GiB, -1) && inverse_streaming_loads(50 * GiB, -1), "beyond it");
  CHECK(inverse_streaming_loads(1, 1) && !inverse_streaming_loads(GiB, 0), "forced");
  // ... but for the rows read first: 1.5 GB of matrices from 6 GiB on, whole rows, none below; the option
  CHECK(inverse_ordinary_rows(16 * GiB, 16384, -1) == 98304 && inverse_ordinary_rows(5 * GiB, 16384, -1) == 0 && inverse_ordinary_rows(16 * GiB, 16000, -1) == 100664, "rows read first");
  CHECK(inverse_ordinary_rows(GiB, 16384, 256) == 16384 && inverse_ordinary_rows(16 * GiB, 16384, 0) == 0 && inverse_ordinary_rows(GiB, 0, 100) == 0, "forced rows");
}

static void test_piece_ring()
{
  for (int it = 0; it < 20000; ++it)
  {
    const size_t bytes = rnd_in(0, 40) == 0 ? 0 : rnd_in(1, (size_t)64 << 20), piece = rnd_in(1, (size_t)4 << 20);
    const unsigned slots = (unsigned)rnd_in(1, 8);
    const PieceRing r(bytes, piece, slots);
    size_t covered = 0;
    std::vector<size_t> occupant(slots, (size_t)-1);
    for (size_t i = 0; i < r.pieces(); ++i)
    {
      CHECK(r.offset(i) == covered && r.length(i) >= 1 && r.length(i) <= piece, "pieces tile the copy: piece %zu", i);
      covered += r.length(i);
      CHECK(r.predecessor(i) == occupant[r.slot(i)], "a slot's previous occupant is the piece that must leave first");
      occupant[r.slot(i)] = i;
    }
    CHECK(covered == bytes, "all bytes: %zu of %zu", covered, bytes);
  }
}

// ---- the route of an analysis (forward_route) ---------------------------------------------------------------------------------
static ForwardQuery random_forward_query()
{
  ForwardQuery q;
  q.fd_bytes = (rnd() & 1) ? 8 : 4; q.fdx_bytes = 2 * q.fd_bytes;
  static const size_t ms[] = {1, 2, 6, 64, 100, 240, 256, 1000, 1024, 1536, 2048, 4096, 5000};
  q.nbins = (rnd() & 3) ? ms[rnd() % 13] : rnd_in(1, 5000);
  q.n = (rnd() & 3) == 0 ? rnd_in(1, 600) : rnd_in(1, 2000000);
  q.channels = (rnd() & 3) == 0 ? rnd_in(1, 64) : 1;
  q.window = (int)rnd_in(0, 3);
  q.cursor = rnd_in(0, 2 * q.nbins - 1);
  q.exact = rnd() & 1; q.fid_canonical = (rnd() & 3) != 0;
  q.fuse = (rnd() & 3) == 0;
  if (q.fuse) { q.fuse_store = (rnd() & 3) == 0; q.reference_order = rnd() & 1; q.coeff_ready = (rnd() & 3) != 0; }
  q.every = !q.fuse && (rnd() & 3) == 0;
  q.row_pointers = !q.fuse && !q.every && (rnd() & 7) == 0;
  q.out = q.row_pointers ? 0 : ((uintptr_t)rnd_in(1, 1000) << 20) + ((rnd() & 3) == 0 ? 8 : 0);
  q.out_stride = q.n * q.nbins + ((rnd() & 3) == 0 ? 1 : 0);
  q.analysis_batch = rnd() & 1; q.pipe_wanted = rnd() & 1;
  if (rnd() & 1) q.prev_out = Range{q.out + 16, q.out + 32};
  q.rows_kernel = (rnd() & 7) != 0; q.row_slots_max = (rnd() & 7) ? 2 : 1; q.interior = (rnd() & 7) ? 0 : (long)rnd_in(1, 64);
  q.chunk = (rnd() & 7) ? 0 : (long)rnd_in(1, 5000); q.self = (rnd() & 7) != 0; q.fused = (rnd() & 7) != 0; q.fold = (rnd() & 7) != 0;
  q.fft_carry = (long)rnd_in(0, 2); q.hop_kernel = (rnd() & 7) != 0; q.chain = (long)rnd_in(0, 2); q.chain_L = (rnd() & 7) ? 0 : (8L << rnd_in(0, 4));
  q.relay_flow = (rnd() & 3) != 0; q.segments = (rnd() & 3) ? 0 : (long)rnd_in(1, 12); q.xcd_map = rnd() & 1; q.rows_f32 = (rnd() & 3) != 0;
  q.pipeline = (long)rnd_in(0, 2);
  return q;
}

static void test_forward_routes()
{
  for (int it = 0; it < 100000; ++it)
  {
    const ForwardQuery q = random_forward_query();
    const bool gate = rnd() & 1;
    int gates = 0;
    const ForwardRoute r = forward_route(q, [&] { ++gates; return gate; });
    const size_t span = 2 * q.nbins;
    CHECK(r.chunks >= 1 && r.len >= 1 && (size_t)r.chunks * (size_t)r.len >= q.n + r.shift && (size_t)(r.chunks - 1) * (size_t)r.len < q.n + r.shift,
          "chunks cover the (shifted) call once: n %zu %ld x %ld shift %u", q.n, r.chunks, r.len, r.shift);
    if (r.chunks == 1 && q.hop_kernel && q.nbins >= 2 && !q.fuse && !q.every) CHECK(r.kernel == FK_HOP, "one chunk, hop kernel on: the hop route");
    if (r.kernel == FK_HOP) CHECK(r.chunks == 1 && !r.self && !r.fused && !r.flow && gates == 0, "the hop route decides nothing else");
    if (q.every) CHECK(r.kernel == FK_EVERY && !r.self && !r.pipelined && !r.flow, "decimated: tiles, never self-carried, pipelined or in flow mode");
    if (q.fd_bytes == 4) CHECK(!r.self && !r.pipelined && !r.fused, "FD float is never self-carried");
    if (q.exact) CHECK(r.sums == SUMS_NONE && r.carry != CARRY_SUMS && r.use_seed && !r.delta_in_carry && !r.self, "exact carries never take a sums form");
    if (r.carry == CARRY_SUMS) CHECK(!q.exact && r.chunks > 1 && r.sums != SUMS_NONE && r.delta_in_carry && !r.use_seed, "pre-pass sums");
    if (r.sums == SUMS_FFT2 || r.sums == SUMS_FFT_MIXED) CHECK(q.fft_carry && (r.len > 64 || q.fft_carry == 2), "short chunks take direct sums");
    if (r.carry == CARRY_RELAY) CHECK(r.relay_L && span % r.relay_L == 0 && r.len % r.relay_L == 0 && r.shift < r.relay_L, "L %u divides 2N %zu and the chunk %ld", r.relay_L, span, r.len);
    else CHECK(r.relay_L == 0 && r.shift == 0, "no relay, no block");
    if (r.flow) CHECK(r.segments == 1 && r.carry == CARRY_RELAY && gate && !r.xcd_map, "flow mode is one segment of the relay form");
    CHECK(gates <= 1, "the gate is asked at most once");
    if (gates) CHECK(r.carry == CARRY_RELAY && q.relay_flow && q.segments <= 0 && !q.every, "the gate is asked only where flow mode is otherwise wanted");
    CHECK(r.segments >= 1 && r.segments <= (q.segments > 0 ? r.chunks : std::min(8L, r.chunks)), "segments %ld of %ld chunks", r.segments, r.chunks);
    if (r.segments > 1) CHECK(r.carry == CARRY_SERIAL || r.carry == CARRY_RELAY, "segments are the exact pass's");
    if (r.vec_store) CHECK(q.out % 16 == 0 && q.out_stride % 2 == 0 && q.fdx_bytes == 8 && q.nbins % 2 == 0 && !q.row_pointers, "16-byte stores need alignment");
    if (r.rows_f32) CHECK(r.kernel == FK_ROWS && !q.fuse && q.fd_bytes == 4 && r.vec_store && q.nbins % 128 == 0, "the bin-pair kernel");
    if (r.fused) CHECK(q.fd_bytes == 8 && r.carry == CARRY_SUMS && (r.kernel == FK_ROWS || q.fuse), "fused arithmetic only where bits are not claimed");
    if (r.self) CHECK(r.chunks > 1 && q.fd_bytes == 8 && !q.exact && !q.every && !q.row_pointers && (r.kernel == FK_ROWS || q.fuse), "self-carried");
    if (r.pipelined) CHECK(!q.fuse && q.pipe_wanted && q.analysis_batch && q.pipeline && r.out.hi > r.out.lo, "pipelined");
    if (r.arm_flag) CHECK(r.segments == 1 && (r.kernel == FK_ROWS || q.fuse), "the completion word");
  }
}

static ForwardQuery fq(size_t n, size_t m, size_t ch, size_t fd, int window, bool exact)
{
  ForwardQuery q;
  q.n = n; q.nbins = m; q.channels = ch; q.fd_bytes = fd; q.fdx_bytes = 2 * fd; q.window = window; q.exact = exact;
  q.out = (uintptr_t)1 << 40; q.out_stride = n * m;
  return q;
}

// routes of named shapes: BASELINE.json configs[0..4], the streaming hop, the decimated analysis and what the GPU tests force
static void test_forward_shapes()
{
  struct Shape { const char* name; ForwardQuery q; int kernel, self, pipelined; long chunks, len; int carry, sums; unsigned L; int flow; long segments; int rows_f32, fused; };
  ForwardQuery pipe = fq(48000, 1024, 1, 8, kWindowHann, false); pipe.analysis_batch = pipe.pipe_wanted = true;
  ForwardQuery tiles_q = fq(48000, 1024, 1, 8, kWindowHann, false); tiles_q.rows_kernel = 0;
  ForwardQuery every = fq(48000, 1024, 1, 8, kWindowHann, false); every.every = true;
  ForwardQuery smoke = fq(6000, 1024, 1, 8, kWindowHann, false); smoke.chunk = 256;
  ForwardQuery smoke32 = fq(6000, 256, 1, 4, kWindowBlackman, true); smoke32.chunk = 512;
  ForwardQuery seg = fq(6000, 256, 1, 8, kWindowHann, true); seg.chunk = 200; seg.segments = 7;
  ForwardQuery serial = seg; serial.chain = 0;
  ForwardQuery mixed = fq(48000, 1000, 1, 8, kWindowHann, false); mixed.self = 0; mixed.fft_carry = 2;
  const Shape shapes[] = {
    {"configs[0], north star", fq(48000, 1024, 1, 8, kWindowHann, false), FK_ROWS, 1, 0, 250, 192, CARRY_STATE, SUMS_NONE, 0, 0, 1, 0, 0},
    {"configs[0], two matrices in turn", pipe, FK_ROWS, 1, 1, 300, 160, CARRY_STATE, SUMS_NONE, 0, 0, 1, 0, 0},
    {"configs[1], n = 1e6", fq(1000000, 1024, 1, 8, kWindowHann, false), FK_ROWS, 0, 0, 511, 1960, CARRY_SUMS, SUMS_FFT2, 0, 0, 1, 0, 1},
    {"configs[2], m = 4096 FD float", fq(262144, 4096, 1, 4, kWindowBlackman, true), FK_ROWS, 0, 0, 2048, 128, CARRY_RELAY, SUMS_NONE, 128, 1, 1, 1, 0},
    {"configs[3], 64 x 48000, m = 2048", fq(48000, 2048, 64, 8, kWindowHann, false), FK_ROWS, 1, 0, 8, 6000, CARRY_STATE, SUMS_NONE, 0, 0, 1, 0, 0},
    {"configs[4], 64 x 48000 per GPU", fq(48000, 1024, 64, 8, kWindowHann, false), FK_ROWS, 1, 0, 8, 6000, CARRY_STATE, SUMS_NONE, 0, 0, 1, 0, 0},
    {"hop of 100 at m = 1000", fq(100, 1000, 1, 8, kWindowHann, false), FK_HOP, 0, 0, 1, 100, CARRY_STATE, SUMS_NONE, 0, 0, 1, 0, 0},
    {"every, n = 48000", every, FK_EVERY, 0, 0, 182, 264, CARRY_SUMS, SUMS_FFT2, 0, 0, 1, 0, 0},
    {"rows_kernel 0", tiles_q, FK_TILES, 0, 0, 750, 64, CARRY_SUMS, SUMS_DIRECT, 0, 0, 1, 0, 0},
    {"smoke, chunk 256", smoke, FK_ROWS, 1, 0, 24, 256, CARRY_STATE, SUMS_NONE, 0, 0, 1, 0, 0},
    {"smoke, f32f32 exact, chunk 512", smoke32, FK_ROWS, 0, 0, 12, 512, CARRY_RELAY, SUMS_NONE, 128, 1, 1, 1, 0},
    {"exact, chunk 200, segments 7", seg, FK_ROWS, 0, 0, 30, 200, CARRY_RELAY, SUMS_NONE, 8, 0, 7, 0, 0},
    {"exact, chain 0, segments 7", serial, FK_ROWS, 0, 0, 30, 200, CARRY_SERIAL, SUMS_NONE, 0, 0, 7, 0, 0},
    {"2N = 2000, mixed-radix sums", mixed, FK_ROWS, 0, 0, 250, 192, CARRY_SUMS, SUMS_FFT_MIXED, 0, 0, 1, 0, 1},
  };
  for (const Shape& s : shapes)
  {
    const ForwardRoute r = forward_route(s.q, [] { return true; });
    CHECK(r.kernel == s.kernel && r.self == (s.self != 0) && r.pipelined == (s.pipelined != 0), "%s: kernel %d self %d pipelined %d", s.name, r.kernel, (int)r.self, (int)r.pipelined);
    CHECK(r.chunks == s.chunks && r.len == s.len, "%s: %ld x %ld", s.name, r.chunks, r.len);
    CHECK(r.carry == s.carry && r.sums == s.sums && r.relay_L == s.L && r.flow == (s.flow != 0) && r.segments == s.segments, "%s: carry %d sums %d L %u flow %d segments %ld",
          s.name, r.carry, r.sums, r.relay_L, (int)r.flow, r.segments);
    CHECK(r.rows_f32 == (s.rows_f32 != 0) && r.fused == (s.fused != 0), "%s: rows_f32 %d fused %d", s.name, (int)r.rows_f32, (int)r.fused);
  }
}

// ---- the form of a synthesis (inverse_route) ----------------------------------------------------------------------------------
static InverseQuery iq(size_t n, size_t m, size_t ch, size_t td, size_t fd)
{
  InverseQuery q;
  q.n = n; q.channels = ch; q.nbins = m; q.td_bytes = td; q.fd_bytes = fd; q.in_stride = n * m; q.y_stride = n; q.in = (uintptr_t)1 << 40;
  const size_t matrix = ch * n * m * 2 * fd;
  q.nt = inverse_streaming_loads(matrix, -1); q.nt_skip = inverse_ordinary_rows(matrix, m * 2 * fd, -1);
  return q;
}

static void test_inverse_routes()
{
  const double GiB = 1073741824.0;
  static const size_t types[4][2] = {{4, 8}, {4, 4}, {8, 8}, {8, 4}};
  static const size_t ms[] = {6, 64, 320, 1000, 1024, 1536, 2048, 4096};
  for (int it = 0; it < 100000; ++it)
  {
    const int ty = (int)rnd_in(0, 3);
    InverseQuery q = iq(rnd_in(0, 2) == 0 ? rnd_in(1, 2000) : rnd_in(1, 1200000), ms[rnd() % 8], (rnd() & 3) ? 1 : rnd_in(1, 64), types[ty][0], types[ty][1]);
    if ((rnd() & 3) == 0) q.in_stride += 1;
    if ((rnd() & 3) == 0) q.in += 8;
    q.row_pointers = (rnd() & 7) == 0; q.lat1 = rnd() & 1; q.ops = (rnd() & 3) == 0;
    if (rnd() & 1) { q.nt = rnd() & 1; q.nt_skip = (rnd() & 1) ? 0 : rnd_in(1, 100000); }
    q.capacity4 = (rnd() & 1) ? 0 : rnd_in(1, 20000); q.capacity8 = q.capacity4 ? rnd_in(1, 20000) : 0;
    q.ordered_failed = (rnd() & 7) == 0;
    q.exact = (rnd() & 7) != 0; q.rows = (rnd() & 7) ? 0 : (1L << rnd_in(0, 5)); q.step = (long)rnd_in(0, 2) - 1; q.ordered = (long)rnd_in(0, 2) - 1;
    q.tune = (rnd() & 3) != 0; q.verify = (rnd() & 7) != 0; q.nt_skip_mb = (rnd() & 3) ? -1 : (long)rnd_in(0, 2000);
    const bool geo = rnd() & 1, events = (rnd() & 7) != 0;
    int geos = 0, evs = 0, caps = 0;
    auto geometry = [&] { ++geos; return geo; };
    auto tune_events = [&] { ++evs; return events; };
    auto capacity = [&](size_t& c4, size_t& c8) { ++caps; c4 = q.capacity4; c8 = q.capacity8; };
    const InverseRoute r = inverse_route(q, geometry, tune_events, capacity);
    const size_t rows = q.channels * q.n;
    const double matrix = (double)rows * (double)q.nbins * (double)(2 * q.fd_bytes);
    const bool ordered_ok = !q.ops && q.exact && q.rows <= 0 && q.ordered >= 0 && rows_ordered_ok(q, [&] { return geo; });
    CHECK(geos <= 1 && evs <= 1 && caps <= 1, "every probe at most once: %d %d %d", geos, evs, caps);
    if (caps) CHECK(!r.tuned && q.capacity4 == 0 && !q.ops && q.rows <= 0 && rows > 1024 && rows < 65536, "the occupancy is asked by the static streaming form only");
    if (evs) CHECK(!q.ops && q.tune && q.exact && q.rows <= 0 && rows >= 8192, "the tuner's events only where it may run");
    if (r.tuned) CHECK(evs == 1 && events, "tuned calls have their events");
    if (q.ops) CHECK(!r.tuned && r.form != F_ORDERED && r.form != F_STEP, "operations never take the ordered, in-step or tuned forms");
    if (!q.exact) CHECK(!r.tuned && r.form == F_TREE, "exact_inverse = 0: the tree sum");
    if (!r.tuned && r.form == F_ORDERED) CHECK(ordered_ok && !q.ordered_failed, "the static ordered form where it applies");
    if (!r.tuned && r.form == F_STEP) CHECK(rows_in_step_ok(q) && q.exact && q.rows <= 0, "rows in step where they apply");
    if (!r.tuned) continue;
    CHECK(r.count >= 1 && r.count <= FormTuner::kMax, "%d candidates", r.count);
    const bool both_loads = q.nt && q.nt_skip_mb < 0 && matrix >= 2.0 * GiB && matrix < 16.0 * GiB;
    for (int i = 0; i < r.count; ++i)
    {
      const int f = r.cand[i].form;
      CHECK(f != F_TREE && f != F_ROW, "candidates are the bit-identical streaming forms");
      CHECK(f != F_32 || q.fd_bytes == 8, "F_32 is never a candidate at FD float");
      CHECK(f != F_8W || !ordered_ok, "F_8W is never a candidate where the ordered form applies");
      CHECK(f != F_ORDERED || ordered_ok, "F_ORDERED only where it applies");
      CHECK(f != F_STEP || rows_in_step_ok(q), "F_STEP only where it applies");
      int same = 0;
      for (int j = 0; j < r.count; ++j)
      {
        if (j != i) CHECK(!(r.cand[j].form == f && r.cand[j].nt_skip == r.cand[i].nt_skip), "no duplicate pairs");
        if (r.cand[j].form == f) ++same;
      }
      CHECK(same == (both_loads ? 2 : 1), "with both kinds of load every form is tried both ways: form %d %d times", f, same);
    }
    CHECK(r.cand[0].nt_skip == q.nt_skip, "entry 0 takes the call's own loads");
    if (q.ordered_failed) continue;
    // entry 0 is the static choice: the route without the tuner (with the same capacities)
    InverseQuery s = q; s.tune = 0;
    const InverseRoute st = inverse_route(s, [&] { return geo; }, [] { return true; }, [&](size_t& c4, size_t& c8) { c4 = q.capacity4; c8 = q.capacity8; });
    CHECK(!st.tuned && st.form == r.cand[0].form, "entry 0 (%d) is the static choice (%d)", r.cand[0].form, st.form);
  }
}

static void test_inverse_shapes()
{
  struct Shape { const char* name; InverseQuery q; bool geo; bool tuned; int form; int count; long code; };
  InverseQuery c1_static = iq(1000000, 1024, 1, 4, 8); c1_static.tune = 0;
  InverseQuery c1_step = c1_static; c1_step.ordered = -1;
  InverseQuery c1_refused = c1_static; c1_refused.ordered_failed = true;
  InverseQuery tree = iq(48000, 1024, 1, 4, 8); tree.exact = 0;
  InverseQuery verify = iq(4096, 1024, 1, 4, 8); verify.tune = 0;
  InverseQuery rows4 = iq(48000, 1024, 1, 4, 8); rows4.rows = 4;
  InverseQuery op = iq(48000, 1024, 1, 8, 8); op.ops = true;
  InverseQuery forced = iq(70000, 1024, 1, 8, 8); forced.ordered = 1;
  const Shape shapes[] = {
    {"configs[0], north star", iq(48000, 1024, 1, 4, 8), true, true, F_ORDERED, 4, 4},
    {"configs[1], n = 1e6", iq(1000000, 1024, 1, 4, 8), true, true, F_ORDERED, 6, 4},
    {"configs[1], inverse_tune 0", c1_static, true, false, F_ORDERED, 0, 4},
    {"configs[1], inverse_tune 0, inverse_ordered -1", c1_step, true, false, F_STEP, 0, 3},
    {"configs[1], the ordered form's LDS refused", c1_refused, true, false, F_STEP, 0, 3},
    {"configs[2], m = 4096 FD float", iq(262144, 4096, 1, 4, 4), false, true, F_16, 6, 1},
    {"configs[3], 64 x 48000, m = 2048", iq(48000, 2048, 64, 4, 8), false, true, F_STEP, 4, 3},
    {"hop of 100 at m = 1000", iq(100, 1000, 1, 4, 8), true, false, F_ROW, 0, 1},
    {"exact_inverse 0", tree, true, false, F_TREE, 0, 0},
    {"n = 4096, inverse_tune 0", verify, true, false, F_VERIFY, 0, 2},
    {"inverse_rows 4", rows4, true, false, F_4, 0, 1},
    {"an operation, f64f64", op, true, false, F_16, 0, 1},
    {"inverse_ordered 1", forced, true, false, F_ORDERED, 0, 4},
  };
  for (const Shape& s : shapes)
  {
    const InverseRoute r = inverse_route(s.q, [&] { return s.geo; }, [] { return true; }, [](size_t& c4, size_t& c8) { c4 = c8 = (size_t)-1; });
    const int form = r.tuned ? r.cand[0].form : r.form;
    CHECK(r.tuned == s.tuned && form == s.form && (!r.tuned || r.count == s.count) && inverse_form_code(form) == s.code,
          "%s: tuned %d form %d count %d", s.name, (int)r.tuned, form, r.count);
  }
  // configs[2]: the whole list -- three forms, each with and without the rows read first by ordinary loads
  const InverseRoute r = inverse_route(iq(262144, 4096, 1, 4, 4), [] { return false; }, [] { return true; }, [](size_t&, size_t&) {});
  const InverseCandidate want[6] = {{F_16, 49152}, {F_16, 0}, {F_8W, 49152}, {F_8W, 0}, {F_16W, 49152}, {F_16W, 0}};
  for (int i = 0; i < 6; ++i) CHECK(r.cand[i].form == want[i].form && r.cand[i].nt_skip == want[i].nt_skip, "configs[2] candidate %d: %d %zu", i, r.cand[i].form, r.cand[i].nt_skip);
  CHECK(inverse_tuned_code(F_ORDERED, false) == 7 && inverse_tuned_code(F_STEP, true) == 16 && inverse_form_rows(F_8W) == 8, "codes");
  CHECK(relays(1024) == 32 && relays(1000) == 32 && relays(1) == 1, "relays of 32 bins");
  CHECK(xcd_groups(true, 16) == 16 && xcd_groups(true, 15) == 0 && xcd_groups(false, 100) == 0, "xcd map");
}

// ---- host memory: the route of an analysis / synthesis call (host_route) ------------------------------------------------------
// what the callables answer, and the order in which they were asked: I ensure_io, M map matrix, S map samples, P ensure_pin, D pin_idle
struct HostEnv { bool io = true, mat = false, smp = false, pin = true, idle = true; std::string asked; };
struct HostTaken { int route, samples; bool refused; };
static HostRoute take(const HostQuery& q, HostEnv& e)
{
  return host_route(q, [&] { e.asked += 'I'; return e.io; }, [&] { e.asked += 'M'; return e.mat; }, [&] { e.asked += 'S'; return e.smp; },
                    [&] { e.asked += 'P'; return e.pin; }, [&] { e.asked += 'D'; return e.idle; });
}
// The two ladders of conditions as sdft_n and isdft_n spelled them before host_route replaced both (the scratch and the "small"
// threshold were two constants of the same value): the models host_route is held against, callable by callable
static HostTaken ladder_analysis(const HostQuery& q, HostEnv& e)
{
  const size_t kIo = (size_t)64 << 10, kSmall = (size_t)64 << 10, kDirect = (size_t)4 << 20;
  const bool xd = q.samples_device, od = q.matrix_device;
  const size_t xbytes = q.samples_bytes, obytes = q.matrix_bytes;
  auto io = [&] { e.asked += 'I'; return e.io; };
  if (xd && od) return {HR_DEVICE, HS_AS_IS, false};
  if (!xd && od && xbytes <= kIo && q.pinned_io && io()) return {HR_SCRATCH, HS_IO, false};
  {
    const bool small_x = xbytes <= kSmall;
    const bool om = od ? true : (e.asked += 'M', e.mat);
    bool xm = xd ? true : ((q.by_value || small_x) ? false : (e.asked += 'S', e.smp));
    bool staged = false;
    if (om && !xm && !xd && small_x) { xm = true; staged = true; }
    if (xm && om) return {HR_MAPPED, xd ? HS_AS_IS : staged ? HS_STAGE_TD : HS_MAPPED, false};
  }
  if (!od && q.host_copy == 0 && q.host_direct && obytes <= kDirect && (xd || xbytes <= kSmall) && (e.asked += 'P', e.pin))
  {
    if (!(e.asked += 'D', e.idle)) return {HR_DIRECT, HS_AS_IS, true};
    int xm = HS_AS_IS;
    if (!xd) xm = (xbytes <= kIo && q.pinned_io && io()) ? HS_IO : HS_STAGE_TD;
    return {HR_DIRECT, xm, false};
  }
  return {HR_STAGED, xd ? HS_AS_IS : HS_STAGE_TD, false};
}
static HostTaken ladder_synthesis(const HostQuery& q, HostEnv& e)
{
  const size_t kIo = (size_t)64 << 10, kSmall = (size_t)64 << 10, kDirect = (size_t)4 << 20;
  const bool yd = q.samples_device, id = q.matrix_device;
  const size_t ybytes = q.samples_bytes, ibytes = q.matrix_bytes;
  auto io = [&] { e.asked += 'I'; return e.io; };
  if (id && yd) return {HR_DEVICE, HS_AS_IS, false};
  if (id && !yd && ybytes <= kIo && q.pinned_io && io()) return {HR_SCRATCH, HS_IO, false};
  {
    const bool small_y = ybytes <= kSmall;
    const bool im = id ? true : (e.asked += 'M', e.mat);
    bool ym = yd ? true : (small_y ? false : (e.asked += 'S', e.smp));       // (y_class is not looked at: the one difference)
    bool staged = false;
    if (im && !ym && !yd && small_y) { ym = true; staged = true; }
    if (im && ym) return {HR_MAPPED, yd ? HS_AS_IS : staged ? HS_STAGE_TD : HS_MAPPED, false};
  }
  if (!id && q.host_copy == 0 && q.host_direct && ibytes <= kDirect && (yd || ybytes <= kSmall) && (e.asked += 'P', e.pin))
  {
    if (!(e.asked += 'D', e.idle)) return {HR_DIRECT, HS_AS_IS, true};
    const bool through_io = !yd && ybytes <= kIo && q.pinned_io && io();
    return {HR_DIRECT, yd ? HS_AS_IS : through_io ? HS_IO : HS_STAGE_TD, false};
  }
  return {HR_STAGED, yd ? HS_AS_IS : HS_STAGE_TD, false};
}

static HostQuery hq(bool analysis, size_t n, size_t m, size_t ch, size_t td, size_t fd, bool samples_device, bool matrix_device)
{
  HostQuery q;
  q.analysis = analysis; q.samples_device = samples_device; q.matrix_device = matrix_device; q.n = n;
  q.samples_bytes = ch * n * td; q.row_bytes = ch * m * 2 * fd; q.matrix_bytes = n * q.row_bytes;
  return q;
}

static void test_host_routes()
{
  static const size_t sizes[] = {0, 1, 400, ((size_t)64 << 10) - 1, (size_t)64 << 10, ((size_t)64 << 10) + 1, (size_t)1 << 20, ((size_t)4 << 20) - 1, (size_t)4 << 20,
                                 ((size_t)4 << 20) + 1, (size_t)256 << 20, (size_t)3 << 30};
  size_t differ = 0;
  for (int it = 0; it < 200000; ++it)
  {
    HostQuery q;
    q.samples_device = (rnd() & 3) == 0; q.matrix_device = (rnd() & 3) == 0; q.by_value = (rnd() & 3) == 0;
    q.samples_bytes = (rnd() & 1) ? sizes[rnd() % 12] : rnd_in(1, (size_t)1 << 22);
    q.matrix_bytes = (rnd() & 1) ? sizes[rnd() % 12] : rnd_in(1, (size_t)1 << 24);
    q.pinned_io = (rnd() & 3) != 0; q.host_copy = (rnd() & 3) == 0; q.host_direct = (rnd() & 3) != 0;
    q.n = rnd_in(1, 2000000); q.row_bytes = (rnd() & 7) ? rnd_in(1, 70000) : 0; q.stage_bytes = (rnd() & 1) ? kDefaultStageBytes : rnd_in(1, (size_t)1 << 26);
    HostEnv e;
    e.io = (rnd() & 7) != 0; e.mat = rnd() & 1; e.smp = rnd() & 1; e.pin = (rnd() & 7) != 0; e.idle = (rnd() & 7) != 0;
    HostTaken both[2]; std::string asked[2];
    for (int analysis = 0; analysis < 2; ++analysis)
    {
      q.analysis = analysis != 0;
      HostEnv a = e, b = e;
      const HostRoute r = take(q, a);
      const HostTaken want = analysis ? ladder_analysis(q, b) : ladder_synthesis(q, b);
      both[analysis] = HostTaken{r.route, r.samples, r.refused}; asked[analysis] = a.asked;
      CHECK(r.route == want.route && r.refused == want.refused && (r.refused || r.samples == want.samples), "the ladder's route: %d / %d, samples %d / %d", r.route, want.route, r.samples, want.samples);
      CHECK(a.asked == b.asked, "the ladder's questions in the ladder's order: '%s' / '%s'", a.asked.c_str(), b.asked.c_str());
      const bool sd = q.samples_device, md = q.matrix_device, small = q.samples_bytes <= kSmallHostBytes;
      // exactly one route, and what belongs to it
      CHECK(r.route >= HR_DEVICE && r.route <= HR_STAGED, "a route");
      CHECK(r.end == (r.route <= HR_SCRATCH ? HE_FINISH : r.route == HR_STAGED ? HE_SYNCHRONIZE : HE_FINISH_MAPPED), "route %d ends in %d", r.route, r.end);
      CHECK(r.pipe_allowed == (r.route == HR_DEVICE) && r.flag_wanted == (r.route <= HR_SCRATCH) && r.synchronous == (r.route == HR_SCRATCH), "flags of route %d", r.route);
      CHECK((r.route == HR_DEVICE) == (sd && md), "the device route exactly for device memory on both sides");
      CHECK((r.samples == HS_AS_IS) == (sd || r.refused), "device samples are used where they are");
      if (r.refused) CHECK(r.route == HR_DIRECT && !e.idle, "only busy pinned pieces refuse a call");
      if (r.route == HR_SCRATCH || r.samples == HS_IO) CHECK(!sd && small && q.pinned_io && e.io, "the scratch only within its size");
      if (r.samples == HS_MAPPED) CHECK(r.route == HR_MAPPED && !small && e.smp, "mapped samples");
      if (r.route == HR_MAPPED) CHECK(md || e.mat, "mapped matrix");
      if (r.route == HR_DIRECT) CHECK(!md && q.matrix_bytes <= kDirectBytes && q.host_copy == 0 && q.host_direct && (sd || small), "the pinned pieces only for a hop-sized matrix");
      CHECK((r.route == HR_STAGED) == (r.seg != 0), "a segment length exactly on the staged route");
      if (r.route == HR_STAGED) CHECK(r.seg >= 1 && r.seg <= q.n && r.seg == stage_rows(q.n, q.row_bytes, q.stage_bytes), "staged segments of %zu rows", r.seg);
      // no callable twice, none where its precondition is false
      for (char c : {'I', 'M', 'S', 'P', 'D'}) CHECK(std::count(a.asked.begin(), a.asked.end(), c) <= 1, "'%c' asked twice: %s", c, a.asked.c_str());
      auto was = [&](char c) { return a.asked.find(c) != std::string::npos; };
      if (was('I')) CHECK(!sd && small && q.pinned_io, "ensure_io without small host samples");
      if (was('M')) CHECK(!md, "a device matrix mapped");
      if (was('S')) CHECK(!sd && !small && !(q.analysis && q.by_value), "samples mapped that are not worth it");
      const bool direct_ok = !md && q.host_copy == 0 && q.host_direct && q.matrix_bytes <= kDirectBytes && (sd || small);
      if (was('P')) CHECK(direct_ok, "ensure_pin off the direct route");
      if (was('D')) CHECK(direct_ok && e.pin && a.asked.find('P') < a.asked.find('D'), "pin_idle before ensure_pin");
      if (was('M') && was('S')) CHECK(a.asked.find('M') < a.asked.find('S'), "the matrix is mapped before the samples");
    }
    // The two directions take the same route and ask the same questions -- but for the ONE difference of the two ladders: the
    // by-value sample of sdft_sdft is never registered in place (x_class == 0 keeps map_host off it), the by-value result of
    // sdft_isdft is (isdft_n does not look at y_class there); it shows only beyond 64 KiB of samples, that is 16 Ki channels
    const bool named = q.by_value && !q.samples_device && q.samples_bytes > kSmallHostBytes;
    const bool same = both[0].route == both[1].route && both[0].samples == both[1].samples && both[0].refused == both[1].refused && asked[0] == asked[1];
    if (!named) CHECK(same, "analysis and synthesis disagree: route %d / %d, asked '%s' / '%s'", both[1].route, both[0].route, asked[1].c_str(), asked[0].c_str());
    else { CHECK(asked[1].find('S') == std::string::npos && asked[0].find('S') != std::string::npos, "the by-value sample is not mapped, the by-value result is"); ++differ; }
  }
  CHECK(differ > 100, "the difference was exercised: %zu", differ);
}

// HostIo::map_host: option host_register on, buffers of 1 MiB ... 256 MiB
static HostEnv registering(const HostQuery& q, bool on)
{
  HostEnv e;
  auto ok = [&](size_t bytes) { return on && bytes >= ((size_t)1 << 20) && bytes <= ((size_t)256 << 20); };
  e.mat = ok(q.matrix_bytes); e.smp = ok(q.samples_bytes);
  return e;
}
static void test_host_shapes()
{
  struct Shape { const char* name; HostQuery q; bool host_register; int route, samples, end; const char* asked; };
  const HostQuery hop = hq(true, 100, 1000, 1, 4, 8, false, false);                       // test/test.c: 100 x 1000 bins, malloc'ed buffers
  HostQuery hop_copy = hop; hop_copy.host_copy = 1;
  HostQuery hop_nodirect = hop; hop_nodirect.host_direct = 0;
  HostQuery hop_nopinned = hop; hop_nopinned.pinned_io = 0;
  HostQuery hop_dev = hq(true, 100, 1000, 1, 4, 8, false, true); 
  HostQuery hop_dev_nopinned = hop_dev; hop_dev_nopinned.pinned_io = 0;
  HostQuery sample = hq(true, 1, 1000, 1, 4, 8, false, true); sample.by_value = true;     // sdft_sdft on a device row
  HostQuery result = sample; result.analysis = false;                                     // sdft_isdft
  const Shape shapes[] = {
    {"the reference driver's hop", hop, false, HR_DIRECT, HS_IO, HE_FINISH_MAPPED, "MPDI"},
    {"the hop, synthesis", hq(false, 100, 1000, 1, 4, 8, false, false), false, HR_DIRECT, HS_IO, HE_FINISH_MAPPED, "MPDI"},
    {"the hop, host_copy 1", hop_copy, false, HR_STAGED, HS_STAGE_TD, HE_SYNCHRONIZE, "M"},
    {"the hop, host_direct 0", hop_nodirect, false, HR_STAGED, HS_STAGE_TD, HE_SYNCHRONIZE, "M"},
    {"the hop, pinned_io 0", hop_nopinned, false, HR_DIRECT, HS_STAGE_TD, HE_FINISH_MAPPED, "MPD"},
    {"the hop, host_register 1 (1.6 MB)", hop, true, HR_MAPPED, HS_STAGE_TD, HE_FINISH_MAPPED, "M"},
    {"half the hop, host_register 1 (below 1 MiB)", hq(true, 50, 1000, 1, 4, 8, false, false), true, HR_DIRECT, HS_IO, HE_FINISH_MAPPED, "MPDI"},
    {"n = 10000, host_register 1 (160 MB)", hq(true, 10000, 1000, 1, 4, 8, false, false), true, HR_MAPPED, HS_STAGE_TD, HE_FINISH_MAPPED, "M"},
    {"n = 300000 f64 samples, host_register 1 (samples 2.4 MB, matrix beyond 256 MiB)", hq(true, 300000, 1000, 1, 8, 8, false, false), true, HR_STAGED, HS_STAGE_TD, HE_SYNCHRONIZE, "MS"},
    {"n = 15000 f64 samples, host_register 1 (matrix 240 MB, samples below 1 MiB)", hq(true, 15000, 1000, 1, 8, 8, false, false), true, HR_STAGED, HS_STAGE_TD, HE_SYNCHRONIZE, "MS"},
    {"n = 8000 x 20 channels, host_register 1 (both mapped)", hq(true, 8000, 64, 20, 8, 8, false, false), true, HR_MAPPED, HS_MAPPED, HE_FINISH_MAPPED, "MS"},
    {"sdft_sdft, device row", sample, false, HR_SCRATCH, HS_IO, HE_FINISH, "I"},
    {"sdft_isdft, device row", result, false, HR_SCRATCH, HS_IO, HE_FINISH, "I"},
    {"host hop, device matrix", hop_dev, false, HR_SCRATCH, HS_IO, HE_FINISH, "I"},
    {"host hop, device matrix, pinned_io 0", hop_dev_nopinned, false, HR_MAPPED, HS_STAGE_TD, HE_FINISH_MAPPED, ""},
    {"device / device", hq(true, 48000, 1024, 1, 4, 8, true, true), false, HR_DEVICE, HS_AS_IS, HE_FINISH, ""},
    {"device samples, host hop matrix", hq(true, 100, 1000, 1, 4, 8, true, false), false, HR_DIRECT, HS_AS_IS, HE_FINISH_MAPPED, "MPD"},
    {"n = 1e6 x 1024, host / host", hq(true, 1000000, 1024, 1, 4, 8, false, false), false, HR_STAGED, HS_STAGE_TD, HE_SYNCHRONIZE, "MS"},
  };
  for (const Shape& s : shapes)
  {
    HostEnv e = registering(s.q, s.host_register);
    const HostRoute r = take(s.q, e);
    CHECK(r.route == s.route && r.samples == s.samples && r.end == s.end && !r.refused, "%s: route %d samples %d end %d", s.name, r.route, r.samples, r.end);
    CHECK(e.asked == s.asked, "%s: asked '%s'", s.name, e.asked.c_str());
  }
  HostEnv e;
  HostRoute r = take(sample, e);
  CHECK(r.synchronous && r.flag_wanted && !r.pipe_allowed, "sdft_sdft on a device row: synchronous, completion word wanted");
  e = HostEnv{}; r = take(hq(false, 48000, 1024, 1, 4, 8, true, true), e);
  CHECK(r.pipe_allowed && r.flag_wanted && !r.synchronous, "device / device may leave the plan's stream");
  e = HostEnv{}; r = take(hq(true, 1000000, 1024, 1, 4, 8, false, false), e);
  CHECK(r.seg == stage_rows(1000000, 16384, kDefaultStageBytes) && r.seg == 65536, "n = 1e6 x 1024 in segments of %zu rows", r.seg);
  // the scratch or the pinned pieces cannot be had, or are busy
  e = HostEnv{}; e.io = false; r = take(hop_dev, e);
  CHECK(r.route == HR_MAPPED && r.samples == HS_STAGE_TD && e.asked == "I", "no scratch: the hop's samples through device scratch (%d, %d)", r.route, r.samples);
  e = HostEnv{}; e.io = false; r = take(hop, e);
  CHECK(r.route == HR_DIRECT && r.samples == HS_STAGE_TD && e.asked == "MPDI", "no scratch beside the pinned pieces (%d, %d)", r.route, r.samples);
  e = HostEnv{}; e.pin = false; r = take(hop, e);
  CHECK(r.route == HR_STAGED && r.seg == 100 && e.asked == "MP", "no pinned pieces: staged (%d)", r.route);
  e = HostEnv{}; e.idle = false; r = take(hop, e);
  CHECK(r.route == HR_DIRECT && r.refused && e.asked == "MPD", "busy pinned pieces fail the call (%d)", r.route);
  // a matrix that was registered stays registered when the samples then cannot be
  e = HostEnv{}; e.mat = true; e.smp = false; r = take(hq(true, 300000, 64, 1, 8, 8, false, false), e);
  CHECK(r.route == HR_STAGED && e.asked == "MS", "matrix mapped, samples not: falls through (%d)", r.route);
}

// ---- the fused call (process_route) ---------------------------------------------------------------------------------------------
static ProcessQuery pq(size_t n, size_t m, size_t ch, size_t fd, bool exact)
{
  ProcessQuery q;
  q.fd_bytes = fd; q.fdx_bytes = 2 * fd;
  q.chunk.n = n; q.chunk.channels = ch; q.chunk.nbins = m; q.chunk.exact = exact; q.chunk.rows_kernel = rows_kernel_ok(m, 2 * fd, false, true, 2);
  q.chunk.row_waves = row_waves(m, 2 * fd); q.chunk.tiles = tiles(m, kWindowHann, 2 * fd, 0);
  return q;
}
// process_n's decisions as it spelled them in place before process_route
static ProcessRoute process_in_place(const ProcessQuery& q, size_t free_b, int& asked)
{
  ProcessRoute r;
  const size_t n = q.chunk.n, nbins = q.chunk.nbins, channels = q.chunk.channels;
  const bool dfts = q.spectrum, ordered = q.fused_exact < 0 ? (q.chunk.exact && q.fd_bytes == 8) : q.fused_exact != 0;
  const long chunks = choose_chunks(q.chunk).chunks;
  const bool walk_loses = row_slots(nbins, q.fdx_bytes) == 2 && q.fd_bytes == 4 && q.chunk.exact && q.fused_exact == 1;
  const bool one_chunk_folded = chunks == 1 && n <= 512 && !ordered && !dfts && q.fold && nbins >= 8 && q.hop_kernel && q.linear && q.gain_rows <= 1;
  if (one_chunk_folded) { r.path = PP_HOP_FOLDED; r.fold = true; r.flag_wanted = q.x_device && q.y_device; return r; }
  if ((q.chunk.rows_kernel || (q.linear && q.gain_rows <= 65535u && !ordered && !dfts && q.fold && nbins >= 8 && nbins <= (size_t)4 * 64 * 16)) && (chunks > 1 || n > 512) && !walk_loses)
  { r.path = PP_FUSED_ROWS; r.fold = !dfts; r.flag_wanted = q.x_device && q.y_device; return r; }
  const size_t row_elems = channels * nbins;
  size_t seg = dfts ? n : std::min(n, std::max<size_t>(1, q.stage_bytes / std::max<size_t>(row_elems * q.fdx_bytes, 1)));
  if (!dfts && seg < n && q.stage_bytes == ((size_t)1 << 30))
  {
    if (q.workspace >= row_elems * n) seg = n;
    else { ++asked; if (free_b) seg = std::max(seg, std::min(n, (free_b / 2) / std::max<size_t>(row_elems * q.fdx_bytes, 1))); }
  }
  r.path = chunks == 1 ? PP_HOP_PAIR : PP_SEGMENTS; r.seg = seg;
  if (q.user)
  {
    const size_t m_first = std::min(seg, n), m_last = n - ((n - 1) / seg) * seg;
    const bool hop_form = q.exact_inverse && q.inverse_rows <= 0;
    r.rtc_hop = hop_form && (channels * m_first <= 1024 || channels * m_last <= 1024);
    r.rtc_rows = !hop_form || channels * m_first > 1024 || channels * m_last > 1024 || dfts;
  }
  return r;
}

static void test_process_routes()
{
  static const size_t ms[] = {4, 7, 8, 64, 1000, 1024, 2048, 2049, 4096, 4097, 8192};
  for (int it = 0; it < 200000; ++it)
  {
    const size_t fd = (rnd() & 1) ? 8 : 4;
    ProcessQuery q = pq((rnd() & 1) ? rnd_in(1, 1200) : rnd_in(1, 2000000), ms[rnd() % 11], (rnd() & 3) ? 1 : rnd_in(1, 64), fd, fd == 4 || (rnd() & 3) == 0);
    if ((rnd() & 7) == 0) q.chunk.rows_kernel = false;
    q.chunk.forced_chunk = (rnd() & 7) ? 0 : (long)rnd_in(1, 5000);
    q.linear = (rnd() & 3) != 0; q.user = !q.linear && (rnd() & 1); q.gain_rows = (rnd() & 3) ? 1 : ((rnd() & 1) ? rnd_in(2, 65535) : rnd_in(65536, 100000));
    q.spectrum = (rnd() & 3) == 0; q.x_device = rnd() & 1; q.y_device = rnd() & 1;
    q.fused_exact = (long)rnd_in(0, 3) - 1; q.fold = (rnd() & 7) != 0; q.hop_kernel = (rnd() & 7) != 0; q.exact_inverse = (rnd() & 7) != 0; q.inverse_rows = (rnd() & 7) ? 0 : 4;
    q.stage_bytes = (rnd() & 1) ? kDefaultStageBytes : rnd_in(1, (size_t)1 << 28);
    q.workspace = (rnd() & 3) ? 0 : rnd_in(1, (size_t)1 << 34);
    const size_t free_b = (rnd() & 7) ? rnd_in(1, (size_t)288 << 30) : 0;
    int asked = 0, want_asked = 0;
    const ProcessRoute r = process_route(q, [&] { ++asked; return free_b; });
    const ProcessRoute w = process_in_place(q, free_b, want_asked);
    CHECK(r.path == w.path && r.fold == w.fold && r.flag_wanted == w.flag_wanted && r.seg == w.seg && r.rtc_hop == w.rtc_hop && r.rtc_rows == w.rtc_rows && asked == want_asked,
          "process_n's own decisions: path %d / %d fold %d / %d seg %zu / %zu asked %d / %d", r.path, w.path, (int)r.fold, (int)w.fold, r.seg, w.seg, asked, want_asked);
    const size_t n = q.chunk.n;
    const bool two_pass = r.path == PP_HOP_PAIR || r.path == PP_SEGMENTS;
    CHECK(r.path >= PP_HOP_FOLDED && r.path <= PP_SEGMENTS && PP_HOP_PAIR == 2 && PP_SEGMENTS == 3, "exactly one path; last_process_path stays 1 / 1 / 2 / 3");
    CHECK(two_pass == (r.seg != 0) && (!two_pass || (r.seg >= 1 && r.seg <= n)), "segments of the two passes: %zu of %zu", r.seg, n);
    if (!two_pass) CHECK(r.flag_wanted == (q.x_device && q.y_device) && !r.rtc_hop && !r.rtc_rows && asked == 0, "one launch");
    else CHECK(!r.flag_wanted && !r.fold, "two passes never fold and never wait for a word");
    if (r.path == PP_HOP_FOLDED) CHECK(n <= (size_t)kHopSamples && q.linear && !q.spectrum && q.fold && q.hop_kernel && q.chunk.nbins >= 8 && q.gain_rows <= 1 && r.fold, "the folded hop");
    if (r.path == PP_FUSED_ROWS) CHECK(r.fold == !q.spectrum && (q.chunk.rows_kernel || (q.linear && q.chunk.nbins <= 4096 && q.gain_rows <= 65535)), "the fused rows");
    if (q.spectrum && two_pass) CHECK(r.seg == n, "the caller's matrix takes the call in one piece");
    if (asked) CHECK(asked == 1 && two_pass && !q.spectrum && q.stage_bytes == kDefaultStageBytes && q.workspace < q.chunk.channels * q.chunk.nbins * n, "free memory asked where the workspace may grow");
    CHECK((r.rtc_hop || r.rtc_rows) == (q.user && two_pass), "run-time-compiled kernels for the host's statements on the two passes only");
    if (q.user && two_pass)
      for (size_t t = 0; t < n; t += std::max<size_t>(r.seg, n / 64 + 1) / r.seg * r.seg)       // (a sample of the segments; always the first)
      {
        const size_t m = std::min(r.seg, n - t);
        const bool hop_form = q.exact_inverse && q.inverse_rows <= 0 && q.chunk.channels * m <= 1024;
        CHECK(hop_form ? r.rtc_hop : r.rtc_rows, "the kernel of segment %zu (%zu rows) was resolved up front", t, m);
      }
    if (q.user && two_pass) { const size_t m = n - ((n - 1) / r.seg) * r.seg; CHECK((q.exact_inverse && q.inverse_rows <= 0 && q.chunk.channels * m <= 1024) ? r.rtc_hop : r.rtc_rows, "the last segment's kernel"); }
  }
}

static void test_process_shapes()
{
  struct Shape { const char* name; ProcessQuery q; int path, fold, flag; size_t seg; int rtc_hop, rtc_rows, asked; };
  const size_t free_b = (size_t)280 << 30;
  const ProcessQuery hop = pq(100, 1000, 1, 8, false), c0 = pq(48000, 1024, 1, 8, false), c1 = pq(1000000, 1024, 1, 8, false);
  ProcessQuery host_hop = hop; host_hop.y_device = false;
  // the shift operation is linear and never comes with a copy of the spectrum (the entry point refuses that): the query of the identity
  ProcessQuery shift_hop = hop, shift_long = c0; shift_hop.linear = shift_long.linear = true; shift_hop.spectrum = shift_long.spectrum = false;
  ProcessQuery fe[3] = {pq(262144, 4096, 1, 4, true), pq(262144, 4096, 1, 4, true), pq(262144, 4096, 1, 4, true)};      // FD float, two-slot rows
  for (int i = 0; i < 3; ++i) fe[i].fused_exact = i;
  ProcessQuery fe1_bounded = fe[1]; fe1_bounded.stage_bytes = (size_t)256 << 20;
  ProcessQuery ordered_hop = hop; ordered_hop.fused_exact = 1;
  ProcessQuery carry_exact = c0; carry_exact.chunk.exact = true;                                   // fused_exact -1 follows the carries at FD double
  ProcessQuery spectrum = c0; spectrum.spectrum = true;
  ProcessQuery spectrum_hop = hop; spectrum_hop.spectrum = true;
  ProcessQuery table_hop = hop; table_hop.gain_rows = 70000;
  ProcessQuery table_long = c0; table_long.gain_rows = 70000;
  ProcessQuery wide_table = pq(48000, 4096, 1, 8, false); wide_table.gain_rows = 1000;               // beyond the row-group kernel: the folded form's four bins per lane
  ProcessQuery wide_table_many = wide_table; wide_table_many.gain_rows = 70000;
  ProcessQuery user_hop = hop; user_hop.linear = false; user_hop.user = true;
  ProcessQuery user_hop_copy = user_hop; user_hop_copy.spectrum = true;
  ProcessQuery user_fused = c0; user_fused.linear = false; user_fused.user = true;
  ProcessQuery user_long = pq(48000, 4096, 1, 8, false); user_long.linear = false; user_long.user = true;
  ProcessQuery user_1024 = user_long; user_1024.stage_bytes = (size_t)64 << 20;                      // segments of 1024 rows, the last of 896
  ProcessQuery user_2048 = user_long; user_2048.stage_bytes = (size_t)128 << 20;                     // 2048 rows, the last of 896
  ProcessQuery user_rows4 = user_1024; user_rows4.inverse_rows = 4;
  ProcessQuery gate_hop = hop; gate_hop.linear = false;
  ProcessQuery nofold_hop = hop; nofold_hop.fold = 0;
  ProcessQuery nofold_long = c0; nofold_long.fold = 0;
  ProcessQuery nohop = hop; nohop.hop_kernel = 0;
  ProcessQuery kept = user_long; kept.user = false; kept.workspace = (size_t)48000 * 4096;
  const Shape shapes[] = {
    {"the hop: n = 100, m = 1000", hop, PP_HOP_FOLDED, 1, 1, 0, 0, 0, 0},
    {"the hop, host samples out", host_hop, PP_HOP_FOLDED, 1, 0, 0, 0, 0, 0},
    {"configs[0]", c0, PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"the shift operation on the hop", shift_hop, PP_HOP_FOLDED, 1, 1, 0, 0, 0, 0},
    {"the shift operation, configs[0]", shift_long, PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"configs[1] fused", c1, PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"FD float, two slots, fused_exact 0", fe[0], PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"FD float, two slots, fused_exact 1: the walk loses", fe[1], PP_SEGMENTS, 0, 0, 262144, 0, 0, 1},
    {"... with stage_bytes bounded", fe1_bounded, PP_SEGMENTS, 0, 0, 8192, 0, 0, 0},
    {"FD float, two slots, fused_exact 2", fe[2], PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"the hop in the reference's order", ordered_hop, PP_HOP_PAIR, 0, 0, 100, 0, 0, 0},
    {"carry = 1 at FD double", carry_exact, PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"dfts given", spectrum, PP_FUSED_ROWS, 0, 1, 0, 0, 0, 0},
    {"dfts given, the hop", spectrum_hop, PP_HOP_PAIR, 0, 0, 100, 0, 0, 0},
    {"70000 gain vectors, the hop", table_hop, PP_HOP_PAIR, 0, 0, 100, 0, 0, 0},
    {"70000 gain vectors, configs[0]", table_long, PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"1000 gain vectors, m = 4096", wide_table, PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"70000 gain vectors, m = 4096", wide_table_many, PP_SEGMENTS, 0, 0, 48000, 0, 0, 1},
    {"OP_USER on a hop", user_hop, PP_HOP_PAIR, 0, 0, 100, 1, 0, 0},
    {"OP_USER on a hop, dfts given", user_hop_copy, PP_HOP_PAIR, 0, 0, 100, 1, 1, 0},
    {"OP_USER, configs[0]", user_fused, PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"OP_USER on long segments", user_long, PP_SEGMENTS, 0, 0, 48000, 0, 1, 1},
    {"OP_USER, segments of 1024", user_1024, PP_SEGMENTS, 0, 0, 1024, 1, 0, 0},
    {"OP_USER, segments of 2048 and a tail of 896", user_2048, PP_SEGMENTS, 0, 0, 2048, 1, 1, 0},
    {"OP_USER, inverse_rows 4", user_rows4, PP_SEGMENTS, 0, 0, 1024, 0, 1, 0},
    {"gate on a hop", gate_hop, PP_HOP_PAIR, 0, 0, 100, 0, 0, 0},
    {"fold 0, the hop", nofold_hop, PP_HOP_PAIR, 0, 0, 100, 0, 0, 0},
    {"fold 0, configs[0]", nofold_long, PP_FUSED_ROWS, 1, 1, 0, 0, 0, 0},
    {"hop_kernel 0", nohop, PP_HOP_PAIR, 0, 0, 100, 0, 0, 0},
    {"nbins < 8, a hop", pq(100, 4, 1, 8, false), PP_HOP_PAIR, 0, 0, 100, 0, 0, 0},
    {"nbins < 8, long", pq(48000, 4, 1, 8, false), PP_SEGMENTS, 0, 0, 48000, 0, 0, 0},
    {"the workspace is there already", kept, PP_SEGMENTS, 0, 0, 48000, 0, 0, 0},
  };
  for (const Shape& s : shapes)
  {
    int asked = 0;
    const ProcessRoute r = process_route(s.q, [&] { ++asked; return free_b; });
    CHECK(r.path == s.path && r.fold == (s.fold != 0) && r.flag_wanted == (s.flag != 0) && r.seg == s.seg, "%s: path %d fold %d flag %d seg %zu", s.name, r.path, (int)r.fold, (int)r.flag_wanted, r.seg);
    CHECK(r.rtc_hop == (s.rtc_hop != 0) && r.rtc_rows == (s.rtc_rows != 0) && asked == s.asked, "%s: rtc %d %d asked %d", s.name, (int)r.rtc_hop, (int)r.rtc_rows, asked);
  }
  // option fused_exact: -1 follows the carries at FD double
  CHECK(reference_order(-1, true, 8) && !reference_order(-1, true, 4) && !reference_order(-1, false, 8) && reference_order(2, false, 4) && !reference_order(0, true, 8), "fused_exact");
  // free memory unknown: the segments stage_bytes gives
  const ProcessRoute r = process_route(fe[1], [] { return (size_t)0; });
  CHECK(r.seg == 32768, "free memory unknown: %zu rows", r.seg);
}

// grid_segment against the lines the nine grid entry points used to carry inline (written out here), over a small exhaustive table
static void test_grid_segment()
{
  const size_t row_bytes = 3 * 2 * 15 * 8, sample_row_bytes = 3 * 4;      // three channels, a band of 15 complex doubles, float samples
  int one = 0, two = 0, many = 0;
  for (size_t n : {(size_t)1, (size_t)7, (size_t)64, (size_t)1000})
    for (size_t every_asked : {(size_t)1, (size_t)3, (size_t)64, n, n + 1})
    {
      const size_t every = std::min(every_asked, n);          // (the entry points clamp every to n)
      for (size_t first : {(size_t)0, (size_t)5, every, every + 1})
      {
        const size_t rows = (n + every - 1) / every + 1;
        // one segment; two (half the rows, or half the samples where these are what is staged); one row or one hop per segment
        for (size_t stage_bytes : {(size_t)1 << 30, std::max(rows * row_bytes / 2, n * sample_row_bytes / 2), row_bytes})
          for (int xd = 0; xd < 2; ++xd)
            for (int od = 0; od < 2; ++od)
              for (int whole = 0; whole < 2; ++whole)
              {
                size_t seg = n;
                if (!od) seg = std::min(seg, stage_rows(n, row_bytes, stage_bytes) * every);
                if (!xd) seg = std::min(seg, std::max<size_t>((size_t)kHopSamples, stage_rows(n, sample_row_bytes, stage_bytes)));
                if (whole && seg < n && seg > every && first % every == 0) seg -= seg % every;
                const size_t got = grid_segment(n, every, first, row_bytes, sample_row_bytes, stage_bytes, xd != 0, od != 0, whole != 0);
                CHECK(got == seg, "grid_segment: n %zu every %zu first %zu stage %zu xd %d od %d whole %d: %zu, the inline lines give %zu", n, every, first, stage_bytes, xd, od, whole, got, seg);
                CHECK(got >= 1 && got <= n, "a segment is 1 ... n samples: %zu of %zu", got, n);
                if (xd && od) CHECK(got == n, "device memory on both sides: one segment");
                if (whole && got < n && got > every && first % every == 0) CHECK(got % every == 0, "whole windows: %zu of %zu", got, every);
                const size_t segments = (n + got - 1) / got;
                if (segments == 1) ++one; else if (segments == 2) ++two; else ++many;
              }
      }
    }
  CHECK(one && two && many, "the table reaches one, two and many segments: %d %d %d", one, two, many);
  // the lag-product call's rule is this one with the plan's channels for the pairs
  CHECK(lag_sum_segment(1000, 7, 5, 3, 15, 8, 4, row_bytes, false, false) == grid_segment(1000, 7, 5, row_bytes, sample_row_bytes, row_bytes, false, false, true), "lag_sum_segment");
}

// nanoseconds per decision over the named shapes (argument "time")
static void time_routes()
{
  const HostQuery hqs[] = {hq(true, 100, 1000, 1, 4, 8, false, false), hq(false, 100, 1000, 1, 4, 8, false, false), hq(true, 1, 1000, 1, 4, 8, false, true),
                           hq(true, 100, 1000, 1, 4, 8, true, true), hq(true, 1000000, 1024, 1, 4, 8, false, false)};
  const ProcessQuery pqs[] = {pq(100, 1000, 1, 8, false), pq(1000000, 1024, 1, 8, false), pq(262144, 4096, 1, 4, true), pq(48000, 4096, 1, 8, false)};
  const int reps = 2000000;
  volatile size_t sink = 0;
  volatile bool yes = true;
  for (const HostQuery& q : hqs)
  {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < reps; ++i) { HostQuery c = q; c.n += (size_t)(i & 1); const HostRoute r = host_route(c, [&] { return (bool)yes; }, [&] { return !yes; }, [&] { return !yes; }, [&] { return (bool)yes; }, [&] { return (bool)yes; }); sink = sink + (size_t)r.route + r.seg; }
    printf("host_route    %s samples %8zu B matrix %12zu B: %6.1f ns\n", q.analysis ? "analysis " : "synthesis", q.samples_bytes, q.matrix_bytes, std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / reps);
  }
  for (const ProcessQuery& q : pqs)
  {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < reps; ++i) { ProcessQuery c = q; c.chunk.n += (size_t)(i & 1); const ProcessRoute r = process_route(c, [&] { return (size_t)1 << 38; }); sink = sink + (size_t)r.path + r.seg; }
    printf("process_route n %8zu m %5zu: %6.1f ns\n", q.chunk.n, q.chunk.nbins, std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / reps);
  }
}

int main(int argc, char** argv)
{
  if (argc > 1 && std::string(argv[1]) == "time") { time_routes(); return 0; }
  test_geometry();
  test_chunks();
  test_relay_and_radices();
  test_call_pattern();
  test_row_ring();
  test_inverse_streams();
  test_small_decisions();
  test_piece_ring();
  test_form_tuner();
  test_forward_routes();
  test_forward_shapes();
  test_inverse_routes();
  test_inverse_shapes();
  test_host_routes();
  test_host_shapes();
  test_process_routes();
  test_process_shapes();
  test_grid_segment();
  if (failures) { fprintf(stderr, "%d failure(s)\n", failures); return 1; }
  printf("plan logic: all properties hold\n");
  return 0;
}
