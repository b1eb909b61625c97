// filterbank_logic_test.cpp -- the host-side decisions of the filterbank analysis (sdft_hip_sdft_filterbank_n) in
// sdft_plan_logic.hpp: the validation of a filterbank, the decomposition of its bands into pieces for a plan's tile geometry, the
// workspace slots of split bands, the row segments of a call and the route.  Compiled by tests/test_filterbank_cpu.py with
// g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated property.

#include "sdft_plan_logic.hpp"

#include <stdio.h>
#include <stdlib.h>

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

struct Bank { std::vector<size_t> bin0, nbins; };
struct Geometry { const char* name; size_t nbins; int window; size_t fdx_bytes; long tiles_expected; };

static void test_check()
{
  const size_t top = (size_t)-1;
  const size_t b0[3] = {0, 10, 1023}, nb[3] = {1024, 5, 1};
  CHECK(filterbank_check(1024, 3, b0, nb, true) == FB_OK, "a valid filterbank");
  CHECK(filterbank_check(1024, 0, nullptr, nullptr, false) == FB_OK, "no bands: removes the filterbank");
  CHECK(filterbank_check(1024, 3, nullptr, nb, true) == FB_NULL, "band_bin0 NULL");
  CHECK(filterbank_check(1024, 3, b0, nullptr, true) == FB_NULL, "band_nbins NULL");
  CHECK(filterbank_check(1024, 3, b0, nb, false) == FB_NULL, "weights NULL");
  { const size_t z[3] = {1024, 0, 1}; CHECK(filterbank_check(1024, 3, b0, z, true) == FB_EMPTY_BAND, "a band of zero bins"); }
  { const size_t z[3] = {1024, 5, 2}; CHECK(filterbank_check(1024, 3, b0, z, true) == FB_PAST_END, "one bin past the end"); }
  { const size_t s[1] = {1024}, z[1] = {1}; CHECK(filterbank_check(1024, 1, s, z, true) == FB_PAST_END, "starts past the last bin"); }
  { const size_t s[1] = {1}, z[1] = {top}; CHECK(filterbank_check(1024, 1, s, z, true) == FB_PAST_END, "bin0 + nbins wraps to 0"); }
  { const size_t s[1] = {top}, z[1] = {2}; CHECK(filterbank_check(1024, 1, s, z, true) == FB_PAST_END, "bin0 + nbins wraps to 1"); }
  { const size_t s[1] = {0}, z[1] = {1}; CHECK(filterbank_check(0, 1, s, z, true) == FB_PAST_END, "a plan without bins"); }
  CHECK(filterbank_check(1024, kFilterbankMaxBands, b0, nb, true) == FB_TOO_LARGE, "more bands than a piece's destination can name");
  for (int i = 0; i < 20000; ++i)
  {
    const size_t N = rnd_in(1, 200), nbands = rnd_in(1, 6);
    std::vector<size_t> s(nbands), z(nbands);
    bool ok = true;
    for (size_t b = 0; b < nbands; ++b) { s[b] = rnd_in(0, 210); z[b] = rnd_in(0, 210); ok = ok && z[b] >= 1 && s[b] + z[b] <= N; }
    CHECK((filterbank_check(N, nbands, s.data(), z.data(), true) == FB_OK) == ok, "N %zu, %zu random bands", N, nbands);
  }
  const size_t z3[3] = {3, 1, 7};
  CHECK(filterbank_weights(3, z3) == 11 && filterbank_weights(0, nullptr) == 0, "weights of a filterbank");
}

// every property of the layout of one filterbank on one geometry
static void check_layout(const Geometry& g, long forced_interior, const Bank& bank, const char* what)
{
  const int bpl = bins_per_lane(g.fdx_bytes);
  const long interior = interior_lanes(g.window, g.fdx_bytes, forced_interior), nt = tiles(g.nbins, g.window, g.fdx_bytes, forced_interior);
  const size_t per = (size_t)interior * (size_t)bpl, nbands = bank.bin0.size();
  CHECK(filterbank_check(g.nbins, nbands, bank.bin0.data(), bank.nbins.data(), true) == FB_OK, "%s %s: valid", g.name, what);
  const FilterbankLayout l = filterbank_layout(nt, interior, bpl, nbands, bank.bin0.data(), bank.nbins.data());
  CHECK(l.nbands == nbands, "%s %s: bands", g.name, what);
  CHECK(l.wsrc.size() == l.pieces.size(), "%s %s: a source per piece", g.name, what);
  CHECK(l.tile_piece0.size() == (size_t)nt + 1 && l.tile_piece0[0] == 0 && l.tile_piece0[(size_t)nt] == l.pieces.size(), "%s %s: the tiles' piece ranges cover the pieces", g.name, what);
  std::vector<size_t> off(nbands + 1, 0);
  for (size_t b = 0; b < nbands; ++b) off[b + 1] = off[b] + bank.nbins[b];
  // covered[weight index]: how many pieces hold this (band, bin) of a support
  std::vector<int> covered(off[nbands], 0);
  std::vector<int> slot_used(l.nslots, 0), direct(nbands, 0);
  std::vector<size_t> band_of_slot(l.nslots, (size_t)-1);
  for (size_t s = 0; s < l.splits.size(); ++s)
  {
    const FilterbankSplit& sp = l.splits[s];
    CHECK(sp.band < nbands && sp.pieces >= 2 && (size_t)sp.slot0 + sp.pieces <= l.nslots, "%s %s: split %zu", g.name, what, s);
    if (s) CHECK(sp.band > l.splits[s - 1].band && sp.slot0 == l.splits[s - 1].slot0 + l.splits[s - 1].pieces, "%s %s: splits in band order, slots dense", g.name, what);
    for (unsigned j = 0; j < sp.pieces && (size_t)sp.slot0 + j < l.nslots; ++j) band_of_slot[sp.slot0 + j] = sp.band;
  }
  for (long t = 0; t < nt; ++t)
  {
    CHECK(l.tile_piece0[(size_t)t] <= l.tile_piece0[(size_t)t + 1], "%s %s: tile %ld", g.name, what, t);
    const size_t own0 = (size_t)t * per, own1 = std::min(own0 + per, g.nbins);
    for (size_t i = l.tile_piece0[(size_t)t]; i < l.tile_piece0[(size_t)t + 1] && i < l.pieces.size(); ++i)
    {
      const FilterbankPiece& p = l.pieces[i];
      CHECK(p.nbins >= 1 && p.bin0 >= own0 && (size_t)p.bin0 + p.nbins <= own1, "%s %s: piece %zu [%u, +%u) lies in the owned bins [%zu, %zu) of tile %ld", g.name, what, i, p.bin0, p.nbins, own0, own1, t);
      size_t band;
      if (p.dst & kFilterbankToWorkspace)
      {
        const size_t slot = p.dst & ~kFilterbankToWorkspace;
        CHECK(slot < l.nslots, "%s %s: slot %zu of %zu", g.name, what, slot, l.nslots);
        if (slot >= l.nslots) continue;
        ++slot_used[slot];
        band = band_of_slot[slot];
        CHECK(band < nbands, "%s %s: slot %zu belongs to no split", g.name, what, slot);
        if (band >= nbands) continue;
        // ascending tile order, contiguous: the slot's place among the band's slots is the tile's place among the band's tiles
        size_t slot0 = 0;
        for (const FilterbankSplit& sp : l.splits) if (sp.band == band) slot0 = sp.slot0;
        CHECK(slot - slot0 == (size_t)t - bank.bin0[band] / per, "%s %s: band %zu: slot %zu is not tile %ld's", g.name, what, band, slot, t);
      }
      else
      {
        band = p.dst;
        CHECK(band < nbands, "%s %s: band %zu", g.name, what, band);
        if (band >= nbands) continue;
        ++direct[band];
        CHECK(p.bin0 == bank.bin0[band] && p.nbins == bank.nbins[band], "%s %s: a direct piece is the whole band", g.name, what);
      }
      CHECK(p.bin0 >= bank.bin0[band] && (size_t)p.bin0 + p.nbins <= bank.bin0[band] + bank.nbins[band], "%s %s: piece %zu inside band %zu", g.name, what, i, band);
      CHECK(l.wsrc[i] == off[band] + (p.bin0 - bank.bin0[band]), "%s %s: piece %zu: the caller's weights from %zu", g.name, what, i, l.wsrc[i]);
      CHECK(p.woff == (i ? l.pieces[i - 1].woff + l.pieces[i - 1].nbins : 0u), "%s %s: piece %zu: tile-ordered weights from %u", g.name, what, i, p.woff);
      for (size_t k = 0; k < p.nbins && l.wsrc[i] + k < covered.size(); ++k) ++covered[l.wsrc[i] + k];
    }
  }
  for (size_t i = 0; i < covered.size(); ++i) CHECK(covered[i] == 1, "%s %s: weight %zu lies in %d pieces", g.name, what, i, covered[i]);
  for (size_t s = 0; s < l.nslots; ++s) CHECK(slot_used[s] == 1, "%s %s: slot %zu has %d pieces", g.name, what, s, slot_used[s]);
  size_t split_bands = 0;
  for (size_t b = 0; b < nbands; ++b)
  {
    const bool one_tile = bank.bin0[b] / per == (bank.bin0[b] + bank.nbins[b] - 1) / per;
    CHECK(direct[b] == (one_tile ? 1 : 0), "%s %s: band %zu in %s: %d direct pieces", g.name, what, b, one_tile ? "one tile" : "several tiles", direct[b]);
    if (!one_tile) ++split_bands;
  }
  CHECK(split_bands == l.splits.size(), "%s %s: %zu split bands, %zu splits", g.name, what, split_bands, l.splits.size());
  for (const FilterbankSplit& sp : l.splits)
    CHECK(sp.pieces == (bank.bin0[sp.band] + bank.nbins[sp.band] - 1) / per - bank.bin0[sp.band] / per + 1, "%s %s: band %u: one slot per tile it touches", g.name, what, sp.band);
  // workspace indices: unique and below the reported size
  const size_t channels = 3, rows = 4, size = filterbank_workspace(channels, rows, l.nslots);
  std::vector<int> hit(size, 0);
  for (size_t c = 0; c < channels; ++c)
    for (size_t r = 0; r < rows; ++r)
      for (size_t s = 0; s < l.nslots; ++s)
      {
        const size_t o = filterbank_slot(c, rows, r, l.nslots, s);
        CHECK(o < size, "%s %s: workspace index %zu of %zu", g.name, what, o, size);
        if (o < size) ++hit[o];
      }
  for (size_t o = 0; o < size; ++o) CHECK(hit[o] == 1, "%s %s: workspace element %zu used %d times", g.name, what, o, hit[o]);
}

static void test_layouts()
{
  // 62 lanes own a bin at FD double with a halo of one lane per side when option "interior" forces all of them (the default
  // keeps 56); FD float has two bins per lane
  const Geometry geos[] = {
    {"1 tile", 40, kWindowHann, 16, 1},
    {"2 tiles", 100, kWindowHann, 16, 2},
    {"3 tiles, the last of 1 bin", 125, kWindowHann, 16, 3},
    {"17 tiles", 1024, kWindowHann, 16, 17},
    {"34 tiles at 2 bins per lane", 4096, kWindowHann, 8, 34},
  };
  for (const Geometry& g : geos)
  {
    const long forced = 62;
    const int bpl = bins_per_lane(g.fdx_bytes);
    const size_t per = (size_t)interior_lanes(g.window, g.fdx_bytes, forced) * (size_t)bpl;
    CHECK(tiles(g.nbins, g.window, g.fdx_bytes, forced) == g.tiles_expected, "%s: %ld tiles of %zu bins", g.name, tiles(g.nbins, g.window, g.fdx_bytes, forced), per);
    if (g.nbins == 125) CHECK(per == 62 && g.nbins - 2 * per == 1, "125 bins at 62 per tile: a last tile of one bin");
    for (long f : {forced, 0L})                                                       // ... and the default interior
    {
      const size_t p = (size_t)interior_lanes(g.window, g.fdx_bytes, f) * (size_t)bpl;
      Bank whole; whole.bin0 = {0}; whole.nbins = {g.nbins};
      check_layout(g, f, whole, "the whole-row band");
      Bank ones;
      for (size_t k = 0; k < g.nbins; ++k) { ones.bin0.push_back(k); ones.nbins.push_back(1); }
      check_layout(g, f, ones, "one-bin bands");
      {
        const FilterbankLayout l = filterbank_layout(tiles(g.nbins, g.window, g.fdx_bytes, f), interior_lanes(g.window, g.fdx_bytes, f), bpl, g.nbins, ones.bin0.data(), ones.nbins.data());
        CHECK(l.nslots == 0 && l.splits.empty() && l.pieces.size() == g.nbins, "%s: one-bin bands need no workspace", g.name);
      }
      // bands ending and starting exactly on a tile boundary, and the ones that straddle it by one bin
      Bank edge;
      for (size_t e = p; e < g.nbins; e += p)
      {
        edge.bin0.push_back(e - std::min(e, (size_t)5)); edge.nbins.push_back(std::min(e, (size_t)5));          // ends on it
        edge.bin0.push_back(e); edge.nbins.push_back(std::min(g.nbins - e, (size_t)5));                            // starts on it
        edge.bin0.push_back(e - 1); edge.nbins.push_back(2);                                                      // straddles it
        edge.bin0.push_back(e - p); edge.nbins.push_back(p);                                                      // a whole tile
      }
      if (!edge.bin0.empty()) check_layout(g, f, edge, "bands on tile boundaries");
      // duplicates, in no order
      Bank dup;
      for (int r = 0; r < 3; ++r) { dup.bin0.push_back(g.nbins / 3); dup.nbins.push_back(g.nbins - g.nbins / 3); dup.bin0.push_back(0); dup.nbins.push_back(1); }
      check_layout(g, f, dup, "duplicate bands");
      for (int i = 0; i < 40; ++i)
      {
        Bank r;
        const size_t nbands = rnd_in(1, 3 * std::min<size_t>(g.nbins, 100));
        for (size_t b = 0; b < nbands; ++b)
        {
          const size_t s = rnd_in(0, g.nbins - 1);
          r.bin0.push_back(s); r.nbins.push_back((rnd() & 3) ? rnd_in(1, std::min<size_t>(g.nbins - s, 2 * p)) : rnd_in(1, g.nbins - s));
        }
        check_layout(g, f, r, "random bands");
      }
    }
  }
}

static void test_segments()
{
  CHECK(filterbank_segment_rows(1, 0, 8) == (size_t)-1, "no split band: no workspace, no bound");
  CHECK(filterbank_workspace(4, 100, 0) == 0, "... and nothing to allocate");
  CHECK(filterbank_segment_rows(1, 1, 8, 64) == 8 && filterbank_segment_rows(2, 1, 8, 64) == 4 && filterbank_segment_rows(1, 3, 4, 64) == 5, "rows within the bound");
  CHECK(filterbank_segment_rows(1, 1000, 8, 64) == 1, "a single row is never cut");
  CHECK(kFilterbankWorkspaceBytes == ((size_t)64 << 20), "the bound sdft_hip.h and DESIGN.md state");
  for (int i = 0; i < 20000; ++i)
  {
    const size_t ch = rnd_in(1, 8), slots = rnd_in(1, 5000), fd = (rnd() & 1) ? 4 : 8, bound = rnd_in(1, (size_t)1 << 28);
    const size_t rows = filterbank_segment_rows(ch, slots, fd, bound);
    CHECK(rows >= 1, "at least one row");
    CHECK(rows == 1 || filterbank_workspace(ch, rows, slots) * fd <= bound, "%zu rows of %zu slots, %zu channels exceed %zu bytes", rows, slots, ch, bound);
    CHECK(filterbank_workspace(ch, rows + 1, slots) * fd > bound, "one more row would fit");
  }
  // the launches of a call: the chunks in order, each once, every row in exactly one launch, at most max_rows rows unless the launch
  // is a single chunk
  for (int i = 0; i < 3000; ++i)
  {
    const size_t n = rnd_in(1, 20000), every = (rnd() & 1) ? rnd_in(1, 8) : rnd_in(9, 3000), first = rnd_in(0, n + 10), max_rows = rnd_in(1, 300);
    const long len = (long)rnd_in(1, 600), shift = (rnd() & 1) ? (long)rnd_in(0, (size_t)len - 1) : 0;
    const long chunks = (long)((n + (size_t)shift + (size_t)len - 1) / (size_t)len);
    const long j0 = (long)rnd_in(0, (size_t)chunks - 1), j1 = (long)rnd_in((size_t)j0 + 1, (size_t)chunks);
    size_t next_row = every_rows(chunk_begin(j0, len, shift), every, first);
    long ja = j0;
    while (ja < j1)
    {
      const FilterbankSpan s = filterbank_next_span(ja, j1, len, shift, n, every, first, max_rows);
      CHECK(s.ja == ja && s.jb > ja && s.jb <= j1, "n %zu: launch [%ld, %ld) of [%ld, %ld)", n, s.ja, s.jb, j0, j1);
      if (s.jb <= ja) break;
      CHECK(s.row0 == next_row, "n %zu: rows from %zu, expected %zu", n, s.row0, next_row);
      CHECK(s.rows <= max_rows || s.jb == ja + 1, "n %zu: %zu rows in %ld chunks, bound %zu", n, s.rows, s.jb - ja, max_rows);
      if (s.jb < j1) CHECK(filterbank_span(ja, s.jb + 1, len, shift, n, every, first).rows > max_rows, "n %zu: one more chunk would fit", n);
      // the rows are those whose samples lie in the launch's chunks
      size_t count = 0;
      for (size_t t = chunk_begin(ja, len, shift); t < chunk_end(s.jb - 1, len, shift, n); ++t) if (t >= first && (t - first) % every == 0) ++count;
      CHECK(count == s.rows, "n %zu every %zu first %zu: %zu rows, counted %zu", n, every, first, s.rows, count);
      next_row += s.rows; ja = s.jb;
    }
    CHECK(next_row == every_rows(chunk_end(j1 - 1, len, shift, n), every, first), "n %zu: all rows", n);
  }
}

// the route of the call: forward_filterbank_kernel whatever the shape, with the power call's chunks
static void test_route()
{
  for (int i = 0; i < 20000; ++i)
  {
    ForwardQuery q;
    q.n = rnd_in(1, 2000000); q.nbins = rnd_in(1, 4200); q.channels = rnd_in(1, 8);
    const bool f32 = rnd() & 1;
    q.fd_bytes = f32 ? 4 : 8; q.fdx_bytes = f32 ? 8 : 16;
    q.window = (int)rnd_in(0, 3); q.cursor = rnd_in(0, 2 * q.nbins - 1); q.exact = f32 || (rnd() & 1); q.fid_canonical = rnd() & 1;
    q.filterbank = true; q.power_every = rnd_in(1, 3000);
    q.analysis_batch = rnd() & 1; q.pipe_wanted = rnd() & 1;
    bool asked = false;
    const ForwardRoute r = forward_route(q, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_FILTERBANK, "n %zu N %zu: kernel %d", q.n, q.nbins, r.kernel);
    CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", q.n, q.nbins);
    CHECK(r.tiles == tiles(q.nbins, q.window, q.fdx_bytes, 0), "tiles");
    ForwardQuery p = q; p.filterbank = false; p.power = true;
    const ForwardRoute rp = forward_route(p, [] { return true; });
    CHECK(rp.kernel == FK_POWER, "the power call keeps its kernel");
    CHECK(rp.chunks == r.chunks && rp.len == r.len && rp.carry == r.carry && rp.relay_L == r.relay_L && rp.shift == r.shift && rp.segments == r.segments && rp.use_seed == r.use_seed,
          "the power call's chunks and carries");
  }
  CHECK(FK_FILTERBANK == 7, "get_option(\"last_kernel\") answers 7");
}

int main()
{
  test_check();
  test_layouts();
  test_segments();
  test_route();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("filterbank-logic: all properties hold\n");
  return 0;
}
