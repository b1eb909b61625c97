// prefix_logic_test.cpp -- the prefix-cell route of long analysis calls in sdft_plan_logic.hpp (forward_route): taken exactly
// where the row-group kernel has the self-carried form and the call is longer than kSelfMax (or the test hook forces it), never
// together with the self-carried route, and never in place of the partial sums + scan of a plan that has self_carry = 0.
// Compiled by tests/test_prefix_logic_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first
// violated property.

#include "sdft_plan_logic.hpp"

#include <stdio.h>
#include <stdlib.h>

using namespace sdfthip::logic;

static int failures = 0;
#define CHECK(cond, ...)                                                                    \
  do {                                                                                      \
    if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); \
      if (failures > 20) exit(1); }                                                         \
  } while (0)

static ForwardRoute route(const ForwardQuery& q) { return forward_route(q, [] { return true; }); }

// a dense analysis call of one plan: FD double unless fd_bytes says otherwise
static ForwardQuery query(size_t n, size_t nbins, size_t channels = 1)
{
  ForwardQuery q;
  q.n = n; q.nbins = nbins; q.channels = channels; q.fd_bytes = 8; q.fdx_bytes = 16;
  q.out = 0x10000000; q.out_stride = n * nbins;
  return q;
}

// the conditions of the route, stated from the chunks the route itself reports
static bool expected(const ForwardQuery& q, const ForwardRoute& r)
{
  const size_t span = 2 * q.nbins;
  const bool pow2 = (span & (span - 1)) == 0;
  const bool rows = !q.every && !q.power && !q.power_sum && rows_kernel_ok(q.nbins, q.fdx_bytes, q.row_pointers, q.rows_kernel != 0, q.row_slots_max);
  if (!rows || q.fuse || r.pipelined || r.kernel != FK_ROWS) return false;
  if (q.fd_bytes != 8 || q.exact || q.self == 0) return false;
  if (self_cells(q.nbins, q.self >= 1, q.fdx_bytes) == 0) return false;
  if (!(r.chunks > 1 && (pow2 || r.len > 64))) return false;
  if (q.prefix_cells == 0) return false;
  // by default: calls beyond kSelfMax of at most kPrefixRowsMax rows per cell; the hook's 2 passes both limits
  return (q.n > kSelfMax && (q.n + span - 1) / span <= kPrefixRowsMax) || q.prefix_cells == 2;
}

static void check(const ForwardQuery& q, const char* what)
{
  const ForwardRoute r = route(q);
  const bool want = expected(q, r);
  CHECK(r.prefix == want, "%s: n=%zu nbins=%zu self=%ld prefix_cells=%ld exact=%d fd=%zu fuse=%d pipelined=%d chunks=%ld len=%ld: prefix=%d want %d", what, q.n,
        q.nbins, q.self, q.prefix_cells, (int)q.exact, q.fd_bytes, (int)q.fuse, (int)r.pipelined, r.chunks, r.len, (int)r.prefix, (int)want);
  CHECK(!(r.self && r.prefix), "%s: n=%zu nbins=%zu: self and prefix both set", what, q.n, q.nbins);
  if (r.prefix)
  {
    CHECK(r.kernel == FK_ROWS && !r.use_seed && r.chunks > 1, "%s: n=%zu: kernel=%d use_seed=%d chunks=%ld", what, q.n, r.kernel, (int)r.use_seed, r.chunks);
    // the flag lies on top of the parent's route, whose fields the existing route tests pin: they stay what they were
    CHECK(r.carry == CARRY_SUMS && r.sums != SUMS_NONE && r.fused == (q.fused != 0) && r.segments == 1 && !r.flow, "%s: n=%zu: carry=%d sums=%d fused=%d", what, q.n, r.carry,
          r.sums, (int)r.fused);
  }
  // beyond the bound the partial sums + scan stay, as at the parent commit
  if (!r.prefix && !r.self && !r.pipelined && q.prefix_cells == 1 && q.n > kSelfMax && q.self != 0 && !q.exact && q.fd_bytes == 8 && !q.fuse && r.chunks > 1 && r.kernel == FK_ROWS)
    CHECK(r.carry == CARRY_SUMS && r.sums != SUMS_NONE && r.delta_in_carry && !r.use_seed, "%s: n=%zu nbins=%zu beyond the bound: carry=%d sums=%d", what, q.n, q.nbins, r.carry, r.sums);
  // self_carry = 0 keeps the pre-pass of partial sums + scan wherever the parent took it: every chunk-parallel fast-carry call
  if (q.self == 0 && !q.exact && r.chunks > 1 && r.kernel != FK_HOP)
    CHECK(r.carry == CARRY_SUMS && !r.prefix && !r.self && r.sums != SUMS_NONE && r.delta_in_carry, "%s: n=%zu nbins=%zu prefix_cells=%ld: carry=%d sums=%d", what, q.n,
          q.nbins, q.prefix_cells, r.carry, r.sums);
}

static void test_sweep()
{
  const size_t lengths[] = {600, 4096, 48000, kSelfMax - 8, kSelfMax, kSelfMax + 1, kSelfMax + 4096, 1000000, (size_t)3 << 20, 10000000,
                            2 * 1024 * kPrefixRowsMax, 2 * 1024 * kPrefixRowsMax + 1};
  const size_t bins[] = {8, 64, 100, 1000, 1024, 2048, 37, 1031, 4096, 3000};       // 2N = 74 and 2062: not smooth; 8192 and 6000: beyond 4096 cells
  for (size_t n : lengths)
    for (size_t nb : bins)
      for (long self : {0L, 1L, 2L, -1L})
        for (long pc : {0L, 1L, 2L})
          for (int variant = 0; variant < 8; ++variant)
          {
            ForwardQuery q = query(n, nb);
            q.self = self; q.prefix_cells = pc;
            const char* what = "plain";
            switch (variant)
            {
              case 1: q.exact = true; what = "exact"; break;
              case 2: q.fd_bytes = 4; q.fdx_bytes = 8; q.exact = true; what = "FD float"; break;
              case 3: q.fd_bytes = 4; q.fdx_bytes = 8; what = "FD float, parallel carries"; break;
              case 4: q.fuse = true; q.coeff_ready = true; what = "fused call"; break;
              case 5: q.analysis_batch = true; q.pipe_wanted = true; q.pipeline = 2; what = "pipelined"; break;
              case 6: q.channels = 3; q.out_stride = n * nb; what = "three channels"; break;
              case 7: q.rows_kernel = 0; what = "tile kernel"; break;
              default: break;
            }
            check(q, what);
          }
}

static void test_named_cases()
{
  // the headline: n = 1e6, N = 1024, FD double -- the route by default, the self-carried form up to kSelfMax
  {
    ForwardQuery q = query(1000000, 1024);
    const ForwardRoute r = route(q);
    CHECK(r.prefix && !r.self && r.kernel == FK_ROWS && r.chunks > 1, "headline: prefix=%d self=%d chunks=%ld", (int)r.prefix, (int)r.self, r.chunks);
    q.prefix_cells = 0;
    const ForwardRoute r0 = route(q);
    CHECK(!r0.prefix && !r0.self && r0.carry == CARRY_SUMS && r0.sums == SUMS_FFT2, "headline, hook 0: carry=%d sums=%d", r0.carry, r0.sums);
    CHECK(r0.chunks == r.chunks && r0.len == r.len, "headline: the route does not change the chunks (%ld x %ld against %ld x %ld)", r.chunks, r.len, r0.chunks, r0.len);
    q.prefix_cells = 1; q.self = 0;
    const ForwardRoute rs = route(q);
    CHECK(!rs.prefix && rs.carry == CARRY_SUMS, "headline, self_carry 0: prefix=%d carry=%d", (int)rs.prefix, rs.carry);
  }
  {
    ForwardQuery q = query(kSelfMax, 64);
    const ForwardRoute r = route(q);
    CHECK(r.self && !r.prefix, "n = kSelfMax: self=%d prefix=%d", (int)r.self, (int)r.prefix);
    q.n = kSelfMax + 4096;
    const ForwardRoute r1 = route(q);
    CHECK(!r1.self && r1.prefix, "n = kSelfMax + 4096: self=%d prefix=%d", (int)r1.self, (int)r1.prefix);
    q.n = 2000; q.chunk = 72; q.prefix_cells = 2;
    const ForwardRoute r2 = route(q);
    CHECK(!r2.self && r2.prefix && r2.chunks == 28 && r2.len == 72, "hook 2, short call: self=%d prefix=%d chunks=%ld len=%ld", (int)r2.self, (int)r2.prefix, r2.chunks, r2.len);
  }
  // chunks of up to 64 samples with 2N not a power of two: neither self-carried form
  {
    ForwardQuery q = query(3000, 100);
    q.chunk = 64; q.prefix_cells = 2;
    const ForwardRoute r = route(q);
    CHECK(!r.prefix && !r.self && r.carry == CARRY_SUMS && r.len == 64, "2N = 200, chunks of 64: prefix=%d self=%d len=%ld", (int)r.prefix, (int)r.self, r.len);
    q.chunk = 72;
    const ForwardRoute r1 = route(q);
    CHECK(r1.prefix, "2N = 200, chunks of 72: prefix=%d", (int)r1.prefix);
    q = query(3000, 64); q.chunk = 64; q.prefix_cells = 2;
    CHECK(route(q).prefix, "2N = 128, chunks of 64");
  }
  // one chunk: the hop kernel or the state's carries, never a pre-pass
  {
    ForwardQuery q = query(400, 64);
    q.prefix_cells = 2;
    const ForwardRoute r = route(q);
    CHECK(!r.prefix && r.kernel == FK_HOP, "one chunk: prefix=%d kernel=%d", (int)r.prefix, r.kernel);
  }
  // the bound by rows per cell: nine passes of 512 rows at most, whatever 2N; the hook's 2 passes it
  {
    CHECK(kPrefixRowsMax == 4608 && prefix_rows(1000000, 1024) == 489 && prefix_rows(kSelfMax + 4096, 64) == 4128, "rows per cell");
    ForwardQuery q = query(kSelfMax + 4096, 8);                       // 33 024 rows on one workgroup
    const ForwardRoute r = route(q);
    CHECK(!r.prefix && !r.self && r.carry == CARRY_SUMS && r.chunks > 1, "m = 8 beyond kSelfMax: prefix=%d self=%d carry=%d", (int)r.prefix, (int)r.self, r.carry);
    q.prefix_cells = 2;
    CHECK(route(q).prefix, "m = 8 beyond kSelfMax, hook 2");
    q = query(10000000, 64);                                          // 78 125 rows on four workgroups
    CHECK(!route(q).prefix && route(q).carry == CARRY_SUMS, "m = 64, n = 1e7");
    q = query(128 * kPrefixRowsMax, 64);
    CHECK(route(q).prefix, "m = 64 at the bound");
    q.n += 1;
    CHECK(!route(q).prefix && route(q).carry == CARRY_SUMS, "m = 64 one sample beyond the bound");
    q = query(2048 * kPrefixRowsMax, 1024);
    CHECK(route(q).prefix, "m = 1024 at the bound");
  }
  // a pipelined long call keeps the full fold
  {
    ForwardQuery q = query(1000000, 1024);
    q.analysis_batch = true; q.pipe_wanted = true; q.pipeline = 2;
    const ForwardRoute r = route(q);
    CHECK(r.pipelined && r.self && !r.prefix, "pipelined long call: pipelined=%d self=%d prefix=%d", (int)r.pipelined, (int)r.self, (int)r.prefix);
  }
}

int main()
{
  test_sweep();
  test_named_cases();
  if (failures) { fprintf(stderr, "prefix-logic: %d failures\n", failures); return 1; }
  printf("prefix-logic: all properties hold\n");
  return 0;
}
