// sdft_plan_entry.inc -- member functions of Plan<TD, FD> (included inside the class body by sdft_plan.hpp): the entry points
// behind the C-ABI -- dense matrices or row-pointer tables, host or device pointers, single samples, the fused call, state
// access -- and the routes host memory takes through them (pinned scratch, registered in place, pinned slots, staged segments).
// Citations are into /root/reference/c/src/sdft/sdft.h.

  // ---- public entry points: dense matrices, host or device pointers ---------------------------
  // x: [channels][n], dfts: [channels][n][N]
  // x_class: -1 = classify x, 0 = x is host memory whatever option "pointers" says (by-value sample)
  bool sdft_n(size_t n, const TD* x, fdx* dfts, int x_class = -1)
  {
    if (n == 0 || nbins == 0) return true;
    if (opt_resident && x_class < 0 && resident_analysis(n, x, dfts)) return true;      // (no runtime call at all: a doorbell and a completion word)
    if (opt_resident && x_class == 0 && n == 1 && resident_analysis_sample(x[0], dfts)) return true;    // sdft_sdft: the sample rides in the call
    if (!bind()) return false;
    const bool xd = x_class < 0 ? on_device(x) : x_class != 0;
    const bool od = on_device(dfts);
    if (xd && od)
    {
      flag_wanted = true;                                    // a call of one time chunk may signal its own completion
      pipe_allowed = true;
      const bool ok = forward_device(n, x, n, dfts, n * nbins, nullptr);
      flag_wanted = false; pipe_allowed = false;
      return ok && finish(matrix_bytes(n));
    }

    // small host samples, device matrix (hop-wise streaming from a host signal, sdft_sdft on a device row): through the
    // pinned scratch, completion by the kernel's word -- the call is complete on return like every host-pointer call
    if (!xd && od && channels * n * sizeof(TD) <= kIoBytes && opt_pinned_io && ensure_io())
    {
      memcpy(h_io, x, channels * n * sizeof(TD));
      const bool saved = async; async = false;
      flag_wanted = true;
      const bool ok = forward_device(n, d_io, n, dfts, n * nbins, nullptr);
      flag_wanted = false;
      const bool done = ok && finish(matrix_bytes(n));
      async = saved;
      return done;
    }
    // host buffers mapped in place (see map_host): the kernels work on the caller's memory
    {
      // (a hop's samples are a different slice of the host's signal every call: a few hundred bytes go through the
      // staging buffer, only buffers beyond 64 KiB are worth a registration)
      const bool small_x = channels * n * sizeof(TD) <= kSmallHostBytes;
      fdx* om = od ? dfts : static_cast<fdx*>(map_host(dfts, channels * n * nbins * sizeof(fdx), true));
      const TD* xm = xd ? x : ((x_class == 0 || small_x) ? nullptr : static_cast<const TD*>(map_host(x, channels * n * sizeof(TD))));
      if (om && !xm && !xd && small_x)
      {
        if (!d_stage_td.reserve(channels * n)) return false;
        if (!to_device(d_stage_td.p, x, channels * n * sizeof(TD))) return false;
        xm = d_stage_td.p;
      }
      if (xm && om)
      {
        const bool ok = forward_device(n, xm, n, om, n * nbins, nullptr);
        return ok && finish_mapped(matrix_bytes(n));   // host memory: complete on return, through the stream
      }
    }
    // a hop-sized matrix for host memory (the reference driver's 100 x 1000 bins = 1.6 MB, test/test.c:62-83): the kernels
    // write it into the plan's pinned pieces over PCIe -- no staging matrix, no DMA launch -- and the host copies it out
    // (scripts/host_hop_paths.py, profiles/r04_host_copy_paths.txt)
    {
      const size_t obytes = channels * n * nbins * sizeof(fdx), xbytes = channels * n * sizeof(TD);
      if (!od && io.opt_host_copy == 0 && io.opt_host_direct && obytes <= HostIo::kDirectBytes && (xd || xbytes <= kSmallHostBytes) && io.ensure_pin())
      {
        if (!io.pin_idle()) return copy_failed();
        const TD* xm = x;
        if (!xd)
        {
          if (xbytes <= kIoBytes && opt_pinned_io && ensure_io()) { memcpy(h_io, x, xbytes); xm = d_io; }
          else
          {
            if (!d_stage_td.reserve(channels * n)) return false;
            if (!to_device(d_stage_td.p, x, xbytes)) return false;
            xm = d_stage_td.p;
          }
        }
        ++io.pin_copies;
        const double t0 = HostIo::now_us();
        if (!forward_device(n, xm, n, reinterpret_cast<fdx*>(io.d_pin), n * nbins, nullptr)) return false;
        if (!finish_mapped(matrix_bytes(n))) return false;
        const double t1 = HostIo::now_us();
        io.copy_bytes(dfts, io.h_pin, obytes);
        io.pin_us_device += t1 - t0; io.pin_us_memcpy += HostIo::now_us() - t1;
        return true;
      }
    }
    // staged path (host pointers): time segments so that the staging matrix stays bounded;
    // the stream state carries over from segment to segment exactly like hop-wise calls do
    const size_t row_bytes = channels * nbins * sizeof(fdx);
    size_t seg = std::max<size_t>(1, stage_bytes / std::max<size_t>(row_bytes, 1));
    seg = std::min(seg, n);
    if (!xd && !d_stage_td.reserve(channels * seg)) return false;
    if (!od && !d_stage_fdx.reserve(channels * seg * nbins)) return false;
    for (size_t t = 0; t < n; t += seg)
    {
      const size_t m = std::min(seg, n - t);
      const TD* xs; size_t xstride;
      if (xd) { xs = x + t; xstride = n; }
      else
      {
        if (!copy2d(d_stage_td.p, m * sizeof(TD), x + t, n * sizeof(TD), m * sizeof(TD), hipMemcpyHostToDevice)) return false;
        xs = d_stage_td.p; xstride = m;
      }
      if (od)
      {
        if (!forward_device(m, xs, xstride, dfts + t * nbins, n * nbins, nullptr)) return false;
      }
      else
      {
        if (!forward_device(m, xs, xstride, d_stage_fdx.p, m * nbins, nullptr)) return false;
        if (!copy2d(dfts + t * nbins, n * nbins * sizeof(fdx), d_stage_fdx.p, m * nbins * sizeof(fdx),
                    m * nbins * sizeof(fdx), hipMemcpyDeviceToHost)) return false;
      }
      if (!xd || !od) SDFT_TRY(hipStreamSynchronize(stream));     // staging buffers are reused
    }
    return synchronize();
  }

  // decimated analysis (sdft_hip_sdft_every_n): the rows sdft_n would write at the call's samples first, first + every, ...
  // < n, dense [channels][rows][N]; the stream state afterwards is the one sdft_n leaves.  `rows` receives the row count.
  // Never resident, pipelined or fused: whatever is in flight is retired / joined first, then one forward_launch on the
  // plan's stream (forward_every_kernel).  Host memory goes through device scratch and the plan's pinned copy path, in
  // time segments that keep both scratch buffers within stage_bytes.
  bool sdft_every_n(size_t n, const TD* x, size_t every, size_t first, fdx* dfts, size_t& rows)
  {
    static const char* fn = "sdft_hip_sdft_every_n";
    rows = 0;
    if (every == 0) { set_error(fn, "every must be at least 1"); return false; }
    rows = logic::every_rows(n, every, first);
    if (rows > 0 && !dfts) { set_error(fn, "dfts is NULL but the call keeps rows"); return false; }
    if (n == 0 || nbins == 0) return true;
    if (every == 1 && first == 0) return sdft_n(n, x, dfts);      // every row: the analysis itself
    if (!bind()) return false;
    if (!pipe_join()) return false;
    if (every > n) every = n;                                // (the same grid: at most one row; keeps first + k * every in range)
    const size_t nb = nbins;
    const bool xd = on_device(x);
    const bool od = rows == 0 || on_device(dfts);
    const size_t row_bytes = channels * nb * sizeof(fdx);
    if (xd && od)
    {
      const EveryGrid g{(unsigned long long)every, (unsigned long long)first};
      if (!forward_device(n, x, n, dfts, rows * nb, nullptr, nullptr, &g)) return false;
      return finish(rows * row_bytes);
    }
    // host memory: segments of at most seg samples, each one forward launch on device scratch
    size_t seg = n;
    if (!od) seg = std::min(seg, std::max<size_t>(1, stage_bytes / std::max<size_t>(row_bytes, 1)) * every);
    if (!xd) seg = std::min(seg, std::max<size_t>((size_t)logic::kHopSamples, stage_bytes / (channels * sizeof(TD))));
    if (!xd && !d_stage_td.reserve(channels * seg)) return false;
    if (!od && !d_stage_fdx.reserve(channels * ((seg + every - 1) / every) * nb)) return false;
    for (size_t t = 0; t < n; t += seg)
    {
      const size_t m = std::min(seg, n - t);
      const size_t f = logic::every_first_from(t, every, first);
      const size_t r = logic::every_rows(m, every, f);
      const size_t r0 = r ? (t + f - first) / every : 0;    // the segment's first row in the call's grid
      const TD* xs; size_t xstride;
      if (xd) { xs = x + t; xstride = n; }
      else
      {
        if (!copy2d(d_stage_td.p, m * sizeof(TD), x + t, n * sizeof(TD), m * sizeof(TD), hipMemcpyHostToDevice)) return false;
        xs = d_stage_td.p; xstride = m;
      }
      const EveryGrid g{(unsigned long long)every, (unsigned long long)f};
      if (od)
      {
        if (!forward_device(m, xs, xstride, r ? dfts + r0 * nb : nullptr, rows * nb, nullptr, nullptr, &g)) return false;
      }
      else
      {
        if (!forward_device(m, xs, xstride, d_stage_fdx.p, r * nb, nullptr, nullptr, &g)) return false;
        if (r && !copy2d(dfts + r0 * nb, rows * nb * sizeof(fdx), d_stage_fdx.p, r * nb * sizeof(fdx), r * nb * sizeof(fdx), hipMemcpyDeviceToHost))
          return false;
      }
      SDFT_TRY(hipStreamSynchronize(stream));                // scratch buffers are reused; host memory is complete on return
    }
    return synchronize();
  }

  // array-of-row-pointers variant (sdft.h:622-628).  Single-channel plans only: the reference's
  // table has one pointer per sample, a batched layout for it is not defined.
  bool single_channel(const char* fn)
  {
    if (channels == 1) return true;
    set_error(fn, "row-pointer variants take single-channel plans only (use sdft_sdft_n / sdft_isdft_n with a batched plan)");
    return false;
  }
  bool sdft_nd(size_t n, const TD* x, fdx** dfts)
  {
    if (n == 0 || nbins == 0) return true;
    if (!single_channel("sdft_sdft_nd")) return false;
    if (!bind()) return false;
    const bool table_on_device = is_device_pointer(dfts);
    bool rows_on_device = false;
    std::vector<fdx*> host_rows;
    if (!table_on_device) { rows_on_device = is_device_pointer(dfts[0]); }
    if (table_on_device || rows_on_device)
    {
      // rows live on the device: hand the pointer table to the kernel
      fdx* const* table = dfts;
      if (!table_on_device)
      {
        if (!d_rowptr.reserve(n)) return false;
        if (!to_device(d_rowptr.p, dfts, n * sizeof(fdx*))) return false;
        table = d_rowptr.p;
      }
      const TD* xs = x;
      if (!is_device_pointer(x))
      {
        if (!d_stage_td.reserve(n)) return false;
        if (!to_device(d_stage_td.p, x, n * sizeof(TD))) return false;
        xs = d_stage_td.p;
      }
      return forward_device(n, xs, n, nullptr, 0, table) && synchronize();
    }
    // host rows: compute dense segments, scatter row by row
    const size_t seg = std::min(n, std::max<size_t>(1, stage_bytes / std::max<size_t>(nbins * sizeof(fdx), 1)));
    std::vector<fdx> host(seg * nbins);
    for (size_t t = 0; t < n; t += seg)
    {
      const size_t m = std::min(seg, n - t);
      const bool saved = async; async = false;
      const bool ok = sdft_n(m, x + t, host.data());
      async = saved;
      if (!ok) return false;
      for (size_t r = 0; r < m; ++r) memcpy(dfts[t + r], host.data() + r * nbins, nbins * sizeof(fdx));
    }
    return true;
  }

  // y_class: -1 = classify y, 0 = y is host memory whatever option "pointers" says (the by-value result of sdft_isdft)
  bool isdft_n(size_t n, const fdx* dfts, TD* y, int y_class = -1)
  {
    if (n == 0) return true;
    if (opt_resident && y_class < 0 && resident_synthesis(n, dfts, y)) return true;
    if (!bind()) return false;
    const bool id = on_device(dfts);
    const bool yd = y_class < 0 ? on_device(y) : y_class != 0;
    if (nbins == 0)
    {
      // empty spectrum: the reference returns (td)(0 * 2)
      if (yd) SDFT_TRY(hipMemsetAsync(y, 0, channels * n * sizeof(TD), stream)); else memset(y, 0, channels * n * sizeof(TD));
      return finish();
    }
    if (id && yd)
    {
      flag_wanted = true;
      pipe_allowed = true;
      const bool ok = inverse_device(n, dfts, n * nbins, nullptr, y, n);
      flag_wanted = false; pipe_allowed = false;
      return ok && finish(matrix_bytes(n));
    }
    // device matrix, small host output: the kernel writes the samples into the pinned scratch
    if (id && !yd && channels * n * sizeof(TD) <= kIoBytes && opt_pinned_io && ensure_io())
    {
      const bool saved = async; async = false;
      flag_wanted = true;
      const bool ok = inverse_device(n, dfts, n * nbins, nullptr, d_io, n);
      flag_wanted = false;
      const bool done = ok && finish(matrix_bytes(n));
      async = saved;
      if (done) memcpy(y, h_io, channels * n * sizeof(TD));
      return done;
    }
    {
      const bool small_y = channels * n * sizeof(TD) <= kSmallHostBytes;
      const fdx* im = id ? dfts : static_cast<const fdx*>(map_host(dfts, channels * n * nbins * sizeof(fdx)));
      TD* ym = yd ? y : (small_y ? nullptr : static_cast<TD*>(map_host(y, channels * n * sizeof(TD), true)));
      if (im && !ym && !yd && small_y) { if (!d_stage_td.reserve(channels * n)) return false; ym = d_stage_td.p; }
      if (im && ym)
      {
        bool ok = inverse_device(n, im, n * nbins, nullptr, ym, n);
        if (ok && ym == d_stage_td.p && !yd)
        {
          ok = to_host(y, ym, channels * n * sizeof(TD));
        }
        return ok && finish_mapped(matrix_bytes(n));
      }
    }
    // a hop-sized matrix in host memory: copied into the plan's pinned pieces, which the kernel reads over PCIe
    {
      const size_t ibytes = channels * n * nbins * sizeof(fdx), ybytes = channels * n * sizeof(TD);
      if (!id && io.opt_host_copy == 0 && io.opt_host_direct && ibytes <= HostIo::kDirectBytes && (yd || ybytes <= kSmallHostBytes) && io.ensure_pin())
      {
        if (!io.pin_idle()) return copy_failed();
        const double t0 = HostIo::now_us();
        io.copy_bytes(io.h_pin, dfts, ibytes);
        const double t1 = HostIo::now_us();
        io.pin_us_memcpy += t1 - t0;
        ++io.pin_copies;
        TD* ym = y;
        const bool through_io = !yd && ybytes <= kIoBytes && opt_pinned_io && ensure_io();
        if (!yd) { if (through_io) ym = d_io; else { if (!d_stage_td.reserve(channels * n)) return false; ym = d_stage_td.p; } }
        if (!inverse_device(n, reinterpret_cast<const fdx*>(io.d_pin), n * nbins, nullptr, ym, n)) return false;
        if (!yd && !through_io && !to_host(y, ym, ybytes)) return false;
        if (!finish_mapped(matrix_bytes(n))) return false;
        io.pin_us_device += HostIo::now_us() - t1;
        if (through_io) memcpy(y, h_io, ybytes);
        return true;
      }
    }
    const size_t row_bytes = channels * nbins * sizeof(fdx);
    size_t seg = std::max<size_t>(1, stage_bytes / std::max<size_t>(row_bytes, 1));
    seg = std::min(seg, n);
    if (!id && !d_stage_fdx.reserve(channels * seg * nbins)) return false;
    if (!yd && !d_stage_td.reserve(channels * seg)) return false;
    for (size_t t = 0; t < n; t += seg)
    {
      const size_t m = std::min(seg, n - t);
      const fdx* in; size_t istride;
      if (id) { in = dfts + t * nbins; istride = n * nbins; }
      else
      {
        if (!copy2d(d_stage_fdx.p, m * nbins * sizeof(fdx), dfts + t * nbins, n * nbins * sizeof(fdx),
                    m * nbins * sizeof(fdx), hipMemcpyHostToDevice)) return false;
        in = d_stage_fdx.p; istride = m * nbins;
      }
      if (yd)
      {
        if (!inverse_device(m, in, istride, nullptr, y + t, n)) return false;
      }
      else
      {
        if (!inverse_device(m, in, istride, nullptr, d_stage_td.p, m)) return false;
        if (!copy2d(y + t, n * sizeof(TD), d_stage_td.p, m * sizeof(TD), m * sizeof(TD), hipMemcpyDeviceToHost)) return false;
      }
      SDFT_TRY(hipStreamSynchronize(stream));
    }
    return synchronize();
  }

  bool isdft_nd(size_t n, const fdx** dfts, TD* y)
  {
    if (n == 0) return true;
    if (!single_channel("sdft_isdft_nd")) return false;
    if (!bind()) return false;
    if (nbins == 0) return isdft_n(n, nullptr, y);
    const bool table_on_device = is_device_pointer(dfts);
    const bool rows_on_device = table_on_device || is_device_pointer(dfts[0]);
    if (rows_on_device)
    {
      const fdx* const* table = dfts;
      if (!table_on_device)
      {
        if (!d_rowptr.reserve(n)) return false;
        if (!to_device(d_rowptr.p, dfts, n * sizeof(fdx*))) return false;
        table = d_rowptr.p;
      }
      TD* yy = y;
      const bool yd = is_device_pointer(y);
      if (!yd) { if (!d_stage_td.reserve(n)) return false; yy = d_stage_td.p; }
      if (!inverse_device(n, nullptr, 0, table, yy, n)) return false;
      if (!yd && !to_host(y, yy, n * sizeof(TD))) return false;
      return synchronize();
    }
    const size_t seg = std::min(n, std::max<size_t>(1, stage_bytes / std::max<size_t>(nbins * sizeof(fdx), 1)));
    std::vector<fdx> host(seg * nbins);
    for (size_t t = 0; t < n; t += seg)
    {
      const size_t m = std::min(seg, n - t);
      for (size_t r = 0; r < m; ++r) memcpy(host.data() + r * nbins, dfts[t + r], nbins * sizeof(fdx));
      const bool saved = async; async = false;
      const bool ok = isdft_n(m, host.data(), y + t);
      async = saved;
      if (!ok) return false;
    }
    return true;
  }

  // single-sample synthesis (sdft.h:635): the result comes back by value, so a device-resident
  // row needs a one-element device buffer (owned by the plan, allocated on the plan's device)
  bool isdft_one(const fdx* dft, TD* y)
  {
    if (nbins == 0) { *y = (TD)0; return true; }           // the reference returns (td)(0 * 2)
    if (opt_resident && resident_synthesis_sample(dft, y)) return true;
    if (!bind()) return false;
    const bool saved = async; async = false;
    const bool ok = isdft_n(1, dft, y, 0);                   // (a device row: through the pinned scratch, see isdft_n; y lives on the host stack)
    async = saved;
    return ok;
  }

  // ---- fused analysis -> spectral operation -> synthesis (SURVEY.md 8 f2) ------------------------
  // y[t] = sdft_isdft( op( sdft_sdft(x[t]) ) ) with the reference's arithmetic, without the (n, N)
  // matrix ever reaching HBM unless the caller asks for a copy of the processed spectrum in `dfts`.
  // params: OP_GAIN -> FD gains[N], OP_CGAIN -> cx<FD> gains[N] (host or device memory), OP_SHIFT -> const long* (host).
  DevBuf<FD> d_gain;
  DevBuf<TD> d_stage_y;
  bool fuse_ok() const { return rows_kernel_ok(false); }
  // fused call: bins summed in the reference's order?  (-1: exactly when the host asked for exact carries at FD double)
  bool wants_reference_order() const
  {
    return opt_fused_exact < 0 ? (carry_mode == CARRY_EXACT && sizeof(FD) == 8) : opt_fused_exact != 0;
  }

  bool process_n(size_t n, const TD* x, TD* y, int op_kind, const void* params, fdx* dfts)
  {
    if (n == 0) return true;
    if (!bind()) return false;
    // public operation numbers (enum sdft_hip_op): 0 identity, 1 gain, 2 shift, 3 cgain, 4 gain_rows, 5 cgain_rows, 6 gate, 7 power,
    // 8 expression
    const int op_public = op_kind;
    if (op_public < 0 || op_public > 8) { set_error("sdft_hip_process_n", "unknown operation"); return false; }
    if ((op_public != 0) && !params) { set_error("sdft_hip_process_n", "the operation needs parameters"); return false; }
    op_kind = op_public == 4 ? OP_GAIN : op_public == 5 ? OP_CGAIN : op_public == 6 ? OP_GATE : op_public == 7 ? OP_POWER : op_public == 8 ? OP_USER : op_public;
    if (op_kind == OP_SHIFT && dfts) { set_error("sdft_hip_process_n", "a copy of the spectrum is not available with the shift operation"); return false; }
    const bool yd = on_device(y);
    if (nbins == 0)
    {
      if (yd) SDFT_TRY(hipMemsetAsync(y, 0, channels * n * sizeof(TD), stream)); else memset(y, 0, channels * n * sizeof(TD));
      return finish();
    }
    if (dfts && !on_device(dfts)) { set_error("sdft_hip_process_n", "dfts must be device memory (or NULL)"); return false; }
    SpectralOp<FD> op{}; op.kind = op_kind; op.gain = nullptr; op.shift = 0; op.rows = 1; op.hop = 0; op.t0 = 0;
    if (op_kind == OP_GAIN || op_kind == OP_CGAIN)
    {
      const FD* g = static_cast<const FD*>(params);
      size_t rows = 1;
      if (op_public >= 4)
      {
        // time-varying gains: { gains, rows, hop } (sdft_hip_gain_rows_t)
        struct table_t { const void* gains; size_t rows, hop; };
        const table_t* tb = static_cast<const table_t*>(params);
        if (!tb->gains || tb->rows == 0 || (tb->rows > 1 && tb->hop == 0)) { set_error("sdft_hip_process_n", "gain table: gains, rows >= 1 and hop >= 1 are required"); return false; }
        if (tb->rows > 0xffffffffull) { set_error("sdft_hip_process_n", "gain table: too many rows"); return false; }
        g = static_cast<const FD*>(tb->gains); rows = tb->rows; op.rows = (unsigned)rows; op.hop = tb->hop;
      }
      const size_t per_bin = op_kind == OP_CGAIN ? 2 : 1;          // real factors, or (re, im) pairs
      if (!on_device(g))
      {
        if (!d_gain.reserve(rows * nbins * 2)) return false;
        if (!to_device(d_gain.p, g, rows * nbins * per_bin * sizeof(FD))) return false;
        g = d_gain.p;
      }
      op.gain = g;
    }
    else if (op_kind == OP_SHIFT) op.shift = *static_cast<const long*>(params);
    else if (op_kind == OP_GATE || op_kind == OP_POWER) { const FD* q = static_cast<const FD*>(params); op.p0 = q[0]; op.p1 = q[1]; }   // host memory
    else if (op_kind == OP_USER)
    {
      // { expr, p, np }: the parameters travel to the device with the call (host memory; np may be 0)
      struct expr_t { const char* expr; const void* p; size_t np; };
      const expr_t* ex = static_cast<const expr_t*>(params);
      if (!ex->expr || !*ex->expr) { set_error("sdft_hip_process_n", "expression: no statements"); return false; }
      user_expr = ex->expr;
      if (ex->np <= 8)
      {
        // up to eight parameters ride in the kernel arguments (SpectralOp::pv)
        for (size_t i = 0; i < ex->np; ++i) op.pv[i] = static_cast<const FD*>(ex->p)[i];
        op.gain = nullptr;
      }
      else
      {
        if (!d_gain.reserve(ex->np)) return false;
        if (!to_device(d_gain.p, ex->p, ex->np * sizeof(FD))) return false;
        op.gain = d_gain.p;
      }
    }
    const bool linear = op_is_linear<FD>(op_kind);
    const bool one_vector = op.rows <= 1;

    // samples: device pointers as they are, host pointers staged (4 bytes per sample each way)
    const bool xd = on_device(x);
    const TD* xs = x;
    if (!xd)
    {
      if (!d_stage_td.reserve(channels * n)) return false;
      if (!to_device(d_stage_td.p, x, channels * n * sizeof(TD))) return false;
      xs = d_stage_td.p;
    }
    TD* ys = y;
    if (!yd) { if (!d_stage_y.reserve(channels * n)) return false; ys = d_stage_y.p; }
    // In place (out == samples) or overlapping device buffers: the two reference calls read every sample before the first
    // output sample is written, the one-launch forms do not (workgroups read the samples of earlier chunks -- fold, delay
    // line, differences -- while others write their outputs).  The samples are copied aside first: 4-8 bytes per sample.
    if (xs == x && yd)
    {
      const uintptr_t xa = reinterpret_cast<uintptr_t>(xs), ya = reinterpret_cast<uintptr_t>(ys), bytes = channels * n * sizeof(TD);
      if (xa < ya + bytes && ya < xa + bytes)
      {
        if (!d_stage_td.reserve(channels * n)) return false;
        SDFT_TRY(hipMemcpyAsync(d_stage_td.p, xs, bytes, hipMemcpyDeviceToDevice, stream));
        xs = d_stage_td.p;
      }
    }

    bool ok;
    const long chunks = logic::choose_chunks(chunk_query(n, rows_kernel_ok(false))).chunks;
    // reference order asked for on two-slot rows at FD float: the ordered walk (N dependent additions shared
    // by the four samples of a group) costs more than the synthesis pass it saves (N = 4096, n = 262144:
    // 5.7 ms against 4.1 ms for the two passes, which give the same bits); fused_exact = 2 insists on the kernel
    const bool walk_loses = row_slots() == 2 && sizeof(FD) == 4 && carry_mode == CARRY_EXACT && opt_fused_exact == 1;
    // calls of one time chunk: the folded form in one launch (process_hop2_kernel) unless the reference's order
    // is wanted -- then the hop kernel + row synthesis pair below, which is bit-identical
    const bool one_chunk_folded = chunks == 1 && n <= (size_t)kHopMax && !wants_reference_order() && !dfts && opt_fold && nbins >= 8 && opt_hop_kernel &&
                                  linear && one_vector;
    if (one_chunk_folded)
    {
      if (!fold_coefficients(op)) return false;
      last_process_path = 1;
      flag_wanted = xd && yd;
      ok = coeff_ready && process_hop(n, xs, n, ys, n);
      flag_wanted = false;
    }
    // the folded form carries up to four bins per lane whatever the bin type is (N <= 4096); the forms that keep the
    // windowed rows in LDS stop at two slots of the row-group kernel (N <= 2048 double / 4096 float)
    else if ((fuse_ok() || (linear && op.rows <= 65535u && !wants_reference_order() && !dfts && opt_fold && nbins >= 8 && nbins <= (size_t)4 * kWave * kRowWavesMax))
             && (chunks > 1 || n > (size_t)kHopMax) && !walk_loses)       // (many channels: one chunk per channel, however long)
    {
      FuseArgs<TD, FD> fz{};
      fz.y = ys; fz.y_stride = n; fz.syn = d_syn.p; fz.sweight = tab.sweight; fz.op = op; fz.store = dfts ? 1 : 0;
      fz.walked = walked_counter();
      if (!dfts) { if (!fold_coefficients(op)) return false; } else coeff_ready = false;
      last_process_path = 1;
      flag_wanted = xd && yd;
      ok = forward_device(n, xs, n, dfts, n * nbins, nullptr, &fz);
      flag_wanted = false;
    }
    else
    {
      // short calls (one time chunk: the hop kernel and the row-per-wave synthesis, two launches) and
      // shapes the row-group kernel does not cover: analysis into the caller's matrix or a bounded
      // workspace, synthesis with the operation applied on the way in
      const size_t row_elems = channels * nbins;
      size_t seg = dfts ? n : std::min(n, std::max<size_t>(1, stage_bytes / std::max<size_t>(row_elems * sizeof(fdx), 1)));
      if (!dfts && seg < n && stage_bytes == kDefaultStageBytes)
      {
        // long calls run best in one piece (time segments restart the carry pipeline): unless the host
        // has bounded it (option stage_bytes), the workspace may take up to half of what the device has free
        if (d_stage_fdx.cap >= row_elems * n) seg = n;
        else
        {
          size_t free_b = 0, total_b = 0;
          if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            seg = std::max(seg, std::min(n, (free_b / 2) / std::max<size_t>(row_elems * sizeof(fdx), 1)));
          (void)hipGetLastError();
        }
      }
      // (batched plans take segments too: the workspace's channel stride is the segment, mstride below)
      if (!dfts && !d_stage_fdx.reserve(row_elems * seg)) return false;
      last_process_path = (chunks == 1) ? 2 : 3;
      last_fused_exact = 0; last_fused_fold = 0;
      if (op_kind == OP_USER)
      {
        // every run-time-compiled kernel the segments below will ask for is resolved BEFORE the first launch: statements
        // that do not compile must not leave the stream advanced by an analysis whose synthesis then fails
        const size_t m_first = std::min(seg, n), m_last = n - ((n - 1) / seg) * seg;
        const bool hop_form = opt_exact_inverse && opt_inverse_rows <= 0;
        const bool any_hop = hop_form && (channels * m_first <= 1024 || channels * m_last <= 1024);
        const bool any_rows = !hop_form || channels * m_first > 1024 || channels * m_last > 1024 || dfts != nullptr;
        hipFunction_t fn = nullptr;
        char name[160];
        if (any_hop)
        {
          snprintf(name, sizeof(name), "sdfthip::inverse_row_kernel<%s, %s, %s, true>", type_name<TD>(), type_name<FD>(), latency == 1 ? "true" : "false");
          if (!rtc_kernel(user_expr.c_str(), name, device, &fn)) return false;
        }
        if (any_rows)
        {
          snprintf(name, sizeof(name), "sdfthip::user_rows_kernel<%s>", type_name<FD>());
          if (!rtc_kernel(user_expr.c_str(), name, device, &fn)) return false;
        }
      }
      ok = true;
      for (size_t t = 0; t < n && ok; t += seg)
      {
        const size_t m = std::min(seg, n - t);
        fdx* mat = dfts ? dfts + t * nbins : d_stage_fdx.p;
        const size_t mstride = dfts ? n * nbins : m * nbins;
        SpectralOp<FD> ops = op; ops.t0 = t;                  // gain vectors count from the start of the call
        if (op_kind == OP_USER && opt_exact_inverse && opt_inverse_rows <= 0 && channels * m <= 1024)
        {
          // a hop: the statements run inside the row synthesis (two launches); a copy of the spectrum is processed afterwards
          ok = forward_device(m, xs + t, n, mat, mstride, nullptr) && inverse_device(m, mat, mstride, nullptr, ys + t, n, &ops);
          if (ok && dfts) ok = user_rows(mat, mstride, m, ops);
        }
        else if (op_kind == OP_USER)                          // the host's operation rewrites the rows in place, then plain synthesis
          ok = forward_device(m, xs + t, n, mat, mstride, nullptr) && user_rows(mat, mstride, m, ops) && inverse_device(m, mat, mstride, nullptr, ys + t, n, nullptr);
        else
        {
        ok = forward_device(m, xs + t, n, mat, mstride, nullptr) && inverse_device(m, mat, mstride, nullptr, ys + t, n, &ops);
        if (ok && (op_kind == OP_GAIN || op_kind == OP_CGAIN || op_kind >= OP_GATE) && dfts) ok = scale_rows(mat, mstride, m, ops);
        }
      }
    }
    if (!ok) return false;
    if (!yd)
    {
      if (!to_host(y, ys, channels * n * sizeof(TD))) return false;
      return synchronize();
    }
    // (the fused call moves the samples only -- unless the host asked for a copy of the spectrum or the shape took the two passes)
    return finish((dfts || last_process_path != 1) ? matrix_bytes(n) : std::max<size_t>(1, channels * n * 2 * sizeof(TD)));
  }

  // the host's own operation on stored rows (two-pass route): user_rows_kernel compiled at run time with its statements
  bool user_rows(fdx* mat, size_t stride, size_t rows, const SpectralOp<FD>& op)
  {
    char name[96];
    snprintf(name, sizeof(name), "sdfthip::user_rows_kernel<%s>", type_name<FD>());
    hipFunction_t fn = nullptr;
    if (!rtc_kernel(user_expr.c_str(), name, device, &fn)) return false;
    if (!pipe_join()) return false;
    const size_t total = channels * rows * nbins;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    fdx* a0 = mat; size_t a1 = stride, a2 = rows; unsigned a3 = (unsigned)nbins, a4 = (unsigned)channels; SpectralOp<FD> a5 = op;
    void* args[] = {&a0, &a1, &a2, &a3, &a4, &a5};
    SDFT_TRY(hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, stream, args, nullptr));
    return true;
  }

  // processed copy of the spectrum on the two-pass path: rows *= gain (the fused kernel stores them scaled)
  bool scale_rows(fdx* mat, size_t stride, size_t rows, const SpectralOp<FD>& op)
  {
    if (!pipe_join()) return false;
    const size_t total = channels * rows * nbins;
    const unsigned blocks = (unsigned)std::min<size_t>((total + kBlock - 1) / kBlock, 65536);
    hipLaunchKernelGGL((scale_rows_kernel<FD>), dim3(blocks), dim3(kBlock), 0, stream, mat, stride, rows, (unsigned)nbins, (unsigned)channels, op);
    SDFT_TRY(hipGetLastError());
    return true;
  }

  // checkpoint / resume: install a state previously read with get_state (any plan of the same
  // dftsize, window, latency, types and channel count -- also on another GPU)
  bool set_state(const fdx* acc, const fdx* fid, const TD* hist, size_t cur)
  {
    if (!bind()) return false;
    if (!pipe_join()) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (nbins)
    {
      if (cur >= 2 * nbins) { set_error("sdft_hip_set_state", "cursor out of range"); return false; }
      if (acc && !to_device(acc_p(), acc, channels * nbins * sizeof(fdx))) return false;
      if (fid) { if (!to_device(fid_p(), fid, channels * nbins * sizeof(fdx))) return false; fid_canonical = false; }
      if (hist && !to_device(d_hist[hist_cur].p, hist, channels * 2 * nbins * sizeof(TD))) return false;
      SDFT_TRY(hipStreamSynchronize(stream));
    }
    cursor = cur;
    return true;
  }

  // state read-back for tests: acc, fid [channels][N]; hist [channels][2N] in time order
  bool get_state(fdx* acc, fdx* fid, TD* hist, size_t* cur)
  {
    if (!bind()) return false;
    if (!pipe_join()) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (nbins)
    {
      if (acc && !to_host(acc, acc_p(), channels * nbins * sizeof(fdx))) return false;
      if (fid && !to_host(fid, fid_p(), channels * nbins * sizeof(fdx))) return false;
      if (hist && !to_host(hist, d_hist[hist_cur].p, channels * 2 * nbins * sizeof(TD))) return false;
      SDFT_TRY(hipStreamSynchronize(stream));
    }
    if (cur) *cur = cursor;
    return true;
  }
