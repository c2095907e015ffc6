// mw_collect.inc — mg_search_collect's host code, included by mw_kernels.hip
// after tiles_enqueue and mg_search_blame (inside its extern "C" block).  The
// kernels are in mw_kernels.hip (mw_collect_count_kernel,
// mw_collect_scatter_kernel), the rules they share with the CPU check in
// mw_collect.h, the sizes in mw_launch_plan.h plan_search_collect.

static_assert(kCollectChunk == (u32)kBlock, "a collect block steps one candidate per thread");
static_assert(kLexScratchBudget / 4 <= (1ull << 32) - kBlock, "a tile's offsets and a block's count fit 32 bits");

// Enqueue mg_search_collect's work (the context's mu held): the result block
// and the blocks' counts in one pool buffer (res), its two base slots zeroed,
// then tiles_enqueue with the count and scatter kernels as every tile's fold,
// the readbacks.
static int search_collect_enqueue(Ctx* c, const Prog* p, uint64_t seed, uint64_t begin, uint64_t count, u32 row,
                                  u32 nrows, u32 cap, const CollectPlan& C, Scratch& vt, Scratch& res) {
  const LexPlan& L = C.tiles;
  if (!vt.p || !res.p) return fail(MG_E_NOMEM, "mg_search_collect: tile and result buffers");
  if (!ensure_readback(c, C.readback_bytes)) return fail(MG_E_NOMEM, "mg_search_collect: readback buffer");
  char* d_res = (char*)res.p;
  u64* d_base = (u64*)d_res;
  u64* d_idx = (u64*)(d_res + collect_idx_offset());
  u32* d_rows = (u32*)(d_res + collect_rows_offset(cap));
  u32* d_cnt = (u32*)(d_res + C.out_bytes);
  int rc = tiles_enqueue(
      c, p, seed, begin, count, L, vt, nullptr, 0,
      [&] { return hipMemsetAsync(d_base, 0, kCollectBaseBytes, c->stream); },
      [&](u64 n, u64 tb, const u32* d_v, const u32* d_t) {
        const u32 slot = collect_base_slot((tb - begin) / L.tile);
        hipLaunchKernelGGL(mw_collect_count_kernel, dim3((u32)L.fold_gx), dim3(kBlock), 0, c->stream, d_v, (u32)n, d_cnt);
        hipLaunchKernelGGL(mw_collect_scatter_kernel, dim3((u32)L.fold_gx), dim3(kBlock), 0, c->stream, d_v, d_t, n,
                           (u32)n, tb, (const u32*)d_cnt, d_base, slot, cap, row, nrows, d_idx, d_rows);
      });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->e1, c->stream));
  HIPCHK(stage_readback(c, 1));   // the counters
  HIPCHK(hipMemcpyAsync(c->h_rb, d_res, C.readback_bytes, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int mg_search_collect(mg_ctx* h, mg_prog* hp, uint64_t seed, uint64_t begin, uint64_t count, uint32_t row,
                      uint32_t nrows, uint64_t tile, uint64_t* out_idx, uint32_t* out_rows, size_t cap,
                      mg_collect_result* out, mg_stats* st) {
  if (!out || !out_idx) return fail(MG_E_ARG, "null argument");
  if (count == 0 || begin + count < begin) return fail(MG_E_ARG, "bad candidate range");
  if (cap == 0 || cap > kCollectMaxCap) return fail(MG_E_ARG, "mg_search_collect: room for 1 to 65536 witnesses");
  if (nrows > kCollectMaxRows) return fail(MG_E_ARG, "mg_search_collect: at most 64 rows per witness");
  if (nrows && !out_rows) return fail(MG_E_ARG, "mg_search_collect: rows are asked for and out_rows is null");
  if (tile % kBlock) return fail(MG_E_ARG, "mg_search_collect: the tile is a multiple of 256 candidates (0: the default)");
  mw::CallMark mark("mg_search_collect");
  mark.step("lock", count);
  CallG call;
  int rc = prog_enter(g_reg, "mg_search_collect", h, hp, call);
  if (rc) return rc;
  Ctx* c = call.c.get();
  const Prog* p = call.ps[0].get();
  if (nrows && (row >= p->desc.n_trace_rows || nrows > p->desc.n_trace_rows - row))
    return fail(MG_E_ARG, "mg_search_collect: the gathered rows are rows of the program's trace");
  double t0;
  rc = reduce_begin(c, mark, &t0);
  if (rc) return rc;
  const CollectPlan C = plan_search_collect(facts_of(p), count, tile, (u32)cap, nrows, p->desc.n_trace_rows, c->ncu,
                                            asm_enabled(), wide_lds_words());
  if (!C.tiles.ntiles)
    return fail(MG_E_ARG, "mg_search_collect: more than 65536 tiles: a larger tile or a shorter range");
  mark.step("enqueue", count);
  Scratch vt(c, C.tiles.scratch_bytes), res(c, C.buffer_bytes);
  rc = search_collect_enqueue(c, p, seed, begin, count, row, nrows, (u32)cap, C, vt, res);
  if (rc == 0) rc = reduce_finish(c, mark, count, {&vt, &res});
  if (rc) return rc;   // (the buffers wait for the stream before they go back to the pool)
  const char* r = (const char*)c->h_rb;
  u64 slots[2];
  std::memcpy(slots, r, kCollectBaseBytes);
  std::memset(out, 0, sizeof(*out));
  out->total = slots[collect_base_slot(C.tiles.ntiles)];
  out->stored = (u32)std::min<u64>(out->total, cap);
  std::memcpy(out_idx, r + collect_idx_offset(), (size_t)out->stored * sizeof(u64));
  if (nrows) std::memcpy(out_rows, r + collect_rows_offset((u32)cap), (size_t)out->stored * nrows * sizeof(u32));
  u64 ctr[kNCounters];
  read_counters(c, ctr);
  // the evaluations alone, as mg_search_lexmin reports them
  const u64 ev[kNCounters] = {C.tiles.engine.kind == kAsm ? ctr[0] : count, 0, 0, 0, 0};
  return fill_stats(c, st, ev, t0, C.nlaunches, (double)ev[0] * (double)p->ops_per_eval);
}
