// mw_repair.inc — mg_search_repair's and mg_repair_leaves' host code, included
// by mw_kernels.hip after tiles_enqueue, mg_search_blame and mw_collect.inc
// (inside its extern "C" block).  The kernel is in mw_kernels.hip
// (mw_repair_kernel, RepairEnv), the mutation rule in mw_mutate.h, the sizes in
// mw_launch_plan.h plan_search_repair, the fold is mg_search_blame's
// (mw_blame_fold_kernel, mw_blame.h's key and totals).

// The call's table as the device reads it: the base assignment canonical at
// each leaf's width, the mutable leaves, their prefix sums.  Null if the
// arguments are fine, else why they are refused.
static const char* repair_table(const Prog* p, const uint32_t* base, const uint32_t* mut, size_t nmut, u32 radius,
                                std::vector<u32>& table) {
  const u32 nl = (u32)p->desc.nleaves;
  if (const char* why = mutant_args_refused(p->h_leaves.data(), nl, mut, nmut, radius)) return why;
  table.resize((size_t)nl * 8 + 2 * nmut + 1);
  std::memcpy(table.data(), base, (size_t)nl * 8 * sizeof(u32));
  for (u32 l = 0; l < nl; ++l) canon(table.data() + (size_t)l * 8, p->h_leaves[(size_t)l * MW_LEAF_WORDS + MW_LEAF_WIDTH]);
  u32* tmut = table.data() + (size_t)nl * 8;
  std::memcpy(tmut, mut, nmut * sizeof(u32));
  mutant_prefix(p->h_leaves.data(), tmut, (u32)nmut, tmut + nmut);
  return nullptr;
}

// Enqueue mg_search_repair's work (the context's mu held): mg_search_blame's
// totals (tot, from the pool) zeroed and their nearest key set to all ones,
// then tiles_enqueue with the table as the launch block's extra records,
// mw_repair_kernel as every tile's evaluation and mw_blame_fold_kernel as its
// fold (over the tile's verdicts when the call names no rows), the readbacks.
static int search_repair_enqueue(Ctx* c, const Prog* p, const std::vector<u32>& table, u32 nmut, u32 radius,
                                 uint64_t seed, uint64_t begin, uint64_t count, u32 row, u32 nrows,
                                 const RepairPlan& R, Scratch& vt, Scratch& tot) {
  const LexPlan& L = R.tiles;
  if (!vt.p || !tot.p) return fail(MG_E_NOMEM, "mg_search_repair: tile and total buffers");
  if (!ensure_readback(c, R.total_bytes)) return fail(MG_E_NOMEM, "mg_search_repair: readback buffer");
  unsigned long long* d_tot = (unsigned long long*)tot.p;
  const u32 frows = R.fold_rows;
  const size_t count_bytes = (size_t)blame_bins(frows) * sizeof(u64);
  std::vector<AsmArgs> recs((table.size() * sizeof(u32) + sizeof(AsmArgs) - 1) / sizeof(AsmArgs));
  std::memset(recs.data(), 0, recs.size() * sizeof(AsmArgs));
  std::memcpy(recs.data(), table.data(), table.size() * sizeof(u32));
  const size_t nl8 = (size_t)p->desc.nleaves * 8;
  // (read by the launches only after tiles_enqueue has sized the launch block)
  auto d_table = [&] { return (const u32*)(c->d_asmargs + tile_records(L)); };
  const TileEval eval = [&](u64 n, u64 tb, u32* d_v, u32* d_t, u64 gx) {
    const u32* t = d_table();
    hipLaunchKernelGGL(mw_repair_kernel, dim3((u32)gx), dim3(kBlock), (size_t)L.nlds * kBlock * 4, c->stream, p->dev, t,
                       t + nl8, t + nl8 + nmut, nmut, radius, n, seed, tb, d_v, d_t, c->d_spill, L.nlds);
    return hipGetLastError();
  };
  int rc = tiles_enqueue(
      c, p, seed, begin, count, L, vt, recs.data(), recs.size(),
      [&] {
        const hipError_t e = hipMemsetAsync(d_tot, 0, count_bytes, c->stream);
        return e != hipSuccess ? e : hipMemsetAsync(d_tot + blame_bins(frows), 0xff, sizeof(u64), c->stream);
      },
      [&](u64 n, u64 tb, const u32* d_v, const u32* d_t) {
        hipLaunchKernelGGL(mw_blame_fold_kernel, dim3((u32)L.fold_gx), dim3(kBlock), 0, c->stream, nrows ? d_t : d_v, n,
                           (u32)n, tb - begin, nrows ? row : 0u, frows, d_tot);
      },
      &eval);
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->e1, c->stream));
  HIPCHK(stage_readback(c, 1));   // the counters
  HIPCHK(hipMemcpyAsync(c->h_rb, d_tot, R.total_bytes, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int mg_search_repair(mg_ctx* h, mg_prog* hp, const uint32_t* base, const uint32_t* mutable_leaves, size_t nmut,
                     uint64_t seed, uint32_t radius, uint64_t begin, uint64_t count, uint32_t row, uint32_t nrows,
                     uint64_t tile, mg_repair_result* out, mg_stats* st) {
  if (!out || !base || !mutable_leaves) return fail(MG_E_ARG, "null argument");
  if (count == 0 || begin + count < begin) return fail(MG_E_ARG, "bad candidate range");
  if (begin + count > (1ull << kBlameOffsetBits))
    return fail(MG_E_ARG, "mg_search_repair: mutant indices stay below 2^48");
  if (nrows > kBlameMaxRows) return fail(MG_E_ARG, "mg_search_repair: at most 1024 conjunct rows");
  if (tile % kBlock) return fail(MG_E_ARG, "mg_search_repair: the tile is a multiple of 256 candidates (0: the default)");
  mw::CallMark mark("mg_search_repair");
  mark.step("lock", count);
  CallG call;
  int rc = prog_enter(g_reg, "mg_search_repair", h, hp, call);
  if (rc) return rc;
  Ctx* c = call.c.get();
  const Prog* p = call.ps[0].get();
  if (nrows && (row >= p->desc.n_trace_rows || nrows > p->desc.n_trace_rows - row))
    return fail(MG_E_ARG, "mg_search_repair: the conjunct rows are rows of the program's trace");
  std::vector<u32> table;
  if (const char* why = repair_table(p, base, mutable_leaves, nmut, radius, table))
    return fail(MG_E_ARG, std::string("mg_search_repair: ") + why);
  double t0;
  rc = reduce_begin(c, mark, &t0);
  if (rc) return rc;
  const RepairPlan R = plan_search_repair(facts_of(p), count, tile, nrows, p->desc.n_trace_rows, (u32)p->desc.nleaves,
                                          (u32)nmut, c->ncu);
  if (!R.tiles.ntiles) return fail(MG_E_ARG, "mg_search_repair: more than 65536 tiles: a larger tile or a shorter range");
  mark.step("enqueue", count);
  Scratch vt(c, R.tiles.scratch_bytes), tot(c, R.total_bytes);
  rc = search_repair_enqueue(c, p, table, (u32)nmut, radius, seed, begin, count, row, nrows, R, vt, tot);
  if (rc == 0) rc = reduce_finish(c, mark, count, {&vt, &tot});
  if (rc) return rc;   // (the buffers wait for the stream before they go back to the pool)
  const u64* t = (const u64*)c->h_rb;
  const u64 key = t[blame_bins(R.fold_rows)];   // count >= 1: some block has written it
  std::memset(out, 0, sizeof(*out));
  out->index = begin + blame_key_offset(key);
  out->nfail = blame_key_nfail(key);
  out->satisfied = t[2 * R.fold_rows];
  const u64 ev[kNCounters] = {count, 0, 0, 0, 0};   // mw_repair_kernel counts nothing, as mw_eval_kernel
  return fill_stats(c, st, ev, t0, R.nlaunches, (double)count * (double)p->ops_per_eval);
}

int mg_repair_leaves(mg_ctx* h, const mg_prog* hp, const uint32_t* base, const uint32_t* mutable_leaves, size_t nmut,
                     uint64_t seed, uint32_t radius, uint64_t index, uint32_t* out) {
  if (!out || !base || !mutable_leaves) return fail(MG_E_ARG, "null argument");
  mw::CallMark mark("mg_repair_leaves");
  mark.step("lock");
  CallG call;
  // nothing is launched: allowed while a begun search is pending
  if (int rc = prog_enter(g_reg, "mg_repair_leaves", h, hp, call, true)) return rc;
  const Prog* p = call.ps[0].get();
  std::vector<u32> table;
  if (const char* why = repair_table(p, base, mutable_leaves, nmut, radius, table))
    return fail(MG_E_ARG, std::string("mg_repair_leaves: ") + why);
  const u32 nl = (u32)p->desc.nleaves;
  const u32* tmut = table.data() + (size_t)nl * 8;
  mutant_leaves(table.data(), p->h_leaves.data(), nl, p->h_pool.data(), tmut, tmut + nmut, (u32)nmut, seed, radius,
                index, out);
  return 0;
}
