/* mythril_witness.h — C-ABI of the MI355X constraint-witness engine.
 *
 * Drop-in boundary.  The reference has no native FFI of its
 * own on this path: Mythril is pure Python and crosses into native code only
 * through z3-solver's and pysha3's ctypes/C-extension bindings.  Each entry
 * point below replaces one of those crossings and is bound from Python with
 * ctypes exactly the way z3's own bindings are:
 *
 *   mg_search     replaces z3 Optimize.check() for feasibility-only queries
 *                 (mythril/laser/smt/solver/solver.py:50-66, reached from
 *                  mythril/support/model.py:58 get_model)
 *   mg_search_min replaces z3 Optimize.minimize() + check() for a bound on the
 *                 first objective (mythril/laser/smt/solver/solver.py:109-114,
 *                  reached from mythril/analysis/solver.py:216-256)
 *   mg_eval       replaces z3 ModelRef.eval / substitute+simplify for a batch
 *                 of assignments (mythril/laser/smt/model.py:52-59)
 *   mg_keccak256  replaces _pysha3.keccak_256 (mythril/support/support_utils.py:50-59,
 *                 called by keccak_function_manager.py:57-69 find_concrete_keccak)
 *
 * Conventions: every call returns 0 on success or a negative MG_E* code; the
 * message for the calling thread is in mg_last_error().  The caller owns all
 * host buffers (copied in/out); program handles are library-owned until
 * mg_prog_free.  Nothing throws across the ABI.
 * Lifetimes and threads (mythril_amd/csrc/mw_handles.h): a handle is an opaque
 * id, never an address, and ids are never reused.  Calls on one context are
 * serialised; calls may come from any thread.  mg_free also frees every
 * program still loaded in that context, after the call in flight on it (from
 * another thread) has finished.  A handle that is not live (already freed,
 * freed with its context, never returned by the library) is refused with
 * MG_E_ARG by every entry point, also when it is freed by another thread
 * while the call waits for the context.  Programs are validated on load (slot ranges, constant offsets,
 * opcodes) so a malformed program can never be launched.
 */
#ifndef MYTHRIL_WITNESS_H
#define MYTHRIL_WITNESS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_E_ARG -1
#define MG_E_HIP -2
#define MG_E_PROG -3
#define MG_E_NOMEM -4

#define MG_NONE UINT64_MAX /* no witness in the searched range */

/* search flags (same values as MW_FLAG_* in mw_isa.h) */
#define MG_FLAG_EARLY_EXIT 1u
#define MG_FLAG_STOP_AFTER_HIT 2u
/* specialised kernels write no launch counters (division-path counts stay 0;
 * evals = count per program); ignored together with MG_FLAG_STOP_AFTER_HIT */
#define MG_FLAG_NO_COUNT 4u

typedef struct mg_ctx mg_ctx;
typedef struct mg_prog mg_prog;

/* A compiled constraint program (produced by mythril_amd.compiler). */
typedef struct {
  const uint32_t* code;   /* 4 words per instruction, ends with MW_END */
  size_t ncode_words;
  const uint32_t* consts; /* constant pool words */
  size_t nconst_words;
  const uint32_t* leaves; /* MW_LEAF_WORDS words per free variable */
  size_t nleaves;
  const uint32_t* pool;   /* candidate pools, MW_POOL_ENTRY_WORDS_OF(width) per entry */
  size_t npool_words;
  uint32_t n_spill;       /* spill-area words per lane (SPILL_W/FILL_W imm: 8-word slot offset, _N: 1 word) */
  uint32_t n_trace_rows;  /* rows written by MW_STORE_* (mg_eval trace) */
  uint32_t n_input_rows;  /* SoA leaf rows mg_eval reads */
  uint32_t reserved;
  uint64_t ops_per_eval;  /* algorithmic u32 ops per candidate */
} mg_prog_desc;

typedef struct {
  double kernel_ms;      /* device time of the search/eval kernels (HIP events) */
  double wall_ms;        /* host wall time of the call */
  uint64_t evals;        /* program x candidate verdicts determined */
  uint64_t launches;
  double ops;            /* algorithmic u32 ops executed (evals x ops_per_eval) */
  /* Wide divisions (mw_alu.h udivrem8) take one of three paths per wave; each
   * count is (events per wave) x (valid lanes of that wave), summed.  bench.py
   * and compiler.Program.executed_ops price the executed division work from
   * them (tests/test_gpu_fullsize.py and tests/test_divcount.py check them against oracle/c). */
  uint64_t lane_div_steps;    /* schoolbook digit positions run (some lane's digit nonzero) */
  uint64_t lane_div_full;     /* one-digit path: every lane's divisor full width */
  uint64_t lane_div_short;    /* short division: every lane's divisor one limb */
  uint64_t lane_div_general;  /* limb-aligned schoolbook entries */
} mg_stats;

int mg_device_count(int* n);
int mg_init(int device, mg_ctx** out);
int mg_free(mg_ctx* ctx);

/* Upload a program (replaces the per-query z3 model construction the
 * reference runs, mythril/support/model.py:15-63, with a device-resident
 * program).  The desc's arrays are copied before the call returns; the device
 * copy is queued on the context's stream, so every later call on the context
 * sees it, and a copy failure is reported by the next call that waits. */
int mg_prog_load(mg_ctx* ctx, const mg_prog_desc* desc, mg_prog** out);
int mg_prog_free(mg_prog* prog);

/* Search candidate indices [begin, begin+count) of every program; out_min_idx[i]
 * receives the lowest index whose assignment satisfies program i, or MG_NONE. */
int mg_search(mg_ctx* ctx, mg_prog* const* progs, size_t nprog, uint64_t seed,
              uint64_t begin, uint64_t count, uint32_t flags, uint64_t* out_min_idx,
              mg_stats* stats);

/* mg_search in two calls, so the caller can work on the host while the device
 * searches (engine.WitnessEngine compiles the witness programs meanwhile).
 * mg_search_begin validates, plans and enqueues the search and returns; until
 * mg_search_end every other call that launches work on this context is
 * refused (MG_E_ARG), and a program of the search freed meanwhile waits for it.
 * mg_search_end completes it: the same out_min_idx and stats as mg_search.
 * witness (nullable): per program, a witness program description (or NULL);
 * each is uploaded and evaluated at the index its program's search found,
 * queued after the search, read back with the same synchronisation into
 * out_trace[i] (its n_trace_rows words; traced[i] = 1), or left for the caller
 * (traced[i] = 0: no witness found, or a program the asm interpreter does not
 * run).  Replaces Optimize.check + model() of mythril/support/model.py:58-60. */
int mg_search_begin(mg_ctx* ctx, mg_prog* const* progs, size_t nprog, uint64_t seed, uint64_t begin,
                    uint64_t count, uint32_t flags);
int mg_search_end(mg_ctx* ctx, uint64_t* out_min_idx, mg_stats* stats, const mg_prog_desc* const* witness,
                  uint32_t* const* out_trace, int32_t* traced);

typedef struct { uint64_t index; uint32_t value[8]; } mg_min_result;
/* Lowest objective among the witnesses of candidates [begin, begin+count): the
 * program's trace rows 0..n_trace_rows-1 (1..8 rows) are the objective's limbs,
 * least significant first (limbs never stored are 0), compared as one unsigned
 * value of up to 256 bits; equal objectives: the lowest index.  Every candidate
 * of the range is evaluated, in one launch and one synchronisation.
 * out->index = MG_NONE (and value = 0) when no candidate satisfies.
 * It always runs the compiled interpreter (mw_search_min_kernel), whatever
 * mg_prog_engine says for the program: the asm interpreter, the assembled and
 * the specialised kernels have no such mode.  Refused with MG_E_ARG for a
 * program of 0 or more than 8 trace rows, for count == 0, and while a search
 * begun with mg_search_begin is pending on the context.  Same handle, lock
 * and in-flight protocol as mg_search.  Replaces Optimize.minimize + check
 * for the first objective (mythril/laser/smt/solver/solver.py:109-114 and
 * :51-66, reached from mythril/analysis/solver.py:216-256): a bound from one
 * pass over the candidates, not the optimum over all assignments. */
int mg_search_min(mg_ctx* ctx, mg_prog* prog, uint64_t seed, uint64_t begin,
                  uint64_t count, mg_min_result* out, mg_stats* stats);

typedef struct { uint32_t row, nrows; } mg_lex_obj;
typedef struct { uint64_t index; uint32_t value[8][8]; } mg_lex_result;   /* value[k]: objective k's limbs */
/* Lexicographic minimum over several objectives among the witnesses of
 * candidates [begin, begin+count).  Objective k is the program's trace rows
 * [objs[k].row, objs[k].row + objs[k].nrows), 1..8 limbs, least significant
 * first, one unsigned value; objs[0] has the highest priority; every objective
 * equal: the lowest index.  Two objectives may name the same rows, and rows
 * need not follow the priority order.  The range is cut into tiles of `tile`
 * candidates (a multiple of 256; 0: the default; cut further so that one
 * tile's verdicts and trace rows fit 64 MiB).  Each tile is evaluated with its
 * trace rows on the engine mg_eval_generated uses when a trace is asked for
 * (the asm interpreter where it runs the program, else the compiled one; an
 * attached specialised or assembled kernel is not used), then folded into a
 * running minimum on the device: stats->launches == 2 * tiles + 1,
 * stats->evals == count, one synchronisation.  out->index = MG_NONE (and value
 * all zero) when no candidate satisfies.  Refused with MG_E_ARG for nobj of 0
 * or above 8, nrows of 0 or above 8, rows outside the program's trace, count
 * == 0 or a wrapping range, a tile that is no multiple of 256, more than
 * 65536 tiles, and while a search begun with mg_search_begin is pending.
 * Same handle, lock and in-flight protocol as mg_search_min.  Replaces
 * Optimize.minimize over the whole objective tuple + check
 * (mythril/laser/smt/solver/solver.py:109-114 and :51-66, reached from
 * mythril/analysis/solver.py:51-68 and :216-256, which minimises
 * (calldatasize, callvalue) per transaction lexicographically): a bound from
 * one pass over the candidates, not the optimum over all assignments. */
int mg_search_lexmin(mg_ctx* ctx, mg_prog* prog, uint64_t seed, uint64_t begin, uint64_t count,
                     const mg_lex_obj* objs, size_t nobj, uint64_t tile, mg_lex_result* out, mg_stats* stats);
/* The tile mg_search_lexmin cuts a range of `count` candidates of this
 * program into when asked for `tile`, in *out.  Replaces nothing in the
 * reference: a diagnostic for tests and benchmarks. */
int mg_search_lexmin_tile(mg_ctx* ctx, mg_prog* prog, uint64_t count, uint64_t tile, uint64_t* out);

typedef struct {
  uint64_t satisfied;      /* candidates failing no row */
  uint64_t near_index;     /* MG_NONE never: count >= 1 */
  uint32_t near_nfail;     /* rows the nearest candidate fails (0: it is a witness) */
  uint32_t reserved;
} mg_blame_result;
/* Why a search missed: per-conjunct failure counts over candidates
 * [begin, begin+count).  The program's trace rows [row, row + nrows), 1..1024
 * of them, each hold one conjunct's truth for a candidate: a row that reads 0
 * is a failed conjunct, any other value a satisfied one.  With F(c) the set of
 * rows candidate c fails: out_fail[j] counts the candidates with j in F(c),
 * out_sole[j] those with F(c) = {j} (rejected by that conjunct alone),
 * out->satisfied those with F(c) empty, and out->near_index / near_nfail are
 * the candidate of lowest (|F(c)|, index).  All counts are exact and depend on
 * neither grid, tile nor engine.  The program's own verdict is ignored (every
 * row of every candidate is stored whatever it is) and so are the rows outside
 * [row, row + nrows).  The range is cut into tiles by mg_search_lexmin's rule
 * (mg_search_lexmin_tile answers for both calls), each tile is evaluated with
 * its trace rows on the engine mg_eval_generated uses when a trace is asked
 * for (no attached kernel), then folded into the call's totals on the device
 * with atomic adds, without a reduction kernel: stats->launches == 2 * tiles,
 * stats->evals == count, one upload and one synchronisation.  Refused with
 * MG_E_ARG for a null output, count == 0 or a wrapping range, nrows of 0 or
 * above 1024, rows outside the program's trace, a tile that is no multiple of
 * 256, more than 65536 tiles, and while a search begun with mg_search_begin is
 * pending.  Same handle, lock and in-flight protocol as mg_search_lexmin.
 * Replaces nothing in the reference: for a set without a model z3's
 * Optimize.check answers unsat or unknown
 * (mythril/laser/smt/solver/solver.py:50-66) and names no conjunct.  A
 * diagnostic for misses (WitnessEngine.explain_miss). */
int mg_search_blame(mg_ctx* ctx, mg_prog* prog, uint64_t seed, uint64_t begin, uint64_t count,
                    uint32_t row, uint32_t nrows, uint64_t tile,
                    uint64_t* out_fail, uint64_t* out_sole,   /* nrows each */
                    mg_blame_result* out, mg_stats* stats);

typedef struct {
  uint64_t total;          /* candidates of the range whose verdict is 1 */
  uint32_t stored;         /* min(total, cap): entries written to out_idx (and out_rows) */
  uint32_t reserved;
} mg_collect_result;
/* Which candidates are witnesses, and how many: over candidates
 * [begin, begin+count), out->total is the exact number whose verdict is 1,
 * out_idx[0..stored) are the stored = min(total, cap) lowest witness indices
 * in ascending order, and out_rows[k * nrows + r] is trace row row + r of
 * witness k.  nrows == 0 gathers nothing: out_rows is ignored (may be NULL)
 * and a program without trace rows is accepted.  Entries past `stored` are
 * left untouched.  Every result is exact and depends on neither grid, tile
 * nor engine.  The range is cut into tiles by mg_search_lexmin's rule
 * (mg_search_lexmin_tile answers for this call too) and each tile is
 * evaluated with its trace rows on the engine mg_eval_generated uses when a
 * trace is asked for (the asm interpreter where it runs the program, else the
 * compiled one; no attached kernel).  Two kernels then fold the tile, in
 * candidate order: one counts the witnesses of each fold block's contiguous
 * segment, one places them behind those of the blocks and tiles before (an
 * order-preserving compaction; ordering comes from kernel boundaries alone,
 * no block waits for another and nothing is atomic).  The whole range is
 * always evaluated: stats->evals == count, stats->launches == 3 * tiles, one
 * upload and one synchronisation; the readback is 16 + cap * (8 + 4 * nrows)
 * bytes.  Refused with MG_E_ARG for a null out or out_idx, cap of 0 or above
 * 65536, nrows above 64, nrows > 0 with a null out_rows, rows outside the
 * program's trace, count == 0 or a wrapping range, a tile that is no multiple
 * of 256, more than 65536 tiles, and while a search begun with
 * mg_search_begin is pending.  Same handle, lock and in-flight protocol as
 * mg_search_blame.  Replaces nothing in the reference: z3's Optimize.model()
 * yields one model (mythril/support/model.py:58-60) and never a count.  For
 * callers that want a second witness when the first is rejected
 * (WitnessEngine.search_all). */
int mg_search_collect(mg_ctx* ctx, mg_prog* prog, uint64_t seed, uint64_t begin, uint64_t count,
                      uint32_t row, uint32_t nrows, uint64_t tile,
                      uint64_t* out_idx,    /* cap */
                      uint32_t* out_rows,   /* cap * nrows, witness-major */
                      size_t cap, mg_collect_result* out, mg_stats* stats);

typedef struct {
  uint64_t index;          /* the nearest mutant: lowest (failed rows, index); never MG_NONE: count >= 1 */
  uint32_t nfail;          /* rows it fails (0: it is a witness) */
  uint32_t reserved;
  uint64_t satisfied;      /* mutants failing no row */
} mg_repair_result;
/* Neighbourhood search around a near-miss: mutants [begin, begin+count) of an
 * explicit base assignment, generated on the device and never stored.  base
 * holds nleaves x 8 limbs in mg_witness_leaves' layout (each value is cut to
 * its leaf's width); mutable_leaves names the nmut leaves (1..1024, indices
 * strictly ascending) a mutant may change; radius (1..4) bounds how many of
 * them it does.  With S the sum of the mutable leaves' widths, mutant m < S
 * flips exactly one bit: bit m - prefix[s] of mutable leaf s, slots in order
 * and bits ascending, so a witness one bit away from base within the mutable
 * leaves is found by count >= S at a known index.  A mutant m >= S applies 1 to
 * radius hashed picks of (leaf, flip a bit | add 2^b | subtract 2^b | replace
 * by a pool entry or a random value); the rule is csrc/mw_mutate.h's, pure in
 * (base, mutable_leaves, seed, radius, m).  Mutants are scored as
 * mg_search_blame scores candidates: the program's trace rows [row, row+nrows)
 * each hold one conjunct's truth (0: failed); with nrows == 0 the program's
 * verdict is the one row.  out->index / out->nfail are the mutant of lowest
 * (failed rows, index), out->satisfied counts the mutants that fail no row:
 * one call either finds a witness (nfail == 0) or returns a nearer base to go
 * on from.  The range is cut into tiles by mg_search_lexmin's rule; each tile
 * is evaluated by mw_repair_kernel, always on the compiled interpreter (the
 * other engines have no such mode), and folded by mg_search_blame's fold:
 * stats->launches == 2 * tiles, stats->evals == count, one upload (the base,
 * the mutable leaves and their prefix sums travel with the launch records)
 * and one synchronisation.  Refused with MG_E_ARG for a null argument, a
 * program without leaves, nmut of 0 or above 1024, a mutable leaf that is no
 * leaf of the program or not above the one before, a radius outside 1..4,
 * count == 0, a wrapping range, begin + count above 2^48, nrows above 1024,
 * rows outside the program's trace, a tile that is no multiple of 256, more
 * than 65536 tiles, and while a search begun with mg_search_begin is pending.
 * Same handle, lock and in-flight protocol as mg_search_blame.  Replaces
 * nothing in the reference: z3 answers a set it finds no model for with unsat
 * or unknown (mythril/laser/smt/solver/solver.py:50-66) and offers no
 * assignment to go on from (WitnessEngine.repair). */
int mg_search_repair(mg_ctx* ctx, mg_prog* prog, const uint32_t* base, const uint32_t* mutable_leaves, size_t nmut,
                     uint64_t seed, uint32_t radius, uint64_t begin, uint64_t count,
                     uint32_t row, uint32_t nrows, uint64_t tile, mg_repair_result* out, mg_stats* stats);
/* The leaf values of mutant `index` of the same base, mutable leaves, seed and
 * radius: what the device evaluated at out->index, in mg_witness_leaves'
 * layout (nleaves x 8 limbs).  Computed on the host from the leaf table and
 * pool the library keeps of a loaded program: no launch, so it is allowed
 * while a begun search is pending.  The same refusals for base,
 * mutable_leaves, nmut and radius.  Replaces nothing in the reference
 * (ModelRef.eval reads a model z3 found; this reads one the search built). */
int mg_repair_leaves(mg_ctx* ctx, const mg_prog* prog, const uint32_t* base, const uint32_t* mutable_leaves,
                     size_t nmut, uint64_t seed, uint32_t radius, uint64_t index, uint32_t* out /* nleaves x 8 */);

/* Evaluate one program on explicit assignments: leaves_soa has n_input_rows
 * rows of ncand u32 (row r, candidate i at [r*ncand + i]).  verdict[i] = 0/1;
 * trace (may be NULL) receives n_trace_rows rows of ncand u32. */
int mg_eval(mg_ctx* ctx, const mg_prog* prog, const uint32_t* leaves_soa, size_t ncand,
            uint32_t* verdict, uint32_t* trace);

/* Evaluate one program on generated candidates [begin, begin+count): the
 * verdict/trace of exactly what mg_search explores (parity tests), trace row
 * r of candidate begin+i at [r*count + i].  Programs the asm interpreter runs
 * are evaluated there, trace rows included (its STORE_W / STORE_N handlers);
 * the rest on the compiled interpreter.  The witness program's evaluation
 * behind WitnessEngine.materialize, in place of z3's model()
 * (mythril/laser/smt/solver/solver.py:68-77) for array cells and function
 * arguments. */
int mg_eval_generated(mg_ctx* ctx, const mg_prog* prog, uint64_t seed, uint64_t begin,
                      size_t count, uint32_t* verdict, uint32_t* trace);

/* The values of every leaf (free variable) of a loaded program at candidate
 * `index`: out receives nleaves x 8 u32 limbs, leaf by leaf in the program's
 * leaf-table order, as the search kernels generate them (the witness values
 * of an index mg_search returned).  Replaces z3's Optimize.model()
 * (mythril/laser/smt/solver/solver.py:68-77) for the free symbols. */
int mg_witness_leaves(mg_ctx* ctx, const mg_prog* prog, uint64_t seed, uint64_t index, uint32_t* out);

/* One-shot evaluation of a program description that is not kept: upload,
 * mg_eval_generated's evaluation of candidates [begin, begin+count) and the
 * release, in one call (a witness program read once at the found index).
 * Same validation, results and trace layout as mg_prog_load +
 * mg_eval_generated + mg_prog_free.  Replaces the reference's model
 * evaluation of the witness (z3 ModelRef.eval, mythril/support/model.py:58-60). */
int mg_eval_program(mg_ctx* ctx, const mg_prog_desc* desc, uint64_t seed, uint64_t begin, size_t count,
                    uint32_t* verdict, uint32_t* trace);

/* Attach a specialised kernel to a loaded program: `image` is a gfx950 code
 * object generated from this program's own IR by mythril_amd/jit.py (one
 * straight-line kernel per program, csrc/mw_jit.h).  It must export
 * `<name>_sig` (the program signature, checked against the loaded program:
 * a code object made for any other program is refused) and `<name>_x`
 * (exhaustive), optionally `<name>_e` (early exit).  mg_search and
 * mg_eval_generated (verdicts only) then launch it instead of the
 * interpreter; witness indices and verdicts are identical.  Same crossing as
 * mg_search (z3 Optimize.check, mythril/laser/smt/solver/solver.py:50-66). */
int mg_prog_attach_kernel(mg_prog* prog, const void* image, size_t size, const char* name);

/* Attach an assembled kernel to a loaded program: `image` is a gfx950 code
 * object that mythril_amd/asmjit.py assembled (llvm-mc + ld.lld, milliseconds)
 * from this program's own code, the asm interpreter's handlers instantiated
 * with literal operands in straight-line order (csrc/mw_asmjit_shell.hip).
 * It must export kernel `<name>` and `<name>_sig` (the program signature,
 * checked as for mg_prog_attach_kernel); the program must be one the asm
 * interpreter runs.  mg_search and mg_eval_generated (verdicts only) then
 * launch it on the asm interpreter's records; results are identical.  A
 * specialised kernel, when also attached, takes precedence.  Same crossing as
 * mg_search (z3 Optimize.check, mythril/laser/smt/solver/solver.py:50-66). */
int mg_prog_attach_asm(mg_prog* prog, const void* image, size_t size, const char* name);

/* 1 if a specialised kernel is attached to the program, else 0. */
int mg_prog_has_kernel(const mg_prog* prog);
/* The engine a search of this program runs on: 0 the compiled interpreter,
 * 1 the threaded-dispatch asm interpreter (every opcode and leaf kind has a
 * handler and the pool fits in LDS; MYTHRIL_AMD_ASM=0 disables it), 2 its
 * specialised kernel, 3 its assembled kernel.  Replaces
 * nothing in the reference: a diagnostic for tests and benchmarks. */
int mg_prog_engine(const mg_prog* prog);

/* Batched Keccak-256 (original 0x01 padding): message i is data[off[i] .. off[i]+len[i]). */
int mg_keccak256(mg_ctx* ctx, const uint8_t* data, size_t ndata, const uint64_t* off,
                 const uint32_t* len, size_t n, uint8_t* out32, mg_stats* stats);

/* Device-resident variant for benchmarking with inputs already in HBM. */
int mg_keccak256_device(mg_ctx* ctx, const uint8_t* d_data, const uint64_t* d_off,
                        const uint32_t* d_len, size_t n, uint8_t* d_out32, mg_stats* stats);

/* Diagnostic: measured INT32 VALU issue rate of the device (v_add_u32, or
 * v_mul_lo_u32 when mul != 0), u32 ops/s — the roofline peak bench.py reports. */
int mg_valu_peak(mg_ctx* ctx, uint32_t mul, double* ops_per_s, double* kernel_ms);

/* Validate a program without a device (the same check mg_prog_load runs). */
int mg_validate_desc(const mg_prog_desc* desc);

const char* mg_last_error(void);

/* Debugging (not a reference crossing): the C-ABI calls in flight on every
 * thread, one line each ("tid=... <call>/<step> arg=N call_ms=T step_ms=T"),
 * written NUL-terminated into buf (at most n bytes); returns how many calls
 * are in flight.  Lock-free: safe from a watchdog thread while another thread
 * is stuck inside a call.  A step slower than MYTHRIL_AMD_SLOW_STEP_MS
 * (default 2000) also prints one line on stderr when it ends. */
int mg_debug_inflight(char* buf, size_t n);

/* Debugging: with MYTHRIL_AMD_STEP_TIMES=1 in the environment, the wall time
 * (ms) and count of every call and step since the last read, one
 * "call/step ms count" line each (the whole call as "call/(call)"); the
 * table is then cleared.  Returns the number of lines (0 when off). */
int mg_debug_step_times(char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif
