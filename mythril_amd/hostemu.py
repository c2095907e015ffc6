"""ctypes binding of the host build of the interpreter (build/host/libmw_host_emu.so).

``csrc/mw_host_emu.cpp`` compiles the very interpreter, ALU and candidate
generator the gfx950 kernels run (mw_interp.h, mw_alu.h, mw_leaf.h) for x86.
It is never a fallback for the device path (runtime.py has none).  Its uses:
tests, and build-time workload preparation — e.g. planting the C5 witness on
the CPU so that ``__graft_entry__.build()`` can pre-compile the benchmark's
specialised kernel (mythril_amd/jit.py) into the in-tree cache, bit for bit
the program bench.py later builds on the device.
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, List, Sequence

import numpy as np

from .compiler import Program, compile_program
from .runtime import MgMinResult, MgProgDesc, make_desc, unpack_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMU = os.path.join(ROOT, "build", "host", "libmw_host_emu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_EMU):
            from .build import build_host_emu
            build_host_emu()
        L = ctypes.CDLL(HOST_EMU)
        L.mwh_eval.restype = ctypes.c_int
        L.mwh_eval.argtypes = [ctypes.POINTER(MgProgDesc), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                               ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.mwh_div_counts.restype = ctypes.c_int
        L.mwh_div_counts.argtypes = [ctypes.POINTER(MgProgDesc), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t,
                                     ctypes.c_void_p]
        L.mwh_search_min.restype = ctypes.c_int
        L.mwh_search_min.argtypes = [ctypes.POINTER(MgProgDesc), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                     ctypes.POINTER(MgMinResult)]
        L.mwh_mutant_leaves.restype = ctypes.c_int
        L.mwh_mutant_leaves.argtypes = [ctypes.POINTER(MgProgDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p]
        L.mg_last_error.restype = ctypes.c_char_p
        _lib = L
    return _lib


def search_min(p: Program, seed: int, begin: int, n: int):
    """(index, objective) of the witness among generated candidates
    [begin, begin+n) whose objective (p's trace rows, 1 to 8 limbs, least
    significant first) is lowest, ties to the lowest index; (None, 0) without
    one.  The host twin of mg_search_min: the same mw_run and the same order
    (csrc/mw_min.h), one candidate after the other."""
    d, keep = make_desc(p)
    out = MgMinResult()
    rc = lib().mwh_search_min(ctypes.byref(d), seed & ((1 << 64) - 1), begin, n, ctypes.byref(out))
    if rc != 0:
        raise RuntimeError(lib().mg_last_error().decode())
    return out.decode()


def search_lexmin(p: Program, seed: int, begin: int, n: int, objs, chunk: int = 1 << 14):
    """(index, [objective values]) of the witness among generated candidates
    [begin, begin+n) whose objectives are lexicographically lowest: objs is a
    list of (row, nrows), objective k the unsigned value of p's trace rows
    [row, row+nrows) (least significant first), objs[0] first in priority,
    ties to the lowest index; (None, [0, ...]) without one.  The CPU twin of
    mg_search_lexmin, over eval_generated with Python integers."""
    if not 1 <= len(objs) <= 8 or n <= 0 or begin + n > 1 << 64:
        raise RuntimeError("search_lexmin: 1 to 8 objectives over a non-empty range")
    for row, nrows in objs:
        if not 1 <= nrows <= 8 or row < 0 or row + nrows > p.n_trace_rows:
            raise RuntimeError("search_lexmin: an objective is 1 to 8 of the program's trace rows")
    best = None
    for at in range(0, n, chunk):
        m = min(chunk, n - at)
        v, tr = eval_generated(p, seed, begin + at, m)
        for j in np.flatnonzero(v):
            j = int(j)
            key = tuple(sum(int(tr[row + k, j]) << (32 * k) for k in range(nrows)) for row, nrows in objs)
            key += (begin + at + j,)
            if best is None or key < best:
                best = key
    if best is None:
        return None, [0] * len(objs)
    return best[-1], list(best[:-1])


def search_blame(p: Program, seed: int, begin: int, n: int, row: int, nrows: int, chunk: int = 1 << 14):
    """(fail, sole, satisfied, near_index, near_nfail) over generated
    candidates [begin, begin+n): p's trace rows [row, row+nrows) each hold one
    conjunct's truth (0: failed); fail[j] counts the candidates failing row j,
    sole[j] those failing row j alone, satisfied those failing none, and
    near_index is the candidate failing the fewest rows (near_nfail), ties to
    the lowest index.  The CPU twin of mg_search_blame, numpy over
    eval_generated's rows; p's own verdict is ignored."""
    if n <= 0 or begin < 0 or begin + n > 1 << 64:
        raise RuntimeError("search_blame: a non-empty range")
    if not 1 <= nrows <= 1024 or row < 0 or row + nrows > p.n_trace_rows:
        raise RuntimeError("search_blame: 1 to 1024 of the program's trace rows")
    fail = np.zeros(nrows, dtype=np.int64)
    sole = np.zeros(nrows, dtype=np.int64)
    satisfied, near = 0, None
    for at in range(0, n, chunk):
        m = min(chunk, n - at)
        _, tr = eval_generated(p, seed, begin + at, m)
        failed = tr[row:row + nrows] == 0
        nfail = failed.sum(axis=0)
        fail += failed.sum(axis=1)
        sole += failed[:, nfail == 1].sum(axis=1)
        satisfied += int((nfail == 0).sum())
        j = int(np.argmin(nfail))          # the first of the lowest
        if near is None or int(nfail[j]) < near[0]:
            near = (int(nfail[j]), begin + at + j)
    return [int(x) for x in fail], [int(x) for x in sole], satisfied, near[1], near[0]


def search_collect(p: Program, seed: int, begin: int, n: int, cap: int, row: int = 0, nrows: int = 0,
                   chunk: int = 1 << 14):
    """(indices, rows, total) over generated candidates [begin, begin+n): total
    is the number whose verdict is 1, indices the min(total, cap) lowest of
    them in ascending order, rows a (len(indices), nrows) uint32 array with p's
    trace rows [row, row+nrows) of each.  The CPU twin of mg_search_collect,
    numpy over eval_generated; the same refusals."""
    if n <= 0 or begin < 0 or begin + n > 1 << 64:
        raise RuntimeError("search_collect: a non-empty range")
    if not 1 <= cap <= 65536:
        raise RuntimeError("search_collect: room for 1 to 65536 witnesses")
    if not 0 <= nrows <= 64 or (nrows and (row < 0 or row + nrows > p.n_trace_rows)):
        raise RuntimeError("search_collect: at most 64 of the program's trace rows")
    total = 0
    indices: list = []
    rows = []
    for at in range(0, n, chunk):
        m = min(chunk, n - at)
        v, tr = eval_generated(p, seed, begin + at, m)
        hit = np.flatnonzero(v)
        total += int(hit.size)
        keep = hit[:cap - len(indices)]
        indices.extend(begin + at + int(j) for j in keep)
        if nrows and keep.size:
            rows.append(np.asarray(tr)[row:row + nrows][:, keep].T)
    out = np.concatenate(rows).astype(np.uint32) if rows else np.zeros((len(indices), nrows), dtype=np.uint32)
    return indices, out, total


def leaf_limbs(p: Program, seed: int, index: int) -> np.ndarray:
    """The leaf values (nleaves x 8 limbs, uint32) of generated candidate
    ``index``: the host twin of mg_witness_leaves (mwh_leaf_values)."""
    d, keep = make_desc(p)
    out = np.zeros(max(1, len(p.leaf_nodes)) * 8, dtype=np.uint32)
    f = lib().mwh_leaf_values
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(MgProgDesc), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    rc = f(ctypes.byref(d), seed & ((1 << 64) - 1), index, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(lib().mg_last_error().decode())
    return out[:len(p.leaf_nodes) * 8].reshape(-1, 8)


def _mutant_args(p: Program, base, mutable):
    nl = len(p.leaf_nodes)
    b = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1)
    if b.size != 8 * nl:
        raise RuntimeError("search_repair: base is nleaves x 8 limbs")
    if any(not 0 <= int(x) < 1 << 32 for x in mutable):
        raise RuntimeError("search_repair: a mutable leaf is not a leaf of the program")
    return b, np.ascontiguousarray(list(mutable), dtype=np.uint32)


def mutant_leaves(p: Program, base, mutable, seed: int, radius: int, m: int) -> np.ndarray:
    """The leaf values (nleaves x 8 limbs, uint32) of mutant m of ``base``
    (the same layout) with the leaves ``mutable`` free to change: csrc/mw_mutate.h's
    rule through mwh_mutant_leaves, the host twin of mg_repair_leaves."""
    b, mut = _mutant_args(p, base, mutable)
    d, keep = make_desc(p)
    out = np.zeros(max(1, b.size), dtype=np.uint32)
    rc = lib().mwh_mutant_leaves(ctypes.byref(d), b.ctypes.data if b.size else None, mut.ctypes.data if mut.size else None,
                                 mut.size, seed & ((1 << 64) - 1), radius, m, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(lib().mg_last_error().decode())
    return out[:b.size].reshape(-1, 8)


def leaves_soa(p: Program, limbs: Sequence[np.ndarray]) -> np.ndarray:
    """mg_eval's SoA input rows from per-candidate leaf limbs (nleaves x 8 each)."""
    rows = np.zeros((max(p.n_input_rows, 1), len(limbs)), dtype=np.uint32)
    for li in range(len(p.leaf_nodes)):
        r0, nl = p.input_rows_for(li)
        for j, v in enumerate(limbs):
            rows[r0:r0 + nl, j] = v[li, :nl]
    return rows


def search_repair(p: Program, base, mutable, seed: int, radius: int, begin: int, n: int, row: int = 0,
                  nrows: int = 0, chunk: int = 1 << 10):
    """(index, nfail, satisfied) over mutants [begin, begin+n) of ``base``:
    the mutant of lowest (failed rows among p's trace rows [row, row+nrows),
    index) and how many fail none; with nrows == 0 p's verdict is the one row.
    The CPU twin of mg_search_repair: the mutants built by mwh_mutant_leaves,
    sent through mwh_eval's SoA inputs; the same key and the same refusals."""
    if n <= 0 or begin < 0 or begin + n > 1 << 48:
        raise RuntimeError("search_repair: a non-empty range of mutant indices below 2^48")
    if not 0 <= nrows <= 1024 or (nrows and (row < 0 or row + nrows > p.n_trace_rows)):
        raise RuntimeError("search_repair: at most 1024 of the program's trace rows")
    d, keep = make_desc(p)
    satisfied, near = 0, None
    for at in range(0, n, chunk):
        k = min(chunk, n - at)
        soa = leaves_soa(p, [mutant_leaves(p, base, mutable, seed, radius, begin + at + j) for j in range(k)])
        v = np.zeros(k, dtype=np.uint32)
        t = np.zeros(max(p.n_trace_rows, 1) * k, dtype=np.uint32)
        rc = lib().mwh_eval(ctypes.byref(d), soa.ctypes.data, 0, 0, k, 0, v.ctypes.data, t.ctypes.data)
        if rc != 0:
            raise RuntimeError(lib().mg_last_error().decode())
        rows = t.reshape(max(p.n_trace_rows, 1), k)[row:row + nrows] if nrows else v.reshape(1, k)
        nfail = (rows == 0).sum(axis=0)
        satisfied += int((nfail == 0).sum())
        j = int(np.argmin(nfail))          # the first of the lowest
        if near is None or int(nfail[j]) < near[0]:
            near = (int(nfail[j]), begin + at + j)
    return near[1], near[0], satisfied


def eval_generated(p: Program, seed: int, begin: int, n: int):
    """Verdicts and trace rows of generated candidates [begin, begin+n) (host build)."""
    d, keep = make_desc(p)
    v = np.zeros(n, dtype=np.uint32)
    t = np.zeros(max(p.n_trace_rows, 1) * n, dtype=np.uint32)
    rc = lib().mwh_eval(ctypes.byref(d), None, seed, begin, n, 0, v.ctypes.data, t.ctypes.data)
    if rc != 0:
        raise RuntimeError(lib().mg_last_error().decode())
    return v, t.reshape(max(p.n_trace_rows, 1), n)


def div_counts(p: Program, seed: int, begin: int, n: int) -> dict:
    """Division path counts (mg_stats.lane_div_* names) of the host build over
    generated candidates [begin, begin+n); a host 'wave' is one candidate."""
    d, keep = make_desc(p)
    out = np.zeros(4, dtype=np.uint64)
    rc = lib().mwh_div_counts(ctypes.byref(d), seed, begin, n, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(lib().mg_last_error().decode())
    return {"lane_div_steps": int(out[0]), "lane_div_full": int(out[1]), "lane_div_short": int(out[2]),
            "lane_div_general": int(out[3])}


def term_values(terms: Sequence, index: int, seed: int) -> List[int]:
    """Values of `terms` at generated candidate `index` (synth.build_c5's evaluate)."""
    p = compile_program([], trace=list(terms))
    _, tr = eval_generated(p, seed, index, 1)
    return [unpack_trace(p, tr, t)[0] for t in terms]
